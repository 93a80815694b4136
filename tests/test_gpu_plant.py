"""mg_harvest_upload on an MI355X (k_xfer_place, k_xfer_scatter_idx), against the
NumPy model of the header's text (tests/plantmodel.py).

a. word for word: sentinel device images of test_gpu_harvest's three kinds of batch
   (600 lanes, 560 uploaded), saturated host rows, lists of 1, 63, 64, 65 and 129
   lanes in every shape, counts on both sides of a 64-dword tile column of every
   plane, host images at the batch's capacities, at the maxima and one below; after
   each call the whole batch is downloaded at full capacity and compared;
b. the resident list (lanes = None), also after an mg_step;
c. the round trip with mg_harvest_download, in place and into other lanes;
d. the resident reset image is not written;
e. the event counters of a planted lane are 0;
f. every refusal, with the image unchanged;
g. the hook loop of tests/test_plant_model_cpu.py on the device.
"""
import ctypes
import dataclasses
from collections import Counter
from copy import copy

import numpy as np
import pytest

import exploremodel
import harvestmodel
import plantmodel
import symcosim
import test_gpu_fork
from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.lanes import (MG_EINVAL, MG_ENOCODE, MG_ESTATE, MG_FENT_NONE, MG_HALT_RETURN, MG_HALT_STOP, MG_HOOK, MG_OK,
                               LaneBatch)
from mythril_amd.laser import symbolic as sym
from test_gpu_fork import _expected_full, _full
from test_gpu_harvest import (ALL, FULL, HPATH_CAP, KINDS, N, UPLOADED, _batch, _chain_batch, _forget, _null_soa,
                              _start)
from test_harvest_model_cpu import FINISHED, PATHS_PER_ROOT, ROOTS, SPARE_ONE_SHOT, SPARE_RECYCLE, DEPTH, finished_paths
from test_plant_model_cpu import model_hook_loop, move_to_free, resolve
from xfermodel import DeviceImage, live_diff, saturated, sentinel_filled, whole_diff

pytestmark = pytest.mark.gpu

A5 = 0xA5A5A5A5
COUNTS = ("sp", "msize", "storage_count", "trace_len", "rec_len", "n_nodes", "n_consts")
CAPS = {"sp": "stack_cap", "msize": "mem_cap", "storage_count": "storage_cap", "trace_len": "trace_cap",
        "rec_len": "rec_cap", "n_nodes": "node_cap", "n_consts": "const_cap"}


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


# ---------------------------------------------------------------- the device image
def _sentinel_image(shape, cid):
    """sentinel_filled as an image mg_lanes_upload accepts and moves whole: every count
    at its capacity, a loaded code, finished statuses (even lanes STOP, odd RETURN)."""
    b = sentinel_filled(shape)
    b.code_id[:] = cid
    b.status[0::2], b.status[1::2] = MG_HALT_STOP, MG_HALT_RETURN
    b.calldata_len[:] = shape.calldata_cap
    for count, cap in CAPS.items():
        if count in ("n_nodes", "n_consts") and not shape.node_cap:
            continue
        getattr(b, count)[:] = getattr(shape, cap)
    return b


class Rig:
    """One batch on the device and its model, kept in step."""

    def __init__(self, dev, kind):
        self.dev, self.kind = dev, kind
        self.shape, self.explore = KINDS[kind]
        _forget(dev)                                          # test_gpu_harvest's batch is replaced
        if not hasattr(dev, "_harvest_cid"):
            dev._harvest_cid = dev.load_code(test_gpu_fork.CODE)
        self.cid = dev._harvest_cid
        dev.alloc(self.shape)
        if self.explore:
            dev.explore_alloc(HPATH_CAP)
        self.sentinel = _sentinel_image(dataclasses.replace(self.shape, n=UPLOADED), self.cid)
        self.model = DeviceImage(self.shape)
        self.paths = exploremodel.Paths(N, HPATH_CAP) if self.explore else None
        self.restore()
        # lanes [560, 600) hold what the allocation left: read once, kept by the model from here on
        self.model.img = _full(dev, self.shape)

    def restore(self):
        """The sentinel image again in lanes [0, 560); lanes [560, 600) keep what they hold."""
        self.dev.upload(self.sentinel)
        self.model.upload(self.sentinel, 0, UPLOADED, host_first=0)
        if self.explore:
            p = exploremodel.Paths(N, HPATH_CAP)
            p.path[:], p.path_len[:], p.root[:] = A5, HPATH_CAP, A5
            self.dev.explore_upload_paths(p.path, p.path_len, p.root)
            self.paths = p

    def check(self, what):
        got, want = _full(self.dev, self.shape), _expected_full(self.model)
        assert whole_diff(got, want) == [], what
        if self.explore:
            path, path_len, root = self.dev.explore_paths(0, N)
            keep = np.arange(HPATH_CAP)[None, :] < self.paths.path_len.astype(np.int64)[:, None]
            assert np.array_equal(path_len, self.paths.path_len) and np.array_equal(root, self.paths.root), what
            assert np.array_equal(path, np.where(keep, self.paths.path, 0)), what


_rigs = {}


def _rig(dev, kind):
    if getattr(dev, "_plant_kind", None) != kind or getattr(dev, "_harvest_kind", None) is not None:
        _rigs.clear()
        _rigs[kind] = Rig(dev, kind)
        dev._plant_kind = kind
    return _rigs[kind]


def _drop_rig(dev):
    dev._plant_kind = None
    _rigs.clear()


def _raw_upload(dev, lanes, host, with_sym=True, rows=None, no_fent=False):
    """mg_harvest_upload as the C ABI takes it: (rc, message)."""
    arr = None if lanes is None else np.ascontiguousarray(np.asarray(lanes, dtype=np.uint32))
    soa = host.soa() if host is not None else None
    if no_fent:
        soa.fent = None
    s = host.sym_soa_range(0, host.n) if host is not None and host.symbolic and with_sym else None
    path, path_len, root = rows if rows is not None else (None, None, None)
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = dev.lib.mg_harvest_upload(dev.ctx, ptr(arr), ctypes.addressof(soa) if soa is not None else None,
                                   ctypes.addressof(s) if s is not None else None, ptr(path), ptr(path_len), ptr(root))
    return rc, dev.lib.mg_last_error(dev.ctx).decode()


# -------------------------------------------------------------------- a. word for word
def _lists():
    """(name, lanes) of 1, 63, 64, 65 and 129 lanes in every shape the issue names."""
    out = [("lane 0", [0]), ("lane 599", [N - 1]), ("one never uploaded", [575]),
           ("never uploaded", list(range(UPLOADED, N)))]
    rng = np.random.default_rng(0x11575)
    for k in (63, 64, 65, 129):
        out.append((f"run of {k}", list(range(100, 100 + k))))
        out.append((f"every other, {k}", list(range(1, 2 * k, 2))))
        edge = [l for e in range(64, N, 64) for l in range(e - 4, e + 4)]          # 8 lanes around each tile edge
        fill = [l for l in range(200, N) if l not in edge][:max(k - len(edge), 0)]   # 72 edge lanes, then others
        out.append((f"tile edges, {k}", sorted(edge[:k] + fill)))
        inner = rng.choice(np.arange(1, N - 1), size=k - 2, replace=False)
        out.append((f"ends, {k}", sorted([0, N - 1] + inner.tolist())))
    out.append(("into the never uploaded, 129", list(range(N - 129, N))))
    return out


def _variants(shape):
    """Largest counts of a call, on both sides of one 64-dword tile column per plane
    (stack and cval 8 units, storage 4, memory 256 bytes, node 16, trace, records, stag
    and mtag 64, sttag 32 -- above this shape's storage capacity, so its largest)."""
    c = lambda **kw: {k: min(v, getattr(shape, CAPS[k])) for k, v in kw.items()}
    return {"column": c(sp=8, n_consts=8, storage_count=4, msize=256, n_nodes=16, trace_len=64, rec_len=64),
            "column + 1": c(sp=9, n_consts=9, storage_count=5, msize=288, n_nodes=17, trace_len=65, rec_len=65),
            "tags": c(sp=20, n_consts=1, storage_count=6, msize=64, n_nodes=1, trace_len=1, rec_len=128),
            "tags + 1": c(sp=19, n_consts=0, storage_count=1, msize=96, n_nodes=35, trace_len=70, rec_len=129),
            "empty": c(sp=0, n_consts=0, storage_count=0, msize=0, n_nodes=0, trace_len=0, rec_len=0)}


def _host_rows(shape, n, top, rng, cid, host_caps, explore, one_holds_it=True):
    """Saturated host rows of `n` lanes whose largest counts are `top`: one row (any)
    holds each maximum, the others lie below it.  host_caps: 'full' (the batch's
    capacities), 'maxima' (the counts' maxima), 'below' (one below: the counts clip)."""
    caps = {cap: getattr(shape, cap) for cap in CAPS.values()}
    if host_caps != "full":
        d = 0 if host_caps == "maxima" else 1
        caps = {CAPS[c]: max(v - (32 if c == "msize" else 1) * d, 0) for c, v in top.items()}
        caps["stack_cap"] = max(caps["stack_cap"], 1)
        if shape.node_cap:
            caps["node_cap"], caps["const_cap"] = max(caps["node_cap"], 1), max(caps["const_cap"], 1)
    if not shape.node_cap:
        caps["node_cap"] = caps["const_cap"] = 0
    hshape = dataclasses.replace(shape, n=n, **caps)
    host = saturated(hshape, rng, cid)
    host.status[:] = rng.integers(1, 12, size=n)              # any status but MG_RUNNING: nothing here may step
    host.flags[:] = rng.integers(0, 8, size=n)
    host.calldata_len[:] = rng.integers(0, hshape.calldata_cap + 1, size=n)
    for count, v in top.items():
        if count in ("n_nodes", "n_consts") and not shape.node_cap:
            continue
        v = min(v, getattr(hshape, CAPS[count]))
        step = 32 if count == "msize" else 1
        a = getattr(host, count)
        a[:] = (rng.integers(0, v // step, size=n) * step) if one_holds_it and v else v
        a[rng.integers(0, n)] = v
    rows = None
    if explore:
        plen = rng.integers(0, HPATH_CAP + 1, size=n).astype(np.uint32)
        rows = (rng.integers(1, 1 << 32, size=(n, HPATH_CAP), dtype=np.uint32), plen,
                rng.integers(0, 1 << 32, size=n, dtype=np.uint32))
    return host, rows


@pytest.mark.parametrize("kind", list(KINDS))
def test_upload_equals_the_model_word_for_word(dev, kind):
    rig = _rig(dev, kind)
    shape, rng = rig.shape, np.random.default_rng(0x97A7)
    variants = _variants(shape)
    checked = 0
    for li, (name, lanes) in enumerate(_lists()):
        assert lanes == sorted(set(lanes)) and 0 <= lanes[0] and lanes[-1] < N
        # every list with two variants in turn; every variant and host capacity with the lists of 65 and 129
        wide = len(lanes) in (65, 129)
        for vi, (vname, top) in enumerate(variants.items()):
            if not wide and vi not in (li % len(variants), (li + 1) % len(variants)):
                continue
            for host_caps in (("full", "maxima", "below") if wide and name.startswith(("ends", "tile")) else ("full",)):
                if host_caps != "full" and vname == "empty":
                    continue
                host, rows = _host_rows(shape, len(lanes), top, rng, rig.cid, host_caps, rig.explore)
                rig.restore()
                rc, msg = _raw_upload(dev, lanes, host, rows=rows)
                assert rc == MG_OK, (name, vname, host_caps, msg)
                plantmodel.upload(rig.model, lanes, host, rig.paths, rows)
                rig.check((kind, name, vname, host_caps))
                checked += 1
    # every row at the maxima (the saturated image itself), through the wrapper
    lanes = list(range(3, 3 + 129 * 4, 4))
    host, rows = _host_rows(shape, 129, {c: getattr(shape, cap) for c, cap in CAPS.items()}, rng, rig.cid, "full",
                            rig.explore, one_holds_it=False)
    rig.restore()
    dev.harvest_upload(lanes, host, *(rows or ()))
    plantmodel.upload(rig.model, lanes, host, rig.paths, rows)
    rig.check((kind, "saturated"))
    # a host image without fent, trace and records: the fills
    slim, rows = _host_rows(dataclasses.replace(shape, trace_cap=0, rec_cap=0), 65, variants["column + 1"], rng, rig.cid,
                            "full", False)
    lanes = list(range(30, 160, 2))
    rig.restore()
    rc, msg = _raw_upload(dev, lanes, slim, no_fent=True)
    assert rc == MG_OK, msg
    slim.fent = None
    plantmodel.upload(rig.model, lanes, slim)
    assert (rig.model.img.fent[lanes] == MG_FENT_NONE).all()
    assert not shape.trace_cap or not rig.model.img.trace_len[lanes].any()
    rig.check((kind, "no fent, trace or records"))
    if shape.node_cap:
        # sym = NULL: the symbolic planes stay; path = NULL: the path planes stay
        host, _ = _host_rows(shape, 65, variants["column"], rng, rig.cid, "full", False)
        rig.restore()
        rc, msg = _raw_upload(dev, lanes, host, with_sym=False)
        assert rc == MG_OK, msg
        plain = LaneBatch(dataclasses.replace(host.shape, node_cap=0, const_cap=0))
        for f in plain._fields():
            getattr(plain, f)[...] = getattr(host, f)
        plantmodel.upload(rig.model, lanes, plain)
        rig.check((kind, "sym is null"))
    print(f"{kind}: {checked + 3} uploads equal the model word for word")


# ------------------------------------------------------------------ b. the resident list
@pytest.mark.parametrize("stepped", [False, True], ids=["at once", "after a step"])
def test_the_resident_list(dev, stepped):
    rig = _rig(dev, "explore")
    rig.restore()
    rng = np.random.default_rng(0xB1)
    skip = sorted(set(range(N)) - set(range(5, 5 + 3 * 65, 3)))
    want_lanes, want = harvestmodel.select(rig.model.img, 1 << MG_HALT_STOP | 1 << MG_HALT_RETURN, skip, None,
                                           rig.paths.path_len)
    info = dev.harvest_select(1 << MG_HALT_STOP | 1 << MG_HALT_RETURN, skip)
    assert info.n == want.n == 65
    lanes, hb, path, path_len, root = dev.harvest_download(info, shape=dataclasses.replace(rig.shape, n=info.n))
    assert lanes.tolist() == want_lanes.tolist()
    if stepped:
        st = dev.step()                                       # no lane runs: the image and the selection stay
        assert st.lane_steps == 0
    # every field changes on the host
    host, rows = _host_rows(rig.shape, info.n, _variants(rig.shape)["column + 1"], rng, rig.cid, "full", True)
    assert not np.array_equal(host.pc, hb.pc) and not np.array_equal(rows[0], path)
    dev.harvest_upload(None, host, *rows)
    plantmodel.upload(rig.model, lanes, host, rig.paths, rows)
    rig.check("the resident list")
    # the selection is still there, and still the same list
    again = dev.harvest_download(info, shape=dataclasses.replace(rig.shape, n=info.n))[0]
    assert again.tolist() == lanes.tolist()


# -------------------------------------------------------------------- c. the round trip
def test_download_then_upload_is_the_identity(dev):
    _drop_rig(dev)
    shape, model, paths = _batch(dev, "explore")
    before, paths_before = _full(dev, shape), dev.explore_paths(0, N)
    chosen = sorted(set(range(0, UPLOADED, 3)) | {UPLOADED - 1})
    info = dev.harvest_select(ALL, sorted(set(range(N)) - set(chosen)))
    lanes, hb, path, path_len, root = dev.harvest_download(info)
    assert lanes.tolist() == chosen
    dev.harvest_upload(None, hb, path, path_len, root)
    assert whole_diff(_full(dev, shape), before) == []
    for a, b in zip(dev.explore_paths(0, N), paths_before):
        assert np.array_equal(a, b)
    dev.harvest_upload(lanes, hb, path, path_len, root)       # the same through a list of the caller's
    assert whole_diff(_full(dev, shape), before) == []
    # into the lanes that were never uploaded: the same live image there
    info = dev.harvest_select(ALL, max_lanes=N - UPLOADED)
    lanes, hb, path, path_len, root = dev.harvest_download(info)
    dest = list(range(UPLOADED, N))
    dev.harvest_upload(dest, hb, path, path_len, root)
    after = _full(dev, shape)
    assert whole_diff(after, before, lanes=range(UPLOADED)) == []
    moved, orig = LaneBatch(dataclasses.replace(shape, n=len(dest))), LaneBatch(dataclasses.replace(shape, n=len(dest)))
    for f in moved._fields():
        getattr(moved, f)[...] = getattr(after, f)[dest]
        getattr(orig, f)[...] = getattr(before, f)[lanes]
    assert live_diff(moved, orig) == []
    got = dev.explore_paths(UPLOADED, N - UPLOADED)
    assert np.array_equal(got[0], path) and np.array_equal(got[1], path_len) and np.array_equal(got[2], root)
    _forget(dev)                                              # the batch is no longer test_gpu_harvest's


def test_moved_lanes_decode_to_the_same_constraints(dev):
    _drop_rig(dev)
    _forget(dev)
    spare = SPARE_ONE_SHOT + 16
    vm, root, shape, b, free = _chain_batch(dev, spare)
    _start(dev, shape, b)
    st = dev.explore(free, max_rounds=64, resume=True)
    assert (st.forks, st.free_used, st.starved) == (ROOTS * DEPTH, ROOTS * DEPTH, 0)
    unused = free[st.free_used:]
    assert len(unused) == 16
    info = dev.harvest_select(FINISHED, unused, max_lanes=16)
    lanes, hb, path, path_len, hroot = dev.harvest_download(info)
    assert info.n == 16 and int(path_len.max()) >= 2
    dev.harvest_upload(unused, hb, path, path_len, hroot)
    whole = LaneBatch(shape)
    dev.download(whole)
    wpath, wlen, wroot = dev.explore_paths(0, shape.n)
    for i in range(16):
        src, dst = int(lanes[i]), unused[i]
        assert wroot[dst] == wroot[src] and wlen[dst] == wlen[src]
        a, c = vm._materialise(whole, src, copy(root)), vm._materialise(whole, dst, copy(root))
        symcosim._replay(whole, src, a)
        symcosim._replay(whole, dst, c)
        ga = sym.path_constraints(whole, src, a, wpath[src, :int(wlen[src])])
        gc = sym.path_constraints(whole, dst, c, wpath[dst, :int(wlen[dst])])
        assert ga is not None and [x.raw for x in ga] == [x.raw for x in gc] and len(ga) == int(wlen[src])


# ------------------------------------------------------------------- d. the reset image
def test_the_reset_image_is_not_written(dev):
    _drop_rig(dev)
    _forget(dev)
    n = 130
    shape = dataclasses.replace(FULL, n=n)
    if not hasattr(dev, "_harvest_cid"):
        dev._harvest_cid = dev.load_code(test_gpu_fork.CODE)
    cid = dev._harvest_cid
    rng = np.random.default_rng(0x4E5)
    known, initial = saturated(shape, rng, cid), saturated(shape, rng, cid)
    for f in ("sp", "msize", "trace_len", "rec_len"):        # what mg_lanes_reset asks of an image
        getattr(initial, f)[:] = 0
    initial.storage_count[:] = rng.integers(0, shape.storage_cap + 1, size=n)
    dev.alloc(shape)
    dev.upload(known)
    dev.upload(initial)
    model = DeviceImage(shape)
    model.upload(known, 0, n)
    model.upload(initial, 0, n)
    lanes = list(range(0, n, 2))
    host, _ = _host_rows(shape, len(lanes), {c: getattr(shape, cap) for c, cap in CAPS.items()}, rng, cid, "full", False,
                         one_holds_it=False)
    dev.harvest_upload(lanes, host)
    plantmodel.upload(model, lanes, host)
    assert whole_diff(_full(dev, shape), _expected_full(model)) == []
    dev.reset()
    dev.sync()
    plantmodel.reset(model, initial)
    assert whole_diff(_full(dev, shape), _expected_full(model)) == []
    assert np.array_equal(model.img.pc, initial.pc) and not model.img.sp.any()


# --------------------------------------------------------------- e. the event counters
def test_the_event_counters_of_a_planted_lane_are_zero(dev):
    _drop_rig(dev)
    _forget(dev)
    cid = dev.load_code(bytes.fromhex("6000600020" "6002600a0a" "00"))      # SHA3 of nothing, 10 ** 2, STOP
    shape = dataclasses.replace(KINDS["no-symbolic-planes"][0], n=130)
    b = LaneBatch(shape)
    for l in range(130):
        b.set_lane(l, code_id=cid)
    dev.alloc(shape)
    dev.upload(b)
    dev.step()
    sha3, exp = dev.event_counts(130)
    assert (sha3 == 1).all() and (exp == 1).all()
    lanes = list(range(1, 130, 2))
    done = LaneBatch(dataclasses.replace(shape, n=len(lanes)))
    for l in range(len(lanes)):
        done.set_lane(l, code_id=cid)
    done.status[:] = MG_HALT_STOP
    dev.harvest_upload(lanes, done)
    sha3, exp = dev.event_counts(130)
    assert not sha3[lanes].any() and not exp[lanes].any()
    assert (sha3[0::2] == 1).all() and (exp[0::2] == 1).all()


# ------------------------------------------------------------------------ f. refusals
def test_refusals_leave_the_image(dev):
    fresh = GpuDevice(0)
    try:
        host = LaneBatch(dataclasses.replace(FULL, n=4))
        rc, msg = _raw_upload(fresh, [0, 1, 2, 3], host)
        assert rc == MG_ESTATE and "mg_lanes_alloc" in msg, (rc, msg)
        fresh.alloc(dataclasses.replace(FULL, n=64))
        rc, msg = _raw_upload(fresh, [0, 1, 2, 3], host)
        assert rc == MG_ESTATE and "mg_lanes_upload" in msg, (rc, msg)
    finally:
        fresh.close()
    _drop_rig(dev)
    rig = _rig(dev, "explore")                                # a new allocation: no selection on it
    shape, rng = rig.shape, np.random.default_rng(0xF0)
    top = _variants(shape)["column + 1"]
    lanes = list(range(10, 80))

    def rows_of(n=70, **kw):
        return _host_rows(dataclasses.replace(shape, **kw), n, top, rng, rig.cid, "full", True)

    def refused(what, want_rc, named, *args, **kw):
        rc, msg = _raw_upload(dev, *args, **kw)
        assert rc == want_rc and named in msg, (what, rc, msg)
        rig.check(what)

    host, rows = rows_of()
    refused("the resident list without a selection", MG_ESTATE, "selection", None, host, rows=rows)
    refused("a null host", MG_EINVAL, "null", lanes, None)
    for what, bad, named in (("equal neighbours", lanes[:68] + [79, 79], "lanes[69]"),
                             ("descending", [11, 10] + lanes[2:], "lanes[1]"),
                             ("outside the batch", lanes[:69] + [N], "lanes[69]"),
                             ("far outside the batch", lanes[:69] + [0xFFFFFFFE], "lanes[69]")):
        refused(what, MG_EINVAL, named, bad, host, rows=rows)
    for what, kw in (("stack_cap", dict(stack_cap=shape.stack_cap + 1)), ("mem_cap", dict(mem_cap=shape.mem_cap + 32)),
                     ("storage_cap", dict(storage_cap=shape.storage_cap + 1)), ("rec_cap", dict(rec_cap=shape.rec_cap + 1)),
                     ("trace_cap", dict(trace_cap=shape.trace_cap + 1)), ("calldata_cap", dict(calldata_cap=shape.calldata_cap + 4)),
                     ("node_cap", dict(node_cap=shape.node_cap + 1)), ("const_cap", dict(const_cap=shape.const_cap + 1))):
        h, r = rows_of(**kw)
        refused(what + " above the batch's", MG_EINVAL, "capacities", lanes, h, rows=r)
    # sym->n != n
    soa, s = host.soa(), host.sym_soa_range(0, 69)
    arr = np.array(lanes, dtype=np.uint32)
    rc = dev.lib.mg_harvest_upload(dev.ctx, arr.ctypes.data, ctypes.addressof(soa), ctypes.addressof(s), None, None, None)
    assert rc == MG_EINVAL and "symbolic host image" in dev.lib.mg_last_error(dev.ctx).decode()
    rig.check("sym->n != n")
    # path, path_len and root go together
    for trio in ((rows[0], None, None), (None, rows[1], rows[2]), (rows[0], rows[1], None)):
        refused("a partial path", MG_EINVAL, "go together", lanes, host, rows=trio)
    # per row; the message names the device lane
    for count in COUNTS + ("calldata_len",):
        h, r = rows_of()
        getattr(h, count)[7] = (getattr(h.shape, CAPS[count]) if count != "calldata_len" else h.shape.calldata_cap) + \
            (32 if count == "msize" else 1)
        refused(count + " above its capacity", MG_EINVAL, "lane 17", lanes, h, rows=r)
    h, r = rows_of()
    h.msize[7] = 48
    refused("msize not a multiple of 32", MG_EINVAL, "lane 17", lanes, h, rows=r)
    h, r = rows_of()
    h.code_id[69] = 0xFFFF
    refused("an unknown code", MG_ENOCODE, "lane 79", lanes, h, rows=r)
    h, r = rows_of()
    r[1][3] = HPATH_CAP + 1
    refused("path_len above path_cap", MG_EINVAL, "lane 13", lanes, h, rows=r)
    # the resident list: host->n != info.n; a bad row is named by its row
    info = dev.harvest_select(1 << MG_HALT_STOP, max_lanes=70)
    assert info.n == 70
    for n in (69, 71):
        h, r = rows_of(n)
        refused("host->n != info.n", MG_EINVAL, "selection of 70", None, h, rows=r)
    h, r = rows_of()
    h.sp[7] = h.shape.stack_cap + 1
    refused("a bad row of the resident list", MG_EINVAL, "row 7", None, h, rows=r)
    # n == 0 succeeds and does nothing, with a list and without a selection's match
    empty = LaneBatch(dataclasses.replace(shape, n=0))
    soa = _null_soa(0)
    assert dev.lib.mg_harvest_upload(dev.ctx, arr.ctypes.data, ctypes.addressof(soa), None, None, None, None) == MG_OK
    dev.harvest_upload([], empty)
    rig.check("no rows")
    # an accepted call after all that
    dev.harvest_upload(None, host, *rows)
    want_lanes, _ = harvestmodel.select(rig.model.img, 1 << MG_HALT_STOP, (), 70, rig.paths.path_len)
    plantmodel.upload(rig.model, want_lanes, host, rig.paths, rows)
    rig.check("an accepted upload")
    # sym without symbolic planes, path without explore planes
    _drop_rig(dev)
    rig = _rig(dev, "no-symbolic-planes")
    symhost = saturated(dataclasses.replace(rig.shape, n=70, node_cap=4, const_cap=4), rng, rig.cid)
    refused("sym without symbolic planes", MG_EINVAL, "symbolic planes", lanes, symhost)
    plain = LaneBatch(dataclasses.replace(rig.shape, n=70))
    plain.code_id[:] = rig.cid
    refused("path without explore planes", MG_EINVAL, "explore planes", lanes, plain, rows=rows)


# ---------------------------------------------------------------------- g. the hook loop
@pytest.mark.parametrize("in_place", [True, False], ids=["in place", "into free lanes"])
def test_the_hook_loop_on_the_device(dev, in_place):
    _drop_rig(dev)
    _forget(dev)
    mask = hook_mask_for([0x5B])
    # the unhooked one-shot run: 8 roots and 48 spare lanes, one call
    vm, root, shape, b, free = _chain_batch(dev, SPARE_ONE_SHOT)
    _start(dev, shape, b)
    st = dev.explore(free, max_rounds=64, resume=True)
    info, lanes, hb, path, path_len, hroot = dev.harvest(FINISHED, skip=free[st.free_used:])
    one_shot = finished_paths(hb, lanes, path, path_len, hroot)
    assert len(one_shot) == ROOTS * PATHS_PER_ROOT == 56
    # hooked, with 4 spare lanes
    want, bound = model_hook_loop(in_place)
    vm, root, shape, b, free = _chain_batch(dev, SPARE_RECYCLE)
    _start(dev, shape, b)
    got, iterations, resolved = [], 0, 0
    while len(free) < shape.n:
        iterations += 1
        assert iterations <= bound, "the hook loop takes more iterations than on the model"
        st = dev.explore(free, hook_mask=mask, max_rounds=2, resume=True)
        free = free[st.free_used:]
        info = dev.harvest_select(1 << MG_HOOK, free)
        if info.n:
            lanes, hb, path, path_len, hroot = dev.harvest_download(info)
            resolve(hb)
            resolved += info.n
            if in_place:
                dev.harvest_upload(None, hb, path, path_len, hroot)
            else:
                dest, hb, rows, free = move_to_free(free, lanes, hb, (path, path_len, hroot))
                dev.harvest_upload(dest, hb, *rows)
        info, lanes, hb, path, path_len, hroot = dev.harvest(FINISHED & ~(1 << MG_HOOK), skip=free)
        if info.n:
            got += finished_paths(hb, lanes, path, path_len, hroot)
        free = harvestmodel.merge_free(free, lanes)
    assert len(got) == 56 and Counter(got) == Counter(one_shot) == Counter(want)
    assert resolved == ROOTS * DEPTH                          # every jump side lands on a pad's JUMPDEST
    print(f"hook loop on the device: {iterations} iterations, {resolved} lanes resolved and put back")
