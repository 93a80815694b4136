"""mg_harvest_select, mg_harvest_download and mg_explore_resume on an MI355X
(lane_harvest.cuh), against the NumPy model of the header's text
(tests/harvestmodel.py).

a. select: n, matched, the eight maxima and the list, over masks, skip lists and
   caps, on 600 lanes (three scan blocks, the last partial; lanes [560, 600) never
   uploaded), under the default and under MG_HARVEST_BLOCKS = 1 and 2 (a tile
   carry inside one block; two blocks of two and one tiles);
b. download: word for word into sentinel-filled host images at full capacities,
   at the selection's maxima and one below each, for selections that cross every
   64-lane tile edge of the gather, with and without sym and path, on three batches;
c. refusals, with the device image unchanged;
d. mg_explore_resume: R rounds in one mg_explore equal one round and R - 1 resumed
   rounds; an uploaded prefix survives a resume and is reset by mg_explore;
e. the recycle loop of tests/test_harvest_model_cpu.py on the device.
"""
import ctypes
import dataclasses
from collections import Counter
from copy import copy

import numpy as np
import pytest

import exploremodel
import harvestmodel
import symcosim
import test_gpu_fork
from mythril_amd import native
from mythril_amd.device import GpuDevice
from mythril_amd.lanes import MG_EINVAL, MG_ESTATE, MG_HALT_STOP, MG_OK, LaneBatch, MgLaneSoa
from mythril_amd.laser import symbolic as sym
from test_gpu_explore import (INVALID, PATH_CAP, ROUNDS, SOURCES, _hand_image, _layout, _paths, _root_image,
                              _upload_known)
from test_gpu_fork import _full
from test_harvest_model_cpu import (CHAIN, CHAIN_PATH_CAP, DEPTH, FINISHED, MAX_ITERATIONS, PATHS_PER_ROOT, ROOTS,
                                    SPARE_ONE_SHOT, SPARE_RECYCLE, chain_step, finished_paths)
from xfermodel import SCALARS, DeviceImage, saturated, sentinel_filled, whole_diff

pytestmark = pytest.mark.gpu

N, UPLOADED = 600, 560
FULL = dataclasses.replace(test_gpu_fork.SHAPE, n=N)         # symbolic planes, a trace and records
KINDS = {"explore": (FULL, True),                            # ... and explore planes
         "no-explore-planes": (FULL, False),
         "no-symbolic-planes": (dataclasses.replace(FULL, node_cap=0, const_cap=0, trace_cap=0, rec_cap=0), False)}
HPATH_CAP = 7
BLOCKS = [None, "1", "2"]
BLOCK_IDS = ["default", "blocks1", "blocks2"]
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


@pytest.fixture(params=BLOCKS, ids=BLOCK_IDS)
def blocks(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("MG_HARVEST_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("MG_HARVEST_BLOCKS", request.param)
    return request.param


def _draw_counts(b, rng):
    """Counts below the capacities, so that a selection's maxima depend on its lanes."""
    sh, n = b.shape, b.n
    b.sp[:] = rng.integers(0, sh.stack_cap + 1, size=n)
    b.msize[:] = 32 * rng.integers(0, sh.mem_cap // 32 + 1, size=n)
    b.storage_count[:] = rng.integers(0, sh.storage_cap + 1, size=n)
    b.trace_len[:] = rng.integers(0, sh.trace_cap + 1, size=n)
    b.rec_len[:] = rng.integers(0, sh.rec_cap + 1, size=n)
    if sh.node_cap:
        b.n_nodes[:] = rng.integers(0, sh.node_cap + 1, size=n)
        b.n_consts[:] = rng.integers(0, sh.const_cap + 1, size=n)


_built = {}


def _batch(dev, kind):
    """The device holds the batch `kind`; returns (shape, model, paths or None).  The
    model and the host images are made once per kind; the device is loaded again
    only when another batch was on it."""
    shape, explore = KINDS[kind]
    if kind not in _built:
        rng = np.random.default_rng(0x4A57)
        up = dataclasses.replace(shape, n=UPLOADED)
        known, host = saturated(up, rng, 0), saturated(up, rng, 0)
        host.status[:] = rng.integers(0, 12, size=UPLOADED)
        _draw_counts(host, rng)
        model = DeviceImage(shape)
        model.img.status[:] = harvestmodel.NEVER_UPLOADED
        model.upload(known, 0, UPLOADED, host_first=0)
        model.upload(host, 0, UPLOADED, host_first=0)
        paths = None
        if explore:
            paths = exploremodel.Paths(N, HPATH_CAP)
            for l in range(N):                               # every length 0 .. path_cap, by hand
                k = l % (HPATH_CAP + 1)
                paths.path_len[l] = k
                paths.path[l, :k] = [(l * 131 + e * 7 + 1) & ALL for e in range(k)]
                paths.root[l] = (l * 7) % N
        _built[kind] = (known, host, model, paths)
    known, host, model, paths = _built[kind]
    if getattr(dev, "_harvest_kind", None) != kind:
        if not hasattr(dev, "_harvest_cid"):
            dev._harvest_cid = dev.load_code(test_gpu_fork.CODE)
        cid = dev._harvest_cid
        for b in (known, host):
            b.code_id[:] = cid
        model.img.code_id[:UPLOADED] = cid
        dev.alloc(shape)
        if explore:
            dev.explore_alloc(HPATH_CAP)
            dev.explore_upload_paths(paths.path, paths.path_len, paths.root)
        dev.upload(known)
        dev.upload(host)
        dev._harvest_kind = kind
    return shape, model, paths


def _forget(dev):
    dev._harvest_kind = None


def _null_soa(n):
    s = MgLaneSoa()
    s.n = n
    return s


def _info_key(info):
    return (info.n, info.matched) + tuple(getattr(info, f) for f in harvestmodel.FIELDS)


def _list(dev, info):
    """The resident list alone: a download with every host field skipped."""
    lanes = np.full(info.n, 0xA5A5A5A5, dtype=np.uint32)
    soa = _null_soa(info.n)
    rc = dev.lib.mg_harvest_download(dev.ctx, lanes.ctypes.data, ctypes.addressof(soa), None, None, None, None)
    assert rc == MG_OK, dev.lib.mg_last_error(dev.ctx)
    return lanes


# ------------------------------------------------------------------------ a. select
@pytest.mark.parametrize("kind", list(KINDS))
def test_select_equals_the_model(dev, blocks, kind):
    shape, model, paths = _batch(dev, kind)
    img, plen = model.img, paths.path_len if paths else None
    masks = [1 << 3, 1 << 1 | 1 << 2 | 1 << 7 | 1 << 11, ALL, 0]
    skips = [[], list(range(N)), list(range(0, N, 2))]
    assert (img.status[UPLOADED:] == harvestmodel.NEVER_UPLOADED).all() and set(img.status[:UPLOADED]) == set(range(12))
    checked = 0
    for mask in masks:
        for skip in skips:
            matched = harvestmodel.select(img, mask, skip, None, plen)[1].matched
            for cap in sorted({0, 1, 63, 64, 65, max(matched - 1, 0), matched, N + 100}):
                want_lanes, want = harvestmodel.select(img, mask, skip, cap, plen)
                info = dev.harvest_select(mask, skip, cap)
                assert _info_key(info) == want.key(), (mask, len(skip), cap)
                assert _list(dev, info).tolist() == want_lanes.tolist(), (mask, len(skip), cap)
                assert info.n == 0 or int(want_lanes.max()) < UPLOADED        # never-uploaded lanes never match
                checked += 1
    # max_lanes=None is every matching lane
    info = dev.harvest_select(ALL)
    assert (info.n, info.matched) == (UPLOADED, UPLOADED)
    print(f"{kind}, MG_HARVEST_BLOCKS={blocks}: {checked} selections equal the model; kernel_ms {info.kernel_ms:.4f}")


# ---------------------------------------------------------------------- b. download
def _selections(rng):
    """Lane sets of 1, 63, 64, 65 and 129 lanes; all but the first hold lane 0 and the last uploaded lane."""
    out = [[0], [UPLOADED - 1]]
    for k in (63, 64, 65, 129):
        inner = rng.choice(np.arange(1, UPLOADED - 1), size=k - 2, replace=False)
        out.append(sorted([0, UPLOADED - 1] + inner.tolist()))
    return out


def _host_shapes(dev_shape, info, with_sym):
    """Full capacities, the selection's maxima, one below each maximum (which clips)."""
    symcaps = lambda nodes, consts: dict(node_cap=max(nodes, 1), const_cap=max(consts, 1)) if with_sym else \
        dict(node_cap=0, const_cap=0)
    full = dataclasses.replace(dev_shape, n=info.n, **symcaps(dev_shape.node_cap, dev_shape.const_cap))
    at = dataclasses.replace(dev_shape, n=info.n, stack_cap=max(info.sp, 1), mem_cap=info.msize,
                             storage_cap=info.storage_count, trace_cap=info.trace_len, rec_cap=info.rec_len,
                             **symcaps(info.n_nodes, info.n_consts))
    below = dataclasses.replace(dev_shape, n=info.n, stack_cap=max(info.sp - 1, 1), mem_cap=max(info.msize - 32, 0),
                                calldata_cap=dev_shape.calldata_cap - 4, storage_cap=max(info.storage_count - 1, 0),
                                trace_cap=max(info.trace_len - 1, 0), rec_cap=max(info.rec_len - 1, 0),
                                **symcaps(info.n_nodes - 1, info.n_consts - 1))
    return {"full": full, "maxima": at, "below": below}


def _download(dev, host, with_path, path_cap):
    """mg_harvest_download into `host` (sym when it has the planes) and, with_path,
    into sentinel-filled path arrays."""
    n = host.n
    lanes = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
    path = np.full((n, path_cap), 0xA5A5A5A5, dtype=np.uint32) if with_path else None
    path_len = np.full(n, 0xA5A5A5A5, dtype=np.uint32) if with_path else None
    root = np.full(n, 0xA5A5A5A5, dtype=np.uint32) if with_path else None
    soa = host.soa()
    s = host.sym_soa_range(0, n) if host.symbolic else None
    rc = dev.lib.mg_harvest_download(dev.ctx, lanes.ctypes.data, ctypes.addressof(soa),
                                     ctypes.addressof(s) if s is not None else None,
                                     path.ctypes.data if with_path else None, path_len.ctypes.data if with_path else None,
                                     root.ctypes.data if with_path else None)
    return rc, lanes, path, path_len, root


@pytest.mark.parametrize("kind", list(KINDS))
def test_download_equals_the_model_word_for_word(dev, blocks, kind):
    shape, model, paths = _batch(dev, kind)
    plen = paths.path_len if paths else None
    everyone = set(range(N))
    checked = 0
    for chosen in _selections(np.random.default_rng(0xD0)):
        skip = sorted(everyone - set(chosen))
        want_lanes, want = harvestmodel.select(model.img, ALL, skip, None, plen)
        info = dev.harvest_select(ALL, skip)
        assert want_lanes.tolist() == chosen and _info_key(info) == want.key()
        for with_sym in ([True, False] if shape.node_cap else [False]):
            for name, hshape in _host_shapes(shape, info, with_sym).items():
                for with_path in ([True, False] if paths else [False]):
                    got, ref = sentinel_filled(hshape), sentinel_filled(hshape)
                    rc, lanes, path, path_len, root = _download(dev, got, with_path, HPATH_CAP)
                    assert rc == MG_OK, dev.lib.mg_last_error(dev.ctx)
                    ref_paths = harvestmodel.download(model, want_lanes, want, ref, paths if with_path else None)
                    assert lanes.tolist() == chosen
                    assert whole_diff(got, ref) == [], (len(chosen), name, with_sym, with_path)
                    if with_path:
                        assert np.array_equal(path, ref_paths[0]) and np.array_equal(path_len, ref_paths[1])
                        assert np.array_equal(root, ref_paths[2])
                        assert all(not path[i, int(path_len[i]):].any() for i in range(len(chosen)))
                    checked += 1
    # the wrapper's default image is the slim one, and holds the same cells
    info = dev.harvest_select(ALL, sorted(everyone - set(range(0, UPLOADED, 5))))
    lanes, slim, path, path_len, root = dev.harvest_download(info)
    want_lanes, want = harvestmodel.select(model.img, ALL, sorted(everyone - set(range(0, UPLOADED, 5))), None, plen)
    ref = LaneBatch(slim.shape)
    ref_paths = harvestmodel.download(model, want_lanes, want, ref, paths)
    assert slim.shape == dev.harvest_shape(info) and slim.shape.mem_cap % 32 == 0
    assert lanes.tolist() == want_lanes.tolist() and whole_diff(slim, ref) == []
    assert (path is None) == (paths is None) and (paths is None or np.array_equal(path, ref_paths[0]))
    print(f"{kind}, MG_HARVEST_BLOCKS={blocks}: {checked} downloads equal the model word for word")


def test_harvest_of_every_lane_equals_a_range_download(dev):
    """The two users of the lane and symbolic transfer plans against each other: a
    harvest of all 130 lanes (two 64-lane tiles and a tail of 2) and
    download_range(first=0, n=130), both into sentinel-filled images of the full
    capacities.  Below the selection's maxima -- so below each lane's own counts --
    every cell is equal; above them the harvest image keeps its sentinels."""
    _forget(dev)
    n = 130
    shape = dataclasses.replace(FULL, n=n)
    if not hasattr(dev, "_harvest_cid"):
        dev._harvest_cid = dev.load_code(test_gpu_fork.CODE)
    rng = np.random.default_rng(0x130)
    known, host = saturated(shape, rng, dev._harvest_cid), saturated(shape, rng, dev._harvest_cid)
    # every count below its capacity: each plane has cells above the selection's maximum
    rows = {"stack": "sp", "memory": "msize", "storage": "storage_count", "trace": "trace_len", "rec": "rec_len",
            "stag": "sp", "node": "n_nodes", "cval": "n_consts", "mtag": "msize", "sttag": "storage_count"}
    caps = {"sp": shape.stack_cap, "storage_count": shape.storage_cap, "trace_len": shape.trace_cap,
            "rec_len": shape.rec_cap, "n_nodes": shape.node_cap, "n_consts": shape.const_cap}
    for count, cap in caps.items():
        getattr(host, count)[:] = rng.integers(0, cap, size=n)
    host.msize[:] = 32 * rng.integers(0, shape.mem_cap // 32, size=n)
    caps["msize"] = shape.mem_cap
    paths = exploremodel.Paths(n, HPATH_CAP)
    for l in range(n):
        k = l % HPATH_CAP                                    # 0 .. path_cap - 1
        paths.path_len[l] = k
        paths.path[l, :k] = [(l * 131 + e * 7 + 1) & ALL for e in range(k)]
        paths.root[l] = (l * 7) % n
    dev.alloc(shape)
    dev.explore_alloc(HPATH_CAP)
    dev.explore_upload_paths(paths.path, paths.path_len, paths.root)
    dev.upload(known)                                        # the whole device image is known and dirty
    dev.upload(host)
    info = dev.harvest_select(ALL)
    assert (info.n, info.matched) == (n, n)
    for count, cap in caps.items():
        assert getattr(info, count) == int(getattr(host, count).max()) < cap, count
    got, ref = sentinel_filled(shape), sentinel_filled(shape)
    rc, lanes, path, path_len, root = _download(dev, got, True, HPATH_CAP)
    assert rc == MG_OK, dev.lib.mg_last_error(dev.ctx)
    dev.download_range(ref, 0, n)
    assert lanes.tolist() == list(range(n))
    for f in list(SCALARS) + ["fent", "trace_len", "rec_len", "n_nodes", "n_consts", "env", "calldata"]:
        assert np.array_equal(getattr(got, f), getattr(ref, f)), f
    for f, count in rows.items():
        top = getattr(info, count)
        g, r = getattr(got, f), getattr(ref, f)
        assert np.array_equal(g[:, :top], r[:, :top]), f
        for i in range(n):                                   # what is live is what was uploaded
            k = int(getattr(host, count)[i])
            assert np.array_equal(g[i, :k], getattr(host, f)[i, :k]), (f, i)
        above = np.ascontiguousarray(g[:, top:]).view(np.uint8)
        assert above.size and (above == 0xA5).all(), f
    want = dev.explore_paths(0, n)
    for a, b in zip((path, path_len, root), want):
        assert np.array_equal(a, b)
    assert np.array_equal(path_len, paths.path_len) and np.array_equal(root, paths.root)


# ------------------------------------------------------------------------ c. refusals
def _select_rc(dev, mask, skip, n_skip=None, cap=ALL, info=True):
    arr = np.ascontiguousarray(np.asarray(skip, dtype=np.uint32)) if skip is not None else None
    out = native.MgHarvestInfo()
    rc = dev.lib.mg_harvest_select(dev.ctx, mask, arr.ctypes.data if arr is not None and arr.size else None,
                                   (arr.size if arr is not None else 0) if n_skip is None else n_skip, cap,
                                   ctypes.byref(out) if info else None)
    return rc, dev.lib.mg_last_error(dev.ctx).decode(), out


def test_refusals_leave_the_image(dev):
    fresh = GpuDevice(0)
    try:
        rc, msg, _ = _select_rc(fresh, ALL, [])
        assert rc == MG_ESTATE and "mg_lanes_alloc" in msg, (rc, msg)
        soa = _null_soa(0)
        assert fresh.lib.mg_harvest_download(fresh.ctx, None, ctypes.addressof(soa), None, None, None, None) == MG_ESTATE
        fresh.alloc(dataclasses.replace(FULL, n=64))
        rc, msg, _ = _select_rc(fresh, ALL, [])
        assert rc == MG_ESTATE and "upload" in msg, (rc, msg)
    finally:
        fresh.close()
    shape, model, paths = _batch(dev, "explore")
    _forget(dev)                                             # the allocs below replace the batch
    # the same batch allocated again: no selection on it yet
    dev.alloc(shape)
    dev.explore_alloc(HPATH_CAP)
    dev.explore_upload_paths(paths.path, paths.path_len, paths.root)
    dev.upload(_built["explore"][0])
    dev.upload(_built["explore"][1])
    before = _full(dev, shape)
    paths_before = dev.explore_paths(0, N)

    def unchanged(what):
        assert whole_diff(_full(dev, shape), before) == [], what
        for a, b in zip(dev.explore_paths(0, N), paths_before):
            assert np.array_equal(a, b), what

    soa = _null_soa(0)
    assert dev.lib.mg_harvest_download(dev.ctx, None, ctypes.addressof(soa), None, None, None, None) == MG_ESTATE
    unchanged("download before the first select")
    bad = {
        "a null info": (dict(mask=ALL, skip=[], info=False), "info"),
        "a null skip": (dict(mask=ALL, skip=None, n_skip=3), "skip"),
        "equal neighbours": (dict(mask=ALL, skip=[5, 9, 9]), "skip[2]"),
        "descending": (dict(mask=ALL, skip=[5, 4]), "skip[1]"),
        "outside the batch": (dict(mask=ALL, skip=[5, N]), "skip[1]"),
        "far outside the batch": (dict(mask=ALL, skip=[0xFFFFFFFE]), "skip[0]"),
    }
    for what, (kw, named) in bad.items():
        rc, msg, _ = _select_rc(dev, **kw)
        assert rc == MG_EINVAL and named in msg, (what, rc, msg)
        unchanged(what)
    # valid and empty: a mask of 0, a cap of 0; a download after n == 0 succeeds and writes nothing
    for kw in (dict(mask=0, skip=[]), dict(mask=ALL, skip=[], cap=0)):
        rc, msg, out = _select_rc(dev, **kw)
        assert rc == MG_OK and out.n == 0, (kw, rc, msg)
        host = sentinel_filled(dataclasses.replace(shape, n=0))
        rc, *_ = _download(dev, host, True, HPATH_CAP)
        assert rc == MG_OK
    unchanged("empty selections")
    # a selection of 70 lanes, then every refused download: nothing is written on either side
    info = dev.harvest_select(ALL, max_lanes=70)
    assert info.n == 70
    wrong = {
        "host->n above": dataclasses.replace(shape, n=71),
        "host->n below": dataclasses.replace(shape, n=69),
        "stack_cap above the batch's": dataclasses.replace(shape, n=70, stack_cap=shape.stack_cap + 1),
        "mem_cap above the batch's": dataclasses.replace(shape, n=70, mem_cap=shape.mem_cap + 32),
        "storage_cap above the batch's": dataclasses.replace(shape, n=70, storage_cap=shape.storage_cap + 1),
        "node_cap above the batch's": dataclasses.replace(shape, n=70, node_cap=shape.node_cap + 1),
        "rec_cap above the batch's": dataclasses.replace(shape, n=70, rec_cap=shape.rec_cap + 1),
    }
    for what, hshape in wrong.items():
        host = sentinel_filled(hshape)
        rc, lanes, path, *_ = _download(dev, host, True, HPATH_CAP)
        assert rc == MG_EINVAL, (what, rc)
        assert whole_diff(host, sentinel_filled(hshape)) == [] and (lanes == 0xA5A5A5A5).all() and \
            (path == 0xA5A5A5A5).all(), what
        unchanged(what)
    # path, path_len and root go together
    host = sentinel_filled(dataclasses.replace(shape, n=70))
    soa, plen = host.soa(), np.zeros(70, dtype=np.uint32)
    assert dev.lib.mg_harvest_download(dev.ctx, None, ctypes.addressof(soa), None, None, plen.ctypes.data, None) == MG_EINVAL
    assert whole_diff(host, sentinel_filled(host.shape)) == []
    # the selection is still good
    rc, lanes, *_ = _download(dev, host, True, HPATH_CAP)
    assert rc == MG_OK and lanes.tolist() == list(range(70))
    unchanged("an accepted download")
    # mg_explore_alloc, mg_sym_alloc and mg_lanes_alloc drop the selection
    plain = KINDS["no-symbolic-planes"][0]
    b = saturated(dataclasses.replace(plain, n=UPLOADED), np.random.default_rng(7), int(before.code_id[0]))
    dev.alloc(plain)
    dev.upload(b)
    assert dev.harvest_select(ALL).n == UPLOADED
    host = sentinel_filled(dataclasses.replace(plain, n=UPLOADED))
    before_plain = _full(dev, plain)
    # path without explore planes, sym without symbolic planes
    rc, *_ = _download(dev, host, True, HPATH_CAP)
    assert rc == MG_EINVAL and whole_diff(host, sentinel_filled(host.shape)) == []
    symhost = sentinel_filled(dataclasses.replace(plain, n=UPLOADED, node_cap=4, const_cap=4))
    rc, *_ = _download(dev, symhost, False, HPATH_CAP)
    assert rc == MG_EINVAL and whole_diff(symhost, sentinel_filled(symhost.shape)) == []
    assert whole_diff(_full(dev, plain), before_plain) == []
    rc, *_ = _download(dev, host, False, HPATH_CAP)
    assert rc == MG_OK
    assert dev.lib.mg_sym_alloc(dev.ctx, 4, 4) == MG_OK
    rc, *_ = _download(dev, host, False, HPATH_CAP)
    assert rc == MG_ESTATE, "mg_sym_alloc drops the selection"
    assert dev.lib.mg_harvest_select(dev.ctx, ALL, None, 0, ALL, ctypes.byref(native.MgHarvestInfo())) == MG_OK
    assert dev.lib.mg_explore_alloc(dev.ctx, 3) == MG_OK
    rc, *_ = _download(dev, host, False, HPATH_CAP)
    assert rc == MG_ESTATE, "mg_explore_alloc drops the selection"
    assert dev.lib.mg_harvest_select(dev.ctx, ALL, None, 0, ALL, ctypes.byref(native.MgHarvestInfo())) == MG_OK
    dev.alloc(plain)
    rc, *_ = _download(dev, host, False, HPATH_CAP)
    assert rc == MG_ESTATE, "mg_lanes_alloc drops the selection"


# ----------------------------------------------------------------- d. mg_explore_resume
@pytest.mark.parametrize("name", ["exceptions.sol.o", "overflow.sol.o"])
def test_r_rounds_equal_one_round_and_resumed_rounds(dev, name):
    _forget(dev)
    roots = (0, 70, 300)
    vm, eng, root, shape, b, free = _root_image(dev, name, roots=roots)
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    _upload_known(dev, shape, b)
    st = dev.explore(free, max_rounds=ROUNDS)
    left, left_paths = _full(dev, shape), _paths(dev, shape.n)
    assert st.rounds == ROUNDS and st.forks >= 3 * 3 and st.starved == 0 and st.path_full == 0
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    _upload_known(dev, shape, b)
    used, sums = 0, Counter()
    for r in range(ROUNDS):
        one = dev.explore(free[used:], max_rounds=1, resume=r > 0)
        assert one.rounds == 1
        used += one.free_used
        for f in ("rounds", "forks", "made_jump", "starved", "path_full", "free_used", "lane_steps"):
            sums[f] += getattr(one, f)
    assert whole_diff(left, _full(dev, shape)) == []
    for got, want in zip(_paths(dev, shape.n), left_paths):
        assert np.array_equal(got, want)
    assert {f: getattr(st, f) for f in sums} == dict(sums) and st.running == one.running
    assert int(left_paths[1].max()) >= 2
    print(f"{name}: {st.forks} forks in {ROUNDS} rounds, one call and {ROUNDS} calls agree bit for bit")


def test_an_uploaded_prefix_survives_resume_and_is_reset_by_explore(dev):
    _forget(dev)
    n, free = _layout("between")
    cid = dev.load_code(test_gpu_fork.CODE)
    shape, host = _hand_image(n, cid, np.random.default_rng(0xE1))
    prefix = exploremodel.Paths(n, PATH_CAP)
    for l in range(n):
        k = l % 4
        prefix.path_len[l] = k
        prefix.path[l, :k] = [(l * 17 + e + 1) << 1 | (e & 1) for e in range(k)]
        prefix.root[l] = (l + 11) % n
    got = {}
    for resume in (True, False):
        dev.alloc(shape)
        dev.explore_alloc(PATH_CAP)
        dev.upload(host)
        dev.explore_upload_paths(prefix.path, prefix.path_len, prefix.root)
        st = dev.explore(free, max_rounds=1, resume=resume)
        assert st.forks >= 14 and st.made_jump >= 13
        got[resume] = (_full(dev, shape), _paths(dev, n), st)
    assert whole_diff(got[True][0], got[False][0]) == []     # the lane image does not depend on the paths
    path, path_len, root = got[True][1]
    forked = [s for s in SOURCES if int(path_len[s]) == s % 4 + 1]
    children = [l for l in free[:got[True][2].free_used]]
    assert len(forked) >= 14 and len(children) == got[True][2].made_jump
    for s in forked:
        k = s % 4
        assert path[s, :k].tolist() == prefix.path[s, :k].tolist() and int(root[s]) == (s + 11) % n and not path[s, k] & 1
    for d in children:
        src = [s for s in forked if path[s, int(path_len[s]) - 1] >> 1 == path[d, int(path_len[d]) - 1] >> 1 and
               int(path_len[s]) == int(path_len[d]) and int(root[s]) == int(root[d])]
        assert src and int(path[d, int(path_len[d]) - 1]) & 1 == 1
        assert any(path[d, :int(path_len[d]) - 1].tolist() == prefix.path[s, :s % 4].tolist() for s in src)
    untouched = [l for l in range(n) if l not in forked and l not in children]
    assert path_len[untouched].tolist() == prefix.path_len[untouched].tolist()
    assert root[untouched].tolist() == prefix.root[untouched].tolist()
    # mg_explore: the same forks from a reset
    path, path_len, root = got[False][1]
    assert path_len[forked].tolist() == [1] * len(forked) and root[forked].tolist() == forked
    assert not path_len[untouched].any() and root[untouched].tolist() == untouched
    assert sorted(int(r) for r in root[children]) == sorted(s for s in forked if s != INVALID)


# -------------------------------------------------------------- e. the recycle loop
def _chain_batch(dev, spare):
    ws, addr = symcosim.deploy_code(CHAIN)
    vm = symcosim.new_vm(dev)
    root = symcosim.initial(ws, addr)
    shape = dataclasses.replace(vm._shape([root]), n=ROOTS + spare)
    b = LaneBatch(shape)
    b.status[:] = MG_HALT_STOP                               # the spare lanes: halted and free
    for lane in range(ROOTS):
        vm._pack(b, lane, root)
        b.steps[lane] = 0
    b.code_id[:] = b.code_id[0]
    return vm, root, shape, b, list(range(ROOTS, shape.n))


def _start(dev, shape, b):
    dev.alloc(shape)
    dev.explore_alloc(CHAIN_PATH_CAP)
    _upload_known(dev, shape, b)
    z = exploremodel.Paths(shape.n, CHAIN_PATH_CAP)          # root[l] = l, no path: what the resumes continue
    dev.explore_upload_paths(z.path, z.path_len, z.root)


def _model_runs(shape, b, spare_free, recycle):
    """The same run on the model, from the same packed image."""
    import forkmodel
    model = DeviceImage(shape)
    model.upload(saturated(shape, np.random.default_rng(0xE2), int(b.code_id[0])), 0, shape.n)
    model.upload(b, 0, shape.n)
    codes = {int(b.code_id[0]): forkmodel.CodeTable(CHAIN)}
    paths, free, out = exploremodel.Paths(shape.n, CHAIN_PATH_CAP), list(spare_free), []
    for _ in range(MAX_ITERATIONS if recycle else 1):
        _, _, used, _ = harvestmodel.explore(model, codes, free, paths, 2 if recycle else 64, chain_step, resume=True)
        free = free[used:]
        lanes, info = harvestmodel.select(model.img, FINISHED, free, None, paths.path_len)
        host = LaneBatch(dataclasses.replace(shape, n=info.n))
        got = harvestmodel.download(model, lanes, info, host, paths)
        if info.n:
            out += finished_paths(host, lanes, *got)
        free = harvestmodel.merge_free(free, lanes)
        if len(free) == shape.n:
            break
    return out


def test_the_recycle_loop_on_the_device(dev):
    _forget(dev)
    # one shot: 8 roots and 48 spare lanes, one call
    vm, root, shape, b, free = _chain_batch(dev, SPARE_ONE_SHOT)
    _start(dev, shape, b)
    st = dev.explore(free, max_rounds=64, resume=True)
    assert (st.forks, st.made_jump, st.starved, st.path_full, st.rounds) == (ROOTS * DEPTH, ROOTS * DEPTH, 0, 0, DEPTH + 1)
    info, lanes, hb, path, path_len, hroot = dev.harvest(FINISHED, skip=free[st.free_used:])
    one_shot = finished_paths(hb, lanes, path, path_len, hroot)
    assert len(one_shot) == ROOTS * PATHS_PER_ROOT and info.matched == info.n
    model_one = _model_runs(shape, b, free, recycle=False)
    assert Counter(one_shot) == Counter(model_one)
    # recycling: 8 roots and 4 spare lanes
    vm, root, shape, b, free = _chain_batch(dev, SPARE_RECYCLE)
    _start(dev, shape, b)
    recycled, iterations, sampled = [], 0, 0
    while len(free) < shape.n:
        iterations += 1
        assert iterations <= MAX_ITERATIONS, "the recycle loop does not terminate"
        st = dev.explore(free, max_rounds=2, resume=True)
        free = free[st.free_used:]
        info, lanes, hb, path, path_len, hroot = dev.harvest(FINISHED, skip=free)
        assert info.n == info.matched
        if info.n:
            recycled += finished_paths(hb, lanes, path, path_len, hroot)
            # the harvested image decodes to the constraints a whole-batch download gives
            whole = LaneBatch(shape)
            dev.download(whole)
            wpath, wlen, _ = dev.explore_paths(0, shape.n)
            for i in range(0, info.n, 3):
                lane = int(lanes[i])
                a, c = vm._materialise(hb, i, copy(root)), vm._materialise(whole, lane, copy(root))
                symcosim._replay(hb, i, a)
                symcosim._replay(whole, lane, c)
                ga = sym.path_constraints(hb, i, a, path[i, :int(path_len[i])])
                gc = sym.path_constraints(whole, lane, c, wpath[lane, :int(wlen[lane])])
                assert ga is not None and [x.raw for x in ga] == [x.raw for x in gc] and len(ga) == int(path_len[i])
                sampled += 1
        free = harvestmodel.merge_free(free, lanes)
    assert len(recycled) == ROOTS * PATHS_PER_ROOT == 56
    assert Counter(recycled) == Counter(one_shot) == Counter(_model_runs(shape, b, list(range(ROOTS, shape.n)), True))
    assert sampled >= 8
    print(f"recycle loop on the device: {iterations} iterations, {len(recycled)} finished paths, {sampled} lanes decoded")
