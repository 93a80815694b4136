"""mg_explore_check on an MI355X (path_eval.cuh): a lane's recorded path evaluated
from its arena against the candidate models, where the arena is.

1. the hand-written arenas of tests/pathcases.py (checked on the CPU against the
   decoder + flattener + kernel-2 oracle route by test_path_check_cpu.py) uploaded
   into 192 lanes: first_sat and sat_bits equal tests/pathmodel.py word for word at
   1, 64, 65 and 130 models, over lane ranges that start and end inside a wave, and
   with the pool left resident by eval_upload;
2. images mg_explore itself made from two roots with different transaction ids:
   the device equals the model on every lane, and kernel 2 on the decoded and
   flattened path on every lane the model does not call unknown;
3. `allowed` masking the first satisfying model moves first_sat to the next one;
4. refusals leave the answers and the image untouched;
5. a check changes nothing of the image.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import pathcases
import pathmodel
import symcases
import symcosim
from mythril_amd import abi, native
from mythril_amd.device import GpuDevice
from mythril_amd.lanes import MG_EINVAL, MG_ESTATE, MG_HALT_STOP, LaneBatch
from mythril_amd.laser import symbolic as sym
from mythril_amd.smt import flatten
from mythril_amd.smt.lower import TableSig
from mythril_amd.smt.program import ArrayInterp, ModelPool
from test_gpu_fork import _full
from xfermodel import whole_diff

pytestmark = pytest.mark.gpu

UNKNOWN, NO_MODEL, UNBOUND = abi.MG_PATH_UNKNOWN, abi.MG_BV_NO_MODEL, abi.MG_PATH_UNBOUND


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def _upload_image(dev, im):
    cid = dev.load_code(b"\x00")
    b = im.batch.copy()
    b.code_id[:] = cid
    dev.alloc(pathcases.SHAPE)
    dev.explore_alloc(pathcases.PATH_CAP)
    dev.upload(b)
    dev.explore_upload_paths(im.path, im.path_len, im.root)
    return b


def _first_of(row) -> int:
    for w, x in enumerate(row):
        x = int(x)
        if x:
            return 64 * w + (x & -x).bit_length() - 1
    return NO_MODEL


# ------------------------------------------------------------ 1. hand-written arenas
@pytest.mark.parametrize("count", pathcases.MODEL_COUNTS)
def test_hand_written_arenas_equal_the_model(dev, count):
    im = pathcases.image(count)
    _upload_image(dev, im)
    path, path_len, root = dev.explore_paths(0, pathcases.N_LANES)
    assert path.tolist() == im.path.tolist() and path_len.tolist() == im.path_len.tolist()
    assert root.tolist() == im.root.tolist()
    want_fs, want_bits = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding)
    fs, bits, ms = dev.explore_check(im.pool, im.bindings, im.lane_binding, bits=True)
    bad = [(i, im.cases[i].name if i < len(im.cases) else "filler", int(fs[i]), int(want_fs[i]))
           for i in range(pathcases.N_LANES) if fs[i] != want_fs[i] or bits[i].tolist() != want_bits[i].tolist()]
    assert bad == []
    assert [i for i in range(pathcases.N_LANES) if fs[i] == UNKNOWN] == im.unknown
    # ranges that start and end inside a wave of lanes; first_sat alone; the resident pool
    for first, n in ((37, 100), (64, 64), (1, 190), (191, 1), (63, 2)):
        part_fs, part_bits, _ = dev.explore_check(None, im.bindings, im.lane_binding, first=first, n=n, bits=True)
        assert part_fs.tolist() == want_fs[first:first + n].tolist(), (first, n)
        assert part_bits.tolist() == want_bits[first:first + n].tolist(), (first, n)
    only_fs, none, _ = dev.explore_check(im.pool, im.bindings, im.lane_binding)
    assert none is None and only_fs.tolist() == want_fs.tolist()
    # models == NULL after mg_eval_upload: the pool that upload left resident
    prog, kept = flatten.compile_sets([[]])
    assert kept == [0]
    dev.eval_upload(prog, im.pool)
    again_fs, again_bits, _ = dev.explore_check(None, im.bindings, im.lane_binding, bits=True)
    assert again_fs.tolist() == want_fs.tolist() and again_bits.tolist() == want_bits.tolist()
    assert dev.eval_run() >= 0.0                                  # the resident programs are still there
    sat = int((fs < count).sum())
    print(f"{count} models: {sat} satisfied, {int((fs == NO_MODEL).sum())} without a model, "
          f"{len(im.unknown)} unknown, kernel {ms:.3f} ms")


# ------------------------------------------------------------ 2. explored images
SPARE = 383
ROOT_LANES = (0, 70)
TXIDS = ("50", "51")
# per contract, by the model: lanes (satisfied, without a model, unknown) under each root's lineage
# over the lanes the three rounds reached
PINNED = {"exceptions.sol.o": ((4, 1, 0), (4, 1, 0)), "overflow.sol.o": ((4, 1, 0), (4, 1, 0))}


def _explored(dev, name):
    ws, addr = symcases.deploy(dev, name)
    vm = symcosim.new_vm(dev)
    roots = [symcosim.initial(ws, addr, txid=t) for t in TXIDS]
    shape = dataclasses.replace(vm._shape(roots), n=1 + SPARE)
    b = LaneBatch(shape)
    b.status[:] = MG_HALT_STOP
    for lane, r in zip(ROOT_LANES, roots):
        vm._pack(b, lane, r)
        b.steps[lane] = 0
    b.code_id[:] = b.code_id[ROOT_LANES[0]]
    free = [l for l in range(shape.n) if l not in ROOT_LANES]
    dev.alloc(shape)
    dev.explore_alloc(16)
    dev.upload(b)
    st = dev.explore(free, max_rounds=3)
    assert st.rounds == 3 and st.starved == 0 and st.path_full == 0 and st.forks >= 6
    out = LaneBatch(shape)
    dev.download(out)
    return roots, shape, out, dev.explore_paths(0, shape.n), st


def _selector_models(code):
    """One model per dispatcher selector and transaction id with 36 bytes of calldata
    (the other id's symbols stay 0), plus empty calldata over a non-zero array, and
    all-zero."""
    sels = sorted({int(h, 16) for h in code.func_hashes})
    assert sels
    ms = [{}]
    for t in TXIDS:
        ms.append({f"{t}_calldatasize": 0, f"{t}_calldata": ArrayInterp(0xFF)})
    for s in sels:
        for t in TXIDS:
            cd = {k: (s >> (8 * (3 - k))) & 0xFF for k in range(4)}
            cd[35] = 1
            ms.append({f"{t}_calldatasize": 36, f"{t}_calldata": ArrayInterp(0, cd), f"sender_{t}": 0xAFFE})
    return ms


@pytest.mark.parametrize("name", sorted(PINNED))
def test_explored_images_equal_model_and_kernel_2(dev, name):
    roots, shape, out, paths, st = _explored(dev, name)
    path, path_len, root = paths
    ms = _selector_models(roots[0].environment.code)
    storage = roots[0].environment.active_account.storage.base_raw.param[0]
    var_names = [f"{t}_calldatasize" for t in TXIDS] + [f"sender_{t}" for t in TXIDS] + \
                [f"call_value{t}" for t in TXIDS] + [f"gas_price{t}" for t in TXIDS]
    tables = [TableSig(f"{t}_calldata", "array", (256,), 8) for t in TXIDS] + [TableSig(storage, "array", (256,), 256)]
    pool = ModelPool.from_dicts(ms, var_names, [256] * len(var_names), tables)
    bindings = [sym.path_binding(r, var_names, tables) for r in roots]
    assert bindings[0].var_cdsize != bindings[1].var_cdsize and bindings[0].tab_calldata != bindings[1].tab_calldata
    lane_binding = np.full(shape.n, UNBOUND, dtype=np.uint32)
    for k, lane in enumerate(ROOT_LANES):
        lane_binding[lane] = k
    fs, bits, ms_kernel = dev.explore_check(pool, bindings, lane_binding, bits=True)
    want_fs, want_bits = pathmodel.check(out, paths, pool, bindings, lane_binding)
    assert fs.tolist() == want_fs.tolist() and bits.tolist() == want_bits.tolist()
    # kernel 2 on the decoded and flattened path, for every lane of a lineage the model knows
    lanes = [l for l in range(shape.n) if int(root[l]) in ROOT_LANES and (l in ROOT_LANES or path_len[l])]
    known = [l for l in lanes if fs[l] != UNKNOWN]
    sets, where, dead = [], [], []
    for l in known:
        cons = sym.path_constraints(out, l, roots[ROOT_LANES.index(int(root[l]))], path[l, :int(path_len[l])])
        if cons is None:
            dead.append(l)
        else:
            sets.append(cons)
            where.append(l)
    prog, kept = flatten.compile_sets(sets)
    assert kept == list(range(len(sets)))
    k2_pool = ModelPool.from_dicts(ms, prog.var_names, prog.var_widths, prog.tables)
    _, _, k2_bits, _ = dev.eval_bits(prog, k2_pool)
    for d, l in enumerate(where):
        assert bits[l].tolist() == k2_bits[d].tolist(), (name, l)
        assert int(fs[l]) == _first_of(k2_bits[d]), (name, l)
    for l in dead:
        assert fs[l] == NO_MODEL and not bits[l].any(), (name, l)
    # not vacuous, and the two lineages read different symbols
    classes = []
    for r in ROOT_LANES:
        mine = [l for l in lanes if int(root[l]) == r]
        classes.append((sum(1 for l in mine if fs[l] < len(ms)), sum(1 for l in mine if fs[l] == NO_MODEL),
                        sum(1 for l in mine if fs[l] == UNKNOWN)))
    print(f"{name}: {len(lanes)} lanes after {st.forks} forks, (satisfied, no model, unknown) per root {classes}, "
          f"{len(dead)} dead paths, kernel {ms_kernel:.3f} ms")
    assert tuple(classes) == PINNED[name]
    assert all(c[0] >= 1 and c[1] >= 1 for c in classes)
    # lanes of the two lineages on the same path (same entries) are satisfied by different models
    by_path = {}
    for l in lanes:
        by_path.setdefault(tuple(path[l, :int(path_len[l])].tolist()), {})[int(root[l])] = l
    pairs = [(p[ROOT_LANES[0]], p[ROOT_LANES[1]]) for p in by_path.values() if len(p) == 2]
    differing = [(a, b) for a, b in pairs if fs[a] < len(ms) and fs[b] < len(ms) and bits[a, 0] != bits[b, 0]]
    assert len(pairs) >= 3 and differing
    # lanes of no lineage (free lanes never handed out keep root = themselves, unbound) are unknown
    others = [l for l in range(shape.n) if l not in lanes]
    assert others and all(fs[l] == UNKNOWN for l in others)


# ------------------------------------------------------------ 3. masking and order
def test_allowed_moves_first_sat_to_the_next_model(dev):
    im = pathcases.image(130)
    _upload_image(dev, im)
    fs, bits, _ = dev.explore_check(im.pool, im.bindings, im.lane_binding, bits=True)
    words = bits.shape[1]
    # one allowed row per lineage: give every lane its own lineage and binding
    n = pathcases.N_LANES
    known = [i for i in range(n) if fs[i] != UNKNOWN]
    dev.explore_upload_paths(im.path, im.path_len, np.arange(n, dtype=np.uint32))
    def binding_of(i):
        r = int(im.root[i])
        b = int(im.lane_binding[r]) if r < n else UNBOUND
        return im.bindings[b if b < len(im.bindings) else 0]

    bindings = [binding_of(i) for i in range(n)]
    lane_binding = np.arange(n, dtype=np.uint32)
    lane_binding[[i for i in range(n) if i not in known]] = UNBOUND
    allowed = np.full((n, words), np.uint64((1 << 64) - 1), dtype=np.uint64)
    for i in known:
        if fs[i] < 130:
            allowed[i, int(fs[i]) >> 6] &= ~np.uint64(1 << (int(fs[i]) & 63))
    got_fs, got_bits, _ = dev.explore_check(None, bindings, lane_binding, allowed=allowed, bits=True)
    moved = 0
    for i in known:
        want = bits[i] & allowed[i]
        assert got_bits[i].tolist() == want.tolist(), i
        assert int(got_fs[i]) == _first_of(want), i
        if fs[i] < 130:
            assert got_fs[i] > fs[i]
            moved += got_fs[i] != NO_MODEL
    assert moved >= 60
    none_fs, none_bits, _ = dev.explore_check(None, bindings, lane_binding, allowed=np.zeros_like(allowed), bits=True)
    assert all(none_fs[i] == NO_MODEL for i in known) and not none_bits.any()


# ------------------------------------------------------------ 4. refusals
SENTINEL = 0x5A5A5A5A


def _rc(dev, pool, bindings, lane_binding, first, n, allowed=None, null_fs=False, null_lb=False, null_bind=False,
        n_bindings=None):
    barr = (native.MgPathBinding * max(len(bindings), 1))(*bindings)
    lb = np.ascontiguousarray(lane_binding, dtype=np.uint32)
    fs = np.full(max(n, 1) + 1, SENTINEL, dtype=np.uint32)
    words = ((pool.n_models if pool is not None else 130) + 63) // 64
    sb = np.full((max(n, 1) + 1, max(words, 1)), SENTINEL, dtype=np.uint64)
    mods = pool.c_struct() if pool is not None else None
    rc = dev.lib.mg_explore_check(dev.ctx, ctypes.byref(mods) if mods is not None else None,
                                  None if null_bind else barr, len(bindings) if n_bindings is None else n_bindings,
                                  None if null_lb else lb.ctypes.data,
                                  allowed.ctypes.data if allowed is not None else None, first, n,
                                  None if null_fs else fs.ctypes.data, sb.ctypes.data, None)
    untouched = bool((fs == SENTINEL).all() and (sb == SENTINEL).all())
    return rc, dev.lib.mg_last_error(dev.ctx).decode(), untouched


def test_refusals_leave_answers_and_image(dev):
    im = pathcases.image(130)
    n = pathcases.N_LANES
    fresh = GpuDevice(0)
    try:
        rc, msg, clean = _rc(fresh, im.pool, im.bindings, im.lane_binding, 0, n)
        assert rc == MG_ESTATE and "mg_lanes_alloc" in msg and clean
    finally:
        fresh.close()
    cid = dev.load_code(b"\x00")
    plain = dataclasses.replace(pathcases.SHAPE, node_cap=0, const_cap=0)
    dev.alloc(plain)
    rc, msg, clean = _rc(dev, im.pool, im.bindings, im.lane_binding, 0, n)
    assert rc == MG_ESTATE and "mg_sym_alloc" in msg and clean
    dev.alloc(pathcases.SHAPE)
    b = im.batch.copy()
    b.code_id[:] = cid
    dev.upload(b)
    rc, msg, clean = _rc(dev, im.pool, im.bindings, im.lane_binding, 0, n)
    assert rc == MG_ESTATE and "mg_explore_alloc" in msg and clean
    _upload_image(dev, im)
    dev.explore_check(im.pool, im.bindings, im.lane_binding)          # a pool is resident from here on
    before, paths_before = _full(dev, pathcases.SHAPE), dev.explore_paths(0, n)

    def binding(**kw):
        x = native.MgPathBinding.unbound()
        for f in ("var_cdsize", "tab_calldata", "tab_storage"):
            setattr(x, f, getattr(im.bindings[1], f))
        for k in range(abi.MG_ENV_WORDS):
            x.var_env[k] = im.bindings[1].var_env[k]
        for f, v in kw.items():
            if f.startswith("env"):
                x.var_env[int(f[3:])] = v
            else:
                setattr(x, f, v)
        return x

    lb = im.lane_binding
    bad_lb, bad_lb_far = lb.copy(), lb.copy()
    bad_lb[150] = 2                                                    # == n_bindings
    bad_lb_far[3] = 0xFFFFFFFE
    empty = ModelPool(np.zeros((4, 0, 8), dtype=np.uint32))
    cases = {
        "binding index == n_bindings": dict(bindings=im.bindings, lane_binding=bad_lb),
        "binding index far out": dict(bindings=im.bindings, lane_binding=bad_lb_far),
        "variable past the batch": dict(bindings=[im.bindings[0], binding(var_cdsize=4)]),
        "environment variable past the batch": dict(bindings=[im.bindings[0], binding(env3=1000)]),
        "calldata table past the batch": dict(bindings=[binding(tab_calldata=2), im.bindings[1]]),
        "storage table past the batch": dict(bindings=[im.bindings[0], binding(tab_storage=0x7FFFFFFF)]),
        "first + n past the lanes": dict(first=100, n=n - 99),
        "first past the lanes": dict(first=n + 1, n=0),
        "first + n wraps": dict(first=0xFFFFFFFF, n=2),
        "null first_sat": dict(null_fs=True),
        "null lane_binding": dict(null_lb=True),
        "null bindings": dict(null_bind=True),
        "no models": dict(pool=empty),
    }
    for what, kw in cases.items():
        args = dict(pool=im.pool, bindings=im.bindings, lane_binding=lb, first=0, n=n)
        args.update(kw)
        rc, msg, clean = _rc(dev, **args)
        assert rc == MG_EINVAL and clean, (what, rc, msg)
        assert whole_diff(_full(dev, pathcases.SHAPE), before) == [], what
        got = dev.explore_paths(0, n)
        assert all(np.array_equal(x, y) for x, y in zip(got, paths_before)), what
    # the resident pool is still the one of before: a refused pool replaced nothing
    want_fs, _ = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding)
    fs, _, _ = dev.explore_check(None, im.bindings, im.lane_binding)
    assert fs.tolist() == want_fs.tolist()
    # n == 0 succeeds and writes nothing, even with null arrays
    rc, msg, clean = _rc(dev, None, im.bindings, lb, 5, 0, null_fs=True)
    assert rc == 0 and clean, msg
    # mg_explore_upload's own refusals
    plen = im.path_len.copy()
    plen[7] = pathcases.PATH_CAP + 1
    assert dev.lib.mg_explore_upload(dev.ctx, im.path.ctypes.data, plen.ctypes.data, im.root.ctypes.data, 0, n) == MG_EINVAL
    assert dev.lib.mg_explore_upload(dev.ctx, im.path.ctypes.data, im.path_len.ctypes.data, im.root.ctypes.data, 1, n) == MG_EINVAL
    assert dev.lib.mg_explore_upload(dev.ctx, None, im.path_len.ctypes.data, im.root.ctypes.data, 0, n) == MG_EINVAL
    got = dev.explore_paths(0, n)
    assert all(np.array_equal(x, y) for x, y in zip(got, paths_before))
    # a context with no resident pool and models == NULL: there are no models
    fresh = GpuDevice(0)
    try:
        fresh.load_code(b"\x00")
        fresh.alloc(pathcases.SHAPE)
        fresh.explore_alloc(pathcases.PATH_CAP)
        rc, msg, clean = _rc(fresh, None, im.bindings, lb, 0, n)
        assert rc == MG_EINVAL and "models" in msg and clean
    finally:
        fresh.close()


# ------------------------------------------------------------ 5. no effect elsewhere
def test_a_check_changes_nothing_of_the_image(dev):
    im = pathcases.image(65)
    _upload_image(dev, im)
    before, paths_before = _full(dev, pathcases.SHAPE), dev.explore_paths(0, pathcases.N_LANES)
    for kw in (dict(bits=True), dict(first=5, n=70), dict(bits=True, first=191, n=1)):
        dev.explore_check(im.pool, im.bindings, im.lane_binding, **kw)
    assert whole_diff(_full(dev, pathcases.SHAPE), before) == []
    after = dev.explore_paths(0, pathcases.N_LANES)
    assert all(np.array_equal(x, y) for x, y in zip(after, paths_before))
