"""mg_explore_check_fn on an MI355X (path_eval.cuh): KECCAK and Power cones evaluated
from the models' function tables, where the arena is.

a. the hand-written arenas of tests/pathfncases.py (checked on the CPU against the
   decoder + flattener + kernel-2 oracle route by test_path_fn_cpu.py) uploaded into
   80 lanes: first_sat and sat_bits equal tests/pathfnmodel.py word for word at 1,
   64, 65 and 130 models, over lane ranges that start and end inside a wave, with the
   resident pool, and under the three kinds of `allowed` rows;
b. the same image through mg_explore_check and through the new call with nothing
   bound: every function case is MG_PATH_UNKNOWN, every other lane is unchanged;
c. an image mg_explore made from a hand-assembled program (a mapping read through
   SHA3 of CALLER and a slot, then EXP) on two roots with different transaction ids:
   no successor is unknown once the tables are bound, the device equals the model
   and kernel 2 on the decoded and flattened paths;
d. refusals leave the answers and the image untouched;
e. a check changes nothing of the image.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import pathfncases
import pathfnmodel
import pathmodel
import symcosim
from mythril_amd import abi, native
from mythril_amd.device import GpuDevice
from mythril_amd.lanes import MG_EINVAL, MG_HALT_STOP, LaneBatch
from mythril_amd.laser import symbolic as sym
from mythril_amd.smt import flatten
from mythril_amd.smt.lower import TableSig
from mythril_amd.smt.program import ArrayInterp, FuncInterp, ModelPool
from test_gpu_fork import _full
from xfermodel import whole_diff

pytestmark = pytest.mark.gpu

UNKNOWN, NO_MODEL, UNBOUND = abi.MG_PATH_UNKNOWN, abi.MG_BV_NO_MODEL, abi.MG_PATH_UNBOUND
N = pathfncases.N_LANES


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def _upload_image(dev, im):
    cid = dev.load_code(b"\x00")
    b = im.batch.copy()
    b.code_id[:] = cid
    dev.alloc(pathfncases.SHAPE)
    dev.explore_alloc(pathfncases.PATH_CAP)
    dev.upload(b)
    dev.explore_upload_paths(im.path, im.path_len, im.root)
    return b


def _first_of(row) -> int:
    for w, x in enumerate(row):
        x = int(x)
        if x:
            return 64 * w + (x & -x).bit_length() - 1
    return NO_MODEL


def _differences(im, got, want):
    (fs, bits), (want_fs, want_bits) = got, want
    return [(i, im.cases[i].name if i < len(im.cases) else "filler", int(fs[i]), int(want_fs[i]))
            for i in range(len(fs)) if fs[i] != want_fs[i] or bits[i].tolist() != want_bits[i].tolist()]


# ------------------------------------------------------------ a. hand-written arenas
@pytest.mark.parametrize("count", pathfncases.MODEL_COUNTS)
def test_hand_written_arenas_equal_the_model(dev, count):
    im = pathfncases.image(count)
    _upload_image(dev, im)
    args = (im.batch, im.paths, im.pool, im.bindings, im.lane_binding)
    want_fs, want_bits = pathfnmodel.check(*args, im.functions)
    fs, bits, ms = dev.explore_check(im.pool, im.bindings, im.lane_binding, bits=True, functions=im.functions)
    assert _differences(im, (fs, bits), (want_fs, want_bits)) == []
    assert [i for i in range(N) if fs[i] == UNKNOWN] == im.unknown
    # ranges that start and end inside a wave of lanes; the resident pool
    for first, n in ((5, 62), (64, 16), (1, 78), (79, 1), (63, 2)):
        part_fs, part_bits, _ = dev.explore_check(None, im.bindings, im.lane_binding, first=first, n=n, bits=True,
                                                  functions=im.functions)
        assert part_fs.tolist() == want_fs[first:first + n].tolist(), (first, n)
        assert part_bits.tolist() == want_bits[first:first + n].tolist(), (first, n)
    only_fs, none, _ = dev.explore_check(None, im.bindings, im.lane_binding, functions=im.functions)
    assert none is None and only_fs.tolist() == want_fs.tolist()
    # Power or the keccak tables alone unbound: the model's answer, the cases that read them unknown
    for fn, gone in ((pathfncases.functions(power=False), im.using("power")),
                     (pathfncases.functions(keccak=False), im.using("keccak"))):
        got_fs, got_bits, _ = dev.explore_check(None, im.bindings, im.lane_binding, bits=True, functions=fn)
        assert _differences(im, (got_fs, got_bits), pathfnmodel.check(*args, fn)) == []
        assert gone and all(got_fs[i] == UNKNOWN for i in gone)
    # the three kinds of allowed rows
    words = bits.shape[1]
    full = np.zeros((len(im.bindings), words), dtype=np.uint64)
    for m in range(count):
        full[:, m >> 6] |= np.uint64(1 << (m & 63))
    masked = full.copy()
    for bi in range(len(im.bindings)):
        firsts = [int(fs[i]) for i in range(N) if fs[i] < count and int(im.lane_binding[im.root[i]]) == bi]
        m = max(set(firsts), key=firsts.count)
        masked[bi, m >> 6] &= ~np.uint64(1 << (m & 63))
    for allowed in (np.zeros_like(full), full, masked):
        got_fs, got_bits, _ = dev.explore_check(None, im.bindings, im.lane_binding, allowed=allowed, bits=True,
                                                functions=im.functions)
        assert _differences(im, (got_fs, got_bits), pathfnmodel.check(*args, im.functions, allowed)) == []
    print(f"{count} models: {int((fs < count).sum())} satisfied, {int((fs == NO_MODEL).sum())} without a model, "
          f"{len(im.unknown)} unknown, kernel {ms:.3f} ms")


# ------------------------------------------------------------ b. nothing bound
def test_nothing_bound_is_the_old_call(dev):
    im = pathfncases.image(65)
    _upload_image(dev, im)
    fs, bits, _ = dev.explore_check(im.pool, im.bindings, im.lane_binding, bits=True, functions=im.functions)
    old_fs, old_bits, _ = dev.explore_check(None, im.bindings, im.lane_binding, bits=True)
    want = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding)
    assert _differences(im, (old_fs, old_bits), want) == []
    function_cases = set(im.using("keccak")) | set(im.using("power"))
    assert len(function_cases) >= 20
    # through the new entry point: a NULL struct, and a struct with nothing bound
    barr = (native.MgPathBinding * len(im.bindings))(*im.bindings)
    null_fs, null_bits = np.zeros(N, dtype=np.uint32), np.zeros((N, bits.shape[1]), dtype=np.uint64)
    rc = dev.lib.mg_explore_check_fn(dev.ctx, None, barr, len(im.bindings), im.lane_binding.ctypes.data, None, None,
                                     0, N, null_fs.ctypes.data, null_bits.ctypes.data, None)
    assert rc == 0, dev.lib.mg_last_error(dev.ctx)
    none_fs, none_bits, _ = dev.explore_check(None, im.bindings, im.lane_binding, bits=True,
                                              functions=native.MgPathFunctions.unbound())
    for got_fs, got_bits in ((old_fs, old_bits), (null_fs, null_bits), (none_fs, none_bits)):
        for i in range(N):
            if i in function_cases:
                assert got_fs[i] == UNKNOWN and not got_bits[i].any(), i
            else:
                assert got_fs[i] == fs[i] and got_bits[i].tolist() == bits[i].tolist(), i


# ------------------------------------------------------------ c. an explored image
# balances[msg.sender] at slot 3 compared with calldata[4:36], then EXP(CALLVALUE, calldata[36:68]) & 1:
#   CALLER PUSH1 0 MSTORE  PUSH1 3 PUSH1 0x20 MSTORE  PUSH1 0x40 PUSH1 0 SHA3 SLOAD
#   PUSH1 4 CALLDATALOAD EQ PUSH1 0x16 JUMPI  JUMPDEST
#   PUSH1 0x24 CALLDATALOAD CALLVALUE EXP PUSH1 1 AND PUSH1 0x23 JUMPI STOP JUMPDEST STOP
PROGRAM = bytes.fromhex("33600052" "6003602052" "6040600020" "54" "600435" "14" "601657" "5b"
                        "602435" "34" "0a" "600116" "602357" "00" "5b" "00")
SPARE = 63
ROOT_LANES = (0, 9)
TXIDS = ("50", "51")
SENDERS = {"50": 0xAFFE, "51": 0xBEEF}
SLOT_HASH = 0x5EED << 200 | 0x40


def _mapping_models(storage):
    """Per transaction id, the four models (balance == calldata word, Power odd) in every
    combination, plus the all-zero model."""
    ms = [{}]
    for t in TXIDS:
        for equal in (True, False):
            for odd in (True, False):
                s, balance, value, e = SENDERS[t], 0x1122 << 64 | 5, 7, 0x33
                word = balance if equal else balance + 1
                cd = {4 + k: (word >> (8 * (31 - k))) & 0xFF for k in range(32)}
                cd[67] = e
                ms.append({f"{t}_calldatasize": 68, f"{t}_calldata": ArrayInterp(0, cd), f"sender_{t}": s,
                           f"call_value{t}": value, storage: ArrayInterp(0, {SLOT_HASH: balance}),
                           "keccak256_512": FuncInterp(0x99, {(s << 256 | 4,): 1, (s + 1 << 256 | 3,): 2,
                                                              (s << 256 | 3,): SLOT_HASH}),
                           "Power": FuncInterp(4, {(e, value): 8 | odd ^ 1, (value, e): 8 | odd})})
    return ms


def test_explored_mapping_and_exp_paths(dev):
    ws, addr = symcosim.deploy_code(PROGRAM)
    vm = symcosim.new_vm(dev)
    roots = [symcosim.initial(ws, addr, txid=t) for t in TXIDS]
    shape = dataclasses.replace(vm._shape(roots), n=1 + SPARE)
    b = LaneBatch(shape)
    b.status[:] = MG_HALT_STOP
    for lane, r in zip(ROOT_LANES, roots):
        vm._pack(b, lane, r)
        b.steps[lane] = 0
    b.code_id[:] = b.code_id[ROOT_LANES[0]]
    symenv = 1 << (abi.MG_LANE_SYMENV_SHIFT + abi.MG_ENV_CALLER)
    assert all(int(b.flags[l]) & f for l in ROOT_LANES for f in (symenv, abi.MG_LANE_SYMCD, abi.MG_LANE_SYMSTORE))
    dev.alloc(shape)
    dev.explore_alloc(8)
    dev.upload(b)
    st = dev.explore([l for l in range(shape.n) if l not in ROOT_LANES], max_rounds=3)
    assert st.forks == 6 and st.starved == 0 and st.path_full == 0 and st.rounds >= 2
    out = LaneBatch(shape)
    dev.download(out)
    paths = path, path_len, root = dev.explore_paths(0, shape.n)
    storage = roots[0].environment.active_account.storage.base_raw.param[0]
    ms = _mapping_models(storage)
    var_names = [f"{t}_calldatasize" for t in TXIDS] + [f"sender_{t}" for t in TXIDS] + \
                [f"call_value{t}" for t in TXIDS] + [f"gas_price{t}" for t in TXIDS]
    tables = [TableSig(f"{t}_calldata", "array", (256,), 8) for t in TXIDS] + \
             [TableSig(storage, "array", (256,), 256), TableSig("keccak256_512", "uf", (512,), 256),
              TableSig("Power", "uf", (256, 256), 256)]
    pool = ModelPool.from_dicts(ms, var_names, [256] * len(var_names), tables)
    bindings = [sym.path_binding(r, var_names, tables) for r in roots]
    fn = sym.path_functions(tables)
    assert fn.tab_power == 4 and fn.n_keccak == 1 and (fn.keccak_bits[0], fn.keccak_tab[0]) == (512, 3)
    lane_binding = np.full(shape.n, UNBOUND, dtype=np.uint32)
    for k, lane in enumerate(ROOT_LANES):
        lane_binding[lane] = k
    successors = [l for l in range(shape.n) if int(root[l]) in ROOT_LANES and path_len[l]]
    assert len(successors) == 8 and sorted(int(path_len[l]) for l in successors) == [2] * 8
    # the contract: every cone of this image is evaluable once the tables are bound
    want_fs, want_bits = pathfnmodel.check(out, paths, pool, bindings, lane_binding, fn)
    bare_fs, _ = pathfnmodel.check(out, paths, pool, bindings, lane_binding, None)
    assert [l for l in successors if want_fs[l] == UNKNOWN] == []
    assert [l for l in successors if bare_fs[l] == UNKNOWN] == successors
    fs, bits, ms_kernel = dev.explore_check(pool, bindings, lane_binding, bits=True, functions=fn)
    assert fs.tolist() == want_fs.tolist() and bits.tolist() == want_bits.tolist()
    old_fs, _, _ = dev.explore_check(None, bindings, lane_binding)
    assert old_fs.tolist() == bare_fs.tolist()
    # kernel 2 on the decoded and flattened paths
    sets = [sym.path_constraints(out, l, roots[ROOT_LANES.index(int(root[l]))], path[l, :int(path_len[l])])
            for l in successors]
    assert all(c is not None for c in sets)
    prog, kept = flatten.compile_sets(sets)
    assert kept == list(range(len(sets)))
    assert {"keccak256_512", "Power"} <= {t.name for t in prog.tables}
    k2_pool = ModelPool.from_dicts(ms, prog.var_names, prog.var_widths, prog.tables)
    _, _, k2_bits, _ = dev.eval_bits(prog, k2_pool)
    for d, l in enumerate(successors):
        assert bits[l].tolist() == k2_bits[d].tolist(), l
        assert int(fs[l]) == _first_of(k2_bits[d]), l
    # not vacuous: among its lineage's four models each of its four paths is satisfied by exactly its own
    for k, r in enumerate(ROOT_LANES):
        mine = [(int(bits[l, 0]) >> (1 + 4 * k)) & 0xF for l in successors if int(root[l]) == r]
        assert sorted(mine) == [1, 2, 4, 8], (r, mine)
    print(f"{len(successors)} successors after {st.forks} forks in {st.rounds} rounds, kernel {ms_kernel:.3f} ms")


# ------------------------------------------------------------ d. refusals
SENTINEL = 0x5A5A5A5A


def _rc(dev, im, fn):
    barr = (native.MgPathBinding * len(im.bindings))(*im.bindings)
    fs = np.full(N + 1, SENTINEL, dtype=np.uint32)
    sb = np.full((N + 1, (im.pool.n_models + 63) // 64), SENTINEL, dtype=np.uint64)
    mods = im.pool.c_struct()
    rc = dev.lib.mg_explore_check_fn(dev.ctx, ctypes.byref(mods), barr, len(im.bindings), im.lane_binding.ctypes.data,
                                     None, ctypes.byref(fn), 0, N, fs.ctypes.data, sb.ctypes.data, None)
    return rc, dev.lib.mg_last_error(dev.ctx).decode(), bool((fs == SENTINEL).all() and (sb == SENTINEL).all())


def test_refusals_leave_answers_and_image(dev):
    im = pathfncases.image(65)
    _upload_image(dev, im)
    want_fs, _ = pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, im.functions)
    fs, _, _ = dev.explore_check(im.pool, im.bindings, im.lane_binding, functions=im.functions)
    assert fs.tolist() == want_fs.tolist()
    before, paths_before = _full(dev, pathfncases.SHAPE), dev.explore_paths(0, N)
    n_tables = len(pathfncases.TABLES)

    def changed(**kw):
        f = pathfncases.functions()
        for name, v in kw.items():
            if name[:4] in ("bits", "tab_") and name[4:].isdigit():
                (f.keccak_bits if name[0] == "b" else f.keccak_tab)[int(name[4:])] = v
            else:
                setattr(f, name, v)
        return f

    cases = {
        "n_keccak above the cap": changed(n_keccak=abi.MG_PATH_KECCAK_WIDTHS + 1),
        "n_keccak far out": changed(n_keccak=0xFFFFFFFF),
        "a width of 0": changed(bits1=0),
        "a width above 512": changed(bits4=513),
        "a repeated width": changed(bits3=256),
        "keccak table == the pool's count": changed(tab_0=n_tables),
        "keccak table far out": changed(tab_4=0xFFFFFFFE),
        "power table == the pool's count": changed(tab_power=n_tables),
    }
    for what, fn in cases.items():
        rc, msg, clean = _rc(dev, im, fn)
        assert rc == MG_EINVAL and clean, (what, rc, msg)
        assert whole_diff(_full(dev, pathfncases.SHAPE), before) == [], what
        got = dev.explore_paths(0, N)
        assert all(np.array_equal(x, y) for x, y in zip(got, paths_before)), what
    # unbound entries and entries past n_keccak are no errors
    ok = changed(tab_2=UNBOUND, n_keccak=3, bits4=0, tab_4=0xFFFFFFFE)
    rc, msg, clean = _rc(dev, im, ok)
    assert rc == 0 and not clean, msg
    got_fs, _, _ = dev.explore_check(None, im.bindings, im.lane_binding, functions=ok)
    assert got_fs.tolist() == pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, ok)[0].tolist()
    # the resident pool is still the one of before
    fs, _, _ = dev.explore_check(None, im.bindings, im.lane_binding, functions=im.functions)
    assert fs.tolist() == want_fs.tolist()


# ------------------------------------------------------------ e. no effect elsewhere
def test_a_check_changes_nothing_of_the_image(dev):
    im = pathfncases.image(65)
    _upload_image(dev, im)
    before, paths_before = _full(dev, pathfncases.SHAPE), dev.explore_paths(0, N)
    for kw in (dict(bits=True), dict(first=5, n=70), dict(bits=True, first=79, n=1)):
        dev.explore_check(im.pool, im.bindings, im.lane_binding, functions=im.functions, **kw)
    assert whole_diff(_full(dev, pathfncases.SHAPE), before) == []
    after = dev.explore_paths(0, N)
    assert all(np.array_equal(x, y) for x, y in zip(after, paths_before))
