"""mg_explore_check's contract on the CPU: tests/pathmodel.py (written from the
contract's rules, Python integers) against the independent route the fork filter
takes today -- ``symbolic.path_constraints`` (the decoder) -> ``flatten.compile_sets``
-> kernel 2's C oracle on a ``ModelPool.from_dicts`` of the same models -- on the
hand-written arenas of tests/pathcases.py: every kind and BIN / UN opcode in both
operand positions, Bools as operands and as conditions, divisors and shift amounts
0, -1, 255, 256, 2^255, every BYTE index, EXTRACT / CONCAT at 8, 248 and 256 bits,
calldata words around every size's edge (sizes 0, 4, 36, 2^255: the bound check is
signed), sparse arrays with non-zero defaults, the SLOAD walks, every cause of
MG_PATH_UNKNOWN inside the cone and outside it, out-of-range references; at 1, 64,
65 and 130 models; with `allowed` rows empty, full and masking the first model.
"""
import numpy as np
import pytest

import pathcases
import pathmodel
from mythril_amd import abi
from mythril_amd.laser import symbolic as sym
from mythril_amd.smt import flatten
from mythril_amd.smt.program import ModelPool
from oracle import bv_ref

UNKNOWN, NO_MODEL = abi.MG_PATH_UNKNOWN, abi.MG_BV_NO_MODEL


def independent(im, lanes):
    """sat_bits [len(lanes), words] by decode -> flatten -> the kernel-2 oracle;
    path_constraints' None is unsatisfied by every model."""
    n_models = len(im.models)
    words = (n_models + 63) // 64
    states = {False: pathcases.state(False), True: pathcases.state(True)}
    sets, where = [], []
    out = np.zeros((len(lanes), words), dtype=np.uint64)
    for j, i in enumerate(lanes):
        symstore = bool(int(im.batch.flags[i]) & abi.MG_LANE_SYMSTORE)
        cons = sym.path_constraints(im.batch, i, states[symstore], im.path[i, :int(im.path_len[i])])
        if cons is not None:
            sets.append(cons)
            where.append(j)
    prog, kept = flatten.compile_sets(sets, flatten.PyCompiler())
    assert kept == list(range(len(sets))), "a hand-written path the flattener does not support"
    mp = ModelPool.from_dicts(im.models, prog.var_names, prog.var_widths, prog.tables)
    bits = np.zeros((prog.n_dags, words), dtype=np.uint64)
    bv_ref.eval_batch(prog, mp, bits=bits)
    tail = n_models & 63
    if tail:
        bits[:, -1] &= np.uint64((1 << tail) - 1)
    for d, j in enumerate(where):
        out[j] = bits[d]
    return out


def first_of(row) -> int:
    for w, x in enumerate(row):
        x = int(x)
        if x:
            return 64 * w + (x & -x).bit_length() - 1
    return NO_MODEL


@pytest.fixture(scope="module", params=pathcases.MODEL_COUNTS)
def checked(request):
    im = pathcases.image(request.param)
    fs, bits = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding)
    return im, fs, bits


def test_model_equals_decode_flatten_oracle(checked):
    im, fs, bits = checked
    n = pathcases.N_LANES
    known = [i for i in range(n) if i not in im.unknown]
    assert [i for i in range(n) if fs[i] == UNKNOWN] == im.unknown
    assert not bits[im.unknown].any()
    want = independent(im, known)
    for j, i in enumerate(known):
        name = im.cases[i].name if i < len(im.cases) else "filler"
        assert bits[i].tolist() == want[j].tolist(), (i, name)
        assert int(fs[i]) == first_of(want[j]), (i, name)
    n_models = len(im.models)
    sat = sum(1 for i in known if fs[i] != NO_MODEL)
    print(f"{n_models} models: {len(known)} known lanes, {sat} satisfied, {len(known) - sat} without a model, "
          f"{len(im.unknown)} unknown")
    if n_models >= 64:
        # not vacuous: most result lanes are satisfied by the picked model and by few others
        assert sat >= 60 and len(known) - sat >= 3
        full = np.uint64((1 << 64) - 1)
        picky = [i for i in known if i < len(im.cases) and 0 < bin(int(bits[i, 0])).count("1") < 8]
        assert len(picky) >= 30 and all(bits[i, 0] == full for i in range(len(im.cases), n - 1))


def test_size_at_or_above_2_255_reads_no_calldata():
    """The bound check of a calldata byte is signed (expr.py: BitVec.__lt__ is bvslt):
    under a model whose size is 2^255 or all-ones (negative) the word at offset 0 is 0
    whatever the array holds; an unsigned check would read the array."""
    im = pathcases.image(130)
    i = next(k for k, c in enumerate(im.cases) if c.name == "selector")
    P = pathmodel._Pool(im.pool)
    lane = pathmodel._Lane(im.batch, i)
    bind = im.bindings[0]
    node = 0                                   # the arena's CDLOAD(const 0)
    assert lane.rows[node][0] & 0xFF == abi.MG_SYM_CDLOAD and lane.const(lane.rows[node][1]) == 0
    nodes = pathmodel.cone(lane, [(node + 1) << 1], bind)
    seen = 0
    for m, model in enumerate(im.models):
        size = model.get(pathcases.CDSIZE, 0)
        if size >= pathcases.TOP and model[pathcases.CD].default:
            assert pathmodel.values(lane, nodes, bind, P, m)[node] == 0, m
            seen += 1
    assert seen >= 3 and im.models[1][pathcases.CDSIZE] == pathcases.M


@pytest.mark.parametrize("how", ["empty", "full", "first masked"])
def test_allowed_rows(checked, how):
    im, fs, bits = checked
    n_models = len(im.models)
    words = (n_models + 63) // 64
    allowed = np.zeros((len(im.bindings), words), dtype=np.uint64)
    if how != "empty":
        for m in range(n_models):
            allowed[:, m >> 6] |= np.uint64(1 << (m & 63))
    if how == "first masked":
        # binding 0 loses the model most of its lanes find first, binding 1 its own
        for bi in range(len(im.bindings)):
            firsts = [int(fs[i]) for i in range(pathcases.N_LANES)
                      if fs[i] < n_models and int(im.lane_binding[im.root[i]]) == bi]
            m = max(set(firsts), key=firsts.count)
            allowed[bi, m >> 6] &= ~np.uint64(1 << (m & 63))
    got_fs, got_bits = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, allowed)
    moved = 0
    for i in range(pathcases.N_LANES):
        if i in im.unknown:
            assert got_fs[i] == UNKNOWN and not got_bits[i].any()
            continue
        want = bits[i] & allowed[int(im.lane_binding[im.root[i]])]
        assert got_bits[i].tolist() == want.tolist(), i
        assert int(got_fs[i]) == first_of(want), i
        moved += int(got_fs[i]) != int(fs[i])
    if how == "empty":
        assert all(got_fs[i] == NO_MODEL for i in range(pathcases.N_LANES) if i not in im.unknown)
    if how == "first masked":
        assert moved >= 1


def test_ranges_and_unknown_without_models():
    im = pathcases.image(65)
    fs, bits = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding)
    part_fs, part_bits = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, first=37, n=100)
    assert part_fs.tolist() == fs[37:137].tolist() and part_bits.tolist() == bits[37:137].tolist()
    for i in range(pathcases.N_LANES):
        row = im.path[i, :int(im.path_len[i])]
        assert pathmodel.lane_unknown(im.batch, i, row, int(im.root[i]), im.bindings, im.lane_binding) == \
            (i in im.unknown), i


def test_counts_past_their_planes():
    """n_nodes above the node plane makes the lane unknown; n_consts above the constant
    plane is clipped to it (a reference inside the plane is still a reference)."""
    from mythril_amd.lanes import LaneBatch
    im = pathcases.image(1)
    b = LaneBatch(pathcases.SHAPE)
    paths = (np.zeros((pathcases.N_LANES, pathcases.PATH_CAP), dtype=np.uint32),
             np.zeros(pathcases.N_LANES, dtype=np.uint32), np.arange(pathcases.N_LANES, dtype=np.uint32))
    for i in (0, 1):
        a = pathcases.Arena()
        v = a.value()
        pathcases.Image._write(b, i, a, a.nodes + [(abi.MG_SYM_BIN | 256 << 8, v, a.c(1), 0x01)])
        paths[0][i, 0], paths[1][i] = (1 + 1) << 1 | 1, 1       # value + 1 != 0
    b.n_nodes[0] = pathcases.NODE_CAP + 1
    b.n_consts[1] = pathcases.CONST_CAP + 7
    fs, bits = pathmodel.check(b, paths, im.pool, im.bindings, np.zeros(pathcases.N_LANES, dtype=np.uint32), n=2)
    assert fs.tolist() == [UNKNOWN, 0] and bits[:, 0].tolist() == [0, 1]


def test_path_binding_names_the_states_own_symbols():
    b0, b1 = pathcases.bindings()
    U = abi.MG_PATH_UNBOUND
    assert (b0.var_cdsize, b0.tab_calldata, b0.tab_storage) == (0, 0, U)
    assert list(b0.var_env) == [U, 1, 1, 2, 3]              # a concrete address; caller and origin share sender_7
    assert (b1.var_cdsize, b1.tab_calldata, b1.tab_storage) == (0, 0, 1) and list(b1.var_env) == list(b0.var_env)
    # a pool without the symbol leaves the word unbound
    b = sym.path_binding(pathcases.state(True), [pathcases.VALUE], [])
    assert (b.var_cdsize, b.tab_calldata, b.tab_storage) == (U, U, U) and list(b.var_env) == [U, U, U, 0, U]
