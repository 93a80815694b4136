"""mg_explore_check_fn's contract on the CPU: tests/pathfnmodel.py (written from the
header's rules, Python integers, tables read at (k0, k1)) against the independent
route -- ``symbolic.path_constraints`` (the decoder, which builds keccak256_<bits>
and Power applications) -> ``flatten.compile_sets`` (which lowers ``uf`` through
smt/lower.py) -> kernel 2's C oracle on a ``ModelPool.from_dicts`` of the same
models -- on the hand-written arenas of tests/pathfncases.py, at 1, 64, 65 and 130
models, with `allowed` rows empty, full and masking the first model; the stated
unknown flag on the rest; what is unknown with Power, the keccak tables or
everything left unbound; and symbolic.path_functions on table lists.
"""
import numpy as np
import pytest

import pathcases
import pathfncases
import pathfnmodel
import pathmodel
from mythril_amd import abi
from mythril_amd.laser import symbolic as sym
from mythril_amd.smt.lower import TableSig
from test_path_check_cpu import first_of, independent

UNKNOWN, NO_MODEL, UNBOUND = abi.MG_PATH_UNKNOWN, abi.MG_BV_NO_MODEL, abi.MG_PATH_UNBOUND
N = pathfncases.N_LANES


@pytest.fixture(scope="module", params=pathfncases.MODEL_COUNTS)
def checked(request):
    im = pathfncases.image(request.param)
    fs, bits = pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, im.functions)
    return im, fs, bits


def test_model_equals_decode_flatten_oracle(checked):
    im, fs, bits = checked
    known = [i for i in range(N) if i not in im.unknown]
    assert [(i, im.cases[i].name if i < len(im.cases) else "filler") for i in range(N) if (fs[i] == UNKNOWN) !=
            (i in im.unknown)] == []
    assert not bits[im.unknown].any()
    want = independent(im, known)
    for j, i in enumerate(known):
        name = im.cases[i].name if i < len(im.cases) else "filler"
        assert bits[i].tolist() == want[j].tolist(), (i, name)
        assert int(fs[i]) == first_of(want[j]), (i, name)
    n_models = len(im.models)
    results = [i for i in known if i < len(im.cases) and im.cases[i].result is not None]
    sat = sum(1 for i in results if fs[i] != NO_MODEL)
    print(f"{n_models} models: {len(results)} result lanes, {sat} satisfied, {len(im.unknown)} unknown")
    if n_models >= 64:
        # not vacuous: the compared value tells the picked model from nearly every other one (an
        # equality lane is satisfied by few models, an inequality lane by all but few)
        ones = [bin(int(bits[i, 0])).count("1") for i in results]
        assert all(0 < c < 64 for c in ones) and sum(1 for c in ones if c < 8 or c > 56) >= len(results) - 4


def test_the_pool_has_every_kind_of_entry():
    """Under the models of one pool a looked-up key is present, absent with a non-zero
    default, present twice, next to an entry that differs only in k0 and next to one
    that differs only in k1; reading with k1 ignored would change an answer."""
    im = pathfncases.image(130)
    t = next(k for k, s in enumerate(pathfncases.TABLES) if s.name == "keccak256_512")
    p = im.pool
    seen = {"present": 0, "absent": 0, "twice": 0, "k0 only": 0, "k1 only": 0, "k1 matters": 0}
    for m, model in enumerate(im.models):
        key = pathfncases.keys_of(model)["keccak256_512"][0][0]
        k0, k1 = key & pathcases.M, key >> 256
        rows = [(pathmodel._word(r[:8]), pathmodel._word(r[8:16]), pathmodel._word(r[16:24]))
                for r in p.tab_entries[int(p.tab_start[t, m]):int(p.tab_start[t, m]) + int(p.tab_count[t, m])]]
        hits = [r for r in rows if r[:2] == (k0, k1)]
        seen["present" if hits else "absent"] += 1
        if not hits:
            assert pathmodel._word(p.tab_default[t, m, :8]) != 0
        seen["twice"] += len(hits) >= 2 and hits[0][2] != hits[1][2]
        seen["k0 only"] += any(r[0] != k0 and r[1] == k1 for r in rows)
        seen["k1 only"] += any(r[0] == k0 and r[1] != k1 for r in rows)
        first_k0 = next((r for r in rows if r[0] == k0), None)
        seen["k1 matters"] += first_k0 is not None and first_k0[1] != k1
    assert all(v >= 10 for v in seen.values()), seen


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
        for bi in range(len(im.bindings)):
            firsts = [int(fs[i]) for i in range(N) if fs[i] < n_models and int(im.lane_binding[im.root[i]]) == bi]
            m = max(set(firsts), key=firsts.count)
            allowed[bi, m >> 6] &= ~np.uint64(1 << (m & 63))
    got_fs, got_bits = pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, im.functions, allowed)
    moved = 0
    for i in range(N):
        if i in im.unknown:
            assert got_fs[i] == UNKNOWN and not got_bits[i].any()
            continue
        want = bits[i] & allowed[int(im.lane_binding[im.root[i]])]
        assert got_bits[i].tolist() == want.tolist(), i
        assert int(got_fs[i]) == first_of(want), i
        moved += int(got_fs[i]) != int(fs[i])
    if how == "empty":
        assert all(got_fs[i] == NO_MODEL for i in range(N) if i not in im.unknown)
    if how == "first masked":
        assert moved >= 1


def test_what_is_unbound_is_unknown():
    """Nothing bound: every function case is unknown and every other lane answers as
    tests/pathmodel.py (the contract of mg_explore_check) does.  Power or the keccak
    tables alone unbound: exactly the cases that read them."""
    im = pathfncases.image(65)
    fs, bits = pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, im.functions)
    old_fs, old_bits = pathmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding)
    keccak, power = set(im.using("keccak")), set(im.using("power"))
    assert len(keccak) >= 15 and len(power) >= 4 and len(keccak & power) >= 1
    for fn, gone in ((None, keccak | power), (pathfncases.functions(power=False), power),
                     (pathfncases.functions(keccak=False), keccak), (sym.path_functions([]), keccak | power)):
        got_fs, got_bits = pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, fn)
        for i in range(N):
            if i in gone:
                assert got_fs[i] == UNKNOWN and not got_bits[i].any(), i
            else:
                assert got_fs[i] == fs[i] and got_bits[i].tolist() == bits[i].tolist(), i
        if fn is None:
            assert got_fs.tolist() == old_fs.tolist() and got_bits.tolist() == old_bits.tolist()
    for i in range(N):
        row = im.path[i, :int(im.path_len[i])]
        assert pathfnmodel.lane_unknown(im.batch, i, row, int(im.root[i]), im.bindings, im.lane_binding,
                                        im.functions) == (i in im.unknown), i


def test_ranges():
    im = pathfncases.image(65)
    fs, bits = pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, im.functions)
    part_fs, part_bits = pathfnmodel.check(im.batch, im.paths, im.pool, im.bindings, im.lane_binding, im.functions,
                                           first=5, n=62)
    assert part_fs.tolist() == fs[5:67].tolist() and part_bits.tolist() == bits[5:67].tolist()


def _sig(name, domain, rng=256, kind="uf"):
    return TableSig(name, kind, domain, rng)


def test_path_functions():
    K = abi.MG_PATH_KECCAK_WIDTHS
    f = sym.path_functions(pathfncases.TABLES)
    at = {t.name: i for i, t in enumerate(pathfncases.TABLES)}
    assert f.tab_power == at["Power"] and f.n_keccak == len(pathfncases.BOUND)
    assert list(f.keccak_bits[:f.n_keccak]) == sorted(pathfncases.BOUND)
    assert [f.keccak_tab[j] for j in range(f.n_keccak)] == [at[f"keccak256_{w}"] for w in sorted(pathfncases.BOUND)]
    # out of order, a width above 512, the inverse functions, an array of the same name: ascending, the rest ignored
    tables = [_sig("keccak256_512", (512,)), _sig("keccak256_520", (520,)), _sig("keccak256_8", (8,)),
              _sig("keccak256_512-1", (256,), 512), _sig("7_calldata", (256,), 8, "array"), _sig("Power", (256, 256)),
              _sig("keccak256_256", (256,)), _sig("keccak256_1024", (1024,)), _sig("keccak256_264", (256,))]
    f = sym.path_functions(tables)
    assert f.tab_power == 5 and f.n_keccak == 3
    assert list(f.keccak_bits[:3]) == [8, 256, 512] and list(f.keccak_tab[:3]) == [2, 6, 0]
    assert all(f.keccak_tab[j] == UNBOUND for j in range(3, K))
    # more widths than the call binds: the first K in ascending width
    widths = [512, 8, 16, 504, 24, 32, 40, 48, 56, 64, 72]
    f = sym.path_functions([_sig(f"keccak256_{w}", (w,)) for w in widths])
    assert f.tab_power == UNBOUND and f.n_keccak == K
    assert list(f.keccak_bits) == sorted(widths)[:K]
    assert list(f.keccak_tab) == [widths.index(w) for w in sorted(widths)[:K]]
    # nothing to bind
    f = sym.path_functions([])
    assert f.tab_power == UNBOUND and f.n_keccak == 0 and all(t == UNBOUND for t in f.keccak_tab)
    assert sym.path_functions(None).n_keccak == 0
