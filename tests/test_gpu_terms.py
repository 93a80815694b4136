"""Kernel 2's term values (k_bv_terms, mg_eval_terms) and lexicographic minimum
(k_bv_lexmin, mg_eval_min) on the MI355X: values against the Python evaluator,
the minimum against a Python restatement computed from the evaluator (never
from device output), refusals, and the global minimisation path end to end.
tests/test_terms_cpu.py runs the same inputs on the CPU stand-in."""
import random

import numpy as np
import pytest

from k2_terms_ref import (NO_MODEL, limbs_to_int, oracle_values, reference_min, run_min_queries, term_models, term_set)
from mythril_amd.device import GpuDevice
from mythril_amd.native import MythGpuError
from mythril_amd.smt.expr import ULT, symbol_factory
from mythril_amd.smt.flatten import compile_sets, compile_terms
from mythril_amd.smt.program import ModelPool, ProgramBatch, enc_w0, ref, REF_CONST, REF_VAR, REF_ACC
from oracle.bv_ref import eval_batch
from smt_eval import evaluate

pytestmark = pytest.mark.gpu
BVS, BVV = symbol_factory.BitVecSym, symbol_factory.BitVecVal
ONES = (1 << 256) - 1


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def ints(values):
    """uint32[..., 8] -> nested lists of Python ints."""
    v = np.ascontiguousarray(values, dtype="<u4")
    flat = [int.from_bytes(v.reshape(-1, 8)[k].tobytes(), "little") for k in range(v.size // 8)]
    return np.array(flat, dtype=object).reshape(v.shape[:-1]).tolist()


def to_limbs(rows):
    """nested lists of ints [n_dags][n_models] -> uint32[n_dags, n_models, 8]."""
    return np.array([[np.frombuffer(int(x).to_bytes(32, "little"), dtype="<u4") for x in r] for r in rows],
                    dtype=np.uint32)


# ------------------------------------------------------------------ 4: values
@pytest.fixture(scope="module")
def term_reference():
    """The term set compiled once, and every term's value under 257 models by
    the Python evaluator (smaller pools are prefixes)."""
    terms, wide = term_set()
    prog, kept = compile_terms(terms)
    assert kept == [k for k in range(len(terms)) if k != wide]
    models = term_models(257, seed=33)
    want = [[int(evaluate(terms[k].raw, m)) for m in models] for k in kept]
    return prog, models, want


@pytest.mark.parametrize("n_models", [1, 63, 64, 65, 257])
def test_term_values_equal_the_python_evaluator(dev, term_reference, n_models):
    prog, models, want = term_reference
    pool = ModelPool.from_dicts(models[:n_models], prog.var_names, prog.var_widths, prog.tables)
    vals, ms = dev.eval_terms(prog, pool)
    print(f"eval_terms {prog.n_dags} programs x {n_models} models: kernel_ms = {ms:.4f}")
    assert vals.shape == (prog.n_dags, n_models, 8) and vals.dtype == np.uint32
    got = ints(vals)
    for d in range(prog.n_dags):
        assert got[d] == want[d][:n_models], d


def test_term_values_of_sixteen_slot_programs(dev):
    """The terms of test_sixteen_slot_programs_equal_oracle -- the 24-variable
    product-sum tree, and the balance store chain read at several keys, which
    keeps more than 8 values live (over 64 KiB of dynamic LDS: k_bv_terms' own
    function attribute) -- over 300 models."""
    from mythril_amd.smt.expr import Array
    from mythril_amd.smt.program import ArrayInterp
    xs = [BVS(f"x{k}", 256) for k in range(24)]

    def tree(lo, hi):
        if hi - lo == 1:
            return xs[lo] * xs[(lo + 7) % 24]
        mid = (lo + hi) // 2
        return tree(lo, mid) + tree(mid, hi)
    bal = Array("balance", 256, 256)
    for k in range(6):
        bal[xs[k]] = bal[xs[k]] + xs[k + 6]
    terms = [tree(0, 24), bal[xs[1]] + bal[xs[2]] * bal[xs[3]], bal[xs[4]] - bal[xs[5]], xs[3]]
    prog, kept = compile_terms(terms)
    assert kept == [0, 1, 2, 3] and prog.n_slots > 8
    rng = random.Random(16)
    models = []
    for _ in range(300):
        a = {f"x{k}": rng.choice([0, 1, 2, rng.getrandbits(256), rng.getrandbits(8)]) for k in range(24)}
        a["balance"] = ArrayInterp(rng.getrandbits(64), {a["x1"]: rng.getrandbits(256)})
        models.append(a)
    pool = ModelPool.from_dicts(models, prog.var_names, prog.var_widths, prog.tables)
    vals, _ = dev.eval_terms(prog, pool)
    got = ints(vals)
    for d, t in enumerate(terms):
        assert got[d] == [int(evaluate(t.raw, m)) for m in models], d


# ------------------------------------------------------------------ 5: fusion
def _chains(n, seed):
    """Hand-built 256-bit chains ((x + y) * z ^ x) - y ...: a head op (any
    256-bit op, so fused tails form) followed by 2..7 simple binary ops over
    variables, constants and a slot."""
    from mythril_amd.smt import synth
    O = synth.OPCODE
    rng = random.Random(seed)
    var = lambda i: ref(REF_VAR, i)
    simple = ["bvadd", "bvsub", "bvmul", "bvand", "bvor", "bvxor", "bvumax", "bvumin", "bvrsub"]
    heads = simple + ["bvnot", "bvshl", "bvlshr", "bvudiv", "bvurem", "bvsdiv", "bvsmin"]
    insns, off = [], [0]
    for _ in range(n):
        prog = [[O["copy"] | (256 << 8) | (1 << 17), var(rng.randrange(3)), 0, 0]]       # slot 0
        head = rng.choice(heads)
        prog.append([O[head] | (256 << 8), var(rng.randrange(3)), 0 if head == "bvnot" else var(rng.randrange(3)), 0])
        for _ in range(rng.randrange(2, 8)):
            b = rng.choice([var(rng.randrange(3)), ref(REF_CONST, rng.randrange(2)), (1 << 30) | 0])
            prog.append([O[rng.choice(simple)] | (256 << 8), ref(REF_ACC, 0), b, 0])
        insns += prog
        off.append(len(insns))
    consts = np.zeros((2, 8), dtype=np.uint32)
    consts[0, 0] = 3
    consts[1, :] = 0xFFFFFFFF
    return ProgramBatch(np.asarray(insns, dtype=np.uint32), np.asarray(off, dtype=np.uint32), consts, 4,
                        ["x0", "x1", "x2"], [256, 256, 256])


def test_fused_term_values_equal_unfused(dev, monkeypatch):
    from test_gpu_eval import _fusable_programs
    mr = random.Random(9)
    specials = [0, 1, (1 << 255), ONES, (1 << 127), (1 << 63) - 1]
    models = [{n: mr.choice(specials) if mr.random() < 0.4 else mr.getrandbits(256) for n in ("x0", "x1", "x2")}
              for _ in range(320)]
    booleans, chains = _fusable_programs(300, 3), _chains(20, 5)
    for prog in (booleans, chains):
        pool = ModelPool.from_dicts(models, prog.var_names, prog.var_widths)
        out = {}
        for fuse in ("5", "0"):
            monkeypatch.setenv("MG_BV_FUSE", fuse)
            out[fuse] = dev.eval_terms(prog, pool)[0]
        assert np.array_equal(out["5"], out["0"])
        if prog is booleans:
            # limb 0 bit 0 = the C oracle's bitmap, every other bit 0
            bits = np.zeros((prog.n_dags, (320 + 63) // 64), dtype=np.uint64)
            eval_batch(prog, pool, bits=bits)
            want = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :320]
            assert np.array_equal(out["5"][:, :, 0], want.astype(np.uint32))
            assert not out["5"][:, :, 1:].any()
            assert 0 < int(want.sum()) < want.size
        else:
            # the C oracle interprets the unfused chains; and they are real 256-bit values
            assert np.array_equal(out["5"], oracle_values(prog, pool))
            assert len({limbs_to_int(out["5"][d, 7]) for d in range(20)}) > 10


# ------------------------------------------------------------- 6: lexicographic minimum
def _check_min(dev, prog, pool, values, cons, objs):
    """dev.eval_min against reference_min over `values` (ints from the evaluator)."""
    best, vals, count, ms = dev.eval_min(prog, pool, cons, objs)
    ref_vals = to_limbs(values)
    for q in range(len(cons)):
        b, v, n = reference_min(ref_vals, cons[q], objs[q])
        assert (int(best[q]), int(count[q])) == (b, n), q
        assert [limbs_to_int(r) for r in vals[q]] == v, q
    return best, vals, count, ms


def test_lexmin_random_queries_with_ties(dev):
    x, y, z = BVS("x", 256), BVS("y", 256), BVS("z", 256)
    terms = [ULT(x, y), x != z, ULT(z, BVV(1 << 200, 256)), y != BVV(7, 256),        # 0..3: constraints
             x, y, z, x + y, x ^ z, LShR_(y), x * z, y - x, x & y]                   # 4..12: objectives
    prog, kept = compile_terms(terms)
    assert kept == list(range(len(terms)))
    rng = random.Random(6)
    few = [0, 1, 7, 1 << 32, (1 << 224) - 1, ONES]
    models = [{n: rng.choice(few) for n in "xyz"} for _ in range(700)]
    values = [[int(evaluate(t.raw, m)) for m in models] for t in terms]
    cons, objs = [], []
    for q in range(70):                                     # more than BV_TILE_DAGS queries, sharing DAGs
        cons.append([[], [rng.randrange(4)], rng.sample(range(4), 3)][q % 3])
        k = [0, 1, 2, 3, 8][q % 5]
        objs.append([rng.randrange(4, 13) for _ in range(k)])
    pool = ModelPool.from_dicts(models, prog.var_names, prog.var_widths)
    best, _, count, ms = _check_min(dev, prog, pool, values, cons, objs)
    print(f"eval_min {prog.n_dags} programs x 700 models, 70 queries: kernel_ms = {ms:.4f}")
    assert (count > 1).all() and len(set(best.tolist())) > 5


def LShR_(y):
    from mythril_amd.smt.expr import LShR
    return LShR(y, BVV(3, 256))


def _pool_of(prog, models):
    return ModelPool.from_dicts(models, prog.var_names, prog.var_widths)


def test_lexmin_limb_order_positions_ties_and_no_candidate(dev):
    ok, v, w = BVS("ok", 256), BVS("v", 256), BVS("w", 256)
    terms = [ok == BVV(1, 256), v, w]
    prog, kept = compile_terms(terms)
    assert kept == [0, 1, 2]

    def run(models, cons, objs):
        values = [[int(evaluate(t.raw, m)) for m in models] for t in terms]
        return _check_min(dev, prog, _pool_of(prog, models), values, cons, objs)

    # (b) limb order: the smallest candidate is 1; a non-candidate holds 0
    vs = [1 << 224, (1 << 224) - 1, 1 << 32, (1 << 32) - 1, 1, 0]
    models = [{"ok": int(k < 5), "v": x} for k, x in enumerate(vs)]
    best, vals, count, _ = run(models, [[0]], [[1]])
    assert (int(best[0]), int(count[0]), limbs_to_int(vals[0][0])) == (4, 5, 1)
    for drop, want in ((4, 3), (3, 2), (2, 1), (1, 0)):          # without the smaller ones, in turn
        models[drop]["ok"] = 0
        best, _, _, _ = run(models, [[0]], [[1]])
        assert int(best[0]) == want
    # (c) the unique minimum at index n - 1, then at index 0
    for n in (65, 257, 300):
        for at in (n - 1, 0):
            models = [{"ok": 1, "v": 5 + (k % 7), "w": k} for k in range(n)]
            models[at]["v"] = 2
            best, _, count, _ = run(models, [[0]], [[1]])
            assert (int(best[0]), int(count[0])) == (at, n)
    # (d) all candidates equal: index 0; a tie on obj_0 broken by obj_1, whose winner
    # sits after another model tied on obj_0
    models = [{"ok": 1, "v": 9, "w": 9} for _ in range(130)]
    best, _, _, _ = run(models, [[0]], [[1, 2]])
    assert int(best[0]) == 0
    models = [{"ok": 1, "v": 4 if k in (3, 100) else 6, "w": 8 if k == 3 else 5 if k == 100 else 0}
              for k in range(130)]
    best, vals, _, _ = run(models, [[0]], [[1, 2]])
    assert int(best[0]) == 100 and [limbs_to_int(r) for r in vals[0]] == [4, 5]
    # (e) no candidate
    models = [{"ok": 0, "v": k, "w": k} for k in range(70)]
    best, vals, count, _ = run(models, [[0], []], [[1, 2], [1]])
    assert (int(best[0]), int(count[0])) == (NO_MODEL, 0)
    assert [limbs_to_int(r) for r in vals[0]] == [ONES, ONES]
    assert (int(best[1]), int(count[1])) == (0, 70)              # no constraint listed: every model


def test_lexmin_without_objectives_is_first_sat(dev):
    """(f) an empty objective list and one constraint DAG: best_model / cand_count
    are dev.eval's first_sat / sat_count, and the C oracle's."""
    from test_smt_programs import _random_constraints
    rng = random.Random(41)
    sets = [_random_constraints(rng, rng.randrange(1, 4)) for _ in range(40)]
    prog, kept = compile_sets(sets)
    mr = random.Random(5)
    models = [{n: (mr.choice([0, 1, 1 << 255, ONES]) if mr.random() < 0.3 else mr.getrandbits(w)) & ((1 << w) - 1)
               for n, w in zip(prog.var_names, prog.var_widths)} for _ in range(300)]
    pool = _pool_of(prog, models)
    best, vals, count, _ = dev.eval_min(prog, pool, [[d] for d in range(prog.n_dags)], [[] for _ in range(prog.n_dags)])
    fs, sc, _ = dev.eval(prog, pool)
    rfs, rsc = eval_batch(prog, pool)
    assert np.array_equal(best, fs) and np.array_equal(count, sc)
    assert np.array_equal(best, rfs) and np.array_equal(count, rsc)
    assert all(v.shape == (0, 8) for v in vals) and 0 < int((sc > 0).sum())


# ------------------------------------------------------------- 7: refusals and state
def test_refusals_leave_the_context_usable(dev):
    x, y = BVS("x", 256), BVS("y", 256)
    terms = [ULT(x, y), x, y, x + y]
    prog, _ = compile_terms(terms)
    models = [{"x": k % 5, "y": (k * 7) % 11} for k in range(100)]
    pool = _pool_of(prog, models)
    values = [[int(evaluate(t.raw, m)) for m in models] for t in terms]
    for cons, objs in (([[prog.n_dags]], [[1]]), ([[0]], [[prog.n_dags]]), ([[0]], [[1] * 9])):
        with pytest.raises(MythGpuError) as e:
            dev.eval_min(prog, pool, cons, objs)
        msg = str(e.value)
        assert "rc=-1" in msg and len(msg.split("rc=-1:")[1].strip()) > 10, msg
    _check_min(dev, prog, pool, values, [[0]], [[3, 1]])
    # an ordinary evaluation on the same context, unchanged by eval_terms in between
    from test_smt_programs import _random_constraints
    rng = random.Random(8)
    sets_prog, _ = compile_sets([_random_constraints(rng, 3) for _ in range(50)])
    mr = random.Random(2)
    spool = _pool_of(sets_prog, [{n: mr.getrandbits(w) if mr.random() < 0.7 else 0
                                  for n, w in zip(sets_prog.var_names, sets_prog.var_widths)} for _ in range(200)])
    fs, sc, _ = dev.eval(sets_prog, spool)
    rfs, rsc = eval_batch(sets_prog, spool)
    assert np.array_equal(fs, rfs) and np.array_equal(sc, rsc)
    dev.eval_terms(prog, pool)
    fs2, sc2, _ = dev.eval(sets_prog, spool)
    assert np.array_equal(fs2, fs) and np.array_equal(sc2, sc)


# ------------------------------------------------------------------ 8: end to end
def test_global_minimum_equals_brute_force_on_the_mi355x(dev):
    best, local, truth, stats = run_min_queries(lambda: dev)
    assert len(truth) >= 200
    assert best == list(truth)
    nonzero = [k for k, t in enumerate(truth) if t is not None and any(t)]
    assert len(nonzero) >= 60, len(nonzero)
    assert len([k for k in nonzero if local[k] > truth[k]]) >= 10
    assert stats["min_unproved"] == 0 and stats["min_device"] > 0 and stats["min_exact"] > 0


def test_flag_array_calldata_under_global_min_on_the_mi355x(dev, monkeypatch, tmp_path):
    """analysis_tests.py:11-17 with MYTHSMT_GLOBAL_MIN=1: the issue set is
    unchanged and transaction 1's input is the calldata the reference's own
    tests pin for z3 Optimize (check_row), with the minimum chosen by mg_eval_min."""
    from fnames import use_signature_db
    from test_integration_cpu import GOLDEN, check_row
    monkeypatch.setenv("MYTHSMT_GLOBAL_MIN", "1")
    use_signature_db(monkeypatch, tmp_path)
    row = next(r for r in GOLDEN["issue_counts"] if r[0] == "flag_array.sol.o")
    _, info = check_row(row, dev, dev)
    assert info["search"]["min_device"] > 0
