"""mythril_amd/smt/exact.py + libmythsmt.so: the exact decision procedure
behind kernel 2.

* sat / unsat against brute force: random DAGs over the whole operator set at
  narrow widths (every assignment of the variables, the array's points and the
  function's table enumerated), each SAT model checked by the product's own
  evaluator (ModelRef.eval, SURVEY Appendix B semantics);
* 256-bit cases with known answers (modular inverse, no-overflow predicates,
  division by zero, shifts past the width), arrays by store chains and
  Ackermann reads, uninterpreted-function congruence;
* the reference's keccak sat/unsat verdicts (tests/laser/keccak_tests.py:7-145,
  tests/golden/keccak_cases.json) through KeccakFunctionManager's axioms;
* lexicographic minimisation and the budget's "unknown"."""
import itertools
import json
import random
from pathlib import Path

import pytest

import exact_rand
from mythril_amd.smt import exact
from mythril_amd.smt import expr as E
from mythril_amd.smt.expr import (UGT, ULT, And, Array, Concat, Function, Not, Or, BVAddNoOverflow,
                                  BVMulNoOverflow, BVSubNoUnderflow, symbol_factory as sf)
from mythril_amd.smt.program import ArrayInterp, FuncInterp

HERE = Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def solver():
    exact.build()
    return exact.ExactSolver(max_ms=20000)


W = 4
GEN = exact_rand.Gen(W)           # the generator and brute force, shared with test_exact_words_cpu.py
holds = exact_rand.holds
rand_bv, rand_bool, enumerate_models = GEN.rand_bv, GEN.rand_bool, GEN.enumerate_models


@pytest.mark.parametrize("seed", range(8))
def test_random_narrow_queries_match_brute_force(solver, seed):
    rng = random.Random(0xB1A57 + seed)
    x, y = E.var("x", W), E.var("y", W)
    checked = sat_seen = unsat_seen = 0
    for _ in range(120):
        conj = [rand_bool(rng, [x, y], 3) for _ in range(rng.randint(1, 3))]
        conj = [c for c in conj if c.op != "const"]
        if not conj:
            continue
        if any("mem4" in repr(c) or "f4" in repr(c) for c in conj):
            continue                 # tables: test_arrays_and_functions_match_brute_force
        st, assign = solver.check(conj)
        want = any(holds(a, conj) for a in enumerate_models(conj, ["x", "y"]))
        assert st == ("sat" if want else "unsat"), (conj, st)
        if st == "sat":
            assert holds(assign, conj), (conj, assign)
            sat_seen += 1
        else:
            unsat_seen += 1
        checked += 1
    assert checked >= 30 and sat_seen and unsat_seen


@pytest.mark.parametrize("mode", [{"MYTHSMT_REL_BUDGET": "0"}, {"MYTHSMT_REL_BUDGET": "1"},
                                  {"MYTHSMT_RELEVANT": "1"}])
def test_session_decision_modes_match_brute_force(monkeypatch, mode):
    """A session query is decided over its cone's inputs first (20 conflicts by
    default), then over every variable: the verdicts and models must not depend
    on that split -- whole-session decisions only, a 1-conflict first phase, and
    cone-only decisions for the whole budget."""
    for k, v in mode.items():
        monkeypatch.setenv(k, v)
    s = exact.ExactSolver(max_ms=20000)
    rng = random.Random(0x5E55)
    x, y = E.var("x", W), E.var("y", W)
    seen = set()
    for _ in range(150):
        conj = [c for c in (rand_bool(rng, [x, y], 3) for _ in range(rng.randint(1, 3))) if c.op != "const"]
        if not conj or any("mem4" in repr(c) or "f4" in repr(c) for c in conj):
            continue
        st, assign = s.check(conj)
        want = any(holds(a, conj) for a in enumerate_models(conj, ["x", "y"]))
        assert st == ("sat" if want else "unsat"), (mode, conj, st)
        if st == "sat":
            assert holds(assign, conj), (mode, conj, assign)
        seen.add(st)
    assert seen == {"sat", "unsat"} and s.stats["sessions"] >= 1
    s.close()


@pytest.mark.parametrize("seed", range(3))
def test_arrays_and_functions_match_brute_force(solver, seed):
    """One-bit reads of a 2-bit-domain array and function, over stores at
    symbolic keys: every variable value and every table enumerated."""
    rng = random.Random(0xA77 + seed)
    x, y = E.var("p", 2), E.var("q", 2)
    f = Function("g2", [2], 1)
    checked = 0
    for _ in range(40):
        a = Array("a2", 2, 1)
        for _ in range(rng.randint(0, 2)):
            a[rng.choice([E.BitVec(x), E.BitVec(y)])] = E.BitVec(E.const(rng.randrange(2), 1))
        ops = []
        for _ in range(rng.randint(1, 3)):
            i = rng.choice([E.BitVec(x), E.BitVec(y), E.BitVec(E.const(rng.randrange(4), 2))])
            lhs = a[i] if rng.random() < 0.6 else f(i)
            rhs = rng.choice([E.BitVec(E.const(rng.randrange(2), 1)), f(E.BitVec(x)), a[E.BitVec(y)]])
            ops.append(E._fold(rng.choice(["eq", "distinct"]), 1, (lhs.raw, rhs.raw)))
        conj = [c for c in ops if c.op != "const"]
        if not conj:
            continue
        st, assign = solver.check(conj)
        want = any(holds({"p": px, "q": qy, "a2": ArrayInterp(0, dict(enumerate(at))),
                          "g2": FuncInterp(0, {(i,): v for i, v in enumerate(ft)})}, conj)
                   for px, qy in itertools.product(range(4), repeat=2)
                   for at in itertools.product(range(2), repeat=4)
                   for ft in itertools.product(range(2), repeat=4))
        assert st == ("sat" if want else "unsat"), (conj, st)
        if st == "sat":
            assert holds(assign, conj)
        checked += 1
    assert checked >= 20


def test_word_sized_known_answers(solver):
    x, y = sf.BitVecSym("x", 256), sf.BitVecSym("y", 256)
    m256 = (1 << 256) - 1
    st, a = solver.check([(x * 3 == 7).raw])
    assert st == "sat" and (a["x"] * 3) & m256 == 7
    assert solver.check([(x + 1 == x).raw])[0] == "unsat"
    # SMT-LIB division by zero (Appendix B)
    assert solver.check([(E.BitVec(E._fold("bvudiv", 256, (x.raw, E.const(0, 256)))) == m256).raw,
                         (x == 5).raw])[0] == "sat"
    assert solver.check([(E.BitVec(E._fold("bvudiv", 256, (x.raw, y.raw))) != m256).raw, (y == 0).raw])[0] == "unsat"
    assert solver.check([(E.BitVec(E._fold("bvurem", 256, (x.raw, y.raw))) != x).raw, (y == 0).raw])[0] == "unsat"
    # overflow predicates (bitvec_helper.py:200-246)
    assert solver.check([Not(BVAddNoOverflow(x, y, False)).raw, ULT(x, 2).raw, ULT(y, 2).raw])[0] == "unsat"
    st, a = solver.check([Not(BVMulNoOverflow(x, y, False)).raw, ULT(x, 1 << 130).raw, ULT(y, 1 << 127).raw])
    assert st == "sat" and a["x"] * a["y"] > m256
    assert solver.check([Not(BVSubNoUnderflow(x, y, False)).raw, ULT(x, y).raw])[0] == "sat"
    assert solver.check([Not(BVSubNoUnderflow(x, y, False)).raw, Not(ULT(x, y)).raw])[0] == "unsat"
    # shifts past the width
    assert solver.check([(E.BitVec(E._fold("bvshl", 256, (x.raw, y.raw))) != 0).raw, UGT(y, 255).raw])[0] == "unsat"
    st, a = solver.check([(E.BitVec(E._fold("bvashr", 256, (x.raw, y.raw))) == m256).raw, UGT(y, 300).raw])
    assert st == "sat" and a["x"] >> 255 == 1


def test_storage_chain_and_congruence(solver):
    x, y = sf.BitVecSym("x", 256), sf.BitVecSym("y", 256)
    s = Array("Storage", 256, 256)
    s[sf.BitVecVal(7, 256)] = sf.BitVecVal(1, 256)
    assert solver.check([(s[x] == 1).raw, (s[y] == 2).raw, (x == y).raw])[0] == "unsat"
    st, a = solver.check([(s[x] == 2).raw, (x == 7).raw])
    assert st == "unsat"
    st, a = solver.check([(s[x] == 2).raw, (s[y] == 1).raw])
    assert st == "sat" and holds(a, [(s[x] == 2).raw, (s[y] == 1).raw])
    k = Function("keccak256_512", [512], 256)
    assert solver.check([(k(Concat(x, y)) != k(Concat(y, x))).raw, (x == y).raw])[0] == "unsat"


def _power_division_query(base=None):
    """flag_array's shape: a packed bool array read as ``(word / 256**(i % 32))
    & 0xff != 0``, with Power(256, e) a function pinned at e = 0..31 (the
    exponent manager's table, exponent_function_manager.py) and `word` a read
    of symbolic storage at `i / 32` (one slot stored)."""
    i = sf.BitVecSym("i", 256)
    pw = Function("Power", [256], 256)
    store = base if base is not None else Array("Storage", 256, 256)
    word = 0x1234 << (8 * 21)
    store[sf.BitVecVal(0x26, 256)] = sf.BitVecVal(word, 256)
    e = E.BitVec(E._fold("bvurem", 256, (i.raw, E.const(32, 256))))
    j = E.BitVec(E._fold("bvudiv", 256, (i.raw, E.const(32, 256))))
    div = E.BitVec(E._fold("bvudiv", 256, (store[j].raw, pw(e).raw)))
    conj = [(pw(sf.BitVecVal(k, 256)) == 256 ** k).raw for k in range(32)]
    conj += [((div & 0xFF) != 0).raw, ULT(i, 1 << 16).raw]
    return conj


def _fresh(conflicts=3000):
    return exact.ExactSolver(max_ms=20000, max_conflicts=conflicts, session=False)


def test_division_by_a_pinned_power_is_decided(monkeypatch):
    """A divisor read at a small-domain argument (the exponent i % 32) whose
    constant-argument reads are pinned to powers of two is blasted as a case
    split -- a shift per pinned point, the general divider only when none
    applies, and not at all when the points cover the argument's domain -- and
    its congruence with the pinned reads is added before the search.  Either one decides flag_array's division in a few conflicts; with
    neither, the same budget runs out."""
    conj = _power_division_query()
    s = _fresh()
    st, a = s.check(conj)
    assert st == "sat" and holds(a, conj)
    # the 32 pinned points cover every value of i % 32: no general divider is
    # built (a 512-bit product: ~270k variables without the split)
    assert s.stats["vars"] < 60_000
    # a session sends such a query straight to a solve of its own (its pins
    # are units there, assumptions in a session)
    s2 = exact.ExactSolver(max_ms=20000)
    st, a = s2.check(conj)
    assert st == "sat" and holds(a, conj)
    assert s2.stats.get("fresh_direct") == 1 and s2.stats["sessions"] == 0
    for env in ({"MYTHSMT_EAGER": "0"}, {"MYTHSMT_DIVCASES": "0"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            st, a = _fresh().check(conj)
            assert st == "sat" and holds(a, conj), env
    monkeypatch.setenv("MYTHSMT_EAGER", "0")
    monkeypatch.setenv("MYTHSMT_DIVCASES", "0")
    assert _fresh().check(conj)[0] == "unknown"          # (never unsat: the query is satisfiable)


def test_reference_keccak_verdicts(solver):
    """tests/laser/keccak_tests.py:7-145 (tests/golden/keccak_cases.json): the
    reference's own sat / unsat verdicts -- z3's, in the reference's suite --
    through KeccakFunctionManager's axioms, decided exactly here."""
    from k2_pins import keccak_cases
    from mythril_amd.smt.solver import _conjuncts
    seen = 0
    for case in keccak_cases():
        conj = [c for k in case.constraints for c in _conjuncts(k.raw) if c is not E.TRUE]
        st, a = solver.check(conj)
        assert st == case.expected, (case.name, st, case.expected)
        if st == "sat":
            assert holds(a, conj)
        seen += 1
    assert seen >= 10


def test_products_of_words_are_decided_alone():
    """A query multiplying two words goes straight to a solve of its own, where
    a bound on one factor folds the multiplier at level 0; a product by a
    constant stays in the session."""
    x, y = sf.BitVecSym("x", 256), sf.BitVecSym("y", 256)
    s = exact.ExactSolver(max_ms=20000)
    st, a = s.check([Not(BVMulNoOverflow(x, y, False)).raw, ULT(x, 21).raw])
    assert st == "sat" and a["x"] * a["y"] >= 1 << 256
    assert s.stats.get("fresh_direct_mul") == 1 and s.stats["sessions"] == 0
    st, a = s.check([(x * 3 == 7).raw])
    assert st == "sat" and s.stats.get("fresh_direct_mul") == 1 and s.stats["sessions"] == 1
    s.close()


def test_minimize_is_lexicographic(solver):
    x, y = sf.BitVecSym("x", 256), sf.BitVecSym("y", 256)
    st, a = solver.check([UGT(x, 100).raw, UGT(y, x).raw], minimize=[x.raw, y.raw])
    assert st == "sat" and a["x"] == 101 and a["y"] == 102


def test_budget_gives_unknown(solver):
    """A hard factoring instance under a 50 ms budget: "unknown" (the reference's
    SolverTimeOutException), never a wrong verdict."""
    x, y = sf.BitVecSym("x", 256), sf.BitVecSym("y", 256)
    p, q = (1 << 61) - 1, (1 << 89) - 1
    st, _ = solver.check([(x * y == p * q).raw, UGT(x, 1).raw, UGT(y, 1).raw, ULT(x, 1 << 100).raw,
                          ULT(y, 1 << 100).raw], max_ms=50)
    assert st in ("unknown", "sat")
