"""The exact procedure (mythril_amd/smt/exact.py, libmythsmt.so) at word widths:
an ``unsat`` it answers is believed as it stands, so its circuits are put
against references that share nothing with them.

* Ill-sorted queries (tests/exactcases.py: one or more per sort rule of
  include/mythsmt.h, and mixed-width kernel-2 programs) raise ``Unsupported``
  from ms_solve and ms_session_solve, in a child process; a stand-alone driver
  (tests/native/bvsat_sorts_main.cpp) runs the same rows under
  -fsanitize=address,undefined.
* Pinned points of kernel 2's case table: ``pins and e != v`` is unsat and
  ``pins and e == v`` is sat with the pins as its model, v the value of
  k2_insn_ref, in a session, stateless and fresh.
* Brute force at widths 3, 5, 6, 7 (the shifter's ``amount >= w`` comparison
  exists only at widths that are no power of two) and over affine store-chain
  keys on a 3-bit domain; affine known answers at 8, 33, 160 and 256 bits.
* Identities between differently built circuits, refuted without pins at 31,
  33, 160, 255 and 256 bits.

No answer may be "unknown": the inputs are chosen so that the default budget
(50,000 conflicts) decides them; what it does not decide is left out in the
file (exactcases' docstring, IDENTITY_CONFLICTS below), never at run time.

Measured wall time on the development host (one core), the whole module 100 s:
  test_sort_checks_under_host_sanitizers       19.9 s (the sanitizer build of bvsat.cpp)
  test_pinned_points_have_the_reference_value  60.2 s over 210 cases; most 0.02 - 0.1 s, the division
      groups 0.8 - 2.7 s, the slowest fuse:tails in a session, 4.3 s
  test_random_queries_match_brute_force        15.8 s over 12 cases; width 7 the slowest, 2.7 s
  test_the_sample_keeps_its_size                2.5 s (it builds kernel 2's case table)
  test_ill_sorted_queries_are_rejected          1.6 s
  test_affine_store_chains_match_brute_force    0.3 s over 9 cases
  test_identities_are_valid                     0.3 s over 15 cases
  test_affine_known_answers                     0.1 s over 12 cases
"""
import itertools
import json
import os
import random
import subprocess
import sys
from pathlib import Path

import pytest

import exact_rand
import exactcases as X
from mythril_amd.smt import exact
from mythril_amd.smt import expr as E
from mythril_amd.smt.expr import Node, const, var
from smt_eval import evaluate

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
GROUPS = X.group_names()
MODES = ("session", "stateless", "fresh")


@pytest.fixture(scope="module", autouse=True)
def built():
    exact.build()


def make_solver(mode):
    return exact.ExactSolver(session=mode != "stateless")


def check(solver, mode, conj):
    st, assign = solver.check(conj, fresh=mode == "fresh")
    assert st != "unknown", conj
    return st, assign


def true_under(assign, conj):
    """The conjuncts under a model, by the test-only evaluator and by the product's."""
    return all(evaluate(c, assign) == 1 for c in conj) and exact_rand.holds(assign, conj)


# ------------------------------------------------------------------ ill-sorted
def test_the_sample_keeps_its_size():
    """The well-sortedness filter cannot silently empty the sample out."""
    for name in GROUPS:
        assert len(X.cases(name)) >= X.floor(name), name
        assert all(X.sort_error(c.e) is None for c in X.cases(name))
    # mixed-width programs of the fusion groups: the rejection table's supply
    for name, at_least in (("fuse:tails", 300), ("fuse:chains", 50), ("fuse:ext_rcat", 16)):
        assert len(X.split(name)[1]) >= at_least, name
    assert 379 in X.split("fuse:tails")[1]


def test_the_python_rules_name_every_row():
    rows = X.ill_sorted_rows()
    for rule, label, conj in rows:
        assert X.sort_error(conj) == rule, label
    for rule in X.RULES:
        labels = [label for r, label, _ in rows if r == rule]
        assert labels, rule
        if rule not in ("operand count", "Boolean operands", "extract bounds"):
            assert any("narrower" in l or " 4 bits" in l or "[4]" in l for l in labels), rule
        if rule != "operand count":
            assert any("wider" in l or "8-bit" in l or "16 bits" in l or "[8] of bits 3..0" in l for l in labels), rule


def test_ill_sorted_queries_are_rejected():
    """Every row through ms_solve and ms_session_solve, in a child process: a
    read out of bounds there is a failed test here."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(ROOT), str(HERE)] + [p for p in [env.get("PYTHONPATH")] if p])
    run = subprocess.run([sys.executable, str(HERE / "exact_reject_child.py")], cwd=str(ROOT), env=env,
                         capture_output=True, text=True, timeout=600)
    lines = run.stdout.strip().splitlines()
    done = [json.loads(l) for l in lines if l.startswith("{")]
    last = done[-1]["label"] if done else "none"
    assert run.returncode == 0, f"the child died (status {run.returncode}) after row {last!r}:\n{run.stderr[-2000:]}"
    n_rows = len(X.ill_sorted_rows()) + len(X.ill_sorted_programs())
    assert lines[-1] == f"DONE {n_rows}" and len(done) == n_rows
    assert any("fuse:tails program 379 " in r["label"] for r in done)
    for r in done:
        assert r["python"] is not None, r
        assert r["ms_solve"] == "Unsupported" and r["ms_session_solve"] == "Unsupported", r
        assert r["session_closed"] and r["before"] == "unsat" and r["decides_after"] and r["fresh_decides"], r


def test_sort_checks_under_host_sanitizers(tmp_path):
    """tests/native/bvsat_sorts_main.cpp with bvsat.cpp under AddressSanitizer and
    UBSan, as a program of its own: the expected return codes, no report."""
    exe = tmp_path / "bvsat_sorts"
    cmd = [exact.CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", str(HERE / "native" / "bvsat_sorts_main.cpp"), str(exact.SRC),
           "-o", str(exe)]
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, report
    assert ", 0 failures" in run.stdout, report


# ---------------------------------------------------------------- pinned points
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", GROUPS)
def test_pinned_points_have_the_reference_value(name, mode):
    cs = X.cases(name)
    if mode == "session":
        cs = cs[::X.SESSION_STRIDE.get(name, 1)]
    assert cs
    solver = make_solver(mode)
    for c in cs:
        pins = X.pin_nodes(c)
        st, _ = check(solver, mode, pins + [X.differs(c.e, c.v)])
        assert st == "unsat", f"{c.label}: e != {c.v:#x} is {st}"
        conj = pins + [X.equals(c.e, c.v)]
        st, assign = check(solver, mode, conj)
        assert st == "sat", f"{c.label}: e == {c.v:#x} is {st}"
        for (n, _), value in c.pins.items():
            assert assign.get(n, 0) == value, (c.label, n)
        assert evaluate(c.e, assign) == c.v, c.label
    solver.close()


# ------------------------------------------------------------------ brute force
# queries per width: the enumeration is 4^w models a query (measured: the module docstring)
BRUTE = {3: 200, 5: 150, 6: 120, 7: 60}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w", sorted(BRUTE))
def test_random_queries_match_brute_force(w, mode):
    gen = exact_rand.Gen(w)
    rng = random.Random(0xB1A57 + w)
    x, y = E.var("x", w), E.var("y", w)
    solver = make_solver(mode)
    seen = {"sat": 0, "unsat": 0}
    while sum(seen.values()) < BRUTE[w]:
        conj = [c for c in (gen.rand_bool(rng, [x, y], 3) for _ in range(rng.randint(1, 3))) if c.op != "const"]
        if not conj or gen.uses_tables(conj):
            continue
        st, assign = check(solver, mode, conj)
        want = any(all(evaluate(c, {"x": a, "y": b}) == 1 for c in conj)
                   for a, b in itertools.product(range(1 << w), repeat=2))
        assert st == ("sat" if want else "unsat"), (conj, st)
        if st == "sat":
            assert true_under(assign, conj), (conj, assign)
        seen[st] += 1
    assert seen["sat"] >= 10 and seen["unsat"] >= 5, seen
    solver.close()


# ----------------------------------------------------------- affine store chains
def _affine_key(rng, p, q):
    """(node, f(p, q)) of a 3-bit key: p, q, p + k, k + p, p - k, (p + j) + k, k."""
    ks = (0, 7, 1, 2, 5)
    k, j = rng.choice(ks), rng.choice(ks)
    N, c = Node, lambda v: const(v, 3)
    return rng.choice([
        (p, lambda a, b: a), (q, lambda a, b: b),
        (N("bvadd", 3, (p, c(k))), lambda a, b: (a + k) & 7),
        (N("bvadd", 3, (c(k), p)), lambda a, b: (k + a) & 7),
        (N("bvsub", 3, (p, c(k))), lambda a, b: (a - k) & 7),
        (N("bvadd", 3, (N("bvadd", 3, (p, c(j))), c(k))), lambda a, b: (a + j + k) & 7),
        (N("bvsub", 3, (c(k), p)), lambda a, b: (k - a) & 7),
        (N("bvadd", 3, (q, c(k))), lambda a, b: (b + k) & 7),
        (c(k), lambda a, b: k),
    ])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", range(3))
def test_affine_store_chains_match_brute_force(seed, mode):
    """One-bit reads of a 3-bit-domain array through zero to three stores at keys
    affine in p (the constants 7 and 0 among them: the offsets wrap), which the
    blaster relates without an equality circuit (Blaster::affine, relate).  Every
    p, q and every table value at the points read is enumerated, in plain
    integers."""
    rng = random.Random(0xAFF1 + seed)
    p, q = var("p", 3), var("q", 3)
    base = Node("array", 0, (), ("a3", 3, 1))
    solver = make_solver(mode)
    seen = {"sat": 0, "unsat": 0}
    for _ in range(60):
        arr, chain = base, []                       # chain: (key function, stored bit), oldest first
        for _ in range(rng.randint(0, 3)):
            (kn, kf), bit = _affine_key(rng, p, q), rng.randrange(2)
            arr = Node("store", 0, (arr, kn, const(bit, 1)), (3, 1))
            chain.append((kf, bit))
        reads, facts, conj = [], [], []             # facts: ("bit", i, bit) | ("eq" | "distinct", i, j) over reads
        for _ in range(rng.randint(1, 3)):
            (kn, kf), bit = _affine_key(rng, p, q), rng.randrange(2)
            reads.append((kf, Node("select", 1, (arr, kn))))     # not expr._select: the chain is the blaster's to walk
            i = len(reads) - 1
            if i and rng.random() < 0.3:
                op, j = rng.choice(["eq", "distinct"]), rng.randrange(i)
                facts.append((op, i, j))
                conj.append(Node(op, 1, (reads[i][1], reads[j][1])))
            else:
                facts.append(("bit", i, bit))
                conj.append(Node("eq", 1, (reads[i][1], const(bit, 1))))

        def value(kf, a, b, table):
            i = kf(a, b)
            for stored_at, bit in reversed(chain):
                if stored_at(a, b) == i:
                    return bit
            return table[i]

        def satisfiable():
            for a, b in itertools.product(range(8), repeat=2):
                points = sorted({kf(a, b) for kf, _ in reads})
                for bits in itertools.product((0, 1), repeat=len(points)):
                    table = dict(zip(points, bits))
                    vals = [value(kf, a, b, table) for kf, _ in reads]
                    if all(vals[i] == k if op == "bit" else (vals[i] == vals[k]) == (op == "eq")
                           for op, i, k in facts):
                        return True
            return False

        st, assign = check(solver, mode, conj)
        assert st == ("sat" if satisfiable() else "unsat"), (conj, st)
        if st == "sat":
            assert true_under(assign, conj), (conj, assign)
        seen[st] += 1
    assert seen["sat"] >= 10 and seen["unsat"] >= 5, seen
    solver.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w", [8, 33, 160, 256])
def test_affine_known_answers(w, mode):
    """Store-chain hits and misses decided from the keys' base + constant form,
    at domain widths whose top limb is masked (8, 33) and whole (160, 256)."""
    M = (1 << w) - 1
    N, c = Node, lambda v: const(v, w)
    p, v1, v2 = var("p", w), var("v1", 8), var("v2", 8)
    mem = N("array", 0, (), ("mem", w, 8))
    add = lambda a, b: N("bvadd", w, (a, b))
    sub = lambda a, b: N("bvsub", w, (a, b))
    store = lambda a, k, v: N("store", 0, (a, k, v), (w, 8))
    read = lambda a, k: N("select", 8, (a, k))
    eq = lambda a, b: N("eq", 1, (a, b))
    ne = lambda a, b: N("distinct", 1, (a, b))
    solver = make_solver(mode)

    def verdict(*conj):
        st, assign = check(solver, mode, list(conj))
        if st == "sat":
            assert true_under(assign, list(conj)), conj
        return st

    # p + (2^w - 1) is p - 1: a hit
    assert verdict(ne(read(store(mem, add(p, c(M)), v1), sub(p, c(1))), v1)) == "unsat"
    # p + 1 and p + 2 differ for every p: the read sees the array below, free of v1
    a = store(mem, add(p, c(1)), v1)
    assert verdict(eq(read(a, add(p, c(2))), v1)) == "sat"
    assert verdict(ne(read(a, add(p, c(2))), v1)) == "sat"
    # (p + 1) + 1 is p + 2, 1 + p is p + 1: hits
    assert verdict(ne(read(store(mem, add(add(p, c(1)), c(1)), v1), add(p, c(2))), v1)) == "unsat"
    assert verdict(ne(read(store(mem, add(c(1), p), v1), add(p, c(1))), v1)) == "unsat"
    # 5 - p is not p - 5: at p = 1 the keys are 4 and 2^w - 4, a miss
    a = store(mem, sub(c(5), p), v1)
    assert verdict(eq(p, c(1)), ne(read(a, sub(p, c(5))), v1)) == "sat"
    assert verdict(eq(p, c(1)), eq(read(a, sub(p, c(5))), v1), ne(read(mem, c(M - 3)), v1)) == "unsat"
    # ... and at p = 5 both are 0, a hit
    assert verdict(eq(p, c(5)), ne(read(a, sub(p, c(5))), v1)) == "unsat"
    # p + 1 and p + 1 + 2^w are one key (the constant folded to 1 by the expression
    # layer, or added in two steps that wrap): the later store wins
    for second in (add(p, c(1 + (1 << w))), add(add(p, c(1 << (w - 1))), c(1 + (1 << (w - 1))))):
        a = store(store(mem, add(p, c(1)), v1), second, v2)
        assert verdict(ne(read(a, add(p, c(1))), v2)) == "unsat"
        assert verdict(ne(read(a, add(p, c(1))), v1)) == "sat"
        assert verdict(ne(read(a, add(p, c(1))), v1), eq(v1, v2)) == "unsat"
    solver.close()


# --------------------------------------------------------------------- validity
def _identities(w):
    """{name: (lhs, rhs, side conditions)}: two circuits of one function of x, y."""
    N, c = Node, lambda v: const(v, w)
    x, y = var("x", w), var("y", w)
    M, MSB = (1 << w) - 1, 1 << (w - 1)
    ext = lambda hi, lo, a: N("extract", hi - lo + 1, (a,), (hi, lo))
    cat = lambda hi, lo: N("concat", hi.width + lo.width, (hi, lo))
    msb = ext(w - 1, w - 1, x)
    out = {}
    for k in (0, 1, w - 1):
        if k == 0:
            shl = lshr = ashr = x
        else:
            shl = cat(ext(w - 1 - k, 0, x), const(0, k))
            lshr = cat(const(0, k), ext(w - 1, k, x))
            ashr = cat(N("ite", k, (N("eq", 1, (msb, const(1, 1))), const((1 << k) - 1, k), const(0, k))),
                       ext(w - 1, k, x))
        out[f"bvshl by {k if k < 2 else 'w-1'}"] = (N("bvshl", w, (x, c(k))), shl, [])
        out[f"bvlshr by {k if k < 2 else 'w-1'}"] = (N("bvlshr", w, (x, c(k))), lshr, [])
        out[f"bvashr by {k if k < 2 else 'w-1'}"] = (N("bvashr", w, (x, c(k))), ashr, [])
    fill = N("ite", w, (N("eq", 1, (msb, const(1, 1))), c(M), c(0)))
    out["bvashr by y >= w"] = (N("bvashr", w, (x, y)), fill, [N("bvuge", 1, (y, c(w)))])
    out["bvshl by y >= w"] = (N("bvshl", w, (x, y)), c(0), [N("bvuge", 1, (y, c(w)))])
    out["bvlshr by y >= w"] = (N("bvlshr", w, (x, y)), c(0), [N("bvuge", 1, (y, c(w)))])
    x31 = var("x31", 31) if w > 31 else var("x7", 7)
    n = w - x31.width
    top = ext(x31.width - 1, x31.width - 1, x31)
    out["sign_extend"] = (N("sign_extend", w, (x31,), n),
                          N("ite", w, (N("eq", 1, (top, const(1, 1))), cat(const((1 << n) - 1, n), x31),
                                       cat(const(0, n), x31))), [])
    out["bvneg"] = (N("bvneg", w, (x,)), N("bvadd", w, (N("bvnot", w, (x,)), c(1))), [])
    flip = lambda a: N("bvxor", w, (a, c(MSB)))
    out["bvslt"] = (N("bvslt", 1, (x, y)), N("bvult", 1, (flip(x), flip(y))), [])
    for op, dual in (("bvule", "bvugt"), ("bvuge", "bvult"), ("bvsle", "bvsgt"), ("bvsge", "bvslt")):
        out[op] = (N(op, 1, (x, y)), N("not", 1, (N(dual, 1, (x, y)),)), [])
    zx = lambda a: N("zero_extend", w + 1, (a,), 1)
    carry = ext(w, w, N("bvadd", w + 1, (zx(x), zx(y))))
    out["bvadd_noovfl_u"] = (N("bvadd_noovfl_u", 1, (x, y)), N("eq", 1, (carry, const(0, 1))), [])
    out["bvsub_noudfl_u"] = (N("bvsub_noudfl_u", 1, (x, y)), N("bvuge", 1, (x, y)), [])
    return out


IDENTITY_WIDTHS = (31, 33, 160, 255, 256)
# (identity, width) -> conflicts of the refutation, stateless, as measured on the
# development host; an identity the default budget does not decide at a width
# has no entry there and is not run at it
IDENTITY_CONFLICTS = {
    ('bvshl by 0', 31): 0, ('bvlshr by 0', 31): 0, ('bvashr by 0', 31): 0, ('bvshl by 1', 31): 0,
    ('bvlshr by 1', 31): 0, ('bvashr by 1', 31): 0, ('bvshl by w-1', 31): 0, ('bvlshr by w-1', 31): 0,
    ('bvashr by w-1', 31): 0, ('bvashr by y >= w', 31): 11, ('bvshl by y >= w', 31): 17,
    ('bvlshr by y >= w', 31): 9, ('sign_extend', 31): 0, ('bvneg', 31): 0, ('bvslt', 31): 0, ('bvule', 31): 0,
    ('bvuge', 31): 0, ('bvsle', 31): 0, ('bvsge', 31): 0, ('bvadd_noovfl_u', 31): 0, ('bvsub_noudfl_u', 31): 0,
    ('bvshl by 0', 33): 0, ('bvlshr by 0', 33): 0, ('bvashr by 0', 33): 0, ('bvshl by 1', 33): 0,
    ('bvlshr by 1', 33): 0, ('bvashr by 1', 33): 0, ('bvshl by w-1', 33): 0, ('bvlshr by w-1', 33): 0,
    ('bvashr by w-1', 33): 0, ('bvashr by y >= w', 33): 16, ('bvshl by y >= w', 33): 19,
    ('bvlshr by y >= w', 33): 13, ('sign_extend', 33): 0, ('bvneg', 33): 0, ('bvslt', 33): 0, ('bvule', 33): 0,
    ('bvuge', 33): 0, ('bvsle', 33): 0, ('bvsge', 33): 0, ('bvadd_noovfl_u', 33): 0, ('bvsub_noudfl_u', 33): 0,
    ('bvshl by 0', 160): 0, ('bvlshr by 0', 160): 0, ('bvashr by 0', 160): 0, ('bvshl by 1', 160): 0,
    ('bvlshr by 1', 160): 0, ('bvashr by 1', 160): 0, ('bvshl by w-1', 160): 0, ('bvlshr by w-1', 160): 0,
    ('bvashr by w-1', 160): 0, ('bvashr by y >= w', 160): 59, ('bvshl by y >= w', 160): 85,
    ('bvlshr by y >= w', 160): 57, ('sign_extend', 160): 0, ('bvneg', 160): 0, ('bvslt', 160): 0,
    ('bvule', 160): 0, ('bvuge', 160): 0, ('bvsle', 160): 0, ('bvsge', 160): 0, ('bvadd_noovfl_u', 160): 0,
    ('bvsub_noudfl_u', 160): 0, ('bvshl by 0', 255): 0, ('bvlshr by 0', 255): 0, ('bvashr by 0', 255): 0,
    ('bvshl by 1', 255): 0, ('bvlshr by 1', 255): 0, ('bvashr by 1', 255): 0, ('bvshl by w-1', 255): 0,
    ('bvlshr by w-1', 255): 0, ('bvashr by w-1', 255): 0, ('bvashr by y >= w', 255): 101,
    ('bvshl by y >= w', 255): 131, ('bvlshr by y >= w', 255): 99, ('sign_extend', 255): 0, ('bvneg', 255): 0,
    ('bvslt', 255): 0, ('bvule', 255): 0, ('bvuge', 255): 0, ('bvsle', 255): 0, ('bvsge', 255): 0,
    ('bvadd_noovfl_u', 255): 0, ('bvsub_noudfl_u', 255): 0, ('bvshl by 0', 256): 0, ('bvlshr by 0', 256): 0,
    ('bvashr by 0', 256): 0, ('bvshl by 1', 256): 0, ('bvlshr by 1', 256): 0, ('bvashr by 1', 256): 0,
    ('bvshl by w-1', 256): 0, ('bvlshr by w-1', 256): 0, ('bvashr by w-1', 256): 0,
    ('bvashr by y >= w', 256): 104, ('bvshl by y >= w', 256): 108, ('bvlshr by y >= w', 256): 102,
    ('sign_extend', 256): 0, ('bvneg', 256): 0, ('bvslt', 256): 0, ('bvule', 256): 0, ('bvuge', 256): 0,
    ('bvsle', 256): 0, ('bvsge', 256): 0, ('bvadd_noovfl_u', 256): 0, ('bvsub_noudfl_u', 256): 0,
}


def test_every_identity_is_kept_somewhere():
    for w in IDENTITY_WIDTHS:
        for name in _identities(w):
            assert (name, w) in IDENTITY_CONFLICTS, (name, w)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w", IDENTITY_WIDTHS)
def test_identities_are_valid(w, mode):
    solver = make_solver(mode)
    ran = 0
    for name, (lhs, rhs, side) in _identities(w).items():
        if (name, w) not in IDENTITY_CONFLICTS:
            continue
        assert X.sort_error([lhs, rhs] + side) is None, name
        st, _ = check(solver, mode, side + [Node("distinct", 1, (lhs, rhs))])
        assert st == "unsat", (name, w, st)
        # the circuits are not vacuous: each side takes a value the other allows
        st, assign = check(solver, mode, side + [Node("eq", 1, (lhs, rhs))])
        assert st == "sat" and true_under(assign, side + [Node("eq", 1, (lhs, rhs))]), (name, w)
        ran += 1
    assert ran >= 15
    solver.close()
