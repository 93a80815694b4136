"""Kernel 2's opcode-level reference (tests/k2_insn_ref.py) pinned three ways
before the device sees it: against the C oracle (oracle/bv_ref.c, read out bit by
bit), against smt_eval.evaluate of the equivalent expression, and on compiler-
produced programs against evaluate of the terms they were compiled from; plus
the coverage conditions of the division case lists, asserted from the digit-level
restatement of Knuth D alone.  tests/test_gpu_k2_ops.py runs the same lists on
the device."""
import random

import numpy as np
import pytest

import k2_opcases as cases
from k2_insn_ref import EVENTS, knuth_events, mask, run_program, values
from k2_terms_ref import oracle_values, term_models, term_set
from mythril_amd.smt.flatten import compile_terms
from mythril_amd.smt.program import ModelPool, ProgramBatch, enc_w0, limbs, ref, REF_ACC, REF_CONST, REF_SLOT, REF_VAR
from smt_eval import evaluate

GROUPS = cases.group_names()
# The oracle reports one bit per run, so a w-bit program costs w runs: it sees a
# seeded subset -- per group ORACLE_PROGRAMS programs over ORACLE_MODELS models
# (division groups: every program over the first 8 lanes of each wave, at most 512 models).
ORACLE_PROGRAMS, ORACLE_MODELS = 24, 64


def test_hand_worked_program():
    """Five instructions on 8-bit and 16-bit values, the integers written out."""
    V, S, K = (lambda i: ref(REF_VAR, i)), (lambda i: ref(REF_SLOT, i)), (lambda i: ref(REF_CONST, i))
    rows = [
        [enc_w0("bvadd", 8, 0), V(0), V(1), 0],         # 0xF0 + 0x25 = 0x115 -> 0x15 (8 bits), kept in slot 0
        [enc_w0("sign_extend", 16), ref(REF_ACC, 0), 5, 0],   # 0x15 read as 5 bits: bit 4 set -> 0xFFF5
        [enc_w0("bvlshr", 16), ref(REF_ACC, 0), K(0), 0],     # 0xFFF5 >> 4 = 0x0FFF
        [enc_w0("rconcat", 16), S(0), K(1), 8],         # slot 0 low (8 bits), constant 0xAB high -> 0xAB15
        [enc_w0("bvsdiv", 16), ref(REF_ACC, 0), K(2), 0],     # 0xAB15 = -21739; / -2 = 10869 = 0x2A75
    ]
    want = [0x15, 0xFFF5, 0x0FFF, 0xAB15, 0x2A75]
    for n in range(1, 6):
        assert run_program(rows[:n], [4, 0xAB, 0xFFFE], [0xF0, 0x25]) == want[n - 1], n
    prog = ProgramBatch(np.asarray(rows, dtype=np.uint32), np.array([0, 5], dtype=np.uint32),
                        np.array([limbs(4), limbs(0xAB), limbs(0xFFFE)], dtype=np.uint32), 1, ["p", "q"], [8, 8])
    # models 1 and 2 differ only in slot 0 (p is masked to its 8 bits: 0xF0; and 0):
    # 0xABF0 = -21520, / -2 = 10760 = 0x2A08; 0xAB00 = -21760, / -2 = 10880 = 0x2A80
    assert values(prog, [{"p": 0xF0, "q": 0x25}, {"p": 0x1F0, "q": 0}, {}]) == [[0x2A75, 0x2A08, 0x2A80]]


def test_zero_divisors_and_shift_edges_by_hand():
    one = lambda op, w, a, b, w3=0: run_program([[enc_w0(op, w), ref(REF_VAR, 0), ref(REF_VAR, 1), w3]], [], [a, b])
    assert one("bvudiv", 8, 7, 0) == 0xFF and one("bvurem", 8, 7, 0) == 7
    assert one("bvsdiv", 8, 0x80, 0) == 1 and one("bvsdiv", 8, 0x7F, 0) == 0xFF
    assert one("bvsrem", 8, 0x85, 0) == 0x85 and one("bvsmod", 8, 0x85, 0) == 0x85
    assert one("bvsdiv", 8, 0x80, 0xFF) == 0x80 and one("bvsrem", 8, 0x80, 0xFF) == 0
    assert one("bvsmod", 8, 0xF9, 3) == 2 and one("bvsrem", 8, 0xF9, 3) == 0xFF      # -7 mod 3 = 2, -7 rem 3 = -1
    assert one("bvsmod", 8, 7, 0xFD) == 0xFE                                       # 7 mod -3 = -2
    assert one("bvshl", 8, 1, 8) == 0 and one("bvshl", 8, 1, 7) == 0x80 and one("bvlshr", 8, 0x80, 8) == 0
    assert one("bvashr", 8, 0x80, 200) == 0xFF and one("bvashr", 8, 0x40, 200) == 0 and one("bvashr", 8, 0x80, 3) == 0xF0
    assert one("bvshl", 64, 1, (1 << 32) + 1) == 0
    assert one("bvadd_noovfl_u", 1, 0xFF, 0, 8) == 1 and one("bvadd_noovfl_u", 1, 0xFF, 1, 8) == 0
    assert one("bvumul_noovfl", 1, 16, 15, 8) == 1 and one("bvumul_noovfl", 1, 16, 16, 8) == 0
    assert one("bvsmin", 8, 0x80, 0x7F) == 0x80 and one("bvumin", 8, 0x80, 0x7F) == 0x7F
    assert one("bvrsub", 8, 1, 0) == 0xFF and one("rconcat", 12, 0xA, 0xBC, 4) == 0xBCA
    assert one("concat", 12, 0xA, 0xBC, 8) == 0xABC


# (tab has no expression form here: the oracle test and the compiled term set pin it)
@pytest.mark.parametrize("name", [n for n in GROUPS if n != "tables"])
def test_reference_equals_the_expression_evaluator(name):
    """Every program of every case list, under every model: k2_insn_ref on the
    instructions == smt_eval.evaluate on the expression the program stands for."""
    g = cases.all_groups()[name]
    got = cases.reference_ints(name)
    assert all(e is not None for e in g.exprs)
    for d, e in enumerate(g.exprs):
        row = got[d]
        for m, model in enumerate(g.models):
            want = evaluate(e, model)
            assert row[m] == want, f"{g.describe(d, m)}: reference {row[m]:#x}, evaluator {want:#x}"


def _oracle_subset(name):
    g = cases.all_groups()[name]
    rng = random.Random(sum(map(ord, name)))
    dags = sorted(rng.sample(range(g.prog.n_dags), min(ORACLE_PROGRAMS, g.prog.n_dags)))
    if g.waves:
        ms = [s + k for _, s in g.waves for k in range(8)][:ORACLE_MODELS * 8]
    else:
        ms = sorted(rng.sample(range(len(g.models)), min(ORACLE_MODELS, len(g.models))))
    return g, dags, ms


@pytest.mark.parametrize("name", GROUPS)
def test_reference_equals_the_c_oracle(name):
    g, dags, ms = _oracle_subset(name)
    pool = ModelPool.from_dicts([g.models[m] for m in ms], g.prog.var_names, g.prog.var_widths, g.prog.tables)
    got = oracle_values(g.prog, pool, dags)
    want = cases.reference_limbs(name)[np.ix_(dags, ms)]
    bad = np.argwhere((got != want).any(axis=2))
    assert not len(bad), f"{g.describe(dags[bad[0][0]], ms[bad[0][1]])}: oracle {got[tuple(bad[0])]}, reference {want[tuple(bad[0])]}"


def test_compiled_term_set_three_ways():
    """compile_terms(term_set()): the interpreter on the compiled programs ==
    evaluate on the terms == the C oracle, tables included."""
    terms, wide = term_set()
    prog, kept = compile_terms(terms)
    models = term_models(96, seed=33)
    got = values(prog, models)
    for k, d in zip(kept, range(prog.n_dags)):
        assert got[d] == [int(evaluate(terms[k].raw, m)) for m in models], (d, terms[k])
    pool = ModelPool.from_dicts(models, prog.var_names, prog.var_widths, prog.tables)
    ora = oracle_values(prog, pool)
    assert [[int.from_bytes(ora[d, m].astype("<u4").tobytes(), "little") for m in range(96)] for d in range(prog.n_dags)] == got


# ------------------------------------------------------------------ coverage
# Which events the digit model can meet below 2^w.  256 / 255: all four.  64: the
# divisor has at most two digits, so the refined estimate is exact (no add-back); a
# two-digit quotient needs a one-digit divisor, whose remainder's top digit is below
# it, and a one-digit quotient's top window digit is a >> bitlen(b) < 2^31 (no
# qmax); two decrements were not met in 150,000 directed pairs.  8: an exhaustive
# run over all 65,280 pairs meets none (the second divisor digit is 0).
REACHABLE = {256: set(EVENTS), 255: set(EVENTS), 64: {"dec1"}, 8: set()}


def test_knuth_digit_model_on_known_pairs():
    """division_operand (seed 5) meets all four events within 4,096 pairs; every step of
    the model checks itself against divmod as it goes."""
    assert knuth_events(7, 3) == set() and knuth_events((1 << 256) - 1, (1 << 255) + 1) == set()
    rng = random.Random(5)
    hits = dict.fromkeys(EVENTS, 0)
    for _ in range(4096):
        a, b = cases.division_operand(rng), cases.division_operand(rng)
        if b & (b - 1):
            for e in knuth_events(a, b):
                hits[e] += 1
    assert all(hits[e] > 0 for e in EVENTS), hits


@pytest.mark.parametrize("w", [256, 255, 64, 8])
def test_division_lists_reach_the_rare_steps(w):
    groups = cases.division_groups()
    for kind in ("unsigned", "signed"):
        g = groups[f"div:{kind} w={w}"]
        counts = cases.event_counts(g.div_pairs)
        print(f"{g.name}: {len(g.models)} models, {len(g.waves)} waves, events {counts}")
        for e in EVENTS:
            if e in REACHABLE[w]:
                assert counts[e] >= (10 if w == 256 else 1), (g.name, counts)
            else:
                assert counts[e] == 0, (g.name, counts)
    if w != 8:
        g = groups[f"div:umul_noovfl w={w}"]
        print(f"{g.name}: {len(g.models)} models, events {cases.event_counts(g.div_pairs)}")


def _bitlen(x):
    return x.bit_length()


def test_every_wave_class_is_what_its_name_says():
    """Wave classes are non-empty, 64 lanes each, and homogeneous in the property the
    device ballots on (checked on the operands, for the width-256 unsigned pool)."""
    g = cases.division_groups()["div:unsigned w=256"]
    assert len(g.models) % 64 == 0 and all(s % 64 == 0 for _, s in g.waves)
    by_name = {}
    for name, s in g.waves:
        by_name[name] = [(g.models[m]["a"], g.models[m]["b"]) for m in range(s, s + 64)]
    count = lambda lanes, f: sum(1 for a, b in lanes if f(a, b))
    pow2 = lambda a, b: b and b & (b - 1) == 0
    assert count(by_name["divisor a power of two"], pow2) == 64
    assert count(by_name["divisor a power of two +1 lane"], pow2) == 63
    short = lambda a, b: _bitlen(a) < _bitlen(b)
    assert count(by_name["bitlen(a) < bitlen(b)"], short) == 64 and count(by_name["bitlen(a) < bitlen(b) +1 lane"], short) == 63
    long_ = lambda a, b: _bitlen(b) > 224 and _bitlen(a) >= _bitlen(b)
    assert count(by_name["long divisor"], long_) == 64 and count(by_name["long divisor +1 lane"], long_) == 63
    assert count(by_name["long divisor"], lambda a, b: _bitlen(b) == 256) >= 8
    for k in range(8):
        in_k = lambda a, b: 32 * k <= _bitlen(a) - _bitlen(b) < 32 * k + 32
        assert count(by_name[f"dl in [{32 * k}, {32 * k + 32})"], in_k) == 64
        assert count(by_name[f"dl in [{32 * k}, {32 * k + 32}) +1 lane"], in_k) == 63
    for q in range(8):
        in_q = lambda a, b: (256 - _bitlen(b)) >> 5 == q and _bitlen(a) >= _bitlen(b)
        assert count(by_name[f"shift limbs {q}"], in_q) == 64 and count(by_name[f"shift limbs {q} +1 lane"], in_q) == 63
    assert len({(256 - _bitlen(b)) >> 5 for _, b in by_name["shift limbs mixed"]}) >= 5
    zero = lambda a, b: b == 0
    assert count(by_name["divisor zero"], zero) == 64
    assert count(by_name["one non-zero divisor among zeros +1 lane"], zero) == 63
    assert count(by_name["one zero divisor +1 lane"], zero) == 1
    for e in EVENTS:
        assert all(e in knuth_events(a, b) for a, b in by_name[f"event {e}"])
    # the signed pools carry every sign combination and MIN / -1, MIN / 1
    s = cases.division_groups()["div:signed w=256"]
    MIN, M = 1 << 255, mask(256)
    have = {(m["a"], m["b"]) for m in s.models[-64:]}
    assert {(MIN, M), (MIN, 1)} <= have
    signs = {(m["a"] >> 255, m["b"] >> 255) for m in s.models}
    assert signs == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_case_lists_cover_what_the_issue_names():
    groups = cases.all_groups()
    assert {f"op:{op}" for op in cases.OPS if op != "tab"} <= set(groups) and "tables" in groups
    for op in cases.ARITH:
        labels = groups[f"op:{op}"].labels
        for w in cases.WIDTHS:
            for ka, kb in cases.AB_KINDS:
                assert f"{op} w={w} A={ka} B={kb}" in labels
    assert cases.shift_amounts(256) == sorted({0, 1, 31, 32, 33, 255, 256, 257, 1 << 32, (1 << 32) + 1, 1 << 255})
    assert cases.shift_amounts(8) == [0, 1, 7, 8, 9, 31, 32, 33, 255]
    # every model of the crossed pool respects the input contract
    models, vals = cases.crossed_models()
    assert len(models) == 196 and all(0 <= v <= mask(w) for w in cases.ALL_WIDTHS for v in vals[w])
