"""Term programs and global minimisation on the CPU: compile_terms against the C
oracle and the Python evaluator, SatSearchBackend(global_min=True) against brute
force with a CPU stand-in for mg_eval_terms / mg_eval_min (tests/k2_terms_ref.py;
tests/test_gpu_terms.py runs the same inputs on the MI355X)."""
import numpy as np
import pytest

from k2_terms_ref import (RefK2, brute_force, min_queries, oracle_values, limbs_to_int, run_min_queries,
                          term_models, term_set)
from mythril_amd.smt.flatten import NativeCompiler, PyCompiler, compile_terms
from mythril_amd.smt.program import REF_ACC, REF_VAR, ModelPool, ProgramBatch, enc_w0, ref
from oracle.bv_ref import eval_batch
from smt_eval import evaluate


def test_compile_terms_native_equals_python_and_values_equal_the_evaluator():
    terms, wide = term_set()
    assert len(terms) >= 40
    pn, kn = compile_terms(terms, NativeCompiler())
    pp, kp = compile_terms(terms, PyCompiler())
    assert kn == kp == [k for k in range(len(terms)) if k != wide]      # the 512-bit root is left out
    assert np.array_equal(pn.prog_off, pp.prog_off) and np.array_equal(pn.insns, pp.insns)
    assert pn.var_names == pp.var_names and np.array_equal(pn.consts, pp.consts)
    # a lone variable / constant is one copy
    for d in (0, 1, 2):
        assert pn.program(d).shape[0] == 1 and int(pn.program(d)[0, 0]) & 0xFF == 0
    widths = [terms[k].raw.width for k in kn]
    assert {1, 8, 255, 256} <= set(widths)
    # values on the C oracle: each program + eq(acc, expect_d) holds under every model
    models = term_models(64, seed=21)
    nv = len(pn.var_names)
    rows, off = [], [0]
    for d, k in enumerate(kn):
        p = pn.program(d)
        assert (int(p[-1, 0]) >> 8) & 0x1FF == widths[d]
        rows += [p, np.array([[enc_w0("eq", 1), ref(REF_ACC, 0), ref(REF_VAR, nv + d), widths[d]]], dtype=np.uint32)]
        off.append(off[-1] + p.shape[0] + 1)
        for m in models:
            m[f"expect_{d}"] = int(evaluate(terms[k].raw, m))
    checked = ProgramBatch(np.concatenate(rows), np.asarray(off, dtype=np.uint32), pn.consts, pn.n_slots,
                           pn.var_names + [f"expect_{d}" for d in range(len(kn))], pn.var_widths + widths, pn.tables)
    pool = ModelPool.from_dicts(models, checked.var_names, checked.var_widths, checked.tables)
    _, sc = eval_batch(checked, pool)
    assert sc.tolist() == [64] * len(kn), [terms[kn[d]] for d in np.flatnonzero(sc != 64)]
    # and the stand-in's bit-by-bit reading of the same programs gives the same integers
    vals = oracle_values(pn, ModelPool.from_dicts(models, pn.var_names, pn.var_widths, pn.tables))
    for d in range(len(kn)):
        assert [limbs_to_int(vals[d, m]) for m in range(64)] == [m[f"expect_{d}"] for m in models], d


def _plain(assign):
    """An assignment with its interpretations as comparable values."""
    return {k: v if isinstance(v, int) else (type(v).__name__, getattr(v, "default", getattr(v, "else_value", None)),
                                             dict(v.entries)) for k, v in assign.items()}


@pytest.fixture(scope="module")
def min_run():
    return run_min_queries(RefK2)


def test_global_minimum_equals_brute_force(min_run):
    best, local, truth, stats = min_run
    assert len(truth) >= 200
    assert best == list(truth)                       # the optimum on every satisfiable query, None on the others
    nonzero = [k for k, t in enumerate(truth) if t is not None and any(t)]
    assert len(nonzero) >= 60, len(nonzero)
    worse = [k for k in nonzero if local[k] > truth[k]]
    assert len(worse) >= 10, len(worse)
    assert all(local[k] is None or local[k] >= truth[k] for k in range(len(truth)) if truth[k] is not None)
    assert stats["min_unproved"] == 0 and stats["min_device"] > 0 and stats["min_exact"] > 0
    assert stats["min_improved"] > 0


def test_global_minimum_is_off_by_default(monkeypatch):
    from mythril_amd.smt.exact import ExactSolver
    from mythril_amd.smt.search import SatSearchBackend
    from mythril_amd.smt.solver import ModelCache, UnsatError
    monkeypatch.delenv("MYTHSMT_GLOBAL_MIN", raising=False)
    calls = []
    monkeypatch.setattr(ModelCache, "lex_min", lambda self, *a, **k: calls.append(a) or (False, [], 0))
    k2s = [RefK2(), RefK2()]
    caches = [ModelCache(device=k) for k in k2s]
    off = SatSearchBackend(caches[0], exact=ExactSolver(), global_min=False)
    plain = SatSearchBackend(caches[1], exact=ExactSolver())
    assert off.global_min is False and plain.global_min is False
    answered = 0
    for conj, objs, _ in min_queries(60, seed=11):
        out = []
        for cache, backend in zip(caches, (off, plain)):
            try:
                model = backend(list(conj), tuple(objs), (), 10000)
                cache.put(model, 1)
                out.append(_plain(model.raw[-1].assignment))
            except UnsatError:
                out.append(None)
        assert out[0] == out[1]
        answered += out[0] is not None
    assert answered > 20
    assert not calls and all(k.terms_calls == 0 and k.min_calls == 0 for k in k2s)
    monkeypatch.setenv("MYTHSMT_GLOBAL_MIN", "1")
    assert SatSearchBackend(caches[1]).global_min is True


def test_flag_array_calldata_under_global_min_on_the_oracle_device(monkeypatch, tmp_path):
    """analysis_tests.py:11-17 with MYTHSMT_GLOBAL_MIN=1: the same issue, the
    transaction input the reference's Optimize prints, and the minimum chosen
    through eval_min."""
    from fnames import use_signature_db
    from oracle_device import OracleDevice
    from test_integration_cpu import GOLDEN, check_row
    monkeypatch.setenv("MYTHSMT_GLOBAL_MIN", "1")
    use_signature_db(monkeypatch, tmp_path)
    row = next(r for r in GOLDEN["issue_counts"] if r[0] == "flag_array.sol.o")
    k2 = RefK2()
    _, info = check_row(row, OracleDevice(), k2)
    assert info["search"]["min_device"] > 0 and k2.min_calls > 0
