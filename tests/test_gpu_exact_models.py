"""The exact procedure's models on kernel 2: unpinned satisfiable queries
``e == v`` from kernel 2's case table (tests/k2_opcases.py; v the value of
k2_insn_ref under one of the table's models, so the query has a model) are
decided by ExactSolver, and the model it returns goes the way
SatSearchBackend._decide sends every exact answer before anyone sees it --
SatSearchBackend._score, one kernel-2 launch over the conjuncts -- and through
smt_eval.evaluate.  Both must say the conjuncts hold.

The list is fixed here: operators other than general division at widths 8,
33, 64, 160 and 256; the default budget decides each (checked on the CPU: at
most 103 conflicts, 0 for most)."""
import functools

import pytest

import k2_opcases as K
from k2_insn_ref import values
from mythril_amd.device import GpuDevice
from mythril_amd.smt.exact import ExactSolver
from mythril_amd.smt.expr import Node, const
from mythril_amd.smt.search import SatSearchBackend
from mythril_amd.smt.solver import ModelCache
from smt_eval import evaluate

pytestmark = pytest.mark.gpu

# (group, program, model, the widest node's width)
QUERIES = [
    ("op:bvadd", 27, 176, 8), ("op:bvadd", 72, 83, 64), ("op:bvsub", 49, 41, 33), ("op:bvsub", 26, 127, 8),
    ("op:bvmul", 71, 126, 64), ("op:bvmul", 111, 166, 256), ("op:bvand", 22, 66, 8), ("op:bvor", 115, 85, 256),
    ("op:bvor", 49, 179, 33), ("op:bvxor", 21, 175, 8), ("op:bvxor", 75, 31, 64), ("op:bvnot", 25, 30, 33),
    ("op:bvneg", 34, 44, 64), ("op:bvneg", 54, 138, 256), ("op:bvult", 23, 154, 8), ("op:bvsle", 112, 61, 256),
    ("op:bvsle", 50, 75, 33), ("op:eq", 77, 194, 64), ("op:bvadd_noovfl_u", 49, 157, 33),
    ("op:bvumul_noovfl", 68, 143, 64), ("op:bvumul_noovfl", 110, 93, 256), ("op:bvsub_noudfl_u", 54, 91, 33),
    ("op:zero_extend", 106, 190, 256), ("op:zero_extend", 75, 118, 33), ("op:zero_extend", 171, 37, 160),
    ("op:sign_extend", 75, 56, 33), ("op:sign_extend", 97, 13, 64), ("op:sign_extend", 175, 120, 160),
    ("op:sign_extend", 172, 5, 160), ("op:extract", 29, 167, 256), ("op:concat", 77, 134, 64),
    ("op:concat", 41, 78, 256), ("op:ite", 214, 70, 256), ("op:ite", 46, 158, 8), ("op:bvumin", 112, 192, 256),
    ("op:bvsmax", 71, 153, 64), ("shift:bvshl", 93, 110, 33), ("shift:bvshl", 41, 148, 8),
    ("shift:bvlshr", 154, 41, 64), ("shift:bvlshr", 264, 141, 256), ("shift:bvashr", 32, 36, 8),
    ("fuse:tails", 52, 174, 256), ("fuse:tails", 53, 46, 256), ("fuse:chains", 53, 8, 256),
    ("fuse:cmp_and", 50, 153, 64), ("slots:9", 3, 114, 256),
]
DIVISIONS = ("bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod")


@functools.lru_cache(maxsize=None)
def _groups():
    out = {}
    for part in (K.op_groups(), K.shift_groups(), K.fusion_groups(), K.slot_groups()):
        out.update(part)
    return out


def _nodes(e):
    seen, stack = set(), [e]
    while stack:
        n = stack.pop()
        if n not in seen:
            seen.add(n)
            stack.extend(n.args)
    return seen


def query(group, d, m):
    """[e == v]: program d's expression and its reference value under model m."""
    g = _groups()[group]
    e = g.exprs[d]
    v = values(g.prog, [g.models[m]])[d][0]
    return [Node("eq", 1, (e, const(v, e.width)))]


def test_the_list_is_what_it_says():
    assert len(QUERIES) >= 40 and {w for *_, w in QUERIES} == {8, 33, 64, 160, 256}
    for group, d, m, w in QUERIES:
        nodes = _nodes(query(group, d, m)[0])
        assert max(n.width for n in nodes) == w, (group, d)
        assert any(n.op == "var" for n in nodes) and not any(n.op in DIVISIONS for n in nodes), (group, d)


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def test_exact_models_hold_on_kernel_2(dev):
    exact = ExactSolver()
    backend = SatSearchBackend(ModelCache(device=dev), search=False, exact=exact)
    for group, d, m, _ in QUERIES:
        conj = query(group, d, m)
        st, assign = exact.check(conj)
        assert st == "sat", (group, d, m, st)
        _, hit = backend._score(conj, [assign])
        assert hit is not False, f"{group} program {d}: kernel 2 has no row for the conjunct"
        assert hit == 0, f"{group} program {d} model {m}: kernel 2 rejects the exact procedure's model {assign}"
        assert evaluate(conj[0], assign) == 1, (group, d, m, assign)
    assert backend.stats["launches"] == len(QUERIES)
    exact.close()
