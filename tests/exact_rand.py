"""Random query DAGs over the exact procedure's whole operator set at one narrow
width, and the brute force that decides them (every assignment of the
variables, and of the array's / function's table over a two-value alphabet).
Shared by tests/test_exact_cpu.py (width 4) and tests/test_exact_words_cpu.py
(widths 3, 5, 6, 7).  Test-only; seeded by the caller's ``random.Random``: the
order of the draws is part of the interface (the width-4 tests keep their
queries).  The array is ``mem{w}``, the function ``f{w}``."""
import itertools

from mythril_amd.smt import expr as E
from mythril_amd.smt.expr import Array, Function, symbol_factory as sf
from mythril_amd.smt.program import ArrayInterp, FuncInterp
from mythril_amd.smt.solver import ModelRef

BIN = ["bvadd", "bvsub", "bvmul", "bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod", "bvand", "bvor", "bvxor",
       "bvshl", "bvlshr", "bvashr"]
CMP = ["eq", "distinct", "bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge",
       "bvadd_noovfl_u", "bvumul_noovfl", "bvsub_noudfl_u"]


def holds(assign, conj):
    m = ModelRef(assign)
    return all(m.eval(c, model_completion=True).param == 1 for c in conj)


class Gen:
    """The generator at width ``w``."""

    def __init__(self, w):
        self.w = w
        self.arr_name, self.func_name = f"mem{w}", f"f{w}"
        self.arr_raw = Array(self.arr_name, w, w).raw
        self.func = Function(self.func_name, [w], w)

    def rand_bv(self, rng, leaves, depth):
        W = self.w
        if depth == 0 or rng.random() < 0.25:
            if rng.random() < 0.3:
                return E.const(rng.randrange(1 << W), W)
            return rng.choice(leaves)
        k = rng.random()
        if k < 0.55:
            return E._fold(rng.choice(BIN), W, (self.rand_bv(rng, leaves, depth - 1),
                                                self.rand_bv(rng, leaves, depth - 1)))
        if k < 0.62:
            return E._fold(rng.choice(["bvnot", "bvneg"]), W, (self.rand_bv(rng, leaves, depth - 1),))
        if k < 0.75:
            return E._fold("ite", W, (self.rand_bool(rng, leaves, depth - 1), self.rand_bv(rng, leaves, depth - 1),
                                      self.rand_bv(rng, leaves, depth - 1)))
        if k < 0.85:
            # extract + extend / concat back to W bits
            a = self.rand_bv(rng, leaves, depth - 1)
            lo = rng.randrange(W)
            hi = rng.randrange(lo, W)
            x = E._fold("extract", hi - lo + 1, (a,), (hi, lo))
            if hi - lo + 1 == W:
                return x
            if rng.random() < 0.5:
                return E._fold(rng.choice(["zero_extend", "sign_extend"]), W, (x,), W - (hi - lo + 1))
            rest = W - (hi - lo + 1)
            b = E._fold("extract", rest, (self.rand_bv(rng, leaves, depth - 1),), (rest - 1, 0))
            return E._fold("concat", W, (x, b))
        if k < 0.93:
            return E._select(self.arr_raw, self.rand_bv(rng, leaves, depth - 1))
        return self.func(sf.BitVecVal(0, W) + E.BitVec(self.rand_bv(rng, leaves, depth - 1))).raw

    def rand_bool(self, rng, leaves, depth):
        k = rng.random()
        if depth == 0 or k < 0.6:
            return E._fold(rng.choice(CMP), 1, (self.rand_bv(rng, leaves, depth - 1 if depth else 0),
                                               self.rand_bv(rng, leaves, depth - 1 if depth else 0)))
        if k < 0.75:
            return E._fold("not", 1, (self.rand_bool(rng, leaves, depth - 1),))
        if k < 0.9:
            op = rng.choice(["and", "or"])
            return E.Node(op, 1, (self.rand_bool(rng, leaves, depth - 1), self.rand_bool(rng, leaves, depth - 1)))
        return E._fold(rng.choice(["xor", "implies"]), 1, (self.rand_bool(rng, leaves, depth - 1),
                                                          self.rand_bool(rng, leaves, depth - 1)))

    def uses_tables(self, conj):
        return any(self.arr_name in repr(c) or self.func_name in repr(c) for c in conj)

    def enumerate_models(self, conj, names):
        W = self.w
        vals = range(1 << W)
        tables = [None]
        if self.uses_tables(conj):
            # the reads' indices range over all 2^W points: enumerate a table as
            # 2^W values drawn from a small alphabet -- exhaustive over {0, 5} per point
            tables = list(itertools.product((0, 5), repeat=1 << W))
        for xs in itertools.product(vals, repeat=len(names)):
            base = dict(zip(names, xs))
            for tab in tables:
                a = dict(base)
                if tab is not None:
                    a[self.arr_name] = ArrayInterp(0, dict(enumerate(tab)))
                    a[self.func_name] = FuncInterp(0, {(i,): v for i, v in enumerate(tab)})
                yield a
