"""Test-only CPU stand-in for kernel 2's term entry points (mg_eval_terms,
mg_eval_min), and the inputs the term tests share (tests/test_terms_cpu.py on
the CPU, tests/test_gpu_terms.py on the MI355X).  Never imported by
``mythril_amd``.

The stand-in reads values out of the C oracle (oracle/bv_ref.c), which reports
one bit per (program, model): a program of result width w is run w times, each
copy followed by ``extract(acc, bit b)``.  The choice of the minimum is made in
Python over those integers."""
import functools
import itertools
import random

import numpy as np

from mythril_amd.smt.expr import (And, BVAddNoOverflow, BVMulNoOverflow, BVSubNoUnderflow, Concat,
                                  Extract, If, LShR, Not, Or, SRem, UDiv, UGE, UGT, ULE, ULT, URem,
                                  SignExt, ZeroExt, symbol_factory)
from mythril_amd.smt.program import REF_ACC, ProgramBatch, enc_w0, ref
from oracle_device import OracleK2
from smt_eval import evaluate

BVS, BVV = symbol_factory.BitVecSym, symbol_factory.BitVecVal
NO_MODEL = 0xFFFFFFFF


def limbs_to_int(row) -> int:
    return int.from_bytes(np.ascontiguousarray(row, dtype="<u4").tobytes(), "little")


def result_width(prog, d: int) -> int:
    """Width of program d's final accumulator (its last instruction's width)."""
    return (int(prog.program(d)[-1, 0]) >> 8) & 0x1FF


def oracle_values(prog, pool, dags=None) -> np.ndarray:
    """uint32[len(dags), n_models, 8]: the final accumulator of each program under
    each model, bit by bit from the C oracle's satisfaction bitmaps."""
    from oracle.bv_ref import eval_batch
    dags = list(range(prog.n_dags)) if dags is None else list(dags)
    n_models = pool.n_models
    out = np.zeros((len(dags), n_models, 8), dtype=np.uint32)
    if not dags:
        return out
    rows, off, owner = [], [0], []
    for k, d in enumerate(dags):
        p = np.asarray(prog.program(d), dtype=np.uint32)
        for b in range(result_width(prog, d)):
            rows.append(p)
            rows.append(np.array([[enc_w0("extract", 1), ref(REF_ACC, 0), b, 0]], dtype=np.uint32))
            off.append(off[-1] + p.shape[0] + 1)
            owner.append((k, b))
    big = ProgramBatch(np.concatenate(rows), np.asarray(off, dtype=np.uint32), prog.consts, prog.n_slots,
                       prog.var_names, prog.var_widths, prog.tables)
    bits = np.zeros((big.n_dags, (n_models + 63) // 64), dtype=np.uint64)
    eval_batch(big, pool, bits=bits)
    flat = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :n_models].astype(np.uint32)
    for r, (k, b) in enumerate(owner):
        out[k, :, b >> 5] |= flat[r] << np.uint32(b & 31)
    return out


def reference_min(values: np.ndarray, cons, objs):
    """mg_eval_min's contract restated over a value array [n_dags, n_models, 8]:
    (best_model, [objective ints], cand_count) of one query."""
    n_models = values.shape[1]
    best = None
    count = 0
    for m in range(n_models):
        if all(int(values[d, m, 0]) & 1 for d in cons):
            count += 1
            key = tuple(limbs_to_int(values[d, m]) for d in objs)
            if best is None or key < best[0]:
                best = (key, m)
    if best is None:
        return NO_MODEL, [(1 << 256) - 1] * len(objs), 0
    return best[1], list(best[0]), count


class RefK2(OracleK2):
    """OracleK2 plus eval_terms / eval_min, with call counters."""

    def __init__(self):
        super().__init__()
        self.terms_calls = 0
        self.min_calls = 0

    def eval_terms(self, prog, pool):
        self.terms_calls += 1
        self.launches += 1
        return oracle_values(prog, pool), 0.0

    def eval_min(self, prog, pool, cons, objs):
        self.min_calls += 1
        self.launches += 1
        used = sorted({d for q in list(cons) + list(objs) for d in q})
        at = {d: k for k, d in enumerate(used)}
        vals = oracle_values(prog, pool, used)
        best, per_query, count = [], [], []
        for c, o in zip(cons, objs):
            b, v, n = reference_min(vals, [at[d] for d in c], [at[d] for d in o])
            best.append(b)
            count.append(n)
            per_query.append(np.array([np.frombuffer(x.to_bytes(32, "little"), dtype="<u4") for x in v],
                                      dtype=np.uint32).reshape(len(o), 8))
        return np.array(best, dtype=np.uint32), per_query, np.array(count, dtype=np.uint32), 0.0


# ------------------------------------------------------------------ the term set
def term_set():
    """About 40 terms: widths 1, 8, 255 and 256, a lone variable and a lone
    constant, arithmetic, selects over store chains, keccak / Power applications
    (the vocabulary of test_smt_programs._random_table_constraints), Bool roots,
    and one 512-bit root (unsupported: left out).  Returns (terms, index of the
    wide one)."""
    from mythril_amd.smt.expr import Array, Function, K
    x, y, z, s = BVS("x", 256), BVS("y", 256), BVS("z", 256), BVS("slot", 256)
    x8, y8 = BVS("x8", 8), BVS("y8", 8)
    p, q = BVS("p255", 255), BVS("q255", 255)
    b1, c1 = BVS("b1", 1), BVS("c1", 1)
    storage = Array("Storage", 256, 256)
    storage[x] = y
    storage[BVV(1, 256)] = x + y
    cd = Array("calldata", 256, 8)
    cd[BVV(0, 256)] = Extract(7, 0, x)
    kz = K(256, 8, 0)
    kz[y] = x8
    f512 = Function("keccak256_512", [512], 256)
    inv512 = Function("keccak256_512-1", [256], 512)
    f256 = Function("keccak256_256", [256], 256)
    power = Function("Power", [256, 256], 256)
    key = Concat(x, s)
    terms = [
        x, BVV(0x1234567890ABCDEF << 130, 256), x8, b1, p, BVV(5, 8),                # lone leaves
        Extract(7, 0, x * y + BVV(3, 256)), UDiv(x, y), URem(z, x), If(ULT(x, y), x, z),
        Concat(Extract(127, 0, x), Extract(127, 0, y)), x + y, x - z, x * y, x / y, SRem(y, z),
        ~x, LShR(x, BVV(7, 256)), x << BVV(3, 256), x >> BVV(200, 256), ZeroExt(248, x8), SignExt(248, y8),
        x8 + y8, x8 * y8, UDiv(x8, y8), SRem(x8, y8), ~x8,                           # 8 bits
        p + q, p * q, UDiv(p, q), ~p, Extract(254, 0, x), If(UGT(p, q), p, q), SignExt(1, p),   # 255 bits
        b1 ^ c1, Extract(0, 0, x), ~b1, Extract(255, 255, y),                       # 1 bit
        ULT(x, y), And(ULE(x8, y8), Not(p == q)), Or(x == y, b1 == c1),             # Bool roots
        storage[s], storage[x], storage[BVV(1, 256)], cd[y], cd[BVV(0, 256)], kz[z],
        f512(key), f256(y), power(BVV(2, 256), y), Extract(255, 0, inv512(f256(x))), storage[f512(key)],
        inv512(f256(y)),                                                             # 512 bits: unsupported
    ]
    return terms, len(terms) - 1


SPECIALS = [0, 1, 1 << 255, (1 << 256) - 1]


def term_models(n: int, seed: int):
    """n models for the term set: test_smt_programs._random_table_models (x, y,
    slot and interpretations that contain the keys the terms touch) plus the
    narrow variables; the first models take the special values 0, 1, 2^255,
    2^256 - 1 in x, y and z."""
    from test_smt_programs import _random_table_models
    rng = random.Random(seed)
    models = _random_table_models(rng, n, None)
    for k, m in enumerate(models):
        m["z"] = rng.choice([0, 1, m["x"], rng.getrandbits(256)])
        if k < 2 * len(SPECIALS):
            m["x"] = SPECIALS[k % 4]
            m["y"] = SPECIALS[(k // 2 + k) % 4]
            m["z"] = SPECIALS[(k + 1) % 4]
        m["x8"], m["y8"] = rng.choice([0, 1, 0x80, 0xFF, rng.getrandbits(8)]), rng.choice([0, 1, 0x80, 0xFF, rng.getrandbits(8)])
        m["p255"] = rng.choice([0, 1, (1 << 255) - 1, 1 << 254, rng.getrandbits(255)])
        m["q255"] = rng.choice([0, 1, (1 << 255) - 1, m["p255"], rng.getrandbits(255)])
        m["b1"], m["c1"] = rng.getrandbits(1), rng.getrandbits(1)
    return models


# ------------------------------------------------------ global-minimisation queries
def _small_conjuncts(rng, vs, w):
    """test_smt_programs._random_constraints' operators at width w (4..6), plus
    conjuncts that link the variables (so that lowering one objective alone, the
    others fixed, stops short of the optimum)."""
    x, y = vs[0], vs[1]
    z = vs[-1]
    h = w // 2
    c = lambda: BVV(rng.randrange(1 << w), w)
    terms = [x + y, x - z, x * y, UDiv(x, y), URem(z, x), x / y, SRem(y, z), x & z, x | y, x ^ y, ~x,
             LShR(x, BVV(1, w)), x << BVV(1, w), x >> BVV(2, w), If(ULT(x, y), x, z),
             Concat(Extract(h - 1, 0, x), Extract(w - h - 1, 0, y)), ZeroExt(w - 2, Extract(1, 0, z)),
             SignExt(w - 2, Extract(1, 0, y)), Extract(w - 1, 0, x + z), c(), c()] + list(vs)
    preds = []
    for _ in range(rng.randrange(1, 4)):
        a, b = rng.choice(terms), rng.choice(terms)
        k = rng.randrange(12)
        preds.append([ULT(a, b), UGT(a, b), ULE(a, b), UGE(a, b), a < b, a > b, a <= b, a >= b,
                      a == b, a != b, BVAddNoOverflow(a, b, False), BVSubNoUnderflow(a, b, False)][k])
    if rng.random() < 0.3:
        preds.append(Or(preds[0], Not(preds[-1])))
    if rng.random() < 0.2:
        preds.append(BVMulNoOverflow(x, y, False))
    for _ in range(rng.randrange(1, 3)):
        k = rng.randrange(4)
        preds.append([x + y == c(), ULT(y, x), x * y == c(), x + z == c()][k])
    return preds


def min_queries(n: int = 200, seed: int = 3):
    """n queries (conjuncts, objectives, variables): 2 variables of 4..6 bits or 3
    of 4 bits (brute force stays at most 4096 assignments), 1..3 objectives,
    mostly bare variables, some terms."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        nv, w = rng.choice([(2, 4), (2, 4), (2, 5), (2, 5), (3, 4), (3, 4), (3, 4), (2, 6)])
        vs = [BVS(f"{'abc'[k]}{w}_{nv}", w) for k in range(nv)]
        conj = _small_conjuncts(rng, vs, w)
        objs = []
        for _ in range(rng.randrange(1, 4)):
            objs.append(rng.choice(vs) if rng.random() < 0.75 else rng.choice([vs[0] + vs[1], vs[-1] ^ vs[0]]))
        out.append((conj, objs, vs))
    return out


def _names(node, out):
    stack, seen = [node], set()
    while stack:
        n = stack.pop()
        if n in seen:
            continue
        seen.add(n)
        if n.op == "var":
            out.add(n.param)
        stack.extend(n.args)
    return out


def brute_force(n: int = 200, seed: int = 3):
    """Per query of min_queries(n, seed): None when no assignment satisfies it,
    else the lexicographic minimum of its objective tuple -- every assignment
    enumerated, every conjunct and objective valued by smt_eval.evaluate (a
    conjunct once per distinct value of the variables it reads).  Computed once
    per process."""
    return _brute_force(n, seed)


@functools.lru_cache(maxsize=None)
def _brute_force(n, seed):
    out = []
    for conj, objs, vs in min_queries(n, seed):
        names = [v.raw.param for v in vs]
        w = vs[0].size()
        cands = list(itertools.product(range(1 << w), repeat=len(vs)))
        for c in conj:
            reads = _names(c.raw, set())
            idx = [k for k, name in enumerate(names) if name in reads]
            memo = {}
            keep = []
            for vals in cands:
                key = tuple(vals[k] for k in idx)
                r = memo.get(key)
                if r is None:
                    r = memo[key] = bool(evaluate(c.raw, {names[k]: vals[k] for k in idx}))
                if r:
                    keep.append(vals)
            cands = keep
        best = None
        for vals in cands:
            m = dict(zip(names, vals))
            t = tuple(int(evaluate(o.raw, m)) for o in objs)
            if best is None or t < best:
                best = t
        out.append(best)
    return tuple(out)


def run_min_queries(make_k2, n: int = 200, seed: int = 3):
    """Every query of min_queries through SatSearchBackend(global_min=True) and
    through the same backend with global_min=False, each over its own ModelCache
    on make_k2().  Returns (optimal tuples, local tuples, brute-force minima,
    the global backend's stats); asserts satisfaction and UnsatError as it goes."""
    from mythril_amd.smt.exact import ExactSolver
    from mythril_amd.smt.search import SatSearchBackend
    from mythril_amd.smt.solver import ModelCache, SolverTimeOutException, UnsatError
    truth = brute_force(n, seed)
    backends = []
    for flag in (True, False):
        cache = ModelCache(device=make_k2())
        backends.append((cache, SatSearchBackend(cache, exact=ExactSolver(), global_min=flag)))
    got = ([], [])
    for (conj, objs, vs), want in zip(min_queries(n, seed), truth):
        for k, (cache, backend) in enumerate(backends):
            try:
                model = backend(list(conj), tuple(objs), (), 10000)
            except UnsatError as e:
                assert not isinstance(e, SolverTimeOutException) and want is None, (conj, want)
                got[k].append(None)
                continue
            assert want is not None, conj
            cache.put(model, 1)                      # as get_model does: later incumbents see it
            a = model.raw[-1].assignment
            assert all(evaluate(c.raw, a) for c in conj), (conj, a)
            got[k].append(tuple(int(evaluate(o.raw, a)) for o in objs))
    return got[0], got[1], truth, backends[0][1].stats
