"""Enumerated case lists for kernel 2's interpreter (bv_interp.cuh), shared by
tests/test_k2_opcases_cpu.py (three references against each other) and
tests/test_gpu_k2_ops.py (the device against k2_insn_ref).  Seeded and
deterministic.  Every program ends in the op under test, so its value is the
final accumulator.  Test-only; never imported by ``mythril_amd``.

A Group is one ProgramBatch with its model dicts, a label per program and, where
the program is expressible in the host's expression layer, the equivalent
expression node (built by interpreting the instructions symbolically).
"""
import functools
import random
from dataclasses import dataclass, field

import numpy as np

from div_operands import division_operand
from k2_insn_ref import EVENTS, knuth_events, mask, values
from mythril_amd.smt.expr import Node, const as const_node, var as var_node
from mythril_amd.smt.program import (OPS, REF_ACC, REF_CONST, REF_SLOT, REF_VAR, TAB_LO_SHIFT, TAB_PART_SHIFT,
                                     ArrayInterp, FuncInterp, ModelPool, ProgramBatch, enc_w0, limbs, ref)

WIDTHS = [1, 2, 8, 31, 32, 33, 63, 64, 65, 128, 255, 256]      # the limb edges
WAVE = 64
ACC = ref(REF_ACC, 0)
SIMPLE = ["bvadd", "bvsub", "bvmul", "bvand", "bvor", "bvxor", "bvumax", "bvumin", "bvrsub"]
CMPS = ["eq", "distinct", "bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge"]
ARITH = ["bvadd", "bvsub", "bvmul", "bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod", "bvand", "bvor", "bvxor",
         "bvshl", "bvlshr", "bvashr", "bvumin", "bvumax", "bvsmin", "bvsmax", "bvrsub"]
PREDS = CMPS + ["bvadd_noovfl_u", "bvumul_noovfl", "bvsub_noudfl_u"]
BOOLS = ["and", "or", "xor", "implies"]
ONE_OPERAND = {"copy", "bvnot", "bvneg", "not", "extract", "zero_extend", "sign_extend"}


# ------------------------------------------------------------------ expressions
def _expr_op(op, width, args, w2, w3):
    a = args[0]
    b = args[1] if len(args) > 1 else None
    if op == "copy":
        return a
    if op == "zero_extend":
        return Node("zero_extend", width, (a,), width - a.width)
    if op == "sign_extend":
        assert a.width == w2
        return Node("sign_extend", width, (a,), width - a.width)
    if op == "extract":
        return Node("extract", width, (a,), (w2 + width - 1, w2))
    if op in ("bvnot", "bvneg", "not"):
        return Node(op, width, (a,))
    if op == "ite":
        return Node("ite", width, tuple(args))
    if op == "bvumin":
        return Node("ite", width, (Node("bvugt", 1, (a, b)), b, a))
    if op == "bvumax":
        return Node("ite", width, (Node("bvult", 1, (a, b)), b, a))
    if op == "bvsmin":
        return Node("ite", width, (Node("bvsgt", 1, (a, b)), b, a))
    if op == "bvsmax":
        return Node("ite", width, (Node("bvslt", 1, (a, b)), b, a))
    if op == "bvrsub":
        return Node("bvsub", width, (b, a))
    if op == "rconcat":
        assert a.width == w3
        return Node("concat", width, (b, a))
    if op == "concat":
        assert b.width == w3
        return Node("concat", width, (a, b))
    if op in PREDS:
        assert a.width == b.width == w3, (op, a.width, b.width, w3)
    return Node(op, width, (a, b))


def program_expr(rows, var_nodes, const_nodes):
    """The expression a program computes (instructions interpreted over nodes), or
    None when it uses ``tab``."""
    acc, slots = const_node(0, 256), {}

    def operand(r):
        kind, idx = r >> 30, r & 0x3FFFFFFF
        return acc if kind == REF_ACC else slots[idx] if kind == REF_SLOT else \
            var_nodes[idx] if kind == REF_VAR else const_nodes[idx]

    for w0, w1, w2, w3 in rows:
        op, width = OPS[w0 & 0xFF], (w0 >> 8) & 0x1FF
        if op == "tab":
            return None
        n = 3 if op == "ite" else 1 if op in ONE_OPERAND else 2
        acc = _expr_op(op, width, [operand(r) for r in (w1, w2, w3)[:n]], w2, w3)
        if (w0 >> 17) & 1:
            slots[(w0 >> 18) & 0xF] = acc
    return acc


# ------------------------------------------------------------------------ groups
@dataclass
class Group:
    name: str
    prog: ProgramBatch
    models: list
    labels: list
    exprs: list
    const_widths: list = field(default_factory=list)
    waves: list = field(default_factory=list)      # division groups: (class name, first model)
    div_pairs: list = field(default_factory=list)  # division groups: the (dividend, divisor) the divider sees

    def pool(self):
        return ModelPool.from_dicts(self.models, self.prog.var_names, self.prog.var_widths, self.prog.tables)

    def describe(self, d, m):
        """Program d's label and the model's values of the variables it reads."""
        read = set()
        for w0, *words in self.prog.program(d).tolist():
            op = OPS[w0 & 0xFF]
            for r in words[:3 if op == "ite" else 1 if op in ONE_OPERAND else 2]:
                if r >> 30 == REF_VAR:
                    read.add(self.prog.var_names[r & 0x3FFFFFFF])
        vals = {n: hex(self.models[m].get(n, 0)) for n in self.prog.var_names
                if n in read and isinstance(self.models[m].get(n, 0), int)}
        return f"{self.name}: program {d} [{self.labels[d]}] model {m} {vals}"


class Builder:
    def __init__(self, name, n_slots=4, tables=()):
        self.name, self.n_slots, self.tables = name, n_slots, list(tables)
        self.var_names, self.var_widths, self._vars = [], [], {}
        self._consts, self.const_vals, self.const_widths = {}, [], []
        self.rows, self.off, self.labels = [], [0], []

    def v(self, name, width):
        if name not in self._vars:
            self._vars[name] = len(self.var_names)
            self.var_names.append(name)
            self.var_widths.append(width)
        assert self.var_widths[self._vars[name]] == width, name
        return ref(REF_VAR, self._vars[name])

    def k(self, value, width=256):
        key = (value, width)
        if key not in self._consts:
            self._consts[key] = len(self.const_vals)
            self.const_vals.append(value)
            self.const_widths.append(width)
        return ref(REF_CONST, self._consts[key])

    def add(self, label, rows):
        assert rows
        self.rows += [list(map(int, r)) for r in rows]
        self.off.append(len(self.rows))
        self.labels.append(label)

    def group(self, models, with_exprs=True, **kw):
        consts = np.array([limbs(c) for c in self.const_vals] or [limbs(0)], dtype=np.uint32)
        prog = ProgramBatch(np.asarray(self.rows, dtype=np.uint32), np.asarray(self.off, dtype=np.uint32), consts,
                            self.n_slots, list(self.var_names), list(self.var_widths), list(self.tables))
        exprs = [None] * prog.n_dags
        if with_exprs:
            vn = [var_node(n, w) for n, w in zip(self.var_names, self.var_widths)]
            cn = [const_node(c, w) for c, w in zip(self.const_vals, self.const_widths)] or [const_node(0, 256)]
            exprs = [program_expr(self.rows[self.off[d]:self.off[d + 1]], vn, cn) for d in range(prog.n_dags)]
        return Group(self.name, prog, models, self.labels, exprs, list(self.const_widths), **kw)


def I(op, width, a, b=0, c=0, store=None):
    return [enc_w0(op, width, store), a, b, c]


def place(b, specs):
    """specs: (kind, source, width, slot) per operand, kind 'var' / 'slot' / 'acc'
    (source = a variable's name) or 'const' (source = the value).  Returns (the
    instructions that set the operands up, the operand references).  Slot
    copies come first, the accumulator's copy last."""
    pre_slots, pre_acc, refs = [], [], []
    for kind, src, w, slot in specs:
        if kind == "const":
            refs.append(b.k(src, w))
        elif kind == "var":
            refs.append(b.v(src, w))
        elif kind == "slot":
            pre_slots.append(I("copy", w, b.v(src, w), store=slot))
            refs.append(ref(REF_SLOT, slot))
        else:
            pre_acc.append(I("copy", w, b.v(src, w)))
            refs.append(ACC)
    assert len(pre_acc) <= 1
    return pre_slots + pre_acc, refs


# ------------------------------------------------------------------ operand values
def operand_values(w, rng):
    """14 values of width w: the edges 0, 1, 2, 2^(w-1) - 1, 2^(w-1), 2^(w-1) + 1,
    2^w - 2, 2^w - 1, alternating all-ones / zero limbs (both phases), and seeded
    random values of several lengths."""
    M, h = mask(w), 1 << (w - 1)
    alt = sum(0xFFFFFFFF << (64 * i) for i in range(4))
    vals = [0, 1, 2, h - 1, h, h + 1, M - 1, M, alt, alt << 32, rng.getrandbits(w),
            rng.getrandbits(w // 2 + 1), rng.getrandbits(min(w, 33)), rng.getrandbits(w) | h]
    return [v & M for v in vals]


N_VALUES = 14
CONCAT_SPLITS = [(256, 1), (256, 31), (256, 32), (256, 33), (256, 128), (256, 255),      # (total, low width)
                 (8, 3), (33, 1), (64, 31), (65, 32), (65, 33)]
PART_WIDTHS = sorted({t - l for t, l in CONCAT_SPLITS} | {l for t, l in CONCAT_SPLITS} | {28, 100, 224})
ALL_WIDTHS = sorted(set(WIDTHS) | set(PART_WIDTHS))


@functools.lru_cache(maxsize=None)
def crossed_models():
    """196 models: per width w the variables a{w}, b{w} take every pair of
    operand_values(w); c1 is a Boolean independent of both."""
    rng = random.Random(2024)
    vals = {w: operand_values(w, rng) for w in ALL_WIDTHS}
    models = []
    for i in range(N_VALUES):
        for j in range(N_VALUES):
            m = {"c1": (i * 3 + j * 5 + (i * j) // 3) & 1}
            for w in ALL_WIDTHS:
                m[f"a{w}"], m[f"b{w}"] = vals[w][i], vals[w][j]
            models.append(m)
    return models, vals


def const_values(w):
    """Two constants per width for the constant operand kind."""
    rng = random.Random(7000 + w)
    return sorted({(rng.getrandbits(w) | 1) & mask(w), 1 << (w - 1)})


AB_KINDS = [("var", "var"), ("slot", "var"), ("const", "var"), ("acc", "var"), ("var", "slot"), ("var", "const"),
            ("acc", "const"), ("slot", "slot")]
A_KINDS = ["var", "slot", "const", "acc"]


def _binary_programs(b, op, width, wa, wb, w3=0, tag=""):
    """op at result width `width` on a{wa}, b{wb} for every operand-kind pair."""
    for ka, kb in AB_KINDS:
        for ca in (const_values(wa) if ka == "const" else [f"a{wa}"]):
            for cb in (const_values(wb)[:1 if ka == "acc" else 2] if kb == "const" else [f"b{wb}"]):
                pre, (ra, rb) = place(b, [(ka, ca, wa, 0), (kb, cb, wb, 1)])
                b.add(f"{op} w={width}{tag} A={ka} B={kb}", pre + [I(op, width, ra, rb, w3)])


@functools.lru_cache(maxsize=None)
def op_groups():
    """One group per op: the op at every width of WIDTHS and every operand kind,
    over the crossed models."""
    models, _ = crossed_models()
    out = {}

    def done(b):
        out[b.name] = b.group(models)

    for op in ARITH:
        b = Builder(f"op:{op}")
        for w in WIDTHS:
            _binary_programs(b, op, w, w, w)
        done(b)
    for op in PREDS:
        b = Builder(f"op:{op}")
        for w in WIDTHS:
            _binary_programs(b, op, 1, w, w, w3=w)
        done(b)
    for op in BOOLS:
        b = Builder(f"op:{op}")
        _binary_programs(b, op, 1, 1, 1)
        done(b)
    for op in ("copy", "bvnot", "bvneg", "not"):
        b = Builder(f"op:{op}")
        for w in ([1] if op == "not" else WIDTHS):
            for ka in A_KINDS:
                for ca in (const_values(w) if ka == "const" else [f"a{w}"]):
                    pre, (ra,) = place(b, [(ka, ca, w, 0)])
                    b.add(f"{op} w={w} A={ka}", pre + [I(op, w, ra)])
        done(b)
    # extensions: source widths on both sides of each limb edge, results one bit wider,
    # up to the next limb edge and 256
    for op in ("zero_extend", "sign_extend"):
        b = Builder(f"op:{op}")
        for ws in WIDTHS:
            for w in sorted({min(256, ws + 1), min(256, (ws // 32 + 1) * 32), min(256, ws + 33), 256}):
                for ka in A_KINDS:
                    for ca in (const_values(ws) if ka == "const" else [f"a{ws}"]):
                        pre, (ra,) = place(b, [(ka, ca, ws, 0)])
                        b.add(f"{op} {ws}->{w} A={ka}", pre + [I(op, w, ra, ws if op == "sign_extend" else 0)])
        done(b)
    b = Builder("op:extract")
    for w in WIDTHS:
        for lo in sorted({x for x in (0, 1, 31, 32, 33, 255 - w, 256 - w) if 0 <= x <= 256 - w}):
            for ka in A_KINDS:
                for ca in (const_values(256) if ka == "const" else ["a256"]):
                    pre, (ra,) = place(b, [(ka, ca, 256, 0)])
                    b.add(f"extract w={w} lo={lo} A={ka}", pre + [I("extract", w, ra, lo)])
    done(b)
    for op in ("concat", "rconcat"):
        b = Builder(f"op:{op}")
        for total, low in CONCAT_SPLITS:
            # concat: A high, B low, w3 = width of B; rconcat: A low, B high, w3 = width of A
            wa, wb = (total - low, low) if op == "concat" else (low, total - low)
            _binary_programs(b, op, total, wa, wb, w3=low, tag=f" low={low}")
        done(b)
    b = Builder("op:ite")
    branch_kinds = [("var", "var"), ("slot", "const"), ("const", "slot"), ("var", "slot"), ("slot", "var"),
                    ("const", "var"), ("var", "const")]
    for w in WIDTHS:
        for kc in A_KINDS:
            for kt, ke in (branch_kinds if kc == "var" else branch_kinds[:3]):
                for cc in ([0, 1] if kc == "const" else ["c1"]):
                    pre, (rc, rt, re) = place(b, [(kc, cc, 1, 0), (kt, const_values(w)[0] if kt == "const" else f"a{w}", w, 1),
                                                  (ke, const_values(w)[-1] if ke == "const" else f"b{w}", w, 2)])
                    b.add(f"ite w={w} C={kc} T={kt} E={ke}", pre + [I("ite", w, rc, rt, re)])
    done(b)
    # the two branches of bvadd_noovfl_u on rc >= 256, with sums 2^w - 1 and 2^w; and
    # bvumul_noovfl at (A, floor((2^w - 1) / A)) and one more, with A = 0 and B = 0
    for op in ("bvadd_noovfl_u", "bvumul_noovfl"):
        b = Builder(f"edge:{op}")
        ms = []
        rng = random.Random(91)
        for w in (255, 256, 64):
            _binary_programs(b, op, 1, w, w, w3=w)
        for k in range(192):
            m = {}
            for w in (255, 256, 64):
                M = mask(w)
                x = [rng.getrandbits(w), rng.getrandbits(w // 2), M, 1, 0, rng.getrandbits(rng.randint(1, w))][k % 6]
                if op == "bvadd_noovfl_u":
                    y = [M - x, min(M, M - x + 1), rng.getrandbits(w), 0][(k // 6) % 4]
                else:
                    y = [M // x if x else M, min(M, M // x + 1) if x else 0, rng.getrandbits(w // 2), 0][(k // 6) % 4]
                m[f"a{w}"], m[f"b{w}"] = (x, y) if (k // 24) % 2 == 0 else (y, x)
            ms.append(m)
        out[b.name] = b.group(ms)
    return out


# ------------------------------------------------------------------------ shifts
def shift_amounts(w):
    """0, 1, 31, 32, 33, w-1, w, w+1, 255, 256, 2^32, 2^32 + 1 (a small low limb
    under a set higher limb), 2^255 -- those that fit a w-bit operand."""
    return sorted({x for x in (0, 1, 31, 32, 33, w - 1, w, w + 1, 255, 256, 1 << 32, (1 << 32) + 1, 1 << 255)
                   if x <= mask(w)})


@functools.lru_cache(maxsize=None)
def shift_groups():
    """Per shift op: each amount once as a constant (the wave-uniform path, one
    program per amount) and once as the variable s{w} whose amounts differ from lane
    to lane within every wave."""
    _, vals = crossed_models()
    amounts = {w: shift_amounts(w) for w in WIDTHS}
    n = N_VALUES * max(len(a) for a in amounts.values())
    models = []
    for m in range(n):
        d = {}
        for w in WIDTHS:
            d[f"a{w}"] = vals[w][m % N_VALUES]
            d[f"s{w}"] = amounts[w][(m // N_VALUES + m) % len(amounts[w])]
        models.append(d)
    # every (value, amount) pair occurs: m -> (m % 14, (m // 14 + m) % len) is onto for the 14 * len models
    out = {}
    for op in ("bvshl", "bvlshr", "bvashr"):
        b = Builder(f"shift:{op}")
        for w in WIDTHS:
            for amt in amounts[w]:
                for ka in ("var", "acc"):
                    pre, (ra, rb) = place(b, [(ka, f"a{w}", w, 0), ("const", amt, w, 1)])
                    b.add(f"{op} w={w} by const {amt:#x} A={ka}", pre + [I(op, w, ra, rb)])
            for ka, kb in (("var", "var"), ("acc", "var"), ("var", "slot"), ("slot", "slot")):
                pre, (ra, rb) = place(b, [(ka, f"a{w}", w, 0), (kb, f"s{w}", w, 1)])
                b.add(f"{op} w={w} by variable A={ka} B={kb}", pre + [I(op, w, ra, rb)])
        out[b.name] = b.group(models)
    return out


# ------------------------------------------------------------------------ fusion
def _tail_operand(b, k):
    return [b.v("b256", 256), b.k(0x0123456789ABCDEF << 96), ref(REF_SLOT, 0), b.v("a256", 256),
            b.k(mask(256))][k % 5]


@functools.lru_cache(maxsize=None)
def fusion_groups():
    """The shapes bv_fuse rewrites (run with the default upload and MG_BV_FUSE=0):
    tails after 256-bit and narrow heads, chains of 2..5 simple ops, comparison ->
    and (stored and unstored), extract -> rconcat."""
    models, _ = crossed_models()
    out = {}
    slot0 = lambda b: I("copy", 256, b.v("b255", 255), store=0)
    # (a) heads: every op with a 256-bit result, then 1..3 simple ops on the accumulator
    heads = [(op, 256, 0, 0) for op in ARITH] + [("bvnot", 256, 0, 0), ("bvneg", 256, 0, 0), ("copy", 256, 0, 0),
             ("sign_extend", 256, 255, 0), ("extract", 256, 0, 0), ("concat", 256, 0, 128), ("rconcat", 256, 0, 33),
             ("ite", 256, 0, 0)]
    narrow = [(op, w, 0, 0) for w in (8, 64, 255) for op in ("bvadd", "bvsub", "bvmul", "bvnot", "bvneg", "bvshl", "bvsdiv",
                                                              "bvsrem", "bvashr", "bvrsub", "bvudiv", "bvsmin")]
    narrow += [("sign_extend", 200, 64, 0), ("concat", 96, 0, 64), ("extract", 100, 33, 0), ("bvult", 1, 0, 64)]
    b = Builder("fuse:tails")
    k = 0
    for op, w, w2, w3 in heads + narrow:
        for n_tail in (1, 2, 3):
            for stored in (False, True):
                k += 1
                if op in ("concat", "rconcat"):
                    wa, wb = (w - w3, w3) if op == "concat" else (w3, w - w3)
                elif op == "sign_extend":
                    wa = wb = w2
                elif op == "extract":
                    wa = wb = 256
                elif op == "bvult":
                    wa = wb = w3
                else:
                    wa = wb = w
                rows = [slot0(b)]
                if op == "ite":
                    head = I("ite", w, b.v("c1", 1), b.v("a256", 256), b.v("b256", 256))
                elif op in ONE_OPERAND:
                    head = I(op, w, b.v(f"a{wa}", wa), w2)
                else:
                    if k % 3 == 0:      # operand A in the accumulator
                        rows.append(I("copy", wa, b.v(f"a{wa}", wa)))
                    head = I(op, w, ACC if k % 3 == 0 else b.v(f"a{wa}", wa), b.v(f"b{wb}", wb), w3)
                if stored:              # a stored head must stay unfused; its slot is read back at the end
                    head[0] |= (1 << 17) | (3 << 18)
                rows.append(head)
                for t in range(n_tail):
                    rows.append(I(SIMPLE[(k + 2 * t) % 9], 256, ACC, _tail_operand(b, k + t)))
                if stored:
                    rows.append(I("bvxor", 256, ACC, ref(REF_SLOT, 3)))
                else:                   # the last tail stores; the slot is read back after the accumulator moved on
                    rows[-1][0] |= (1 << 17) | (2 << 18)
                    rows += [I("copy", 8, b.v("a8", 8)), I("copy", 256, ref(REF_SLOT, 2))]
                b.add(f"{op} w={w} + {n_tail} tail ops{' (head stored)' if stored else ''}", rows)
    out[b.name] = b.group(models)
    # (b) chains of 2, 3, 4, 5 (must split) and 7 simple ops, every op in every position
    b = Builder("fuse:chains")
    for length in (2, 3, 4, 5, 7):
        for rot in range(9):
            for store_at in (None, 1):
                rows = [slot0(b), I(SIMPLE[rot], 256, b.v("a256", 256), b.v("b256", 256))]
                for t in range(1, length):
                    rows.append(I(SIMPLE[(rot + 4 * t) % 9], 256, ACC, _tail_operand(b, rot + t)))
                if store_at is not None and length > 2:      # a store in mid-chain ends the fused run there
                    rows[1 + store_at][0] |= (1 << 17) | (1 << 18)
                    rows.append(I("bvadd", 256, ACC, ref(REF_SLOT, 1)))
                b.add(f"chain of {length} from {SIMPLE[rot]}{' stored mid-chain' if store_at is not None else ''}", rows)
    out[b.name] = b.group(models)
    # (c) comparison -> and with a slot, stored (stays unfused) and unstored
    b = Builder("fuse:cmp_and")
    for cmp in CMPS:
        for w in (1, 8, 64, 255, 256):
            for stored in (False, True):
                for ka in ("var", "acc"):
                    rows = [I("copy", 1, b.v("c1", 1), store=1)]
                    if ka == "acc":
                        rows.append(I("copy", w, b.v(f"a{w}", w)))
                    rows.append(I(cmp, 1, ACC if ka == "acc" else b.v(f"a{w}", w), b.v(f"b{w}", w), w,
                                  store=2 if stored else None))
                    rows.append(I("and", 1, ACC, ref(REF_SLOT, 1)))
                    if stored:
                        rows.append(I("xor", 1, ACC, ref(REF_SLOT, 2)))
                    b.add(f"{cmp} w={w} A={ka} -> and{' (comparison stored)' if stored else ''}", rows)
    out[b.name] = b.group(models)
    # (d) extract -> rconcat, including a total of 256
    b = Builder("fuse:ext_rcat")
    # (the last three: a high part wider than the total leaves room for -- the result is cut to its width)
    for ew, hw, lo, total in ((128, 128, 0, 256), (128, 128, 128, 256), (1, 255, 255, 256), (255, 1, 1, 256),
                              (100, 28, 50, 128), (8, 8, 31, 16), (32, 224, 33, 256), (33, 31, 223, 64), (31, 33, 32, 64),
                              (1, 1, 0, 2), (64, 256, 7, 200), (128, 255, 100, 256), (8, 64, 0, 33)):
        for stored in (False, True):
            rows = [I("copy", hw, b.v(f"b{hw}", hw), store=3),
                    I("extract", ew, b.v("a256", 256), lo, store=2 if stored else None),
                    I("rconcat", total, ACC, ref(REF_SLOT, 3), ew)]
            if stored:
                rows.append(I("bvxor", 256, ACC, ref(REF_SLOT, 2)))
            b.add(f"extract w={ew} lo={lo} -> rconcat of {hw} high bits, total {total}"
                  f"{' (extract stored)' if stored else ''}", rows)
    out[b.name] = b.group(models)
    return out


# ------------------------------------------------------------------ slots, tables
@functools.lru_cache(maxsize=None)
def slot_groups():
    """n_slots = 1, 8, 9, 16 (dynamic LDS passes 64 KiB between 8 and 9): every slot
    written with a distinct per-model value, each read back by its own program."""
    rng = random.Random(16)
    models = [{"x": rng.getrandbits(256), "y": rng.getrandbits(64)} for _ in range(300)]
    out = {}
    for n in (1, 8, 9, 16):
        b = Builder(f"slots:{n}", n_slots=n)
        for j in range(n):
            rows = [I(("bvadd", "bvxor", "bvmul")[s % 3], 256, b.v("x", 256), b.k((s + 2) * 0x9E3779B97F4A7C15), store=s)
                    for s in range(n)]
            rows.append(I("copy", 64, b.v("y", 64)))
            rows.append(I("copy", 256, ref(REF_SLOT, j)))
            b.add(f"n_slots={n}: read slot {j}", rows)
        out[b.name] = b.group(models)
    return out


@functools.lru_cache(maxsize=None)
def table_group():
    """``tab`` on the tables of test_smt_programs._random_table_constraints (Storage, calldata,
    keccak256_512 and its inverse, keccak256_256, Power) at part 0 and 1 and lo 0, 8, 248."""
    from mythril_amd.smt.lower import TableSig
    from test_smt_programs import _random_table_models
    sigs = [TableSig("Storage", "array", (256,), 256), TableSig("calldata", "array", (256,), 8),
            TableSig("keccak256_512", "uf", (512,), 256), TableSig("keccak256_512-1", "uf", (256,), 512),
            TableSig("keccak256_256", "uf", (256,), 256), TableSig("Power", "uf", (256, 256), 256)]
    b = Builder("tables", tables=sigs)
    x, y, s, zero, two = b.v("x", 256), b.v("y", 256), b.v("slot", 256), b.k(0), b.k(2)
    keys = {0: [(x, zero), (s, zero), (b.k(1), zero)], 1: [(y, zero), (zero, zero)], 2: [(s, x), (zero, y)],
            3: [(b.v("h", 256), zero), (x, zero)], 4: [(y, zero), (x, zero)], 5: [(two, y), (y, two)]}
    for t, sig in enumerate(sigs):
        for part in ((0, 1) if sig.range > 256 else (0,)):
            for lo, w in ((0, 256), (0, 8), (8, 8), (248, 8), (8, 248), (0, 1), (255, 1), (31, 33)):
                for ka, (k0, k1) in enumerate(keys[t]):
                    imm = t | (part << TAB_PART_SHIFT) | (lo << TAB_LO_SHIFT)
                    rows = [I("copy", 256, k0), I("tab", w, ACC, k1, imm)] if ka == 0 else [I("tab", w, k0, k1, imm)]
                    b.add(f"tab {sig.name} part={part} lo={lo} w={w} key {ka}", rows)
    models = _random_table_models(random.Random(11), 200, None)
    for m in models:      # h: often a key of the inverse's interpretation
        inv = m.get("keccak256_512-1")
        m["h"] = next(iter(inv.entries))[0] if inv is not None and random.Random(m["x"]).random() < 0.8 else m["y"]
    return b.group(models, with_exprs=False)


# ------------------------------------------------------------ division, by wave
def _bits(rng, n):
    """A random value of exactly n bits (0 for n = 0)."""
    return (rng.getrandbits(n) | (1 << (n - 1))) if n > 0 else 0


def _nonpow2(rng, n):
    """Exactly n bits (n >= 2), not a power of two."""
    x = _bits(rng, n)
    return x | 1 if x & (x - 1) == 0 else x


def tie_pair(rng, w):
    """A pair whose second quotient digit is estimated from a remainder that shares
    the divisor's top limb (qhat = 2^32 - 1), when w allows it."""
    if w < 70:
        lb = rng.randint(max(2, w - 40), max(2, w - 33)) if w > 36 else 2
    else:
        lb = rng.randint(34, w - 33)
    b = _nonpow2(rng, lb)
    low = b & mask(max(lb - 32, 0))
    t = rng.randint(1, max(1, low)) if low else 1
    q1 = rng.randint(0, 3)
    a = (((q1 * b + b - t) << 32) | rng.getrandbits(32)) & mask(w)
    return a, b


def addback_pair(rng, w):
    """Divisors with a top limb of 0x80000000 over a zero limb and all-ones below
    (the estimate ignores what lies under the second limb), dividends just below a
    multiple: where add-backs come from."""
    k = rng.randint(3, max(3, w // 32))
    b = (((1 << 31) << (32 * (k - 1))) | mask(32 * (k - 2))) >> rng.choice([0, 0, 1, 7])
    b &= mask(w)
    if b < 2:
        b = 3
    q = rng.getrandbits(max(1, w - b.bit_length())) | rng.choice([0, 0xFFFFFFFF])
    a = (q * b + rng.choice([0, 1, b - 1, b >> 1])) & mask(w)
    return a, b


def wave_classes(w, rng):
    """[(class name, 64 (dividend, divisor) pairs below 2^w)]: waves homogeneous in one
    class of the wave-uniform shortcuts of kernel 2's division (u_divmod_nz_t<true>),
    each followed by the same wave with a single lane of another class."""
    out = []
    full = lambda: (_bits(rng, w), _nonpow2(rng, rng.randint(2, w)))

    def wave(name, gen, other=None):
        lanes = [gen() for _ in range(WAVE)]
        out.append((name, lanes))
        if other is not None:
            mixed = list(lanes)
            mixed[rng.randrange(WAVE)] = other()
            out.append((name + " +1 lane", mixed))

    def short():
        lb = rng.randint(2, w)
        return rng.getrandbits(lb - 1), _nonpow2(rng, lb)

    def long_divisor():
        lb = rng.choice([w, rng.randint(max(2, w - 31), w)])
        return _bits(rng, rng.randint(lb, w)), _nonpow2(rng, lb)

    def dl_class(k):
        def g():
            dl = rng.randint(32 * k, min(32 * k + 31, w - 2))
            lb = rng.randint(2, w - dl)
            return _bits(rng, lb + dl), _nonpow2(rng, lb)
        return g

    def shift_class(q):        # normalisation shift s = 256 - bitlen(b) with s >> 5 == q
        def g():
            lb = rng.randint(max(2, 256 - 32 * q - 31), min(w, 256 - 32 * q))
            return _bits(rng, rng.randint(lb, w)), _nonpow2(rng, lb)
        return g

    wave("divisor a power of two", lambda: (rng.getrandbits(w), 1 << rng.randrange(w)), full)
    wave("bitlen(a) < bitlen(b)", short, full)
    wave("long divisor", long_divisor, lambda: (_bits(rng, w), _nonpow2(rng, max(2, w // 3))))
    ks = [k for k in range(8) if 32 * k <= w - 2]
    for k in ks:
        wave(f"dl in [{32 * k}, {32 * k + 32})", dl_class(k), dl_class(ks[(ks.index(k) + 1 + len(ks) // 2) % len(ks)])
             if len(ks) > 1 else short)
    qs = [q for q in range(8) if max(2, 256 - 32 * q - 31) <= min(w, 256 - 32 * q)]
    for q in qs:
        wave(f"shift limbs {q}", shift_class(q), shift_class(qs[(qs.index(q) + 1) % len(qs)]) if len(qs) > 1 else short)
    wave("shift limbs mixed", lambda: shift_class(rng.choice(qs))())
    wave("divisor zero", lambda: (rng.getrandbits(w), 0))
    wave("one non-zero divisor among zeros", lambda: (rng.getrandbits(w), 0), full)
    wave("one zero divisor", full, lambda: (rng.getrandbits(w), 0))
    for n in range(4):
        wave(f"division_operand {n}", lambda: (division_operand(rng) & mask(w), division_operand(rng) & mask(w)))
    wave("top-limb ties", lambda: tie_pair(rng, w))
    wave("add-back forms", lambda: addback_pair(rng, w))
    return out


def event_waves(w, rng, tries=3000, want=32):
    """Waves of pairs the digit model (k2_insn_ref.knuth_events) shows to meet each
    event, found by a seeded directed search below 2^w."""
    found = {e: [] for e in EVENTS}
    gens = [lambda: (division_operand(rng) & mask(w), division_operand(rng) & mask(w)),
            lambda: tie_pair(rng, w), lambda: addback_pair(rng, w)]
    for k in range(tries):
        a, b = gens[k % 3]()
        if b == 0 or b & (b - 1) == 0:
            continue
        for e in knuth_events(a, b):
            if len(found[e]) < want:
                found[e].append((a, b))
    out = []
    for e in EVENTS:
        if found[e]:
            out.append((f"event {e}", [found[e][k % len(found[e])] for k in range(WAVE)]))
    return out


def _div_models(waves, to_model):
    models, starts = [], []
    for name, lanes in waves:
        starts.append((name, len(models)))
        models += [to_model(a, b, k) for k, (a, b) in enumerate(lanes)]
    return models, starts


@functools.lru_cache(maxsize=None)
def division_groups():
    """bvudiv / bvurem at width 256, 255, 64 and 8; bvsdiv / bvsrem / bvsmod over the
    four sign combinations of the same magnitudes (with MIN / -1 and MIN / 1);
    bvumul_noovfl at 256, 255 and 64: pools laid out wave by wave (a wave = 64
    consecutive models)."""
    out = {}
    for w in (256, 255, 64, 8):
        rng = random.Random(500 + w)
        waves = wave_classes(w, rng) + event_waves(w, rng)
        b = Builder(f"div:unsigned w={w}")
        for op in ("bvudiv", "bvurem"):
            b.add(f"{op} w={w} A=var B=var", [I(op, w, b.v("a", w), b.v("b", w))])
            b.add(f"{op} w={w} A=acc B=var", [I("copy", w, b.v("a", w)), I(op, w, ACC, b.v("b", w))])
        models, starts = _div_models(waves, lambda a, bb, k: {"a": a, "b": bb})
        out[b.name] = b.group(models, waves=starts, div_pairs=[p for _, lanes in waves for p in lanes])
    for w in (256, 255, 64, 8):
        rng = random.Random(900 + w)
        M, MIN = mask(w), 1 << (w - 1)
        mags = wave_classes(w - 1, rng) + event_waves(w - 1, rng)
        waves = []
        for name, lanes in mags:
            for sa, sb in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                waves.append((f"{name} signs {sa:+d}/{sb:+d}", [((sa * a) & M, (sb * bb) & M) for a, bb in lanes]))
        special = [(MIN, M), (MIN, 1), (MIN, MIN), (M, MIN), (MIN, 0), (0, MIN), (MIN, 2), (MIN + 1, M), (1, M), (0, 0)]
        waves.append(("MIN and -1", [special[k % len(special)] for k in range(WAVE)]))
        b = Builder(f"div:signed w={w}")
        for op in ("bvsdiv", "bvsrem", "bvsmod"):
            b.add(f"{op} w={w} A=var B=var", [I(op, w, b.v("a", w), b.v("b", w))])
        models, starts = _div_models(waves, lambda a, bb, k: {"a": a, "b": bb})
        pairs = [(min(a, (-a) & M) if a != MIN else MIN, min(bb, (-bb) & M) if bb != MIN else MIN)
                 for _, lanes in waves for a, bb in lanes]
        out[b.name] = b.group(models, waves=starts, div_pairs=pairs)
    for w in (256, 255, 64):
        rng = random.Random(1300 + w)
        M = mask(w)
        waves = wave_classes(w, rng)
        b = Builder(f"div:umul_noovfl w={w}")
        b.add(f"bvumul_noovfl w={w} A=var B=var", [I("bvumul_noovfl", 1, b.v("a", w), b.v("b", w), w)])
        b.add(f"bvumul_noovfl w={w} A=acc B=var", [I("copy", w, b.v("a", w)), I("bvumul_noovfl", 1, ACC, b.v("b", w), w)])

        def to_model(_, x, k):      # the divider sees (2^w - 1) / A: A takes the classes' divisors
            y = [M // x if x else M, min(M, M // x + 1) if x else 0, rng.getrandbits(w), 0, M][k % 5]
            return {"a": x, "b": y}
        models, starts = _div_models(waves, to_model)
        out[b.name] = b.group(models, waves=starts, div_pairs=[(M, m["a"]) for m in models])
    return out


# --------------------------------------------------------------------- everything
def all_groups():
    out = {}
    for part in (op_groups(), shift_groups(), fusion_groups(), slot_groups(), {"tables": table_group()},
                 division_groups()):
        out.update(part)
    return out


def group_names(prefix=""):
    return [n for n in all_groups() if n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def reference_ints(name):
    """values[d][m] of a group by k2_insn_ref, computed once per process."""
    g = all_groups()[name]
    return values(g.prog, g.models)


@functools.lru_cache(maxsize=None)
def reference_limbs(name):
    """The same as uint32[n_dags, n_models, 8] (read-only)."""
    ints = reference_ints(name)
    raw = b"".join(v.to_bytes(32, "little") for row in ints for v in row)
    out = np.frombuffer(raw, dtype="<u4").reshape(len(ints), len(ints[0]), 8).astype(np.uint32)
    out.setflags(write=False)
    return out


def event_counts(pairs):
    """How many (dividend, divisor) pairs meet each Knuth event (power-of-two and zero
    divisors never reach the digit loop)."""
    counts = dict.fromkeys(EVENTS, 0)
    for a, b in pairs:
        if b and b & (b - 1):
            for e in knuth_events(a, b):
                counts[e] += 1
    return counts
