"""Kernel 2's case table (tests/k2_opcases.py) as the reference of the exact
procedure (mythril_amd/smt/exact.py, libmythsmt.so).  Test-only; seeded and
deterministic; never imported by ``mythril_amd``.

* ``sort_error`` states the sort rules of include/mythsmt.h in Python.  The
  expression of a mixed-width kernel-2 program (k2_opcases.program_expr) may
  break them -- kernel 2 masks, the blaster must reject --, so it splits every
  group into well-sorted programs (sampled below) and ill-sorted ones
  (``ill_sorted_programs``, rows of the rejection table, ``ill_sorted_rows``).
* ``cases(name)``: per group the sampled points ``Case(e, pins, v)``: the
  expression of program d, the values model m gives the variables it reads, and
  the reference value ``k2_opcases.reference_ints(name)[d][m]`` (k2_insn_ref:
  pinned against the C oracle, smt_eval and the device elsewhere; nothing the
  exact procedure computes).  About 60 points (30 programs, two models each: in
  a session one blast of e then serves both) per op:*, edge:*, shift:*,
  fuse:cmp_and and slots:* group, every well-sorted program of the other fuse:*
  groups once, and the samples of SAMPLE for the division groups.  Programs are
  drawn round-robin over their widest node's width, so every width of
  k2_opcases.WIDTHS occurs.
* General division (bvudiv, bvurem, bvsdiv, bvsrem, bvsmod by a divisor that
  is not 0, 1 or a power of two) is taken only at widths <= 65: the divider
  is stated as a = q * b + r, so a pinned point is a search for q.  Measured on
  the development host: 24 pinned 64-bit points 0.9 - 2.1 s together, at most
  2,400 conflicts a point; eight pinned 256-bit points 0 - 21,000 conflicts and
  0.0 - 30 s each (the issue that asked for this table reports 4.7k - 97k
  conflicts, some over the 50,000-conflict budget: "unknown").  So a program
  with a division node wider than 65 bits is left out here
  (``wide_division``), in every group (18 of fuse:tails' programs), and the
  groups div:unsigned / div:signed w=256 and w=255 entirely.  In their place
  ``wide_division_group`` pins, at 255 and 256 bits, the divisors the blaster
  decides without the divider: 0, 1, powers of two and, for the signed
  operators, -1 and the most negative dividend and divisor.
"""
import functools
import random
from collections import namedtuple

import k2_opcases as K
from k2_insn_ref import mask, values
from mythril_amd.smt.expr import Node, const, var

Case = namedtuple("Case", "group d m e pins v label")     # pins: {(name, width): value}

DIVS = ("bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod")
DIV_MAX_WIDTH = 65
WORD_OPS = {"bvadd", "bvsub", "bvmul", "bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod", "bvand", "bvor", "bvxor",
            "bvshl", "bvlshr", "bvashr"}
COMPARISONS = {"eq", "distinct", "bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge",
               "bvadd_noovfl_u", "bvumul_noovfl", "bvsub_noudfl_u"}
ARRAY_SORTED = {"array", "K", "store"}


# ------------------------------------------------------------------- the sorts
def _node_error(n, signatures):
    """The rule node n breaks (its operands taken as they declare themselves), or None."""
    op, w, na = n.op, n.width, len(n.args)
    aw = [a.width for a in n.args]
    words = lambda count, width: na == count and width >= 1 and all(x == width for x in aw)
    if op in ("const", "var"):
        return None if na == 0 and w >= 1 else "leaf"
    if op == "array":
        return None if na == 0 and w == 0 and n.param[-1] >= 1 else "array"
    if op in WORD_OPS:
        return None if words(2, w) else ("operand count" if na != 2 else "word operator widths")
    if op in ("bvnot", "bvneg"):
        return None if words(1, w) else ("operand count" if na != 1 else "word operator widths")
    if op in COMPARISONS:
        if na != 2:
            return "operand count"
        return None if w == 1 and words(2, aw[0]) else "comparison widths"
    if op in ("and", "or"):
        return None if w == 1 and na >= 1 and words(na, 1) else ("operand count" if na < 1 else "Boolean operands")
    if op in ("not", "xor", "implies"):
        count = 1 if op == "not" else 2
        return None if w == 1 and words(count, 1) else ("operand count" if na != count else "Boolean operands")
    if op == "ite":
        if na != 3:
            return "operand count"
        return None if w >= 1 and aw[0] == 1 and aw[1] == w and aw[2] == w else "ite widths"
    if op == "concat":
        if na != 2:
            return "operand count"
        return None if aw[0] >= 1 and aw[1] >= 1 and aw[0] + aw[1] == w else "concat widths"
    if op == "extract":
        if na != 1:
            return "operand count"
        hi, lo = n.param
        return None if lo <= hi < aw[0] and hi - lo + 1 == w else "extract bounds"
    if op in ("zero_extend", "sign_extend"):
        if na != 1:
            return "operand count"
        return None if aw[0] >= 1 and n.param + aw[0] == w else "extension widths"
    if op in ("select", "store"):
        if na != (2 if op == "select" else 3):
            return "operand count"
        arr, idx = n.args[0], n.args[1]
        if arr.op not in ARRAY_SORTED or aw[1] < 1:
            return "select / store operands"
        rng = arr.param[-1]
        if op == "select" and w != rng:
            return "select / store range"
        if op == "store" and not (w == 0 and n.param[-1] == rng and aw[2] == rng):
            return "select / store range"
        # the array's domain: here the expression layer's own record (the node
        # table carries none: the blaster takes a store's index width, or the
        # first index a symbolic array met -- include/mythsmt.h)
        if op == "store" and n.param[-2] != arr.param[-2]:
            return "select index against the domain"
        return None if arr.param[-2] == aw[1] else "select index against the domain"
    if op == "K":
        return None if w == 0 and words(1, n.param[-1]) else "K"
    if op == "uf":
        if w < 1 or any(x < 1 for x in aw):
            return "function application widths"
        sig = signatures.setdefault(n.param, tuple(aw) + (w,))
        return None if sig == tuple(aw) + (w,) else "function application widths"
    return "unknown operator"


def sort_error(roots):
    """The first rule a DAG (a node or a list of roots) breaks, in the post order
    the node table is sent in, or None when every node is well-sorted."""
    roots = [roots] if isinstance(roots, Node) else list(roots)
    seen, signatures = set(), {}
    for root in roots:
        stack = [(root, False)]
        while stack:
            n, ready = stack.pop()
            if n in seen:
                continue
            if not ready:
                stack.append((n, True))
                stack.extend((a, False) for a in reversed(n.args) if a not in seen)
                continue
            seen.add(n)
            err = _node_error(n, signatures)
            if err:
                return err
    return None


def nodes_of(e):
    seen, stack = set(), [e]
    while stack:
        n = stack.pop()
        if n not in seen:
            seen.add(n)
            stack.extend(n.args)
    return seen


def variables(e):
    """The variable nodes e reads, by name."""
    return sorted((n for n in nodes_of(e) if n.op == "var"), key=lambda n: n.param)


def wide_division(e):
    """A division node wider than DIV_MAX_WIDTH (left out: the module docstring)."""
    return any(n.op in DIVS and n.width > DIV_MAX_WIDTH for n in nodes_of(e))


# ---------------------------------------------------------------------- sampling
# (points, models per program); None: every eligible program once
PER_GROUP = (60, 2)
SAMPLE = {
    # the divider's search per pinned 64-bit point (the module docstring): fewer points
    "div:unsigned w=64": (24, 2), "div:signed w=64": (24, 2), "div:unsigned w=8": (60, 6), "div:signed w=8": (60, 6),
    # a 2w-bit product per point
    "div:umul_noovfl w=256": (24, 6), "div:umul_noovfl w=255": (24, 6), "div:umul_noovfl w=64": (24, 6),
    "fuse:tails": None, "fuse:chains": None, "fuse:ext_rcat": None,
}
# In a session a point's pins are assumptions: the wide divider (a 2w-bit product)
# stays in the clause database and every point propagates through it, 30 ms a
# point at 256 bits on the development host (810 points: 49 s; as units 0.4 s).
# The session mode takes every SESSION_STRIDE-th point of such a group.
SESSION_STRIDE = {"exact:wide_division " + op: 13 for op in DIVS}
SKIPPED = ("tables", "div:unsigned w=256", "div:unsigned w=255", "div:signed w=256", "div:signed w=255")
WIDE_DIVISION = tuple("exact:wide_division " + op for op in DIVS)      # one group per operator

# well-sorted points per group, at least (the sample cannot silently empty out)
FLOORS = {"fuse:tails": 70, "fuse:chains": 30, "fuse:ext_rcat": 8, "op:and": 60, "op:or": 60, "op:xor": 60,
          "op:implies": 60, "op:not": 60, "slots:1": 60}


def floor(name):
    if name in FLOORS:
        return FLOORS[name]
    if name in WIDE_DIVISION:
        return 100
    return (SAMPLE.get(name) or PER_GROUP)[0]


def group_names():
    return [n for n in K.all_groups() if n not in SKIPPED] + list(WIDE_DIVISION)


@functools.lru_cache(maxsize=None)
def wide_division_group(name):
    """255- and 256-bit division the blaster decides without its divider.  The
    unsigned operators divide by u: 0, 1, 2, 2^31, 2^(w-2), 2^(w-1); the signed
    ones by s: the same (2^(w-1) is the most negative value there) and -1, -2,
    -2^(w-2).  Dividends: 0, 1, -1, the most negative value and its neighbours,
    and seeded random ones.  Every dividend meets every divisor.  The reference
    is k2_insn_ref, as for the table's own groups."""
    b = K.Builder(name)
    op = name.split()[-1]
    for w in (255, 256):
        if op in ("bvudiv", "bvurem"):
            b.add(f"{op} w={w} divisor 0 / 1 / 2^k", [K.I(op, w, b.v(f"a{w}", w), b.v(f"u{w}", w))])
        else:
            b.add(f"{op} w={w} divisor 0 / +-1 / +-2^k", [K.I(op, w, b.v(f"a{w}", w), b.v(f"s{w}", w))])
    rng = random.Random(255256)
    models = []
    per_width = {}
    for w in (255, 256):
        M, MIN = mask(w), 1 << (w - 1)
        dividends = [0, 1, M, MIN, MIN - 1, MIN + 1, rng.getrandbits(w), rng.getrandbits(w) | MIN,
                     rng.getrandbits(w // 2)]
        unsigned = [0, 1, 2, 1 << 31, 1 << (w - 2), MIN]
        signed = unsigned + [M, M - 1, (-(1 << (w - 2))) & M]
        per_width[w] = [(a, unsigned[k % len(unsigned)], s) for a in dividends for k, s in enumerate(signed)]
    for k in range(len(per_width[255])):
        m = {}
        for w in (255, 256):
            m[f"a{w}"], m[f"u{w}"], m[f"s{w}"] = per_width[w][k]
        models.append(m)
    return b.group(models)


@functools.lru_cache(maxsize=None)
def _group(name):
    return wide_division_group(name) if name in WIDE_DIVISION else K.all_groups()[name]


@functools.lru_cache(maxsize=None)
def _reference(name):
    if name in WIDE_DIVISION:
        g = wide_division_group(name)
        return values(g.prog, g.models)
    return K.reference_ints(name)


@functools.lru_cache(maxsize=None)
def split(name):
    """(well-sorted programs, ill-sorted programs, programs left out for a wide
    division) of a group, as program indices."""
    g = _group(name)
    good, ill, wide = [], [], []
    for d, e in enumerate(g.exprs):
        if e is None:
            continue
        if sort_error(e):
            ill.append(d)
        elif name not in WIDE_DIVISION and wide_division(e):
            wide.append(d)
        else:
            good.append(d)
    return good, ill, wide


@functools.lru_cache(maxsize=None)
def cases(name):
    g = _group(name)
    good, _, _ = split(name)
    rng = random.Random("exactcases:" + name)
    if name in WIDE_DIVISION:
        pairs = [(d, m) for d in good for m in range(len(g.models))]
    else:
        plan = SAMPLE.get(name, PER_GROUP)
        if plan is None:
            pairs = [(d, rng.randrange(len(g.models))) for d in good]
        else:
            points, per_program = plan
            # round-robin over the widest node's width, seeded within each width
            by_width = {}
            for d in good:
                by_width.setdefault(max(n.width for n in nodes_of(g.exprs[d])), []).append(d)
            for ds in by_width.values():
                rng.shuffle(ds)
            order = []
            while any(by_width.values()):
                for w in sorted(by_width):
                    if by_width[w]:
                        order.append(by_width[w].pop())
            n_programs = -(-points // per_program)
            pairs = []
            for i in range(n_programs):
                d = order[i % len(order)]
                for m in rng.sample(range(len(g.models)), per_program):
                    pairs.append((d, m))
            pairs = pairs[:points]
    ref = _reference(name)
    out = []
    for d, m in pairs:
        e = g.exprs[d]
        pins = {(v.param, v.width): g.models[m].get(v.param, 0) & mask(v.width) for v in variables(e)}
        value = ref[d][m]
        assert 0 <= value <= mask(e.width), (name, d, m)
        out.append(Case(name, d, m, e, pins, value, g.describe(d, m) if name not in WIDE_DIVISION else
                        f"{name}: {g.labels[d]} model {m}"))
    return out


def pin_nodes(case):
    return [Node("eq", 1, (var(name, w), const(value, w))) for (name, w), value in sorted(case.pins.items())]


def equals(e, v):
    return Node("eq", 1, (e, const(v, e.width)))


def differs(e, v):
    return Node("distinct", 1, (e, const(v, e.width)))


# ---------------------------------------------------------- the rejection table
def ill_sorted_programs():
    """[(label, conjuncts)]: ill-sorted expressions of kernel-2 programs, as the
    pinned query `pins and e != v` -- program 379 of fuse:tails (the query that
    read out of bounds inside ms_solve) and the first three of each fusion group
    that has any."""
    rows = []
    for name, picks in (("fuse:tails", None), ("fuse:chains", None), ("fuse:ext_rcat", None)):
        g = K.all_groups()[name]
        _, ill, _ = split(name)
        picks = ill[:3] + ([379] if name == "fuse:tails" else [])
        for d in picks:
            e = g.exprs[d]
            assert sort_error(e), (name, d)
            model = g.models[(7 * d) % len(g.models)]
            pins = [Node("eq", 1, (v, const(model.get(v.param, 0), v.width))) for v in variables(e)]
            rows.append((f"{name} program {d} [{g.labels[d]}]", pins + [differs(e, 5)]))
    return rows


def ill_sorted_rows():
    """[(rule, label, conjuncts)]: one ill-sorted query per rule of
    include/mythsmt.h, the offending operand narrower and wider where a width is
    at fault.  Built with Node directly (the expression layer pads)."""
    a4, a8, b8, a16 = var("a4", 4), var("a8", 8), var("b8", 8), var("a16", 16)
    c1, c2 = var("c1", 1), var("c2", 1)
    N = Node
    nz = lambda e: N("distinct", 1, (e, const(0, e.width)))            # a word as a root
    rows = []

    def row(rule, label, *conj):
        rows.append((rule, label, list(conj)))

    # operand count per opcode
    row("operand count", "bvadd of one operand", nz(N("bvadd", 8, (a8,))))
    row("operand count", "bvnot of two operands", nz(N("bvnot", 8, (a8, b8))))
    row("operand count", "bvult of one operand", N("bvult", 1, (a8,)))
    row("operand count", "eq of three operands", N("eq", 1, (a8, b8, a8)))
    row("operand count", "not of two operands", N("not", 1, (c1, c2)))
    row("operand count", "ite of two operands", nz(N("ite", 8, (c1, a8))))
    row("operand count", "concat of one operand", nz(N("concat", 8, (a8,))))
    row("operand count", "extract of two operands", nz(N("extract", 4, (a8, b8), (3, 0))))
    row("operand count", "zero_extend of two operands", nz(N("zero_extend", 16, (a8, b8), 8)))
    row("operand count", "select of one operand", nz(N("select", 8, (N("array", 0, (), ("m", 8, 8)),))))
    # arithmetic, bitwise and shift operators: operand widths == node width
    for op in ("bvadd", "bvsub", "bvmul", "bvudiv", "bvsrem", "bvand", "bvor", "bvxor", "bvshl", "bvashr"):
        row("word operator widths", f"{op}[8] with a narrower second operand", nz(N(op, 8, (a8, a4))))
        row("word operator widths", f"{op}[8] with a wider second operand", nz(N(op, 8, (a8, a16))))
    row("word operator widths", "bvxor[8] with a narrower first operand", nz(N("bvxor", 8, (a4, b8))))
    row("word operator widths", "bvadd[16] of two narrower operands", nz(N("bvadd", 16, (a8, b8))))
    row("word operator widths", "bvadd[4] of two wider operands", nz(N("bvadd", 4, (a8, b8))))
    row("word operator widths", "bvneg[8] of a narrower operand", nz(N("bvneg", 8, (a4,))))
    row("word operator widths", "bvnot[8] of a wider operand", nz(N("bvnot", 8, (a16,))))
    # comparisons and the overflow predicates: equal operand widths, node width 1
    for op in ("eq", "bvult", "bvsle", "bvadd_noovfl_u", "bvumul_noovfl", "bvsub_noudfl_u"):
        row("comparison widths", f"{op} with a narrower second operand", N(op, 1, (a8, a4)))
        row("comparison widths", f"{op} with a wider second operand", N(op, 1, (a8, a16)))
    row("comparison widths", "bvult of width 2", nz(N("bvult", 2, (a8, b8))))
    # Boolean connectives: 1-bit operands
    row("Boolean operands", "and with an 8-bit operand", N("and", 1, (c1, a8)))
    row("Boolean operands", "not of an 8-bit operand", N("not", 1, (a8,)))
    row("Boolean operands", "implies with a 4-bit operand", N("implies", 1, (a4, c1)))
    row("Boolean operands", "or with an array operand (no bits)", N("or", 1, (c1, N("array", 0, (), ("m", 8, 8)))))
    # ite
    row("ite widths", "ite with an 8-bit condition", nz(N("ite", 8, (a8, a8, b8))))
    row("ite widths", "ite[8] with a narrower arm", nz(N("ite", 8, (c1, a8, a4))))
    row("ite widths", "ite[8] with a wider arm", nz(N("ite", 8, (c1, a16, b8))))
    # concat
    row("concat widths", "concat[16] of 8 and 4 bits", nz(N("concat", 16, (a8, a4))))
    row("concat widths", "concat[16] of 8 and 16 bits", nz(N("concat", 16, (a8, a16))))
    # extensions
    for op in ("zero_extend", "sign_extend"):
        row("extension widths", f"{op}[16] by 8 of a narrower operand", nz(N(op, 16, (a4,), 8)))
        row("extension widths", f"{op}[16] by 8 of a wider operand", nz(N(op, 16, (a16,), 8)))
    row("extension widths", "sign_extend[256] by 200 of 8 bits", nz(N("sign_extend", 256, (a8,), 200)))
    # extract
    row("extract bounds", "extract[4] of bits 7..0", nz(N("extract", 4, (a8,), (7, 0))))
    row("extract bounds", "extract[8] of bits 3..0", nz(N("extract", 8, (a8,), (3, 0))))
    row("extract bounds", "extract[8] of bits 11..4 of 8 bits", nz(N("extract", 8, (a8,), (11, 4))))
    row("extract bounds", "extract with lo > hi", nz(N("extract", 2, (a8,), (2, 3))))
    # select against the array's recorded domain
    mem = N("array", 0, (), ("m", 8, 8))
    stored = N("store", 0, (mem, a8, b8), (8, 8))
    row("select index against the domain", "select at a narrower index than the store below it",
        nz(N("select", 8, (stored, a4))))
    row("select index against the domain", "select at a wider index than the store below it",
        nz(N("select", 8, (stored, a16))))
    row("select index against the domain", "two reads of one array, the second index narrower",
        nz(N("select", 8, (mem, a8))), nz(N("select", 8, (mem, a4))))
    row("select index against the domain", "two reads of one array, the second index wider",
        nz(N("select", 8, (mem, a8))), nz(N("select", 8, (mem, a16))))
    row("select index against the domain", "a store at a narrower index than the store below it",
        nz(N("select", 8, (N("store", 0, (stored, a4, b8), (8, 8)), a4))))
    row("select / store range", "select[4] of an array of bytes", nz(N("select", 4, (mem, a8))))
    row("select / store range", "select[16] of an array of bytes", nz(N("select", 16, (mem, a8))))
    row("select / store range", "a stored value wider than the range",
        nz(N("select", 8, (N("store", 0, (mem, a8, a16), (8, 8)), b8))))
    row("select / store operands", "select of a word", nz(N("select", 8, (a8, b8))))
    # function applications: the widths of the other applications
    sig = ("f", (8,), 8)
    good = N("uf", 8, (a8,), sig)
    row("function application widths", "a second application at a narrower argument",
        nz(good), nz(N("uf", 8, (a4,), sig)))
    row("function application widths", "a second application at a wider argument",
        nz(good), nz(N("uf", 8, (a16,), sig)))
    row("function application widths", "a second application of a narrower range",
        nz(good), N("distinct", 1, (N("uf", 4, (b8,), sig), a4)))
    row("function application widths", "a second application with one more argument",
        nz(good), nz(N("uf", 8, (a8, b8), sig)))
    return rows


RULES = ("operand count", "word operator widths", "comparison widths", "Boolean operands", "ite widths",
         "concat widths", "extension widths", "extract bounds", "select index against the domain",
         "function application widths")
