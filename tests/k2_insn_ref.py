"""Test-only reference of kernel 2's program format (mg_dag_batch, include/mythgpu.h)
on Python ints.  Never imported by ``mythril_amd``.

``values(prog, models)`` interprets every program of a ProgramBatch under every
model dict and returns the final accumulators as Python ints.  It is written
from the header's contract (four u32 per instruction, an accumulator, slots,
variables, constants, tables, the immediates w2 / w3) and the SMT-LIB / z3
definitions of the operators; it knows nothing of fusion,
predecoding or limbs, and shares no code with ``semantics.apply_op``, the C
oracle or the device.

``knuth_events(a, b)`` restates Knuth's algorithm D on 32-bit digits the way
the device's division is laid out (same normalisation, digits top-down) and
reports which of its rare steps an operand pair meets; it is what the case
lists' coverage conditions are asserted with (never device output).
"""
from mythril_amd import abi
from mythril_amd.smt.program import ArrayInterp, FuncInterp, model_value

OPS = [host for _, host in abi.BV_OPS]
TAB_INDEX_MASK = abi.MG_BV_TAB_INDEX_MASK
TAB_PART_SHIFT = abi.MG_BV_TAB_PART_SHIFT
TAB_LO_SHIFT = abi.MG_BV_TAB_LO_SHIFT


def mask(w):
    return (1 << w) - 1


def signed(x, w):
    """The two's-complement reading of the w-bit value x."""
    return x - (1 << w) if (x >> (w - 1)) & 1 else x


def _trunc_div(sa, sb):
    q = abs(sa) // abs(sb)
    return -q if (sa < 0) != (sb < 0) else q


def _sdiv(a, b, w):
    sa, sb = signed(a, w), signed(b, w)
    if sb == 0:
        return 1 if sa < 0 else -1
    return _trunc_div(sa, sb)


def _srem(a, b, w):
    sa, sb = signed(a, w), signed(b, w)
    if sb == 0:
        return sa
    return sa - sb * _trunc_div(sa, sb)


def _smod(a, b, w):
    sa, sb = signed(a, w), signed(b, w)
    if sb == 0:
        return sa
    return sa % sb          # Python's % takes the divisor's sign, as bvsmod does


# op name -> f(width, a, b, w2, w3); the result is masked to `width` by the caller
_BINARY = {
    "bvadd": lambda w, a, b, w2, w3: a + b,
    "bvsub": lambda w, a, b, w2, w3: a - b,
    "bvmul": lambda w, a, b, w2, w3: a * b,
    "bvudiv": lambda w, a, b, w2, w3: -1 if b == 0 else a // b,
    "bvurem": lambda w, a, b, w2, w3: a if b == 0 else a % b,
    "bvsdiv": lambda w, a, b, w2, w3: _sdiv(a, b, w),
    "bvsrem": lambda w, a, b, w2, w3: _srem(a, b, w),
    "bvsmod": lambda w, a, b, w2, w3: _smod(a, b, w),
    "bvand": lambda w, a, b, w2, w3: a & b,
    "bvor": lambda w, a, b, w2, w3: a | b,
    "bvxor": lambda w, a, b, w2, w3: a ^ b,
    "bvshl": lambda w, a, b, w2, w3: a << b if b < w else 0,
    "bvlshr": lambda w, a, b, w2, w3: a >> b if b < w else 0,
    "bvashr": lambda w, a, b, w2, w3: signed(a, w) >> (b if b < w else w),
    "eq": lambda w, a, b, w2, w3: a == b,
    "distinct": lambda w, a, b, w2, w3: a != b,
    "bvult": lambda w, a, b, w2, w3: a < b,
    "bvule": lambda w, a, b, w2, w3: a <= b,
    "bvugt": lambda w, a, b, w2, w3: a > b,
    "bvuge": lambda w, a, b, w2, w3: a >= b,
    "bvslt": lambda w, a, b, w2, w3: signed(a, w3) < signed(b, w3),
    "bvsle": lambda w, a, b, w2, w3: signed(a, w3) <= signed(b, w3),
    "bvsgt": lambda w, a, b, w2, w3: signed(a, w3) > signed(b, w3),
    "bvsge": lambda w, a, b, w2, w3: signed(a, w3) >= signed(b, w3),
    "and": lambda w, a, b, w2, w3: a & b & 1,
    "or": lambda w, a, b, w2, w3: (a | b) & 1,
    "xor": lambda w, a, b, w2, w3: (a ^ b) & 1,
    "implies": lambda w, a, b, w2, w3: (not a & 1) or b & 1,
    "concat": lambda w, a, b, w2, w3: (a << w3) | b,
    "bvadd_noovfl_u": lambda w, a, b, w2, w3: a + b < (1 << w3),
    "bvumul_noovfl": lambda w, a, b, w2, w3: a * b < (1 << w3),
    "bvsub_noudfl_u": lambda w, a, b, w2, w3: b <= a,
    "bvumin": lambda w, a, b, w2, w3: min(a, b),
    "bvumax": lambda w, a, b, w2, w3: max(a, b),
    "bvsmin": lambda w, a, b, w2, w3: b if signed(b, w) < signed(a, w) else a,
    "bvsmax": lambda w, a, b, w2, w3: b if signed(a, w) < signed(b, w) else a,
    "bvrsub": lambda w, a, b, w2, w3: b - a,
    "rconcat": lambda w, a, b, w2, w3: (b << w3) | a,
}
_UNARY = {
    "copy": lambda w, a, w2: a,
    "zero_extend": lambda w, a, w2: a,
    "bvnot": lambda w, a, w2: ~a,
    "bvneg": lambda w, a, w2: -a,
    "not": lambda w, a, w2: (a & 1) ^ 1,
    "extract": lambda w, a, w2: a >> (w2 & 0xFF),
    "sign_extend": lambda w, a, w2: signed(a, w2),
}
assert set(_BINARY) | set(_UNARY) | {"ite", "tab"} == set(OPS), set(OPS) ^ (set(_BINARY) | set(_UNARY) | {"ite", "tab"})


def _tables_of(prog, model):
    """Per table index: (default, {(k0, k1): value}) of this model's interpretation,
    each value up to 512 bits; a table the model does not interpret is all 0."""
    out = []
    for sig in prog.tables:
        interp = model.get(sig.name)
        if isinstance(interp, ArrayInterp):
            out.append((interp.default, {sig.key_chunks((k,)): v for k, v in interp.entries.items()}))
        elif isinstance(interp, FuncInterp):
            out.append((interp.else_value, {sig.key_chunks(tuple(k)): v for k, v in interp.entries.items()}))
        else:
            out.append((0, {}))
    return out


def decode(insns):
    """Rows of four ints -> (form, function, width, store slot or -1, w1, w2, w3);
    form 0: one operand, 1: two, 2: ite, 3: tab."""
    out = []
    for w0, w1, w2, w3 in insns:
        name = OPS[w0 & 0xFF]
        form = 0 if name in _UNARY else 2 if name == "ite" else 3 if name == "tab" else 1
        fn = _UNARY.get(name) or _BINARY.get(name)
        out.append((form, fn, (w0 >> 8) & 0x1FF, (w0 >> 18) & 0xF if (w0 >> 17) & 1 else -1, w1, w2, w3))
    return out


def run_program(insns, consts, var_values, tables=None, n_slots=16, decoded=False):
    """The final accumulator of one program.  insns: rows of four ints; consts /
    var_values: ints by index; tables: per index (default, {(k0, k1): value}).
    Slots start at 0."""
    acc = 0
    slots = [0] * n_slots

    def operand(ref):
        kind, idx = ref >> 30, ref & 0x3FFFFFFF
        if kind == 0:
            return acc
        if kind == 1:
            return slots[idx]
        if kind == 2:
            return var_values[idx]
        return consts[idx]

    for form, fn, width, store, w1, w2, w3 in (insns if decoded else decode(insns)):
        a = operand(w1)
        if form == 1:
            r = fn(width, a, operand(w2), w2, w3)
        elif form == 0:
            r = fn(width, a, w2)
        elif form == 2:
            r = operand(w2) if a & 1 else operand(w3)
        else:
            default, entries = tables[w3 & TAB_INDEX_MASK]
            v = entries.get((a, operand(w2)), default)
            r = v >> (256 * ((w3 >> TAB_PART_SHIFT) & 1) + ((w3 >> TAB_LO_SHIFT) & 0xFF))
        acc = int(r) & ((1 << width) - 1)
        if store >= 0:
            slots[store] = acc
    return acc


def values(prog, models):
    """values[d][m]: the final accumulator of program d under model dict m."""
    consts = [int.from_bytes(row.astype("<u4").tobytes(), "little") for row in prog.consts]
    rows = prog.insns.tolist()
    off = prog.prog_off.tolist()
    progs = [decode(rows[off[d]:off[d + 1]]) for d in range(prog.n_dags)]
    out = [[0] * len(models) for _ in progs]
    n_slots = max(prog.n_slots, 1)
    for m, model in enumerate(models):
        vv = [model_value(model, name) & mask(w) for name, w in zip(prog.var_names, prog.var_widths)]
        tabs = _tables_of(prog, model) if prog.tables else None
        for d, p in enumerate(progs):
            out[d][m] = run_program(p, consts, vv, tabs, n_slots, decoded=True)
    return out


# ---------------------------------------------------------------- Knuth D, digit level
EVENTS = ("qmax", "dec1", "dec2", "addback")
B32 = 1 << 32


def knuth_events(a, b):
    """Knuth's algorithm D on 32-bit digits for 0 <= a < 2^256, 0 < b < 2^256: b
    normalised so that its top bit is bit 255, a shifted by the same amount into 17
    digits, the 8 quotient digits top-down, each estimated from the top two
    remainder digits, refined against the divisor's second digit (at most two
    decrements) and corrected by one add-back.  Every step is checked against
    divmod.  Returns the set of events met in a digit the quotient needs
    (32 j <= bitlen(a) - bitlen(b)): "qmax" (the estimate is 2^32 - 1 because the
    top remainder digit is not below the divisor's), "dec1" / "dec2" (one / two
    refinement decrements), "addback"."""
    assert 0 <= a < 1 << 256 and 0 < b < 1 << 256
    s = 256 - b.bit_length()
    vn, un = b << s, a << s
    v = [(vn >> (32 * i)) & (B32 - 1) for i in range(8)]
    u = [(un >> (32 * i)) & (B32 - 1) for i in range(17)]
    v7, v6 = v[7], v[6]
    assert v7 >> 31 == 1
    dl = a.bit_length() - b.bit_length()
    events, q = set(), 0
    for j in range(7, -1, -1):
        window = sum(u[j + i] << (32 * i) for i in range(9))
        true_q, true_r = divmod(window, vn)
        assert true_q < B32
        u2, u1, u0 = u[j + 8], u[j + 7], u[j + 6]
        met = set()
        if u2 >= v7:
            qh, rh = B32 - 1, u1 + v7
            met.add("qmax")
        else:
            qh, rh = divmod((u2 << 32) | u1, v7)
        dec = 0
        for _ in range(2):
            if rh < B32 and qh * v6 > ((rh << 32) | u0):
                qh, rh, dec = qh - 1, rh + v7, dec + 1
        if dec:
            met.add("dec%d" % dec)
        assert true_q <= qh <= true_q + 1, (a, b, j)
        rest = window - qh * vn
        if rest < 0:
            qh, rest = qh - 1, rest + vn
            met.add("addback")
        assert (qh, rest) == (true_q, true_r), (a, b, j)
        for i in range(9):
            u[j + i] = (rest >> (32 * i)) & (B32 - 1)
        q |= qh << (32 * j)
        if dl >= 32 * j:
            events |= met
        else:
            assert qh == 0, (a, b, j)         # a digit the quotient does not need is 0
    rem = sum(u[i] << (32 * i) for i in range(8)) >> s
    assert (q, rem) == divmod(a, b), (a, b)
    return events
