"""Hand-written arenas for mg_explore_check_fn's tests: KECCAK nodes over every
input shape the contract takes or refuses, and EXP's Power, in the transaction of
tests/pathcases.py (whose Arena, Case, state and base models these reuse).  The CPU
module checks tests/pathfnmodel.py on them against the decoder + flattener +
kernel-2 oracle route; the GPU module uploads the image and compares the device
with the model word for word.

The pool carries Power and keccak256_<bits> for the widths in BOUND; keccak256_16
is deliberately absent.  Every function is read at keys the models' own values
make, so each table of a model holds, in this order: an entry that differs from
the looked-up key only in k1 (512-bit keys), one that differs only in k0, the key
itself, and -- every other model -- the key again with another value (the first
wins).  Every fifth model lacks the key and answers with its non-zero default.
"""
from __future__ import annotations

import numpy as np

import pathcases
import pathfnmodel
from mythril_amd import abi
from mythril_amd.keccak import keccak256
from mythril_amd.lanes import LaneBatch, LaneShape
from mythril_amd.laser import symbolic as sym
from mythril_amd.smt.lower import TableSig
from mythril_amd.smt.program import ArrayInterp, FuncInterp, ModelPool
from pathcases import M, PRICE, SENDER, STORAGE_NAME, VALUE, VAR_NAMES, Arena, Case

C = abi.MG_SYM_CONST
N_LANES = 80                  # one wave of lanes and a part of the next
NODE_CAP, CONST_CAP, STORAGE_CAP, PATH_CAP = 96, 16, 4, 4
SHAPE = LaneShape(n=N_LANES, stack_cap=4, mem_cap=32, calldata_cap=4, storage_cap=STORAGE_CAP,
                  node_cap=NODE_CAP, const_cap=CONST_CAP)
MODEL_COUNTS = pathcases.MODEL_COUNTS
BOUND = (8, 256, 264, 504, 512)
UNBOUND_WIDTH = 16
SLOT = 3                      # balances: mapping at slot 3
CONST_IN = 0x1234_5678_9ABC   # the constant input; its table entry is its real hash
CONST_HASH = int.from_bytes(keccak256(CONST_IN.to_bytes(32, "big")), "big")
HASHES = (0xAA00 << 240 | 0x40, 0xBB00 << 240 | 0x80, 0xCC00 << 240 | 0xC0)
TABLES = pathcases.TABLES + [TableSig("Power", "uf", (256, 256), 256)] + \
    [TableSig(f"keccak256_{w}", "uf", (w,), 256) for w in BOUND]


# ------------------------------------------------------------------ models
def keys_of(model) -> dict:
    """function name -> the argument tuples the cases look up under `model`."""
    s, v, g = (model.get(n, 0) for n in (SENDER, VALUE, PRICE))
    b = v & 0xFF
    return {
        "keccak256_8": [(b,)],
        "keccak256_256": [(v,), (CONST_IN,), (v & ~0xFF & M | g >> 248,)],
        "keccak256_264": [(v << 8 | g & 0xFF,)],
        "keccak256_504": [((v >> 8) << 256 | g,)],
        "keccak256_512": [(s << 256 | SLOT,), (v << 256 | g,), ((int("%x" % (v & 0xF) * 62, 16) << 8 | b) << 256 | v,),
                          ((v >> 8) << 264 | (b << 8 | g >> 248) << 248 | g & ((1 << 248) - 1),)],
        "Power": [(v, g), (g, v), (256, v)],
    }


def models(count: int = 130):
    rng = np.random.default_rng(0xF17)

    def word():
        return int.from_bytes(rng.bytes(32), "little") | 1

    out = []
    for m, base in enumerate(pathcases.models(130)):
        d = dict(base)
        slot_hash = HASHES[m % 3] if m % 4 else word()
        for name, keys in keys_of(d).items():
            entries = {}
            for j, key in enumerate(keys):
                if key in entries:
                    continue
                mapping = name == "keccak256_512" and j == 0
                if name == "Power":
                    entries[(key[0], key[1] ^ 1)] = word()               # differs only in k1
                    entries[(key[0] ^ 1, key[1])] = word()               # differs only in k0
                else:
                    if name == "keccak256_512":
                        entries[(key[0] ^ 1 << 256,)] = word()           # differs only in k1
                    entries[(key[0] ^ 1,)] = word()                      # differs only in k0
                if (m + j) % 5 == 1 and key != (CONST_IN,):
                    continue                                             # absent: the default answers
                entries.setdefault(key, CONST_HASH if key == (CONST_IN,) else slot_hash if mapping else word())
                if (m + j) % 2 and name != "Power":
                    entries[(key[0] + (1 << 512),)] = word()             # the same (k0, k1) again: the first wins
            d[name] = FuncInterp(word(), entries)
        # the balances the mapping reads: storage at the slot's hash
        st = d.get(STORAGE_NAME)
        if isinstance(st, ArrayInterp) and m % 2:
            d[STORAGE_NAME] = ArrayInterp(st.default, {**st.entries, slot_hash: word()})
        out.append(d)
    return out[:count]


def pool(ms) -> ModelPool:
    return ModelPool.from_dicts(ms, VAR_NAMES, [256] * len(VAR_NAMES), TABLES)


def bindings():
    return [sym.path_binding(pathcases.state(False), VAR_NAMES, TABLES),
            sym.path_binding(pathcases.state(True), VAR_NAMES, TABLES)]


def functions(power: bool = True, keccak: bool = True):
    """path_functions of TABLES, or with Power / every keccak table left unbound."""
    f = sym.path_functions(TABLES)
    if not power:
        f.tab_power = abi.MG_PATH_UNBOUND
    if not keccak:
        f.n_keccak = 0
    return f


# ------------------------------------------------------------------- arenas
def keccak(a: Arena, y: int, bits: int) -> int:
    return a.push(abi.MG_SYM_KECCAK, 256, y, 0, bits)


def power(a: Arena, base: int, exponent: int) -> int:
    return a.push(abi.MG_SYM_BIN, 256, base, exponent, 0x0A)


def byte_parts(a: Arena, v: int, g: int):
    """value and gas price as 8 + 8 parts of 32 bits, high part first: [(node, width)]."""
    return [(a.extract(255 - 32 * k, 224 - 32 * k, x), 32) for x in (v, g) for k in range(8)]


def left_chain(a: Arena, parts) -> int:
    """sym_mem_ref's shape: the accumulator is the high operand."""
    acc, accw = parts[0]
    for p, pw in parts[1:]:
        acc, accw = a.concat(acc, accw, p, pw), accw + pw
    return acc


def right_chain(a: Arena, parts) -> int:
    acc, accw = parts[-1]
    for p, pw in reversed(parts[:-1]):
        acc, accw = a.concat(p, pw, acc, accw), accw + pw
    return acc


def balanced(a: Arena, parts):
    if len(parts) == 1:
        return parts[0]
    h = len(parts) // 2
    (l, lw), (r, rw) = balanced(a, parts[:h]), balanced(a, parts[h:])
    return a.concat(l, lw, r, rw), lw + rw


def _cases():
    out = []

    def add(name, a, result=None, uses=("keccak",), **kw):
        case = Case(name, a, result, **kw)
        case.uses = set(uses)
        out.append(case)

    # ---- inputs of one part
    a = Arena()
    add("keccak of one 256-bit node", a, keccak(a, a.value(), 256))
    a = Arena()
    add("keccak of an 8-bit node", a, keccak(a, a.extract(7, 0, a.value()), 8))
    a = Arena()
    add("keccak of a constant", a, a.bin(0x01, keccak(a, a.c(CONST_IN), 256), a.value()))
    a = Arena()
    v, g = a.value(), a.price()
    add("keccak of a 256-bit concat node", a, keccak(a, a.concat(a.extract(255, 8, v), 248, a.extract(255, 248, g), 8), 256))
    # ---- the mapping slot and the chains
    a = Arena()
    add("mapping slot: concat(caller, const slot)", a, keccak(a, a.concat(a.sender(), 256, a.c(SLOT), 256), 512))
    a = Arena()
    v, g = a.value(), a.price()
    add("left chain of 264 bits", a, keccak(a, left_chain(a, [(a.extract(255, 128, v), 128), (a.extract(127, 0, v), 128),
                                                             (a.extract(7, 0, g), 8)]), 264))
    a = Arena()
    v, g = a.value(), a.price()
    add("left chain of 504 bits", a, keccak(a, left_chain(a, [(a.extract(255, 8, v), 248), (a.extract(255, 128, g), 128),
                                                             (a.extract(127, 0, g), 128)]), 504))
    for name, shape in (("left chain", left_chain), ("right chain", right_chain),
                        ("balanced tree", lambda a, p: balanced(a, p)[0])):
        a = Arena()
        v, g = a.value(), a.price()
        add(f"{name} of 512 bits, 16 parts", a, keccak(a, shape(a, byte_parts(a, v, g)), 512))
    a = Arena()
    v, g = a.value(), a.price()
    add("left chain of 512 bits, whole words", a, keccak(a, left_chain(a, [(v, 256), (a.extract(255, 128, g), 128),
                                                                          (a.extract(127, 0, g), 128)]), 512))
    a = Arena()
    v, g = a.value(), a.price()
    mid = a.concat(a.extract(7, 0, v), 8, a.extract(255, 248, g), 8)
    add("248 + 16 + 248: the middle part straddles bit 256", a,
        keccak(a, left_chain(a, [(a.extract(255, 8, v), 248), (mid, 16), (a.extract(247, 0, g), 248)]), 512))
    a = Arena()
    add("mapping slot with the constant in two parts, right chain", a,
        keccak(a, right_chain(a, [(a.sender(), 256), (a.c(0), 248), (a.c(SLOT), 8)]), 512))
    # every concat above a 256-bit low part is wide, so every part is a leaf of the tree
    a = Arena()
    v = a.value()
    b8, n4 = a.extract(7, 0, v), a.extract(3, 0, v)
    add("64 leaves", a, keccak(a, right_chain(a, [(n4, 4)] * 62 + [(b8, 8), (v, 256)]), 512))
    a = Arena()
    v = a.value()
    n4 = a.extract(3, 0, v)
    add("65 leaves in 512 bits", a, conds=[(keccak(a, right_chain(a, [(n4, 4)] * 64 + [(v, 256)]), 512), 1)],
        unknown=True)
    a = Arena()
    v, g = a.value(), a.price()
    add("520 bits", a, conds=[(keccak(a, left_chain(a, [(v, 256), (g, 256), (a.extract(7, 0, v), 8)]), 520), 1)],
        unknown=True)
    # ---- each single width mismatch
    a = Arena()
    v, g = a.value(), a.price()
    add("w = 512 over a 504-bit tree", a, conds=[(keccak(a, a.concat(a.extract(255, 8, v), 248, g, 256), 512), 1)],
        unknown=True)
    a = Arena()
    v, g = a.value(), a.price()
    bad = a.push(abi.MG_SYM_CONCAT, 512, a.extract(255, 8, v), g, 256 | 256 << 16)
    add("concat states 256 bits for a 248-bit part", a, conds=[(keccak(a, bad, 512), 1)], unknown=True)
    a = Arena()
    v, g = a.value(), a.price()
    bad = a.push(abi.MG_SYM_CONCAT, 512, v, g, 256 | 248 << 16)
    add("concat widths do not sum to its own", a, conds=[(keccak(a, bad, 512), 1)], unknown=True)
    a = Arena()
    add("w = 256 over an 8-bit node", a, conds=[(keccak(a, a.extract(7, 0, a.value()), 256), 1)], unknown=True)
    a = Arena()
    add("a constant of 264 bits", a, conds=[(keccak(a, a.c(5), 264), 1)], unknown=True)
    a = Arena()
    v = a.value()
    bad = a.push(abi.MG_SYM_CONCAT, 512, v, a.c(SLOT), 248 | 264 << 16)
    add("a constant part of 264 bits", a, conds=[(keccak(a, bad, 512), 1)], unknown=True)
    a = Arena()
    add("keccak node of width 8", a, conds=[(a.push(abi.MG_SYM_KECCAK, 8, a.extract(7, 0, a.value()), 0, 8), 1)],
        unknown=True)
    a = Arena()
    add("w = 0", a, conds=[(keccak(a, a.value(), 0), 1)], unknown=True)
    a = Arena()
    v = a.value()
    fwd = len(a.nodes) + 1
    bad = a.push(abi.MG_SYM_CONCAT, 512, v, fwd + 1, 256 | 256 << 16)
    k = keccak(a, bad, 512)
    a.price()
    add("a part above its referrer", a, conds=[(k, 1)], unknown=True)
    a = Arena()
    bad = a.push(abi.MG_SYM_CONCAT, 512, a.value(), C | 9, 256 | 256 << 16)
    add("a constant part past n_consts", a, conds=[(keccak(a, bad, 512), 1)], unknown=True)
    a = Arena()
    ml = a.push(abi.MG_SYM_MLOADK, 256, a.value(), 0, 32)
    add("an MLOADK input", a, conds=[(keccak(a, ml, 256), 1)], unknown=True)
    # ---- widths bound and not bound
    a = Arena()
    v = a.value()
    good = a.bin(0x14, keccak(a, v, 256), a.c(1))
    add("a width with no table next to a bound one", a,
        conds=[(good, 0), (keccak(a, a.extract(15, 0, v), UNBOUND_WIDTH), 1)], unknown=True)
    a = Arena()
    v = a.value()
    add("two widths in one path", a,
        a.bin(0x03, keccak(a, v, 256), keccak(a, a.concat(a.sender(), 256, a.c(SLOT), 256), 512)))
    # ---- a wide concat reached any other way
    a = Arena()
    wide = a.concat(a.value(), 256, a.price(), 256)
    add("a wide concat as the condition", a, conds=[(keccak(a, wide, 512), 1), (wide, 1)], unknown=True)
    a = Arena()
    wide = a.concat(a.value(), 256, a.price(), 256)
    add("a wide concat as a BIN operand", a, conds=[(a.bin(0x01, wide, a.c(1)), 1)], unknown=True)
    a = Arena()
    wide = a.concat(a.value(), 256, a.price(), 256)
    add("a wide concat as an EXTRACT source", a, conds=[(a.extract(300, 45, wide), 1)], unknown=True)
    a = Arena()
    wide = a.concat(a.value(), 256, a.price(), 256)
    a.store(("n", wide), ("c", 1))
    add("a wide concat as a chain tag", a, conds=[(a.sload(a.c(1), 1), 1)], unknown=True)
    # ---- the hash as a storage key
    for symstore in (True, False):
        a = Arena(symstore)
        a.store(("c", HASHES[0]), ("c", 77))
        h = keccak(a, a.concat(a.sender(), 256, a.c(SLOT), 256), 512)
        add(f"sload at the mapping slot, {'array' if symstore else 'K(0)'}", a, a.sload(h, 1), binding=int(symstore))
    a = Arena(True)
    h = keccak(a, a.concat(a.sender(), 256, a.c(SLOT), 256), 512)
    a.store(("n", h), ("n", a.value()))
    a.store(("c", 9), ("c", 4))
    add("the hash as a chain entry's key", a, a.sload(a.c(HASHES[1]), 2), binding=1)
    # ---- Power
    a = Arena()
    add("power of two symbols", a, power(a, a.value(), a.price()), uses=("power",))
    a = Arena()
    add("power of base 256", a, power(a, a.c(256), a.value()), uses=("power",))
    a = Arena()
    v, g = a.value(), a.price()
    add("power with the operands swapped", a, a.bin(0x03, power(a, v, g), power(a, g, v)), uses=("power",))
    a = Arena()
    v, g = a.value(), a.price()
    add("power of a hash", a, a.bin(0x01, power(a, v, g), keccak(a, v, 256)), uses=("power", "keccak"))
    a = Arena()
    add("power of width 8", a, conds=[(a.push(abi.MG_SYM_BIN, 8, a.value(), a.price(), 0x0A), 1)], unknown=True,
        uses=("power",))
    # ---- the same path without a function: known whatever is bound
    a = Arena()
    add("no function in the cone", a, a.bin(0x01, a.value(), a.price()), uses=())
    a = Arena()
    v = a.value()
    keccak(a, a.extract(15, 0, v), UNBOUND_WIDTH)
    power(a, v, v)
    add("functions outside the cone", a, a.bin(0x02, v, a.price()), uses=())
    assert len(out) <= N_LANES - 2, len(out)
    return out


class Image(pathcases.Image):
    """The cases as a LaneBatch with path planes, laid out as pathcases.Image lays its
    own out; a result is compared with its value under one model with everything bound."""

    def __init__(self, ms):
        self.cases = _cases()
        self.models = ms
        self.pool = pool(ms)
        self.bindings = bindings()
        self.functions = functions()
        fn = pathfnmodel.Functions(self.functions)
        P = pathfnmodel._Pool(self.pool)
        b = self.batch = LaneBatch(SHAPE)
        n = SHAPE.n
        self.path = np.zeros((n, PATH_CAP), dtype=np.uint32)
        self.path_len = np.zeros(n, dtype=np.uint32)
        self.root = np.arange(n, dtype=np.uint32)
        self.lane_binding = np.zeros(n, dtype=np.uint32)
        b.flags[:] = abi.MG_LANE_SYMBOLIC
        b.status[:] = abi.MG_HALT_STOP
        last_of = {}
        for i, case in enumerate(self.cases):
            a = case.arena
            bi = case.binding if case.binding is not None else int(a.symstore)
            if i % 5 == 4 and bi in last_of:
                self.root[i] = last_of[bi]
            else:
                self.lane_binding[i] = bi
                last_of.setdefault(bi, i)
            if a.symstore:
                b.flags[i] |= abi.MG_LANE_SYMSTORE
            conds = list(case.conds)
            if case.result is not None:
                j = (case.pick if case.pick is not None else i % 65) % len(ms)
                self._write(b, i, a, a.nodes)
                lane = pathfnmodel._Lane(b, i)
                bind = self.bindings[bi]
                nodes = pathfnmodel.cone(lane, [(case.result + 1) << 1], bind, fn)
                k = pathfnmodel.values(lane, nodes, bind, fn, P, j)[case.result]
                conds.append((a.bin(0x14, case.result, a.c(k)), i & 1 if i % 7 else 1))
            self._write(b, i, a, a.nodes)
            assert len(conds) <= PATH_CAP and len(a.nodes) <= NODE_CAP and len(a.consts) <= CONST_CAP, case.name
            self.path_len[i] = len(conds)
            for e, (node, side) in enumerate(conds):
                self.path[i, e] = (node + 1) << 1 | side
        self.root[n - 1] = n + 3
        self.unknown = [i for i, c in enumerate(self.cases) if c.unknown] + [n - 1]

    def using(self, what: str):
        """The lanes of known cases whose cone reads `what` ("keccak" / "power")."""
        return [i for i, c in enumerate(self.cases) if not c.unknown and what in c.uses]


_IMAGES = {}


def image(count: int) -> Image:
    """The image whose comparison constants come from a pool of `count` models
    (built once per count and shared; nothing changes it)."""
    if count not in _IMAGES:
        _IMAGES[count] = Image(models(count))
    return _IMAGES[count]
