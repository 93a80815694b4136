"""Hand-written arenas, paths and model pools for mg_explore_check's tests: the CPU
module checks tests/pathmodel.py on them against the decoder + flattener + kernel-2
oracle route, the GPU module uploads the same image and compares the device with
the model word for word.

One symbolic message call (transaction id 7, as tests/test_symbolic_cpu.py's):
``7_calldatasize`` / ``7_calldata``, ``sender_7`` (caller and origin),
``call_value7``, ``gas_price7``; the callee's address is concrete, so
MG_ENV_ADDRESS stays unbound.  Two lineages: binding 0 over K(0) storage, binding 1
(MG_LANE_SYMSTORE lanes) over ``Storage<address>``.
"""
from __future__ import annotations

import numpy as np

import pathmodel
from mythril_amd import abi, workloads
from mythril_amd.lanes import LaneBatch, LaneShape, word_to_limbs
from mythril_amd.laser import (Account, Disassembly, MessageCallTransaction, SymbolicCalldata,
                               WorldState)
from mythril_amd.laser import symbolic as sym
from mythril_amd.smt.expr import symbol_factory
from mythril_amd.smt.lower import TableSig
from mythril_amd.smt.program import ArrayInterp, ModelPool

M = (1 << 256) - 1
TOP = 1 << 255
C = abi.MG_SYM_CONST
N_LANES = 192                 # three waves of lanes
NODE_CAP, CONST_CAP, STORAGE_CAP, PATH_CAP = 96, 48, 6, 4
SHAPE = LaneShape(n=N_LANES, stack_cap=4, mem_cap=32, calldata_cap=4, storage_cap=STORAGE_CAP,
                  node_cap=NODE_CAP, const_cap=CONST_CAP)
MODEL_COUNTS = (1, 64, 65, 130)
CD, CDSIZE, SENDER, VALUE, PRICE = "7_calldata", "7_calldatasize", "sender_7", "call_value7", "gas_price7"


def state(symstore: bool = False):
    BVS = symbol_factory.BitVecSym
    ws = WorldState()
    acct = Account(workloads.CONTRACT, code=Disassembly("00"), concrete_storage=not symstore)
    ws.put_account(acct)
    tx = MessageCallTransaction(world_state=ws, identifier="7", callee_account=acct, caller=BVS(SENDER, 256),
                                origin=BVS(SENDER, 256), call_data=SymbolicCalldata("7"),
                                gas_price=BVS(PRICE, 256), gas_limit=8_000_000, call_value=BVS(VALUE, 256))
    gs = tx.initial_global_state()
    gs.transaction_stack.append((tx, None))
    return gs


STORAGE_NAME = state(True).environment.active_account.storage.base_raw.param[0]
VAR_NAMES = [CDSIZE, SENDER, VALUE, PRICE]
TABLES = [TableSig(CD, "array", (256,), 8), TableSig(STORAGE_NAME, "array", (256,), 256)]

# ------------------------------------------------------------------ models
SPECIAL = (0, 1, M, 255, 256, TOP, TOP - 1, 31, 32)
SIZES = (0, 4, 36, TOP, 100, 33, M, TOP + 5)


def models(count: int = 130):
    """`count` models, a prefix of one fixed list: all-zero, all-ones, two that differ
    only in calldata byte 3, then every pair of the special operand values (call
    value, gas price) with the calldata sizes and sparse calldata / storage arrays
    with non-zero defaults."""
    rng = np.random.default_rng(0x9A7)

    def word():
        return int.from_bytes(rng.bytes(32), "little")

    out = [{},
           {CDSIZE: M, SENDER: M, VALUE: M, PRICE: M, CD: ArrayInterp(0xFF), STORAGE_NAME: ArrayInterp(M)}]
    base = {CDSIZE: 36, SENDER: 0xABCD, VALUE: 5, PRICE: 256, STORAGE_NAME: ArrayInterp(7, {9: 0x99, 5: 1})}
    for b3 in (0x11, 0x12):
        out.append(dict(base, **{CD: ArrayInterp(0, {0: 0xA9, 1: 0x05, 2: 0x9C, 3: b3, 35: 0x77})}))
    k = 0
    while len(out) < 130:
        v, g = SPECIAL[k % 9], SPECIAL[(k // 9) % 9]
        if k >= 81:
            v, g = word(), (word() if k % 2 else 256)
        size = SIZES[k % len(SIZES)]
        entries = {int(i): int(rng.integers(0, 256)) for i in rng.integers(0, 40, size=int(rng.integers(0, 12)))}
        entries.update({M: 0xEE, 3: k & 0xFF})
        if size < TOP:
            for i in range(max(size - 34, 0), size + 2):
                if rng.integers(0, 3):
                    entries[i] = int(rng.integers(1, 256))
        store = {5: word(), 9: k, v: g, 256: 1}
        out.append({CDSIZE: size, SENDER: word() if k % 3 else v, VALUE: v, PRICE: g,
                    CD: ArrayInterp(int(rng.integers(0, 256)) if k % 4 else 0, entries),
                    STORAGE_NAME: ArrayInterp(word() if k % 5 else 0, store)})
        k += 1
    return out[:count]


def pool(ms) -> ModelPool:
    return ModelPool.from_dicts(ms, VAR_NAMES, [256] * len(VAR_NAMES), TABLES)


def bindings():
    """[binding 0: K(0) storage, binding 1: the symbolic storage array], by path_binding."""
    return [sym.path_binding(state(False), VAR_NAMES, TABLES), sym.path_binding(state(True), VAR_NAMES, TABLES)]


# ------------------------------------------------------------------- arenas
class Arena:
    """One lane being written: nodes, constants, a store chain."""

    def __init__(self, symstore=False):
        self.nodes, self.consts, self.chain, self.symstore = [], [], [], symstore
        self.n_nodes = self.n_consts = self.n_chain = None        # overrides of the lane's counts

    def c(self, v: int) -> int:
        v &= M
        if v not in self.consts:
            self.consts.append(v)
        return C | self.consts.index(v)

    def push(self, kind, width, y=0, z=0, w=0) -> int:
        self.nodes.append((kind | width << 8, y, z, w))
        return len(self.nodes) - 1

    # sources
    def cdload(self, off): return self.push(abi.MG_SYM_CDLOAD, 256, off)
    def cdsize(self): return self.push(abi.MG_SYM_CDSIZE, 256)
    def env(self, w): return self.push(abi.MG_SYM_ENV, 256, 0, 0, w)
    def value(self): return self.env(abi.MG_ENV_CALLVALUE)
    def price(self): return self.env(abi.MG_ENV_GASPRICE)
    def sender(self): return self.env(abi.MG_ENV_CALLER)
    # terms
    def bin(self, op, y, z): return self.push(abi.MG_SYM_BIN, 1 if 0x10 <= op <= 0x14 else 256, y, z, op)
    def un(self, op, y): return self.push(abi.MG_SYM_UN, 256, y, 0, op)
    def extract(self, hi, lo, y): return self.push(abi.MG_SYM_EXTRACT, hi - lo + 1, y, 0, hi << 16 | lo)
    def concat(self, y, wy, z, wz): return self.push(abi.MG_SYM_CONCAT, wy + wz, y, z, wy | wz << 16)
    def sload(self, key, z): return self.push(abi.MG_SYM_SLOAD, 256, key, z)

    def store(self, key, val):
        """Append a chain entry; key / val: ("c", int) for limbs or ("n", node)."""
        self.chain.append((key, val))


class Case:
    def __init__(self, name, arena, result=None, conds=(), unknown=False, binding=None, pick=None):
        # result: a 256-bit node compared with the value some model gives it (EQ, both sides);
        # conds: [(node, side)] used as they are
        self.name, self.arena, self.result, self.conds = name, arena, result, list(conds)
        self.unknown, self.binding, self.pick = unknown, binding, pick


def _cases():
    out = []

    def add(name, a, result=None, **kw):
        out.append(Case(name, a, result, **kw))

    # every BIN opcode: (symbolic, symbolic), (symbolic, constant), (constant, symbolic)
    operands = (0, 1, M, 255, 256, TOP, 7)
    for op in sorted(pathmodel.BIN):
        a = Arena()
        v, g = a.value(), a.price()
        r = a.bin(op, v, g)
        if a.nodes[r][0] >> 8 == 1:
            r = a.bin(0x01, r, v)                              # a Bool feeding a bit-vector operand
        add(f"bin {op:#x} sym sym", a, r)
        for pos in (0, 1):
            a = Arena()
            v = a.value()
            acc = None
            for k in operands:
                t = a.bin(op, v, a.c(k)) if pos else a.bin(op, a.c(k), v)
                if a.nodes[t][0] >> 8 == 1:
                    t = a.bin(0x03, a.c(k + 3), t)             # const - Bool
                acc = t if acc is None else a.bin(0x18 if k & 1 else 0x01, acc, t)
            add(f"bin {op:#x} const in {'z' if pos else 'y'}", a, acc)
    # the comparisons as the condition itself (a Bool), both sides
    for op in (0x10, 0x11, 0x12, 0x13, 0x14):
        a = Arena()
        cnd = a.bin(op, a.value(), a.price())
        out.append(Case(f"bool {op:#x} taken", a, conds=[(cnd, 1)]))
        out.append(Case(f"bool {op:#x} not taken", a, conds=[(cnd, 0)]))
    a = Arena()
    cnd = a.bin(0x12, a.value(), a.price())
    out.append(Case("both sides of one condition: no model", a, conds=[(cnd, 1), (cnd, 0)]))
    a = Arena()
    out.append(Case("unsigned below zero: no model", a, conds=[(a.bin(0x10, a.value(), a.c(0)), 1)]))
    # SAR of a negative word, shifts by symbolic amounts
    a = Arena()
    add("sar negative", a, a.bin(0x1D, a.value(), a.c(TOP | 0x1234)))
    a = Arena()
    add("shl sym amount of const", a, a.bin(0x1B, a.value(), a.c(M - 2)))
    # every BYTE index
    a = Arena()
    w = a.cdload(a.c(0))
    acc = None
    for k in range(32):
        t = a.bin(0x1A, a.c(k), w)
        acc = t if acc is None else a.bin(0x01, a.bin(0x02, acc, a.c(3)), t)
    add("byte every index", a, acc)
    # ISZERO (of a word and of a Bool), NOT
    a = Arena()
    v = a.value()
    add("iszero word", a, a.bin(0x01, a.un(0x15, v), a.un(0x15, a.bin(0x10, v, a.price()))))
    a = Arena()
    add("not", a, a.un(0x19, a.bin(0x01, a.value(), a.c(1))))
    a = Arena()
    out.append(Case("iszero as the condition", a, conds=[(a.un(0x15, a.value()), 1)]))
    out.append(Case("a word as the condition, not taken", a, conds=[(0, 0)]))
    # EXTRACT / CONCAT at 8, 248 and 256 bits
    a = Arena()
    v = a.value()
    lo8, hi8, mid = a.extract(7, 0, v), a.extract(255, 248, v), a.extract(255, 8, v)
    add("extract 8 + 248 concat", a, a.concat(lo8, 8, mid, 248))
    a = Arena()
    v = a.value()
    add("concat 248 + 8", a, a.concat(a.extract(247, 0, v), 248, a.extract(255, 248, v), 8))
    a = Arena()
    v = a.value()
    add("extract 256", a, a.bin(0x01, a.extract(255, 0, v), a.c(1)))
    a = Arena()
    v = a.value()
    b16 = a.concat(a.extract(15, 8, v), 8, a.c(0x5A), 8)
    add("concat with constants", a, a.concat(a.c(0x1234), 240, b16, 16))
    # calldata: size, bytes, copies from a symbolic offset, words around every size's edge
    a = Arena()
    add("calldatasize", a, a.bin(0x01, a.cdsize(), a.value()))
    a = Arena()
    byte3 = a.push(abi.MG_SYM_CDBYTE, 8, 0, 0, 3)
    out.append(Case("calldata byte 3", a, a.concat(a.c(0), 248, byte3, 8), pick=2))
    a = Arena()
    bx = a.push(abi.MG_SYM_CDBYTEX, 8, a.value(), 0, 5)
    by = a.push(abi.MG_SYM_CDBYTEX, 8, a.c(M - 3), 0, 4)       # wraps to index 0
    add("calldata byte at symbolic offset", a, a.concat(a.concat(a.c(1), 240, bx, 8), 248, by, 8))
    a = Arena()
    add("cdload symbolic offset", a, a.cdload(a.value()))
    # offsets size - 33 .. size + 1 for the sizes 0, 4, 36 (together -33 .. 37, with 0 and
    # 2^256 - 1 among them) and 2^255.  Words of one lane lie 32 bytes apart: overlapping
    # words share their byte loads, and the flattener of the independent route keeps at
    # most 8 shared values live
    wanted = sorted({(s + d) & M for s in (0, 4, 36, TOP) for d in range(-33, 2)} | {0, M})
    seen = set()
    for k in range(32):
        offs = [o & M for o in (k - 33, k - 1, k + 31, TOP + k - 33, TOP + k - 1) if o & M in wanted]
        seen.update(offs)
        a = Arena()
        acc = None
        for off in offs:
            t = a.cdload(a.c(off))
            acc = t if acc is None else a.bin(0x01 if len(a.nodes) & 2 else 0x18, acc, t)
        add(f"cdload at {k - 33} + 32 j and 2^255 + {k - 33} + 32 j", a, acc)
    assert seen == set(wanted)
    a = Arena()
    sel = a.bin(0x1C, a.c(224), a.cdload(a.c(0)))
    out.append(Case("selector", a, conds=[(a.bin(0x14, sel, a.c(0xA9059C11)), 1)]))
    out.append(Case("selector and size", a, conds=[(a.bin(0x14, sel, a.c(0xA9059C12)), 1),
                                                   (a.bin(0x10, a.cdsize(), a.c(4)), 0)]))
    # SLOAD
    for symstore in (False, True):
        tag = "array" if symstore else "K(0)"
        a = Arena(symstore)
        v, g = a.value(), a.price()
        a.store(("c", 5), ("n", v))
        a.store(("c", 5), ("c", 77))
        a.store(("n", g), ("c", 0xBEEF))
        add(f"sload newest of equal keys, {tag}", a, a.sload(a.c(5), 2), binding=int(symstore))
        add(f"sload below the chain length, {tag}", a, a.sload(a.c(5), 1), binding=int(symstore))
        add(f"sload miss, {tag}", a, a.sload(a.c(9), 2), binding=int(symstore))
        add(f"sload symbolic entry key, {tag}", a, a.sload(a.c(256), 3), binding=int(symstore))
        add(f"sload symbolic key, {tag}", a, a.sload(v, 3), binding=int(symstore))
        add(f"sload of an empty chain, {tag}", a, a.sload(v, 0), binding=int(symstore))
    a = Arena(True)
    v = a.value()
    a.store(("n", v), ("n", a.sload(v, 0)))                     # x = storage[x] over the array
    add("sload feeds a store", a, a.sload(a.c(256), 1), binding=1)
    # empty path
    out.append(Case("empty path", Arena()))
    out.append(Case("empty path, symbolic storage", Arena(True), binding=1))
    # ------------------------------------------------ unknown: in the cone, and outside it
    def bad_nodes(a):
        v = a.value()
        return {
            "keccak": a.push(abi.MG_SYM_KECCAK, 256, v, 0, 256),
            "term": a.push(abi.MG_SYM_TERM, 256, 0, 0, 0),
            "mstorek": a.push(abi.MG_SYM_MSTOREK, 256, v, v, 1),
            "mloadk": a.push(abi.MG_SYM_MLOADK, 256, v, 0, 0),
            "balance": a.push(abi.MG_SYM_BALANCE, 256, v),
            "env gas": a.env(abi.MG_ENV_GAS),
            "env address (unbound)": a.env(abi.MG_ENV_ADDRESS),
            "exp": a.bin(0x0A, v, a.c(3)),
            "signextend": a.bin(0x0B, a.c(0), v),
            "byte with a symbolic index": a.bin(0x1A, v, v),
            "byte index 32": a.bin(0x1A, a.c(32), v),
            "unary 0x20": a.un(0x20, v),
            "kind 11": a.push(11, 256, v),
            "kind 200": a.push(200, 256, v),
            "width 0": a.push(abi.MG_SYM_BIN, 0, v, v, 0x01),
            "width 257": a.push(abi.MG_SYM_BIN, 257, v, v, 0x01),
            "extract past the source": a.extract(8, 1, a.extract(7, 0, v)),
            "concat widths": a.push(abi.MG_SYM_CONCAT, 256, v, v, 128 | 64 << 16),
            "node ref past n_nodes": a.bin(0x01, v, 90),
            "forward ref": a.bin(0x01, v, len(a.nodes) + 1),
            "self ref": a.bin(0x01, v, len(a.nodes)),
            "const ref past n_consts": a.bin(0x01, v, C | 40),
            "const ref past the plane": a.bin(0x01, v, C | 0x7FFFFFFF),
            "sload past the chain": a.sload(v, 3),
        }

    probe = Arena()
    for what in bad_nodes(probe):
        a = Arena()
        a.store(("c", 1), ("c", 2))
        bad = bad_nodes(a)[what]
        good = a.bin(0x14, a.value(), a.c(5))
        # as an operand of a good node and, every other time, as the condition itself
        cnd = bad if len(out) & 1 else a.bin(0x01, bad, a.c(1))
        out.append(Case(f"unknown in the cone: {what}", a, conds=[(good, 1), (cnd, 1)], unknown=True))
    a = Arena()
    a.store(("c", 1), ("c", 2))
    bad_nodes(a)
    out.append(Case("every bad node outside the cone", a, a.bin(0x01, a.value(), a.price())))
    a = Arena()
    g = a.price()
    a.store(("c", 1), ("n", a.push(abi.MG_SYM_TERM, 256, 0, 0, 0)))
    a.store(("c", 2), ("c", 3))
    out.append(Case("unknown through a chain tag", a, conds=[(a.sload(g, 1), 1)], unknown=True))
    out.append(Case("a chain tag above z does not matter", a, conds=[(a.sload(g, 0), 0)]))
    a = Arena()
    a.store(("c", 1), ("c", 2))
    a.chain.append((("t", 60), ("c", 3)))                       # a key tag past the arena
    out.append(Case("chain tag past the arena", a, conds=[(a.sload(a.price(), 2), 1)], unknown=True))
    a = Arena()
    out.append(Case("cond_tag 0", a, conds=[(a.value(), 1), (-1, 1)], unknown=True))
    a = Arena()
    out.append(Case("cond_tag past n_nodes", a, conds=[(a.value() + 5, 1)], unknown=True))
    # (counts past their planes are refused by mg_sym_upload; the CPU module has them)
    out.append(Case("lineage unbound", Arena(), unknown=True, binding=abi.MG_PATH_UNBOUND))
    a = Arena()
    out.append(Case("lineage unbound, with a path", a, conds=[(a.value(), 1)], unknown=True,
                    binding=abi.MG_PATH_UNBOUND))
    assert len(out) <= N_LANES - 2, len(out)
    return out


class Image:
    """The cases as a LaneBatch with path planes.  Lane i holds case i; the lanes
    above the cases are empty-path lanes; the last lane's root lies outside the
    batch.  lane_binding is indexed by root: most lanes are their own root, every
    fifth one hangs under an earlier lane with the same binding."""

    def __init__(self, ms):
        self.cases = _cases()
        self.models = ms
        self.pool = pool(ms)
        self.bindings = bindings()
        P = pathmodel._Pool(self.pool)
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
                # compare the result with its value under one model of the pool
                j = (case.pick if case.pick is not None else i % 65) % len(ms)
                self._write(b, i, a, a.nodes)
                lane = pathmodel._Lane(b, i)
                bind = self.bindings[bi]
                k = pathmodel.values(lane, pathmodel.cone(lane, [(case.result + 1) << 1], bind), bind, P, j)[case.result]
                eq = a.bin(0x14, case.result, a.c(k))
                conds.append((eq, i & 1 if i % 7 else 1))
            self._write(b, i, a, a.nodes)
            assert len(conds) <= PATH_CAP
            self.path_len[i] = len(conds)
            for e, (node, side) in enumerate(conds):
                self.path[i, e] = (node + 1) << 1 | side
        self.root[n - 1] = n + 3
        self.unknown = [i for i, c in enumerate(self.cases) if c.unknown] + [n - 1]

    @staticmethod
    def _write(b, i, a, nodes):
        b.node[i] = 0
        b.cval[i] = 0
        for k, row in enumerate(nodes):
            b.node[i, k] = row
        for k, v in enumerate(a.consts):
            b.cval[i, k] = word_to_limbs(v)
        b.n_nodes[i] = len(nodes) if a.n_nodes is None else a.n_nodes
        b.n_consts[i] = len(a.consts) if a.n_consts is None else a.n_consts
        b.storage[i] = 0
        b.sttag[i] = 0
        for e, (key, val) in enumerate(a.chain):
            for h, (how, x) in enumerate((key, val)):
                if how == "c":
                    b.storage[i, e, 8 * h:8 * h + 8] = word_to_limbs(x)
                else:
                    b.sttag[i, e, h] = x + 1
        b.storage_count[i] = len(a.chain) if a.n_chain is None else a.n_chain

    @property
    def paths(self):
        return self.path, self.path_len, self.root


_IMAGES = {}


def image(count: int) -> Image:
    """The image whose comparison constants come from a pool of `count` models
    (built once per count and shared; nothing changes it)."""
    if count not in _IMAGES:
        _IMAGES[count] = Image(models(count))
    return _IMAGES[count]
