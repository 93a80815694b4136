"""Directed programs for the symbolic stepper (k_sym_step): one list per family
of paths the whole-contract co-simulation (tests/symcases.py) does not reach --
the partition of a memory range into parts, the hygiene of memory byte tags, the
store-chain walk of SLOAD, the ALU's quirks and escapes, and stops in the middle
of an instruction (capacities, gas, the stack limit, write protection).

Every program is a message call with symbolic calldata, caller and call value,
written as assembly (`asm` turns it into code; the text is the source).  Every
case states what must happen on the device, so that a lane which escapes early
cannot pass by doing nothing: the number of instructions executed, the final
status and aux, arena node kinds (with their widths) and records that must
appear.  The expectations are worked out from the reference's semantics --
instructions.py (the mutators), state/memory.py (get_word_at, write_word_at),
state/account.py (Storage), as tests/symref.py restates and cites them -- and
tests/test_sym_directed_cpu.py pins them against the restatement without a GPU.
Never from a device run."""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Tuple

import symref
from mythril_amd.lanes import (MG_ESC_STACK, MG_ESC_SYMBOLIC, MG_ESCAPE, MG_EXC_OUT_OF_GAS, MG_EXC_STACK_OVERFLOW,
                               MG_EXC_WRITE_PROTECTION, MG_FORK, MG_HALT_RETURN, MG_HALT_STOP, MG_VMEXC)
from mythril_amd.laser.opcodes import ADDRESS_OPCODE_MAPPING
from mythril_amd.laser.symbolic import (MG_SYM_BALANCE, MG_SYM_BIN, MG_SYM_CDBYTE, MG_SYM_CDBYTEX, MG_SYM_CDLOAD,
                                        MG_SYM_CDSIZE, MG_SYM_CONCAT, MG_SYM_ENV, MG_SYM_EXTRACT, MG_SYM_KECCAK,
                                        MG_SYM_MLOADK, MG_SYM_MSTOREK, MG_SYM_SLOAD, MG_SYM_UN)

_BYTE_OF = {name: op for op, name in ADDRESS_OPCODE_MAPPING.items()}


def asm(src: str) -> bytes:
    """Assemble whitespace-separated mnemonics; PUSHn takes the next token as its
    value (decimal or 0x hex)."""
    out = bytearray()
    toks = src.split()
    k = 0
    while k < len(toks):
        t = toks[k]
        out.append(_BYTE_OF[t])
        if t.startswith("PUSH"):
            n = int(t[4:])
            out += int(toks[k + 1], 0).to_bytes(n, "big")
            k += 1
        k += 1
    return bytes(out)


def n_instructions(src: str) -> int:
    toks = src.split()
    return len(toks) - sum(1 for t in toks if t.startswith("PUSH"))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    src: str                                  # assembly: the program's source
    steps: int                                # instructions executed on the device
    status: int                               # final status
    aux: Optional[int] = None                 # final aux (None: a halt, whose aux says nothing)
    kinds: Tuple = ()                         # (node kind, width or None) that must be in the arena
    records: Tuple = ()                       # record kinds that must be in the log
    concrete_storage: bool = False            # an empty concrete storage (every slot reads 0)
    static: bool = False                      # a static call (WriteProtection)
    creation: bool = False                    # the code of a symbolic creation, not of a message call
    calldata: Optional[bytes] = None          # concrete calldata (None: symbolic calldata)
    caps: Optional[Dict[str, int]] = None     # capacities the default shape lacks

    @property
    def code(self) -> bytes:
        return asm(self.src)


def _esc(op: str, reason: int = MG_ESC_SYMBOLIC) -> int:
    return _BYTE_OF[op] | (reason << 8)


def _stop(name, src, kinds=(), records=(), **kw) -> Case:
    """A program that runs to its final STOP: every instruction executes."""
    return Case(name, src, n_instructions(src), MG_HALT_STOP, None, tuple(kinds), tuple(records), **kw)


def _escape(name, src, op, kinds=(), records=(), **kw) -> Case:
    """A program whose last instruction `op` is the host's: MG_ESC_SYMBOLIC before it."""
    assert src.split()[-1] == op
    return Case(name, src, n_instructions(src) - 1, MG_ESCAPE, _esc(op), tuple(kinds), tuple(records), **kw)


# ---------------------------------------------------------------------------------------
# memparts: sym_mem_ref's partition of a byte range (memory.py:56-82: get_word_at is
# simplify(Concat(bytes)), byte j of a stored word w being Extract(255 - 8j, 248 - 8j, w))
# ---------------------------------------------------------------------------------------
_TWO_WORDS = "CALLER PUSH1 0 MSTORE CALLVALUE PUSH1 32 MSTORE "      # A = caller at 0, B = call value at 32


def _sweep(lo: int, hi: int) -> Case:
    """MLOAD at every offset in [lo, hi] over A at 0..31 and B at 32..63.  At offset
    32q + j (j != 0) the word is bytes j..31 of one stored word (Extract of 8 (32 - j)
    bits, hi = 255 - 8j, lo = 0) then bytes 0..j-1 of what follows: the next stored
    word (Extract of 8j bits, lo = 256 - 8j) or, past 63, zeros; j == 0 reads a
    stored word whole (no node) or, at 64, plain zeros."""
    src = _TWO_WORDS + "".join(f"PUSH1 {k} MLOAD POP " for k in range(lo, hi + 1)) + "STOP"
    kinds = set()
    for k in range(lo, hi + 1):
        q, j = divmod(k, 32)
        if j and q < 2:
            kinds.add((MG_SYM_EXTRACT, 8 * (32 - j)))
            kinds.add((MG_SYM_CONCAT, 256))
            if q == 0:
                kinds.add((MG_SYM_EXTRACT, 8 * j))
    return _stop(f"mload_sweep_{lo}_{hi}", src, sorted(kinds))


# A at 0, the constants 0x11 at 32..63 and 0x2233 at 64..95, B at 96: SHA3 over n bytes from 5
_MIXED = ("CALLER PUSH1 0 MSTORE PUSH1 0x11 PUSH1 32 MSTORE PUSH2 0x2233 PUSH1 64 MSTORE "
          "CALLVALUE PUSH1 96 MSTORE ")


def _sha3_len(n: int) -> str:
    return f"PUSH1 {n} PUSH1 5 SHA3 POP "


MEMPARTS = [
    _sweep(0, 21), _sweep(22, 43), _sweep(44, 64),
    # a load that straddles the memory's end: MLOAD at 16 of a 32-byte memory extends it
    # (mload_: mem_extend first), then reads A's bytes 16..31 and 16 zero bytes
    _stop("mload_straddles_msize", "CALLER PUSH1 0 MSTORE PUSH1 16 MLOAD POP STOP",
          [(MG_SYM_EXTRACT, 128), (MG_SYM_CONCAT, 256)]),
    # a word, then calldata bytes of a symbolic CALLDATACOPY (calldata[4..11] at 32..39):
    # MLOAD at 8 = A's bytes 8..31 (192 bits) then eight 8-bit calldata bytes
    _stop("mload_word_then_cdbytes",
          "CALLER PUSH1 0 MSTORE PUSH1 8 PUSH1 4 PUSH1 32 CALLDATACOPY PUSH1 8 MLOAD POP "
          "PUSH1 33 MLOAD POP STOP",
          [(MG_SYM_EXTRACT, 192), (MG_SYM_CDBYTE, 8), (MG_SYM_CONCAT, 200), (MG_SYM_CONCAT, 256)]),
    # SHA3 over 1, 31, 32, 33, 64 and 100 bytes from offset 5 of mixed memory.  The input
    # is simplify(Concat(memory[5 : 5 + n])) (sha3_, instructions.py:1032-1039):
    #   1: A's byte 5 (8 bits);  31..: A's bytes 5..31 (216 bits) then constants;
    #   100: A[5..31], 64 constant bytes (two constants on the device, one after the
    #   host's join), B's bytes 0..8 (72 bits)
    _stop("sha3_mixed_lengths", _MIXED + "".join(_sha3_len(n) for n in (1, 31, 32, 33, 64, 100)) + "STOP",
          [(MG_SYM_EXTRACT, 8), (MG_SYM_EXTRACT, 216), (MG_SYM_EXTRACT, 72), (MG_SYM_CONCAT, 248),
           (MG_SYM_CONCAT, 512), (MG_SYM_CONCAT, 800), (MG_SYM_KECCAK, 256)], ["symkeccak"]),
]

# ---------------------------------------------------------------------------------------
# taghygiene: writes over symbolic bytes, each followed by MLOADs of the range and of
# both neighbours (memory.py:102-115 write_word_at; mstore8_, instructions.py:1472-1493;
# _calldata_copy_helper :807-875; codecopy_ :1074-1104)
# ---------------------------------------------------------------------------------------
_THREE_WORDS = _TWO_WORDS + "CALLER PUSH1 64 MSTORE "                   # A, B, A at 0, 32, 64
_LOADS_0_32_64 = "PUSH1 0 MLOAD POP PUSH1 32 MLOAD POP PUSH1 64 MLOAD POP "
_BOOL = "CALLVALUE CALLER LT "                                          # ULT(caller, call value): a Bool


def _codecopy_tail() -> Case:
    # CODECOPY of 16 bytes from 4 bytes before the end of the code into 40..55, inside
    # the tagged word B (32..63): the four bytes of code replace bytes 40..43; past the
    # end of the code nothing is written, so 44..55 keep B's bytes (what symref's
    # _oracle_step restates, after codecopy_'s concrete branch)
    body = _THREE_WORDS + "PUSH1 16 PUSH1 {src} PUSH1 40 CODECOPY " + _LOADS_0_32_64 + "PUSH1 36 MLOAD POP STOP"
    n = len(asm(body.format(src=0)))
    return _stop("codecopy_to_code_end_in_tagged_word", body.format(src=n - 4),
                 [(MG_SYM_EXTRACT, 64), (MG_SYM_EXTRACT, 160), (MG_SYM_CONCAT, 256)])


TAGHYGIENE = [
    # a concrete MSTORE over bytes 16..47: the second half of A and the first half of B
    _stop("mstore_over_two_halves", _THREE_WORDS + "PUSH1 0x77 PUSH1 16 MSTORE " + _LOADS_0_32_64 +
          "PUSH1 16 MLOAD POP PUSH1 8 MLOAD POP STOP",
          [(MG_SYM_EXTRACT, 128), (MG_SYM_CONCAT, 256), (MG_SYM_EXTRACT, 64)]),
    # a concrete MSTORE8 at 40 splits B into bytes 0..7 (64 bits) and 9..31 (184 bits)
    _stop("mstore8_inside_word", _THREE_WORDS + "PUSH1 0xAB PUSH1 40 MSTORE8 " + _LOADS_0_32_64 +
          "PUSH1 41 MLOAD POP STOP",
          [(MG_SYM_EXTRACT, 64), (MG_SYM_EXTRACT, 184), (MG_SYM_CONCAT, 256)]),
    # MSTORE8 of a symbolic value (Extract(7, 0, call value)) into the middle of A at 64
    _stop("mstore8_symbolic_inside_word", _THREE_WORDS + "CALLVALUE PUSH1 70 MSTORE8 " + _LOADS_0_32_64 +
          "PUSH1 60 MLOAD POP STOP",
          [(MG_SYM_EXTRACT, 48), (MG_SYM_EXTRACT, 8), (MG_SYM_EXTRACT, 200), (MG_SYM_CONCAT, 256)]),
    # a Bool stored whole (If(b, 1, 0), memory.py:102-115) and read back whole and in part
    _stop("mstore_bool", _BOOL + "PUSH1 0 MSTORE PUSH1 0 MLOAD POP PUSH1 1 MLOAD POP PUSH1 31 MLOAD POP STOP"),
    _stop("mstore8_bool", _TWO_WORDS + _BOOL + "PUSH1 33 MSTORE8 PUSH1 32 MLOAD POP PUSH1 33 MLOAD POP "
          "PUSH1 2 MLOAD POP STOP"),
    # a symbolic CALLDATACOPY (calldata[0..9] to 28..37) over the end of A and the start of B
    _stop("calldatacopy_over_tagged", _THREE_WORDS + "PUSH1 10 PUSH1 0 PUSH1 28 CALLDATACOPY " + _LOADS_0_32_64 +
          "PUSH1 20 MLOAD POP STOP",
          [(MG_SYM_CDBYTE, 8), (MG_SYM_EXTRACT, 224), (MG_SYM_EXTRACT, 208), (MG_SYM_CONCAT, 256)]),
    # the same copy of concrete calldata (six bytes, so 34..37 are the zero fill past its
    # end) on a lane that is symbolic by its caller and call value: kernel 1's concrete
    # CALLDATACOPY, after which the ten bytes are concrete (calldatacopy_, :878-891)
    _stop("calldatacopy_concrete_over_tagged", _THREE_WORDS + "PUSH1 10 PUSH1 0 PUSH1 28 CALLDATACOPY " +
          _LOADS_0_32_64 + "PUSH1 20 MLOAD POP STOP",
          [(MG_SYM_EXTRACT, 224), (MG_SYM_EXTRACT, 208), (MG_SYM_CONCAT, 256)], calldata=bytes.fromhex("c1c2c3c4c5c6")),
    _codecopy_tail(),
    # CODECOPY wholly inside the code over the tagged bytes 30..33
    _stop("codecopy_over_tagged", _THREE_WORDS + "PUSH1 4 PUSH1 0 PUSH1 30 CODECOPY " + _LOADS_0_32_64 + "STOP",
          [(MG_SYM_EXTRACT, 240), (MG_SYM_CONCAT, 256)]),
    # CALLDATACOPY of a symbolic size copies 320 bytes (instructions.py:822-826)
    _stop("calldatacopy_symbolic_size", "CALLER PUSH1 0 PUSH1 0 CALLDATACOPY PUSH1 0 MLOAD POP PUSH2 300 MLOAD POP "
          "MSIZE POP STOP", [(MG_SYM_CDBYTE, 8), (MG_SYM_CONCAT, 256)], caps={"node_cap": 512}),
    # ... of a symbolic memory offset is dropped (:810-814): memory stays empty
    _stop("calldatacopy_symbolic_memory_offset", "PUSH1 32 PUSH1 0 CALLER CALLDATACOPY MSIZE POP STOP"),
    # ... of a symbolic calldata offset reads calldata[simplify(offset + k)] (:816-820)
    _stop("calldatacopy_symbolic_source", "PUSH1 4 CALLVALUE PUSH1 0 CALLDATACOPY PUSH1 0 MLOAD POP STOP",
          [(MG_SYM_CDBYTEX, 8), (MG_SYM_CONCAT, 256)]),
    # ... of size 0 copies and extends nothing
    _stop("calldatacopy_size_zero", _TWO_WORDS + "PUSH1 0 PUSH1 0 PUSH1 16 CALLDATACOPY PUSH1 0 MLOAD POP MSIZE POP STOP"),
]

# ---------------------------------------------------------------------------------------
# chain: the store-chain walk of SLOAD (account.py:43-87: simplify(Select(Store(..), k)))
# ---------------------------------------------------------------------------------------
_X = "PUSH1 0 CALLDATALOAD "                                            # x = calldata[0:32], kept on the stack
_CHAIN = (
    "PUSH1 1 SLOAD POP "                           # empty chain: a Select of the base array / 0
    "CALLER PUSH1 1 SSTORE "                       # [1] = caller
    "PUSH1 7 PUSH1 2 SSTORE "                      # [2] = 7
    "PUSH1 1 SLOAD POP "                           # skips the distinct constant 2, hits 1: the caller
    "PUSH1 2 SLOAD POP "                           # hits 2: the constant 7
    "PUSH1 3 SLOAD POP "                           # skips both: the base array / 0
    + _X +
    "DUP1 SLOAD POP "                              # x against a constant key: the walk stops, a Select
    "PUSH1 9 DUP2 SSTORE "                         # [x] = 9
    "DUP1 SLOAD POP "                              # the same term: 9
    "PUSH1 1 SLOAD POP "                           # a constant against x: the walk stops, a Select
    "PUSH1 5 PUSH1 1 DUP3 ADD SSTORE "             # [x + 1] = 5
    "PUSH1 1 DUP2 ADD SLOAD POP "                  # x + 1 built again: the same term, 5
    "PUSH1 2 DUP2 ADD SLOAD POP "                  # x + 2: a different term, a Select
    "POP STOP")
_DEEP_OPS = "".join("PUSH1 1 ADD PUSH1 3 MUL " for _ in range(10))     # 20 nested operations
# a key nested deeper than the device compares (sym_same's 32-entry stack), built twice:
# the device keeps a Select node, the host's decode finds the same hash-consed term: 5.
# Why 20 levels suffice: `PUSH1 c OP` makes the constant the first pop (operand y) and the
# nested term the second (z).  sym_same pushes the y pair, then the z pair, and pops the z
# pair first, so every level leaves its pair of constants on the stack while it descends:
# two entries a level, and `top + 4 > 32` answers false at level 15.  With the constant
# as z the stack would not grow and the device would fold the Select; the SLOAD node the
# cases demand (DEVICE_ONLY below) is what tells the two apart.
_DEEP = _X + "PUSH1 5 DUP2 " + _DEEP_OPS + "SSTORE " + _DEEP_OPS + "SLOAD POP STOP"

CHAIN = [
    _stop("chain_symbolic_base", _CHAIN, [(MG_SYM_SLOAD, 256), (MG_SYM_CDLOAD, 256), (MG_SYM_BIN, 256)]),
    _stop("chain_concrete_base", _CHAIN, [(MG_SYM_SLOAD, 256)], concrete_storage=True),
    _stop("chain_deep_key_symbolic_base", _DEEP, [(MG_SYM_SLOAD, 256)]),
    _stop("chain_deep_key_concrete_base", _DEEP, [(MG_SYM_SLOAD, 256)], concrete_storage=True),
]
# kinds only the device's arena shows: the host's decode folds the Select away
DEVICE_ONLY = {"chain_deep_key_symbolic_base": [(MG_SYM_SLOAD, 256)],
               "chain_deep_key_concrete_base": [(MG_SYM_SLOAD, 256)]}

# ---------------------------------------------------------------------------------------
# aluquirks (instructions.py:356-800): every binary opcode of sym_bin_ok, ISZERO and NOT
# over concrete/symbolic, symbolic/concrete, symbolic/symbolic operands and a Bool on
# either side; the folds; the escapes
# ---------------------------------------------------------------------------------------
BIN_OPS = ("ADD", "MUL", "SUB", "DIV", "SDIV", "MOD", "SMOD", "LT", "GT", "SLT", "SGT", "EQ", "AND", "OR", "XOR",
           "BYTE", "SHL", "SHR", "SAR")
_CMP = ("LT", "GT", "SLT", "SGT", "EQ")
_OPERAND = {"c": "PUSH1 5 ", "s": "CALLVALUE ", "t": "CALLER ", "b": _BOOL}


def _alu(op: str) -> Case:
    """`op` on (first pop, second pop) = (5, call value), (call value, 5), (call value,
    caller), (Bool, call value), (call value, Bool); the second pop is pushed first.
    XOR of a Bool and BYTE with a symbolic index are the host's (below)."""
    pairs = [("c", "s"), ("s", "c"), ("s", "t"), ("b", "s"), ("s", "b")]
    if op == "XOR":
        pairs = pairs[:3]
    if op == "BYTE":
        pairs = [("c", "s"), ("c", "b")]
    src = "".join(_OPERAND[y] + _OPERAND[x] + op + " POP " for x, y in pairs) + "STOP"
    return _stop(f"alu_{op}", src, [(MG_SYM_BIN, 1 if op in _CMP else 256)])


ALUQUIRKS = [_alu(op) for op in BIN_OPS] + [
    _stop("alu_ISZERO_NOT", "CALLVALUE ISZERO POP CALLVALUE NOT POP " + _BOOL + "ISZERO POP " + _BOOL +
          "ISZERO ISZERO POP STOP", [(MG_SYM_UN, 256)]),
    # a concrete zero divisor gives a fresh 0 (div_, instructions.py:505-519); a symbolic one does not
    _stop("alu_zero_divisor", "".join(f"PUSH1 0 CALLVALUE {op} POP CALLVALUE PUSH1 0 {op} POP CALLER CALLVALUE {op} POP "
                                      for op in ("DIV", "SDIV", "MOD", "SMOD")) + "STOP", [(MG_SYM_BIN, 256)]),
    # a concrete BYTE index >= 32 gives 0 (byte_, :427-455); index 31 and 0 do not
    _stop("alu_byte_index", "CALLVALUE PUSH1 32 BYTE POP CALLVALUE PUSH2 0x100 BYTE POP "
          "CALLVALUE PUSH32 0x8000000000000000000000000000000000000000000000000000000000000000 BYTE POP "
          "CALLVALUE PUSH1 31 BYTE POP CALLVALUE PUSH1 0 BYTE POP STOP", [(MG_SYM_BIN, 256)]),
    # x == x folds to 1: the same stack word, the same term built twice, and a nested one
    _stop("alu_eq_same_term", "CALLVALUE DUP1 EQ POP CALLVALUE CALLVALUE EQ POP "
          "PUSH1 1 CALLVALUE ADD PUSH1 1 CALLVALUE ADD EQ POP PUSH1 2 CALLVALUE ADD PUSH1 1 CALLVALUE ADD EQ POP STOP",
          [(MG_SYM_BIN, 256), (MG_SYM_BIN, 1)]),
    # EXP of a symbolic operand: Power(base, exponent) and the manager's condition (:624-638)
    _stop("alu_exp_symbolic", "CALLVALUE PUSH1 2 EXP POP PUSH1 3 CALLVALUE EXP POP STOP", [(MG_SYM_BIN, 256)],
          ["symexp"]),
    _escape("esc_not_bool", _BOOL + "NOT", "NOT"),
    _escape("esc_xor_bool_first", "CALLVALUE " + _BOOL + "XOR", "XOR"),
    _escape("esc_xor_bool_second", _BOOL + "CALLVALUE XOR", "XOR"),
    _escape("esc_exp_bool", "PUSH1 2 " + _BOOL + "EXP", "EXP"),
    _escape("esc_balance_bool", _BOOL + "BALANCE", "BALANCE"),
    _escape("esc_sha3_bool_length", "CALLER PUSH1 0 MSTORE " + _BOOL + "PUSH1 0 SHA3", "SHA3"),
    _escape("esc_byte_symbolic_index", "CALLER CALLVALUE BYTE", "BYTE"),
    _escape("esc_addmod", "PUSH1 7 PUSH1 1 CALLVALUE ADDMOD", "ADDMOD"),
    _escape("esc_mulmod", "PUSH1 7 CALLVALUE PUSH1 2 MULMOD", "MULMOD"),
    _escape("esc_signextend", "CALLVALUE PUSH1 0 SIGNEXTEND", "SIGNEXTEND"),
]

# escapes the restatement has no semantics for (symref raises Unsupported: the host's
# reference steps them); the others are Bool operands, which the restatement's stack
# holds as If(b, 1, 0) and steps like any word
NO_RESTATEMENT = {"esc_byte_symbolic_index", "esc_addmod", "esc_mulmod", "esc_signextend"}

# ---------------------------------------------------------------------------------------
# stops: one program that consumes every per-lane resource through every block that can
# exhaust it; at most about 48 nodes, 16 constants, 6 records, 8 chain entries, 20 stack words
# ---------------------------------------------------------------------------------------
_CONSUME = (
    "CALLER CALLVALUE ADD "                        # ENV, ENV, BIN                         [s]
    "PUSH1 4 CALLDATALOAD "                        # x: CDLOAD with a constant operand    [s x]
    "DUP1 ISZERO "                                 # UN                                    [s x z]
    "CALLDATASIZE GAS "                            # n: CDSIZE; a fresh ENV word          [s x z n g]
    "DUP4 PUSH1 0 MSTORE "                         # x into memory at 0
    "PUSH1 3 MLOAD "                               # EXTRACT, a constant, CONCAT           6 words
    "PUSH1 32 PUSH1 0 SHA3 "                       # KECCAK over symbolic memory, a record 7
    "PUSH1 4 PUSH1 8 PUSH1 40 CALLDATACOPY "       # four CDBYTE nodes
    "PUSH1 40 MLOAD "                              # the four bytes and a constant, CONCATs 8
    "DUP7 SLOAD "                                  # SLOAD of the symbolic key x           9
    "PUSH1 1 DUP9 SSTORE PUSH1 2 PUSH1 9 SSTORE DUP1 PUSH1 3 SSTORE "   # [x] = 1, [9] = 2, [3] = the read
    "PUSH1 9 SLOAD "                               # a hit past a distinct constant: 2     10
    "PUSH1 2 DUP10 EXP "                           # Power(x, 2): BIN, a record            11
    "PUSH1 7 DUP11 MSTORE "                        # MSTOREK at the symbolic offset x, a constant
    "DUP10 MLOAD "                                 # MLOADK                                12
    "PUSH1 32 DUP12 SHA3 "                         # MLOADK + KECCAK at a symbolic offset, a record  13
    "DUP10 PUSH1 0 SHA3 "                          # SHA3 of the symbolic length n: two records      14
    "DUP13 BALANCE "                               # BALANCE node                          15
    "PUSH1 4 DUP2 SSTORE PUSH1 5 PUSH1 6 SSTORE "  # two more chain entries
    "CALLER PUSH1 0 PUSH1 0 LOG1 "                 # a LOG with a symbolic topic: popped, its gas
    "CALLER CALLVALUE TIMESTAMP CALLDATASIZE GAS DUP1 "   # pushes of every kind, to 21 words
    "STOP")
CONSUME = _stop("consume", _CONSUME,
                [(MG_SYM_ENV, 256), (MG_SYM_BIN, 256), (MG_SYM_CDLOAD, 256), (MG_SYM_UN, 256), (MG_SYM_CDSIZE, 256),
                 (MG_SYM_EXTRACT, 232), (MG_SYM_CONCAT, 256), (MG_SYM_KECCAK, 256), (MG_SYM_CDBYTE, 8),
                 (MG_SYM_SLOAD, 256), (MG_SYM_MSTOREK, None), (MG_SYM_MLOADK, 256), (MG_SYM_BALANCE, 256)],
                ["symkeccak", "symexp", "symlen"])

# (c) the stack limit: a caller and 1022 (1023) DUP1s leave 1023 (1024) words, then one push
_PUSHERS = ("CALLER", "CALLDATASIZE", "GAS")


def _filled(n: int) -> str:
    return "CALLER " + "DUP1 " * (n - 1)


STACK_LIMIT = (
    # 1023 words, one more is the 1024th: it runs
    [_stop(f"stack_1023_then_{p}", _filled(1023) + p + " STOP") for p in _PUSHERS] +
    # 1024 words: StackOverflowException (machine_state.py:32-43), a VmException counted as a step
    [Case(f"stack_1024_then_{p}", _filled(1024) + p, 1025, MG_VMEXC, MG_EXC_STACK_OVERFLOW) for p in _PUSHERS] +
    # a stack plane of 1023 rows: the lane stops for the host to regrow it, before the push
    [Case(f"stack_cap_1023_then_{p}", _filled(1023) + p + " STOP", 1023, MG_ESCAPE, _esc(p, MG_ESC_STACK),
          caps={"stack_cap": 1023}) for p in _PUSHERS] +
    # a creation's CODESIZE (the code's size + 0x200, with calldata.size pinned to it: a record)
    [_stop("creation_stack_1023_then_CODESIZE", _filled(1023) + "CODESIZE STOP", records=["cdsize"], creation=True),
     Case("creation_stack_1024_then_CODESIZE", _filled(1024) + "CODESIZE", 1025, MG_VMEXC, MG_EXC_STACK_OVERFLOW,
          creation=True),
     Case("creation_stack_cap_1023_then_CODESIZE", _filled(1023) + "CODESIZE STOP", 1023, MG_ESCAPE,
          _esc("CODESIZE", MG_ESC_STACK), caps={"stack_cap": 1023}, creation=True)])

# (d) a static call: SSTORE and LOG0..LOG4 with a symbolic operand raise WriteProtection
# (StateTransition, instructions.py:98-202), counted as an executed step
STATIC = [Case("static_sstore", "CALLER PUSH1 1 SSTORE", 3, MG_VMEXC, MG_EXC_WRITE_PROTECTION, static=True)] + [
    Case(f"static_log{n}", "CALLER " * n + "PUSH1 0 " + ("CALLER " if n == 0 else "PUSH1 0 ") + f"LOG{n}",
         n + 3, MG_VMEXC, MG_EXC_WRITE_PROTECTION, static=True) for n in range(5)]
# the same opcodes in an ordinary call run: the words are popped (log_, :1710-1723)
LOGS = [_stop(f"log{n}", "CALLER " * n + "PUSH1 0 " + ("CALLER " if n == 0 else "PUSH1 0 ") + f"LOG{n} STOP")
        for n in range(5)]

# a JUMPI on a symbolic condition: the lane stops with MG_FORK before it
FORK = Case("fork", "JUMPDEST CALLER PUSH1 0 MSTORE PUSH1 0 MLOAD PUSH1 1 SLOAD POP PUSH1 32 PUSH1 0 SHA3 POP "
                    "PUSH1 0 JUMPI", 14, MG_FORK, 0x57, ((MG_SYM_KECCAK, 256),), ("symkeccak",))

# three more places where gas is counted on a symbolic path, for the gas sweep:
# RETURNDATACOPY of a symbolic size (returndatacopy_, instructions.py:1314-1343: the words
# are popped, the table gas, the check); a JUMPI to a symbolic target (jumpi_, :1572-1579:
# falls through with its gas added by hand and no check, so the gas may pass the limit);
# RETURN of a concrete length at a symbolic offset (return_, :1858-1870: check_gas_usage_limit,
# which is what stops a lane the JUMPI took past its limit)
GAS_TAIL = Case("gas_tail", "CALLER PUSH1 0 PUSH1 0 RETURNDATACOPY PUSH1 32 CALLER PUSH1 1 CALLER JUMPI RETURN",
                10, MG_HALT_RETURN)

FAMILIES = {"memparts": MEMPARTS, "taghygiene": TAGHYGIENE, "chain": CHAIN, "aluquirks": ALUQUIRKS,
            "stacklimit": STACK_LIMIT, "static": STATIC, "logs": LOGS, "stops": [CONSUME, FORK, GAS_TAIL]}
ALL = [c for cases in FAMILIES.values() for c in cases]
GAS_SWEPT = MEMPARTS + [CONSUME, GAS_TAIL]
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)


# ---------------------------------------------------------------------------------------
# the restatement's account of a case (no device): used by both test modules
# ---------------------------------------------------------------------------------------
def initial_state(case: Case, gas_limit: int = 8_000_000):
    import symcosim
    if case.creation:
        return symcosim.initial_creation(case.code, gas_limit=gas_limit)
    ws, addr = symcosim.deploy_code(case.code, case.concrete_storage)
    return symcosim.initial(ws, addr, gas_limit=gas_limit, static=case.static, calldata=case.calldata)


def restate(case: Case, gas_limit: int = 8_000_000, eng=None):
    """Run the restatement from the case's first state until it ends, raises or
    leaves an instruction to the host.  Returns (the states before each
    instruction, how it ended): "stop" / "exception" / ..., "fork", or
    "unsupported" (the restatement has no semantics: the host's reference does)."""
    eng = eng or symref.Engine()
    s = initial_state(case, gas_limit)
    states = [s]
    while True:
        before = len(eng.ended)
        try:
            succ = eng.step(s)
        except symref.Unsupported:
            return states, "unsupported"
        if len(succ) == 1:
            s = succ[0]
            states.append(s)
        elif not succ:
            assert len(eng.ended) == before + 1
            return states, eng.ended[-1][0]
        else:
            return states, "fork"


def expected_under_gas(case: Case, gas_limit: int):
    """(steps, status, aux) of the device lane of a case that runs to its STOP or
    RETURN, under this gas limit: where the restatement raises (only the limit
    differs from the run that reaches the halt, so what it raises is
    OutOfGasException), or the case's own end if the restatement gets there."""
    halt = {MG_HALT_STOP: "stop", MG_HALT_RETURN: "return"}[case.status]
    states, end = restate(case, gas_limit)
    n = len(states) - 1
    if (n, end) == (case.steps - 1, halt):
        return case.steps, case.status, case.aux
    if end == "exception":
        return n + 1, MG_VMEXC, MG_EXC_OUT_OF_GAS
    # the SHA3 of a symbolic length that runs out of gas: the reference has appended
    # `length == 64` before the check, so the device leaves it to the host
    assert end == "unsupported", (case.name, gas_limit, end)
    return n, MG_ESCAPE, _esc(states[-1].environment.code.instruction_list[states[-1].mstate.pc]["opcode"])


def gas_limits(case: Case):
    """c - 1, c and c + 1 for every cumulative min_gas_used c the restatement reaches."""
    states, _ = restate(case)
    cs = sorted({s.mstate.min_gas_used for s in states})
    return sorted({c + d for c in cs for d in (-1, 0, 1) if c + d > 0})
