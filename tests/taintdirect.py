"""Directed programs for the taint stepper of k_sym_step (sym_step.cuh: t_result_mask,
t_commit, t_gc and the action block): one list per family of paths the C2 /
crafted-code co-simulation of tests/test_gpu_taint.py does not reach -- the
annotation set of every ALU result, slots refilled by plain pushes, object
identity through DUP / SWAP / the environment, handle compaction, the atom and
record capacities, rollback and stack underflow, and the yield conditions.

Every program is a concrete message call written as assembly (symdirect.asm).
Every case carries a hand-written outcome -- the instructions executed, the
final status and aux, the atom count, the sink and yield masks, the environment
objects' masks, the kinds of the records in log order and the final stack as
(object class, atom set) per slot -- so that a lane which stops early on the
device and in the restatement alike cannot pass.  The outcomes are worked out
from the reference's semantics as tests/taintref.py cites them, and
tests/test_taint_directed_cpu.py pins them against the restatement without a
GPU.  Never from a device run.

Stack underflow.  svm.py:391-402 raises the underflow of an instruction that has
fewer stack elements than the opcode table requires BEFORE the pre-hooks of
:405, so no batch-safe action (annotation, deferred record, yield, if-lane
yield, atom or record capacity escape) applies there: the lane ends with the VM
exception.  The table's counts are the reference's own (support/opcodes.py):
ADD 2, SLOAD 1, JUMPI 2 -- but SSTORE 1, so an SSTORE over one word passes the
check, its pre-hooks do run, and the mutator's pop raises afterwards.  On the
device that is a record written and rolled back with the exception, or, when
the log has no room for the record, MG_ESC_RECORD (the host then runs the hook
and raises).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Tuple

import numpy as np

from mythril_amd.lanes import (MG_ESC_RECORD, MG_ESC_TAINT, MG_ESCAPE, MG_EXC_OUT_OF_GAS, MG_EXC_STACK_OVERFLOW,
                               MG_EXC_STACK_UNDERFLOW, MG_HALT_STOP, MG_HOOK, MG_LANE_HOOK_ACK, MG_LANE_TAINT,
                               MG_REC_ANNOT_WORDS, MG_REC_HEADER, MG_TAINT_EXPCOND, MG_TAINT_IFLANE, MG_TAINT_OBJ0,
                               MG_TAINT_POST, MG_TAINT_YCLASS, MG_VMEXC, LaneBatch, LaneShape, word_to_limbs)
from mythril_amd.laser.opcodes import OPCODES
from symdirect import asm, n_instructions
from taintref import UNION2, ZERODIV

# ---------------------------------------------------------------------------------------
# action tables
# ---------------------------------------------------------------------------------------
# the table of tests/test_gpu_taint.py (test_taint_directed_cpu.py pins the two equal)
DEFAULT_ACTIONS = {
    "ADD": 1, "MUL": 1, "SUB": 1, "EXP": 1 | MG_TAINT_EXPCOND,
    "SSTORE": (2 << 8) | (1 << 16),
    "JUMPI": (2 << 8) | (2 << 12) | (1 << 20),
    "ORIGIN": MG_TAINT_POST | MG_TAINT_YCLASS,
    "MSTORE": 2 << 16,
    "JUMP": (1 << 16) | (1 << 20),
    "SLOAD": MG_TAINT_IFLANE,
}
# family `result`: PUSH2 pushes an annotated word (a post-hook), nothing else acts, so
# that the opcode under test sees exactly the operands' sets
PUSH2_POST = {"PUSH2": MG_TAINT_POST}
EXP_COND = {"EXP": 1 | MG_TAINT_EXPCOND}
# family `capacity`: MUL with a pre-hook and a post-hook (two atoms), SUB with pre-hook,
# deferred hook and post-hook at once
CAP_ACTIONS = dict(DEFAULT_ACTIONS, MUL=1 | MG_TAINT_POST, SUB=1 | MG_TAINT_POST | (1 << 16))
# family `rollback`: post-hooks on a DUP and a PUSH
LIMIT_ACTIONS = dict(DEFAULT_ACTIONS, DUP1=MG_TAINT_POST, PUSH1=MG_TAINT_POST)


def action_words(table: Dict[str, int]) -> np.ndarray:
    out = np.zeros(256, dtype=np.uint32)
    for name, w in table.items():
        out[OPCODES[name]] = w
    return out


ANNOT_WORDS = MG_REC_ANNOT_WORDS              # an MG_REC_ANNOT record
HOOK1_WORDS = MG_REC_HEADER + 3               # an MG_REC_HOOK record of one word

CALLER = 0xDEADBEEF
ADDRESS = 0xAFFE


@dataclasses.dataclass(frozen=True)
class Outcome:
    steps: int                       # instructions executed
    status: int
    aux: Optional[int]               # None: a halt, whose aux says nothing
    n_atoms: int
    sink: int
    ymask: int
    env: Tuple[int, ...]             # masks of ADDRESS, CALLER, ORIGIN, CALLVALUE, GASPRICE, calldata size
    records: Tuple                   # ("pre", atom) / ("post", atom) / ("hook", n) / ("exp",) / ("keccak",)
    stack: Tuple                     # per slot (object class by first appearance, atom mask)
    tflags: int = 0


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str
    src: str
    out: Outcome
    actions: Tuple = tuple(sorted(DEFAULT_ACTIONS.items()))
    obj_cap: int = 64
    rec_cap: int = 512
    stack_cap: int = 64
    gas_limit: int = 8_000_000
    n_atoms: int = 0
    tflags: int = 0
    ymask: int = 0
    rec_len: int = 0                 # words of the log already in use
    flags: int = 0                   # lane flags besides MG_LANE_TAINT
    stack0: Tuple = ()               # preloaded stack: (word, handle) per slot
    omask0: Tuple = ()               # preloaded object masks: (handle, mask)
    n_fixed: int = MG_TAINT_OBJ0     # host handles end here; n_obj starts past the preloaded ones
    n_obj: int = MG_TAINT_OBJ0
    force: Tuple = ()                # (instruction index, flag) of set_taint_force
    dev_n_obj: Optional[int] = None  # the device's n_obj at the end (at this obj_cap)
    slots: Tuple = ()                # (slot, handle) that must hold at the end
    masks: Tuple = ()                # (handle, mask) that must hold at the end
    out_uncapped: Optional[Outcome] = None    # the outcome at obj_cap 64, where it differs

    @property
    def code(self) -> bytes:
        return asm(self.src)

    @property
    def shape_key(self):
        return (self.actions, self.obj_cap, self.rec_cap, self.stack_cap)


def _acts(table) -> Tuple:
    return tuple(sorted(table.items()))


def _esc(op: str, reason: int) -> int:
    return OPCODES[op] | (reason << 8)


NO_ENV = (0, 0, 0, 0, 0, 0)


def _stop(src, n_atoms, records, stack, sink=0, ymask=0, env=NO_ENV, tflags=0) -> Outcome:
    """The program runs to its final STOP: every instruction executes."""
    assert src.split()[-1] == "STOP"
    return Outcome(n_instructions(src), MG_HALT_STOP, None, n_atoms, sink, ymask, tuple(env), tuple(records),
                   tuple(stack), tflags)


def _pre(*atoms):
    return [("pre", a) for a in atoms]


def T(v: int) -> str:
    """An annotated word of value v under the integer action: ADD's pre-hook gives
    the 0 on top a new atom and the sum takes the union (three instructions, one
    atom, one record, two object handles of which the first is dead at once)."""
    return f"PUSH1 {v} PUSH1 0 ADD "


# ---------------------------------------------------------------------------------------
# a. result: the annotation set of a pushed word (t_result_mask; bitvec.py's unions)
# ---------------------------------------------------------------------------------------
_NAME = {b: n for n, b in OPCODES.items()}


def _operand(v: int, annotated: bool) -> str:
    if not annotated:
        return f"PUSH1 {v} " if v < 256 else f"PUSH32 {v} "
    if v < 65536:
        return f"PUSH2 {v} "
    return f"PUSH32 {v} PUSH2 0 ADD "          # ADD has no action here: the sum takes the 0's atom


def _result(tag, op, vals, ann, carry, actions=PUSH2_POST, extra_records=()) -> Case:
    """`op` over vals = [stack[-1], stack[-2], ...] with the operands in `ann`
    annotated (one atom each, numbered in push order: deepest first); the pushed
    word must carry the atoms of the operands in `carry`."""
    src, atom, k = "", {}, 0
    if not ann:
        # an annotated word pushed and popped first: its slot's handle must not come back
        src, k = "PUSH2 9 POP ", 1
    for idx in reversed(range(len(vals))):
        src += _operand(vals[idx], idx in ann)
        if idx in ann:
            atom[idx] = k
            k += 1
    src += f"{op} STOP"
    mask = 0
    for idx in carry:
        if idx in atom:
            mask |= 1 << atom[idx]
    records = [("post", j) for j in range(k)] + list(extra_records) + ([("exp",)] if op == "EXP" else [])
    # "none": handle 0 in the slot and no object made by the opcode
    n_obj = MG_TAINT_OBJ0 + k + (1 if mask else 0) + sum(1 for i in ann if vals[i] >= 65536)
    return Case(f"{tag}_{op.lower()}_{'_'.join(map(str, sorted(ann))) or 'none'}", "result", src,
                _stop(src, k, records, [(0, mask)]), actions=_acts(actions), dev_n_obj=n_obj)


def _patterns(n):
    return [{0}, {1}] + ([{2}] if n == 3 else []) + [set(range(n)), set()]


RESULT = []
for _b in sorted(UNION2):
    for _ann in _patterns(2):
        RESULT.append(_result("u2", _NAME[_b], [5, 3], _ann, (0, 1)))
for _b in sorted(ZERODIV):
    for _div in (0, 3):
        for _ann in _patterns(2):
            # a concrete zero divisor pushes a fresh 0 (instructions.py:505-592)
            RESULT.append(_result(f"div{_div}", _NAME[_b], [7, _div], _ann, () if _div == 0 else (0, 1)))
for _op in ("ADDMOD", "MULMOD"):
    for _mod in (0, 5):
        for _ann in _patterns(3):
            RESULT.append(_result(f"mod{_mod}", _op, [7, 9, _mod], _ann, (0, 1, 2)))
for _op in ("ISZERO", "NOT"):
    for _ann in ({0}, set()):
        RESULT.append(_result("un", _op, [6], _ann, (0,)))
for _idx in (0, 31, 32, 1 << 32, (1 << 64) + 5, 1 << 255):
    # BYTE keeps the value's set for an index inside the word, never the index's
    # (instructions.py:426-456); 2^32 and 2^64 + 5 have a low limb below 32
    for _ann in ({1}, {0}, {0, 1}, set()):
        RESULT.append(_result(f"idx{_idx:x}", "BYTE", [_idx, 0xA1B2], _ann, (1,) if _idx < 32 else ()))
for _base in (0, 1, 2, 1 << 32, (1 << 32) + 1):
    for _ex in (0, 1, 1 << 32):
        # integer.py:161-166: the pre-hook annotates the base unless exponent == 0 or
        # base < 2; 2^32 has low limb 0
        _hit = _ex != 0 and _base >= 2
        _src = f"PUSH32 {_ex} PUSH32 {_base} EXP STOP"
        RESULT.append(Case(f"exp_{_base:x}_{_ex:x}", "result", _src,
                           _stop(_src, int(_hit), (_pre(0) if _hit else []) + [("exp",)], [(0, int(_hit))]),
                           actions=_acts(EXP_COND), dev_n_obj=MG_TAINT_OBJ0 + 2 * int(_hit)))

# ---------------------------------------------------------------------------------------
# b. fresh: a pushed word with no set clears the slot's old handle
# ---------------------------------------------------------------------------------------
# (name, the code that pops the annotated word(s) pushed from byte 2 on, records,
# sink): byte offsets are for a program that starts with `PUSH1 9`
_POPPERS = [
    ("pop", T(1) + "POP ", _pre(0), 0),
    ("mstore", T(1) + "PUSH1 0 MSTORE ", _pre(0) + [("hook", 2)], 0),
    ("sstore", T(1) + "PUSH1 0 SSTORE ", _pre(0) + [("hook", 1)], 1),      # the value's set is collected
    ("jump", T(8) + "JUMP JUMPDEST ", _pre(0) + [("hook", 1)], 0),
    ("jumpi_taken", T(1) + "PUSH1 10 JUMPI JUMPDEST ", _pre(0), 1),       # the condition's set is collected
    ("jumpi_not", T(0) + "PUSH1 10 JUMPI JUMPDEST ", _pre(0), 1),
    ("log1", T(1) + "PUSH1 0 PUSH1 0 LOG1 ", _pre(0), 0),
]
_FILLERS = [
    ("push1", "PUSH1 7 ", []), ("push32", f"PUSH32 {(1 << 255) + 1} ", []), ("mload", "PUSH1 0 MLOAD ", []),
    ("sload", "PUSH1 0 SLOAD ", []), ("cdload", "PUSH1 0 CALLDATALOAD ", []), ("cdsize", "CALLDATASIZE ", []),
    ("pc", "PC ", []), ("msize", "MSIZE ", []), ("sha3", "PUSH1 32 PUSH1 0 SHA3 ", [("keccak",)]),
]
FRESH = []
for _pn, _pc, _pr, _ps in _POPPERS:
    for _fn, _fc, _fr in _FILLERS:
        # the anchor, the filler as an object of its own without atoms, its DUP: the
        # copy shares the filler's (new) object, not the popped one's
        _src = "PUSH1 9 " + _pc + _fc + "DUP1 STOP"
        FRESH.append(Case(f"fresh_{_pn}_{_fn}", "fresh", _src,
                          _stop(_src, 1, _pr + _fr, [(0, 0), (1, 0), (1, 0)], sink=_ps, tflags=1 if _ps else 0)))

# ---------------------------------------------------------------------------------------
# c. identity: DUPn pushes stack[-n] itself, SWAPn swaps the references, the environment
# opcodes push the environment's own objects (instructions.py:325-338, 895-955)
# ---------------------------------------------------------------------------------------
IDENTITY = []
for _n in (1, 2, 15, 16):
    _src = T(1) + "".join(f"PUSH1 {k} " for k in range(2, _n + 1)) + f"DUP{_n} STOP"
    IDENTITY.append(Case(f"dup{_n}_annotated", "identity", _src,
                         _stop(_src, 1, _pre(0), [(0, 1)] + [(k, 0) for k in range(1, _n)] + [(0, 1)])))
    _src = T(1) + "".join(f"PUSH1 {k} " for k in range(2, _n + 2)) + f"SWAP{_n} STOP"
    IDENTITY.append(Case(f"swap{_n}_annotated", "identity", _src,
                         _stop(_src, 1, _pre(0), [(k, 0) for k in range(_n)] + [(_n, 1)])))
_src = "PUSH1 5 DUP1 DUP1 PUSH1 0 SWAP1 ADD STOP"
# 5 5' 5'' -> 5 5' 0 5'' -> ADD annotates 5'' = the one object: both copies left carry it
IDENTITY.append(Case("dup_then_annotate_a_copy", "identity", _src, _stop(_src, 1, _pre(0), [(0, 1), (0, 1), (1, 1)])))
_ANN_ENV = "PUSH1 0 SWAP1 {} POP "           # annotates the environment word on top, drops the result
_src = "CALLER " + _ANN_ENV.format("ADD") + "CALLER ORIGIN STOP"
# the caller object carries atom 0; ORIGIN (same value) is another object: only its own post atom
IDENTITY.append(Case("caller_again_origin_apart", "identity", _src,
                     _stop(_src, 2, _pre(0) + [("post", 1)], [(0, 1), (1, 2)], ymask=2, env=(0, 1, 2, 0, 0, 0))))
_src = ("ADDRESS " + _ANN_ENV.format("ADD") + "CALLVALUE " + _ANN_ENV.format("MUL") + "GASPRICE " +
        _ANN_ENV.format("SUB") + "ADDRESS CALLVALUE GASPRICE CALLER STOP")
IDENTITY.append(Case("env_objects_apart", "identity", _src,
                     _stop(_src, 3, _pre(0, 1, 2), [(0, 1), (1, 2), (2, 4), (3, 0)], env=(1, 0, 0, 2, 4, 0))))
_src = "CALLER " + _ANN_ENV.format("ADD") + T(7) + "CALLER SWAP1 DUP2 STOP"
IDENTITY.append(Case("swap_env_with_device_object", "identity", _src,
                     _stop(_src, 2, _pre(0, 1), [(0, 1), (1, 2), (0, 1)], env=(0, 1, 0, 0, 0, 0))))

# ---------------------------------------------------------------------------------------
# d. compaction (t_gc).  obj_cap 16: t_gc runs before an instruction once n_obj >= 13.
# Each T() takes two handles (the annotated 0, dead at once, and the sum), so after
# T(1) T(2) T(3) the table reads 7d 8 9d 10 11d 12 (d = dead) and n_obj = 13.
# ---------------------------------------------------------------------------------------
def _gc(name, src, out, dev_n_obj, **kw) -> Case:
    return Case(name, "compaction", src, out, obj_cap=16, dev_n_obj=dev_n_obj, **kw)


COMPACTION = []
# (i) at an opcode with an action: 8, 10, 12 -> 7, 8, 9; ADD annotates the top (atom 3)
# and the sum takes {2, 3} | {1}
_src = T(1) + T(2) + T(3) + "ADD STOP"
COMPACTION.append(_gc("gc_at_action", _src, _stop(_src, 4, _pre(0, 1, 2, 3), [(0, 1), (1, 14)]), 11))
# (ii) at an opcode without one (PUSH1): live 8 {0} and 12 {2}, dead 7 9 10 11
_src = T(1) + T(2) + "POP " + T(3) + "PUSH1 4 POP DUP1 DUP3 STOP"
COMPACTION.append(_gc("gc_at_plain", _src, _stop(_src, 3, _pre(0, 1, 2), [(0, 1), (1, 4), (1, 4), (0, 1)]), 9))
# (iii) a DUP-shared pair survives (8 8 12 -> 7 7 8 before the POP) and is annotated
# afterwards: every slot of the pair gets atom 3
_src = T(1) + "DUP1 " + T(2) + "POP " + T(3) + "POP DUP1 PUSH1 0 SWAP1 ADD STOP"
COMPACTION.append(_gc("gc_shared_pair", _src, _stop(_src, 4, _pre(0, 1, 2, 3), [(0, 9), (0, 9), (1, 9)]), 10))
# (iv) host handles 7 (no longer on the stack) and 8 (slot 0) below n_fixed = 9: both
# keep number and mask; the device's 10 and 12 become 9 and 10
_src = T(1) + T(2) + "POP DUP1 DUP3 STOP"
COMPACTION.append(_gc("gc_host_handles", _src,
                      Outcome(n_instructions(_src), MG_HALT_STOP, None, 4, 0, 0, NO_ENV, tuple(_pre(2, 3)),
                              ((0, 2), (1, 4), (1, 4), (0, 2))), 11,
                      n_atoms=2, stack0=((5, 8),), omask0=((7, 1), (8, 2)), n_fixed=9, n_obj=9,
                      slots=((0, 8), (3, 8)), masks=((7, 1), (8, 2))))
# (v) a stack of 20 slots, objects at 0, 18 and 19; SWAP16 (no action) compacts, then
# moves the top object to slot 3
_src = T(1) + "".join(f"PUSH1 {k} " for k in range(17)) + T(2) + T(3) + "SWAP16 STOP"
_stk = [(s, 0) for s in range(20)]
_stk[0], _stk[3], _stk[18] = (0, 1), (3, 4), (18, 2)
COMPACTION.append(_gc("gc_deep_stack", _src, _stop(_src, 3, _pre(0, 1, 2), _stk), 10))
# (vi) two compactions: at the POPs after T(3) and after T(5) (n_obj 13 -> 9 each time)
_src = T(1) + T(2) + "POP " + T(3) + "POP " + T(4) + "POP " + T(5) + "POP " + T(6) + "POP DUP1 STOP"
COMPACTION.append(_gc("gc_twice", _src, _stop(_src, 6, _pre(0, 1, 2, 3, 4, 5), [(0, 1), (0, 1)]), 11))
# (vii) six live device objects: after compaction n_obj = 13 still: MG_ESC_TAINT before
# the PUSH1, nothing changed; at obj_cap 64 the program runs to its STOP
_src = "".join(T(k) for k in range(1, 7)) + "PUSH1 9 STOP"
_six = [(k, 1 << k) for k in range(6)]
COMPACTION.append(_gc("gc_all_live", _src,
                      Outcome(18, MG_ESCAPE, _esc("PUSH1", MG_ESC_TAINT), 6, 0, 0, NO_ENV,
                              tuple(_pre(0, 1, 2, 3, 4, 5)), tuple(_six)), 13,
                      out_uncapped=_stop(_src, 6, _pre(0, 1, 2, 3, 4, 5), _six + [(6, 0)])))
# (viii) the acknowledged instruction at a full table: no action word, but the table
# check stands; at obj_cap 64 the acknowledged ADD runs without its hook
_src = "ADD STOP"
COMPACTION.append(_gc("gc_acked_full", _src,
                      Outcome(0, MG_ESCAPE, _esc("ADD", MG_ESC_TAINT), 6, 0, 0, NO_ENV, (), tuple(_six)), 13,
                      n_atoms=6, flags=MG_LANE_HOOK_ACK, n_obj=13,
                      stack0=tuple((k + 1, MG_TAINT_OBJ0 + k) for k in range(6)),
                      omask0=tuple((MG_TAINT_OBJ0 + k, 1 << k) for k in range(6)),
                      out_uncapped=_stop(_src, 6, [], _six[:4] + [(4, 48)])))
GC_ESCAPES = ("gc_all_live", "gc_acked_full")

# ---------------------------------------------------------------------------------------
# e. capacity: the 64 atoms and the record log
# ---------------------------------------------------------------------------------------
CAPACITY = []
for _n0 in (61, 62, 63, 64):
    _kw = dict(actions=_acts(CAP_ACTIONS), n_atoms=_n0)
    # need 1, a pre-hook
    _src = "PUSH1 1 PUSH1 2 ADD STOP"
    _o = _stop(_src, _n0 + 1, _pre(_n0), [(0, 1 << _n0)]) if _n0 <= 63 else \
        Outcome(2, MG_ESCAPE, _esc("ADD", MG_ESC_TAINT), _n0, 0, 0, NO_ENV, (), ((0, 0), (1, 0)))
    CAPACITY.append(Case(f"atoms_pre_{_n0}", "capacity", _src, _o, **_kw))
    # need 1, a post-hook (its atom joins the yield class)
    _src = "ORIGIN STOP"
    _o = _stop(_src, _n0 + 1, [("post", _n0)], [(0, 1 << _n0)], ymask=1 << _n0, env=(0, 0, 1 << _n0, 0, 0, 0)) \
        if _n0 <= 63 else Outcome(0, MG_ESCAPE, _esc("ORIGIN", MG_ESC_TAINT), _n0, 0, 0, NO_ENV, (), ())
    CAPACITY.append(Case(f"atoms_post_{_n0}", "capacity", _src, _o, **_kw))
    # need 2: the post atom is the one after the pre atom
    _src = "PUSH1 1 PUSH1 2 MUL STOP"
    _o = _stop(_src, _n0 + 2, _pre(_n0) + [("post", _n0 + 1)], [(0, 3 << _n0)]) if _n0 <= 62 else \
        Outcome(2, MG_ESCAPE, _esc("MUL", MG_ESC_TAINT), _n0, 0, 0, NO_ENV, (), ((0, 0), (1, 0)))
    CAPACITY.append(Case(f"atoms_two_{_n0}", "capacity", _src, _o, **_kw))
# the record sweep's program: an annotating ADD (atom 0), an SSTORE with sink and
# deferred hook, ORIGIN's post-hook (atom 1, yield class), a JUMP with a deferred hook,
# and SUB with pre-hook (atom 2), deferred hook and post-hook (atom 3): pre, hook, post
_src = "PUSH1 1 PUSH1 2 ADD PUSH1 0 SSTORE ORIGIN PUSH1 12 JUMP JUMPDEST PUSH1 1 PUSH1 2 SUB STOP"
CAPREC = Case("records_all_kinds", "capacity", _src,
              _stop(_src, 4, [("pre", 0), ("hook", 1), ("post", 1), ("hook", 1), ("pre", 2), ("hook", 1), ("post", 3)],
                    [(0, 2), (1, 12)], sink=1, ymask=2, env=(0, 0, 2, 0, 0, 0), tflags=1),
              actions=_acts(CAP_ACTIONS))
CAPACITY.append(CAPREC)
# (record words the log must hold, instructions executed when it does not): an
# instruction's records fit all at once or the lane stops before it
CAPREC_STOPS = ((ANNOT_WORDS, 2), (ANNOT_WORDS + HOOK1_WORDS, 4), (2 * ANNOT_WORDS + HOOK1_WORDS, 5),
                (2 * ANNOT_WORDS + 2 * HOOK1_WORDS, 7), (4 * ANNOT_WORDS + 3 * HOOK1_WORDS, 11))
SWEPT = ("atoms_pre_61", "atoms_post_61", "atoms_two_61", "records_all_kinds")


def caprec_steps(rec_cap: int) -> int:
    for words, steps in CAPREC_STOPS:
        if rec_cap < words:
            return steps
    return CAPREC.out.steps


# ---------------------------------------------------------------------------------------
# f. rollback and underflow
# ---------------------------------------------------------------------------------------
ROLLBACK = []
# PUSH 3 + PUSH 3 + ADD 3 = 9 >= the limit: the pre-hook's record and atom are dropped
_src = "PUSH1 1 PUSH1 2 ADD STOP"
ROLLBACK.append(Case("add_out_of_gas", "rollback", _src,
                     Outcome(3, MG_VMEXC, MG_EXC_OUT_OF_GAS, 0, 0, 0, NO_ENV, (), ((0, 0), (1, 0))), gas_limit=9))
_full = tuple((1, 0) for _ in range(1024))
for _op, _s in (("DUP1", "DUP1 STOP"), ("PUSH1", "PUSH1 1 STOP")):
    ROLLBACK.append(Case(f"{_op.lower()}_post_at_stack_limit", "rollback", _s,
                         Outcome(1, MG_VMEXC, MG_EXC_STACK_OVERFLOW, 0, 0, 0, NO_ENV, (),
                                 tuple((k, 0) for k in range(1024))),
                         actions=_acts(LIMIT_ACTIONS), stack_cap=1024, stack0=_full))
UNDERFLOW = []
_REC_CAP = 512
for _n0 in (63, 64):
    for _short in (0, 1):
        def _uf(name, src, steps, words, out=None, **kw):
            # the log has room for exactly `words` more, or one word less
            o = out or Outcome(steps, MG_VMEXC, MG_EXC_STACK_UNDERFLOW, _n0, 0, kw.get("ymask", 0), NO_ENV, (),
                               tuple((k, 0) for k in range(steps - 1)), kw.get("tflags", 0))
            UNDERFLOW.append(Case(f"{name}_{_n0}_{'short' if _short else 'fits'}", "underflow", src, o,
                                  n_atoms=_n0, rec_cap=_REC_CAP, rec_len=_REC_CAP - words + _short, **kw))
        # ADD requires 2: no pre-hook, no atom or record escape
        _uf("add_sp1", "PUSH1 1 ADD STOP", 2, ANNOT_WORDS)
        # SSTORE requires 1 in the reference's table: the deferred hook runs, the
        # mutator's second pop raises; without room for the record the host's
        _uf("sstore_sp1", "PUSH1 1 SSTORE STOP", 2, HOOK1_WORDS,
            out=Outcome(1, MG_ESCAPE, _esc("SSTORE", MG_ESC_RECORD), _n0, 0, 0, NO_ENV, (), ((0, 0),))
            if _short else None)
        # SLOAD requires 1: no if-lane yield
        _uf("sload_sp0_iflane", "SLOAD STOP", 1, ANNOT_WORDS, tflags=2)
        # JUMPI requires 2: no yield (every atom is in the yield class here), no sink
        _uf("jumpi_sp1", "PUSH1 1 JUMPI STOP", 2, ANNOT_WORDS, ymask=(1 << 63) - 1)
ROLLBACK += UNDERFLOW

# ---------------------------------------------------------------------------------------
# g. yield
# ---------------------------------------------------------------------------------------
YIELD = []
# ORIGIN's atom 0 (yield class) through ADD (atom 1, not of the class), ISZERO and DUP
# to the JUMPI's condition: MG_HOOK before it
_src = "ORIGIN PUSH1 0 ADD ISZERO DUP1 PUSH1 9 JUMPI JUMPDEST STOP"
YIELD.append(Case("yield_class_atom_reaches_jumpi", "yield", _src,
                  Outcome(6, MG_HOOK, OPCODES["JUMPI"], 2, 0, 1, (0, 0, 1, 0, 0, 0), (("post", 0), ("pre", 1)),
                          ((0, 3), (0, 3), (1, 0)))))
# the same chain from the integer action's atom: the JUMPI runs (its sink collects it)
_src = "PUSH1 5 PUSH1 0 ADD ISZERO DUP1 PUSH1 10 JUMPI JUMPDEST STOP"
YIELD.append(Case("other_atom_does_not_yield", "yield", _src, _stop(_src, 1, _pre(0), [(0, 1)], sink=1, tflags=1)))
_src = "PUSH1 0 SLOAD STOP"
YIELD.append(Case("iflane_clear", "yield", _src, _stop(_src, 0, [], [(0, 0)])))
YIELD.append(Case("iflane_set", "yield", _src,
                  Outcome(1, MG_HOOK, OPCODES["SLOAD"], 0, 0, 0, NO_ENV, (), ((0, 0),), 2), tflags=2))
# cached issue addresses: 1 = the host's hooks, 2 = no action at all, 0 next to it
_src = "PUSH1 1 PUSH1 2 ADD PUSH1 3 ADD STOP"
YIELD.append(Case("force_host", "yield", _src,
                  Outcome(2, MG_HOOK, OPCODES["ADD"], 0, 0, 0, NO_ENV, (), ((0, 0), (1, 0))), force=((2, 1),)))
YIELD.append(Case("force_none_then_action", "yield", _src, _stop(_src, 1, _pre(0), [(0, 1)]),
                  force=((2, 2), (4, 0)), dev_n_obj=MG_TAINT_OBJ0 + 2))

FAMILIES = {"result": RESULT, "fresh": FRESH, "identity": IDENTITY, "compaction": COMPACTION,
            "capacity": CAPACITY, "rollback": ROLLBACK, "yield": YIELD}
ALL = [c for cases in FAMILIES.values() for c in cases]
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)

# a plain concrete program for the lanes between the cases (no MG_LANE_TAINT: kernel 1's)
PLAIN_SRC = "PUSH1 3 PUSH1 5 DUP2 ADD PUSH1 0 SSTORE CALLER PUSH1 0 MSTORE PUSH1 32 PUSH1 0 SHA3 STOP"


# ---------------------------------------------------------------------------------------
# lanes
# ---------------------------------------------------------------------------------------
def partition(b, i):
    """Per stack slot: (object class, atoms) with classes numbered by first
    appearance; handle-0 slots are objects of their own."""
    seen, out = {}, []
    for s in range(int(b.sp[i])):
        h = int(b.sobj[i, s])
        key = ("fresh", s) if h == 0 else h
        if key not in seen:
            seen[key] = len(seen)
        out.append((seen[key], int(b.omask[i, h]) if h else 0))
    env = [int(b.omask[i, h]) for h in range(1, 7)]
    return out, env


def record_kinds(b, i, start=0):
    out = []
    for r in b.records(i, start):
        if r[1] == "annot":
            out.append(("post" if r[5] else "pre", r[2]))
        elif r[1] == "hook":
            out.append(("hook", len(r[2])))
        else:
            out.append((r[1],))
    return tuple(out)


def observe(b, i, case: Case, want: Optional[Outcome] = None) -> Outcome:
    """Lane i's outcome in the form of the case's hand-written one."""
    want = want or case.out
    stack, env = partition(b, i)
    return Outcome(int(b.steps[i]), int(b.status[i]), None if want.aux is None else int(b.aux[i]),
                   int(b.n_atoms[i]), int(b.sink[i]), int(b.ymask[i]), tuple(env),
                   record_kinds(b, i, case.rec_len), tuple(stack), int(b.tflags[i]))


def shape_of(case: Case, n: int, **caps) -> LaneShape:
    kw = dict(n=n, stack_cap=case.stack_cap, mem_cap=128, calldata_cap=32, storage_cap=4, rec_cap=case.rec_cap,
              obj_cap=case.obj_cap)
    kw.update(caps)
    return LaneShape(**kw)


def set_case_lane(b: LaneBatch, i: int, case: Case, code_id: int) -> None:
    b.set_lane(i, code_id=code_id, calldata=bytes(range(1, 33)), address=ADDRESS, caller=CALLER, origin=CALLER,
               callvalue=3, gasprice=1, gas_limit=case.gas_limit, flags=MG_LANE_TAINT | case.flags)
    b.rec_len[i] = case.rec_len
    b.n_obj[i], b.n_fixed[i], b.n_atoms[i] = case.n_obj, case.n_fixed, case.n_atoms
    b.tflags[i], b.ymask[i], b.sink[i] = case.tflags, case.ymask, 0
    b.sobj[i] = 0
    b.omask[i] = 0
    for s, (w, h) in enumerate(case.stack0):
        b.stack[i, s] = word_to_limbs(w)
        b.sobj[i, s] = h
    b.sp[i] = len(case.stack0)
    for h, m in case.omask0:
        b.omask[i, h] = m


def force_flags(case: Case) -> Optional[np.ndarray]:
    if not case.force:
        return None
    f = np.zeros(n_instructions(case.src), dtype=np.uint8)
    for k, v in case.force:
        f[k] = v
    return f


def check_pins(b, i, case: Case) -> None:
    """Handle numbers and masks a case states outright (the host's handles)."""
    for s, h in case.slots:
        assert int(b.sobj[i, s]) == h, (case.name, "slot", s, int(b.sobj[i, s]), h)
    for h, m in case.masks:
        assert int(b.omask[i, h]) == m, (case.name, "mask", h, int(b.omask[i, h]), m)
    assert int(b.n_fixed[i]) == case.n_fixed, case.name


def groups(cases):
    """Cases by shape and action table: a batch has one of each."""
    out = {}
    for c in cases:
        out.setdefault(c.shape_key, []).append(c)
    return list(out.values())


def restated(cases, max_steps=1 << 20, launches=1, hook=None, watch=None, **caps):
    """The cases (of one group), one lane each, run by the restatement over the C
    oracle (tests/oracle_device.py): the batch at the end."""
    from oracle_device import OracleDevice
    ora = OracleDevice()
    ora.taint_watch = watch
    b = LaneBatch(shape_of(cases[0], len(cases), **caps))
    for i, c in enumerate(cases):
        cid = ora.load_code(c.code)
        set_case_lane(b, i, c, cid)
        if c.force:
            ora.set_taint_force(cid, force_flags(c))
    ora.alloc(b.shape)
    ora.set_taint_program(action_words(dict(cases[0].actions)))
    ora.upload(b)
    for _ in range(launches):
        ora.step(hook, max_steps=max_steps)
    ora.download(b)
    return b
