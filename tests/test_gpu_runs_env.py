"""Kernel 1's straight-line runs with the environment pushes in the run set
(run_table.h, lane_step.cuh): ADDRESS, ORIGIN, CALLER, CALLVALUE, GASPRICE,
CALLDATASIZE, CODESIZE, GASLIMIT, PC and MSIZE no longer split a run, and a
lane of a creation transaction leaves a run that holds CALLDATASIZE or
CODESIZE.

Every case is bit-exact against oracle/evm_ref.c (parity scalars, stacks,
coverage), run with the defaults, with ``MG_K1_RUNENV=0`` (the run table
without the environment pushes) and with ``MG_K1_RUNS=reg`` (the register
form only).  The cases without an environment opcode pin the two run forms
themselves at the edges the wider run set moves: shuffles, closing jumps,
entries, limits."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from mythril_amd import workloads
from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.lanes import (MG_ESCAPE, MG_RUNNING, LaneBatch, LaneShape, bucket_order, diff_batches, permuted,
                               word_to_limbs)
from oracle.evm_ref import OracleEVM

pytestmark = pytest.mark.gpu

M = (1 << 256) - 1
SWITCHES = [{}, {"MG_K1_RUNENV": "0"}, {"MG_K1_RUNS": "reg"}]
EDGE = [0, 1, 1 << 255, M, (1 << 160) - 1, 31, 32, 255, 256, 0x80, 0xFF00, 7]
STOP, ADD, MUL, SUB, SIGNEXTEND = 0x00, 0x01, 0x02, 0x03, 0x0B
LT, GT, SLT, SGT, EQ, ISZERO, AND, OR, XOR, NOT, BYTE, SHL, SHR, SAR = range(0x10, 0x1E)
POP, JUMP, JUMPI, JUMPDEST, RETURNDATASIZE = 0x50, 0x56, 0x57, 0x5B, 0x3D
NONCOMM = [SUB, LT, SGT, SHL, SHR, SAR, BYTE, SIGNEXTEND]


def push(v, k=None):
    k = k or max(1, (int(v).bit_length() + 7) // 8)
    return bytes([0x5F + k]) + int(v).to_bytes(k, "big")


def dup(n):
    return bytes([0x7F + n])


def swap(n):
    return bytes([0x8F + n])


def asm(*parts):
    return b"".join(bytes([p]) if isinstance(p, int) else p for p in parts)


TAIL = b"\x00" * 44          # the loader drops a 43-byte metadata tail


@contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _batch(n, stacks, stack_cap=32, gas=None, flags=None, **lane_kw):
    """n lanes at pc 0; lane i starts with stacks[i % len(stacks)] (bottom first)."""
    b = LaneBatch(LaneShape(n=n, stack_cap=stack_cap, mem_cap=64, calldata_cap=32, storage_cap=1))
    for i in range(n):
        kw = {k: (v[i % len(v)] if isinstance(v, list) else v) for k, v in lane_kw.items()}
        b.set_lane(i, gas_limit=gas[i % len(gas)] if gas else 10 ** 7,
                   flags=flags[i % len(flags)] if flags else 0, **kw)
        st = stacks[i % len(stacks)]
        for k, w in enumerate(st):
            b.stack[i, k] = word_to_limbs(w)
        b.sp[i] = len(st)
    return b


def _stacks(depth, n=64, salt=0):
    """n stacks of `depth` words: edge words rotated through every slot, and wide ones."""
    rng = np.random.Generator(np.random.PCG64(77 + salt))
    out = []
    for i in range(n):
        st = []
        for k in range(depth):
            if (i + k) % 3 == 0:
                st.append(int.from_bytes(rng.bytes(32), "big"))
            else:
                st.append(EDGE[(i + 5 * k) % len(EDGE)])
        out.append(st)
    return out


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def _check(dev, code, batch, hook_mask=None, max_steps=1 << 30, rounds=1, loop_bound=0, dev_env=None):
    """Oracle once, then the device under every switch setting: each exact,
    coverage included.  rounds > 1: that many launches of `max_steps` each."""
    code = code + TAIL
    o = OracleEVM()
    ref = batch.copy()
    ocid = o.load_code(code)
    ref.code_id[:] = ocid
    ocov = np.zeros(len(o.code_table(ocid)[0]), dtype=np.uint8)
    o.set_coverage(ocid, ocov)
    kw = {"loop_bound": loop_bound} if loop_bound else {}
    for _ in range(rounds):
        o.run(ref, hook_mask=hook_mask or (0, 0, 0, 0), max_steps=max_steps, **kw)
    o.set_coverage(ocid, None)
    ref.code_id[:] = 0
    out = None
    for sw in SWITCHES:
        with _env(**sw, **(dev_env or {})):
            d = GpuDevice(0) if dev_env else dev
            try:
                cid = d.load_code(code)
                gpu_in = batch.copy()
                gpu_in.code_id[:] = cid
                d.alloc(batch.shape, coverage=True)
                d.coverage_clear()
                d.upload(gpu_in)
                d.set_loop_bound(loop_bound)
                for _ in range(rounds):
                    d.step(hook_mask, max_steps=max_steps)
                out = LaneBatch(batch.shape)
                d.download(out)
                cov = d.coverage(cid)
            finally:
                if dev_env:
                    d.close()
        out.code_id[:] = 0
        assert not diff_batches(out, ref), sw
        assert np.array_equal(cov != 0, ocov != 0), sw
    return out


# ---- shuffles and ALU operands -------------------------------------------------

@pytest.mark.parametrize("n", range(1, 17))
def test_every_dup_and_swap(dev, n):
    """DUPn and SWAPn inside a run, around each non-commutative ALU op whose
    operands come from an input slot, an immediate (either side) and an
    earlier result.  The lanes start at depth n + 1 and the runs grow the stack,
    so from n of about 10 on they leave the window and run in the register form
    (test_deep_dup_and_swap_in_the_window keeps those depths at the window)."""
    body = b""
    for k, op in enumerate(NONCOMM):
        imm = EDGE[(n + k) % len(EDGE)]
        body += asm(dup(n), push(imm), op,          # immediate first popped, input second
                    swap(n), push(imm, 32), swap(1), op,   # input first, immediate second
                    dup(1), dup(n), op,             # earlier result and an input
                    swap(n), POP)
        if k % 3 == 2:
            body += asm(JUMPDEST)
    code = asm(body, STOP)
    _check(dev, code, _batch(128, _stacks(n + 1, salt=n)))


def test_known_shuffles(dev):
    m20 = push((1 << 160) - 1, 20)
    code = asm(swap(1), push(0), ADD, swap(1), swap(3), swap(2), swap(1), m20, AND, m20, AND,
               0x5A, POP,                               # GAS: not in the run set, splits the runs
               ADD, POP, push(3), push(4), MUL, POP, POP, POP, POP, STOP)
    _check(dev, code, _batch(128, _stacks(6)))


def test_pop_chain_to_empty_stack(dev):
    code = asm(ADD, POP, POP, POP, POP, STOP)
    _check(dev, code, _batch(64, _stacks(5)))


@pytest.mark.parametrize("length", [64, 65])
def test_run_of_64_and_65(dev, length):
    """A run of exactly RUN_MAX instructions, and one longer by one (split)."""
    body = asm(*[asm(dup(2), NOT, swap(2), XOR)] * (length // 4), *[JUMPDEST] * (length % 4))
    assert len(body) == length
    _check(dev, asm(body, 0x5A, STOP), _batch(64, _stacks(3)))


def test_run_peak_above_the_window(dev):
    """Nine pushes and eight ADDs on a stack of 8: the run peaks at 17 slots,
    past any window (at most 16), so the deep lanes take the register form; the
    shallow lanes of the same wave run it in the window."""
    code = asm(*[push(k + 1) for k in range(9)], *[ADD] * 8, 0x5A, POP, STOP)
    deep = _stacks(8, 32)
    _check(dev, code, _batch(128, deep + _stacks(1, 32)))


def test_rotation_at_the_window_edge(dev):
    """A run of peak 0 (SWAP1 SWAP3 SWAP2 SWAP1 JUMPDEST JUMPDEST) and one of
    peak 1 at every depth from 8 to 17: the window is 10 to 16 slots by the LDS
    plan, so the depth equal to it and its neighbours are among them."""
    for code in (asm(swap(1), swap(3), swap(2), swap(1), JUMPDEST, JUMPDEST, 0x5A, POP, STOP),
                 asm(swap(1), swap(3), swap(2), swap(1), dup(1), ISZERO, ISZERO, POP, 0x5A, POP, STOP)):
        for depth in range(8, 18):
            _check(dev, code, _batch(64, _stacks(depth, salt=depth)))


@pytest.mark.parametrize("n", range(11, 17))
def test_deep_dup_and_swap_in_the_window(dev, n):
    """DUPn SUB and SWAPn POP at depth 15, 16 and 17: around a 16-slot window's
    edge for the deep DUPs and SWAPs (DUPn SUB peaks at 1, SWAPn POP at 0)."""
    for code in (asm(dup(n), SUB, STOP), asm(swap(n), POP, STOP)):
        for depth in (15, 16, 17):
            _check(dev, code, _batch(64, _stacks(depth, salt=n)))


# ---- entries ----------------------------------------------------------------------

def test_entry_in_the_middle_and_after_a_budget(dev):
    """Lanes enter a long run at its head or at a JUMPDEST inside it (their
    JUMPI taken); with one-step launches every pc of the run is entered, most of
    them non-entry pcs."""
    run = asm(dup(1), dup(3), SUB, swap(1), POP, JUMPDEST, dup(2), ADD, swap(2), swap(1), dup(1), LT, POP, 0x5A,
              POP, STOP)
    head = asm(dup(1), push(9), JUMPI)          # the JUMPDEST inside `run` is at byte 4 + 5
    assert asm(head, run)[9] == JUMPDEST
    code = asm(head, run)
    stacks = [st + [i % 2] for i, st in enumerate(_stacks(3))]
    _check(dev, code, _batch(128, stacks))
    _check(dev, code, _batch(128, stacks), max_steps=1, rounds=20)
    _check(dev, code, _batch(128, stacks), max_steps=3, rounds=7)


# ---- closing jumps ----------------------------------------------------------------

# byte 0 JUMPDEST (a function entry: address 0), then per-case code from byte 1
def _jump_code(target, op, cond_from_stack=True):
    # [cond] PUSH2 target JUMP/JUMPI ; fall-through: PUSH1 1 STOP ; 0x20: JUMPDEST PUSH1 2 STOP
    pre = asm(JUMPDEST, dup(1), ISZERO, ISZERO)
    body = asm(pre, push(target, 2), op, push(1), STOP)
    body = body.ljust(0x20, b"\x00")
    return asm(body, JUMPDEST, push(2), STOP)


@pytest.mark.parametrize("op", [JUMP, JUMPI])
@pytest.mark.parametrize("target", [0x20, 0x21, 0x1F, 0x0400, 0])
def test_static_jumps(dev, op, target):
    """To a JUMPDEST, into the middle of code (not a JUMPDEST), to a STOP, beyond
    the code, and to address 0 (a function entry: fent switches); JUMPI taken
    and not taken by alternating lanes of one wave."""
    stacks = [[5, i % 2 * (i + 1)] for i in range(64)]
    out = _check(dev, _jump_code(target, op), _batch(128, stacks))
    if target == 0 and op == JUMP:
        assert (out.fent == 0).all()


def test_static_jump_to_dispatcher_entry(dev):
    """A landing that the dispatcher table names: PUSH4 sel EQ PUSH2 entry JUMPI."""
    code = asm(dup(1), push(0xA9059CBB, 4), EQ, push(0x20, 2), JUMPI, push(7), push(0x20, 2), JUMP)
    code = asm(code.ljust(0x20, b"\x00"), JUMPDEST, push(1), ADD, STOP)
    stacks = [[0xA9059CBB if i % 3 else i] for i in range(64)]
    out = _check(dev, code, _batch(128, stacks))
    assert (out.fent != 0xFFFFFFFF).all()


def test_dynamic_targets(dev):
    """The target DUPed from below the run: per lane valid, invalid, beyond."""
    code = asm(JUMPDEST, push(1), ADD, dup(2), JUMP).ljust(0x10, b"\x00")
    code = asm(code, JUMPDEST, dup(3), swap(1), POP, dup(2), JUMPI, STOP).ljust(0x20, b"\x00")
    code = asm(code, JUMPDEST, POP, STOP)
    tg = [0x10, 0x20, 0x11, 0x999, 1 << 200, 0]
    stacks = [[i % 2, tg[i % len(tg)], i] for i in range(64)]
    _check(dev, code, _batch(128, stacks))
    _check(dev, code, _batch(128, stacks), max_steps=40)


def test_two_depths_and_two_pcs_in_one_wave(dev):
    """Lanes of one wave at two stack depths (same pc) and, after a JUMPI that
    half of them take, at two pcs."""
    code = asm(dup(1), push(0x10, 2), JUMPI, swap(1), dup(2), SUB, swap(1), POP, 0x5A, POP, STOP)
    code = asm(code.ljust(0x10, b"\x00"), JUMPDEST, dup(2), dup(2), LT, swap(2), POP, POP, 0x5A, POP, STOP)
    stacks = [([9] * (i % 4 // 2) + [i + 3, 2 * i, i % 2]) for i in range(64)]
    _check(dev, code, _batch(128, stacks))


# ---- limits -----------------------------------------------------------------------

def test_stack_cap_inside_a_run(dev):
    """The run's transient peak crosses the lane's stack limit although its net
    effect does not: the lane leaves the run form and stops at
    the instruction that crosses it."""
    code = asm(push(1), push(2), push(3), ADD, ADD, POP, dup(1), POP, 0x5A, POP, STOP)
    for depth in (5, 6, 7, 8):
        _check(dev, code, _batch(64, _stacks(depth, salt=depth), stack_cap=8))


def test_gas_runs_out_inside_a_run(dev):
    """Gas limits from the run's first instruction to past its last."""
    code = asm(dup(1), push(5), ADD, swap(1), POP, dup(1), MUL, push(0x0B, 2), JUMP, JUMPDEST, 0x5A, POP, STOP)
    gas = list(range(1, 44))
    _check(dev, code, _batch(128, _stacks(2), gas=gas))


def test_step_budget_ends_inside_a_run(dev):
    code = asm(dup(1), push(5), ADD, swap(1), POP, dup(1), MUL, NOT, 0x5A, POP, dup(1), dup(1), XOR, POP, STOP)
    for ms in (1, 2, 5, 8, 9):
        _check(dev, code, _batch(64, _stacks(2)), max_steps=ms, rounds=3)


# ---- environment pushes inside runs --------------------------------------------------

ENV_OPS = [0x30, 0x32, 0x33, 0x34, 0x3A, 0x36, 0x38, 0x45, 0x58, 0x59]
MG_LANE_CREATION, MG_LANE_RETDATA = 2, 16384


def _env_batch(n=128, flags=None, stacks=None):
    return _batch(n, stacks or _stacks(2), flags=flags,
                  address=[0xA0 + i for i in range(7)], caller=[(i + 1) << (8 * i) for i in range(20)],
                  origin=[M - i for i in range(5)], callvalue=[i * 10 ** 18 for i in range(9)],
                  gasprice=[i for i in range(3)], calldata=[bytes(range(i)) for i in range(0, 32, 5)])


@pytest.mark.parametrize("op", ENV_OPS)
def test_each_env_opcode_inside_a_run(dev, op):
    """The opcode between shuffles and ALU steps, twice (one lane constant, two
    uses), with per-lane differing caller, value and calldata length; MSIZE
    after a memory write that starts the run's block."""
    code = asm(push(7), push(0), 0x52,                # MSTORE: msize 32 from here on
               dup(1), op, SUB, swap(1), op, dup(1), swap(3), POP, XOR, push(3), op, LT, 0x5A, POP, STOP)
    _check(dev, code, _env_batch())


def test_all_env_opcodes_in_one_run(dev):
    code = asm(*[asm(op, XOR) for op in ENV_OPS], dup(1), 0x5A, POP, STOP)
    _check(dev, code, _env_batch())
    _check(dev, code, _env_batch(), max_steps=7, rounds=4)


@pytest.mark.parametrize("op", [0x36, 0x38])
def test_creation_lanes_escape_inside_the_run(dev, op):
    """Every other lane is a creation transaction: it escapes at CALLDATASIZE /
    CODESIZE with `steps` exact while its neighbours run the run."""
    code = asm(dup(1), 0x33, ADD, swap(1), op, SUB, 0x34, XOR, 0x5A, POP, STOP)
    out = _check(dev, code, _env_batch(flags=[0, MG_LANE_CREATION]))
    assert (out.status[1::2] == MG_ESCAPE).all() and (out.steps[1::2] == 4).all()
    assert (out.steps[0::2] == 8).all()            # the others reach the GAS after the run


def test_returndatasize_stays_a_single_dispatch(dev):
    """Lanes with MG_LANE_RETDATA escape at the RETURNDATASIZE between two runs."""
    code = asm(push(1), 0x33, ADD, RETURNDATASIZE, ADD, 0x34, dup(1), POP, STOP)
    out = _check(dev, code, _env_batch(flags=[0, 0, MG_LANE_RETDATA], stacks=[[]]))
    assert (out.status[2::3] == MG_ESCAPE).all() and (out.steps[2::3] == 3).all()


# ---- launches where runs are off, other geometries ----------------------------------

RUNS = asm(swap(1), push(0), ADD, swap(1), swap(3), swap(2), swap(1), dup(2), dup(2), LT, push(0x20, 2), JUMPI,
           POP, STOP).ljust(0x20, b"\x00") + asm(JUMPDEST, SUB, swap(1), POP, NOT, STOP)


def test_staged_prefix(dev):
    """MG_K1_PD_CAP: only a prefix of the code is staged; runs that cross it and
    jumps beyond it stay exact."""
    for cap in (4, 9, 14, 20):
        _check(dev, RUNS, _batch(128, _stacks(4)), dev_env={"MG_K1_PD_CAP": str(cap)})


def test_hook_mask_and_loop_bound_launches(dev):
    """Launches in which runs are off: nothing changes."""
    _check(dev, RUNS, _batch(128, _stacks(4)), hook_mask=hook_mask_for([0x10]))
    b = LaneBatch(LaneShape(n=64, stack_cap=32, mem_cap=64, calldata_cap=32, storage_cap=1, trace_cap=64))
    src = _batch(64, _stacks(4))
    for f in ("stack", "sp", "status", "gas_limit", "env"):
        getattr(b, f)[...] = getattr(src, f)
    _check(dev, RUNS, b, loop_bound=3)


@pytest.mark.parametrize("lpw", [32, 16])
def test_narrow_waves(dev, lpw):
    _check(dev, RUNS, _batch(192, _stacks(4)), dev_env={"MG_LANES_PER_WAVE": str(lpw)})


def test_c2_batches_bucketed(dev):
    """run_batches(3) on the C2 code at 1,024 lanes, bucketed: every lane's
    parity scalars, stack, memory, storage and records equal the oracle's."""
    code = workloads.bytecode("overflow.sol.o")
    o = OracleEVM()
    b = workloads.c2_batch(1024, stack_cap=64, mem_cap=1024, rec_cap=128)
    b = permuted(b, bucket_order(b))
    ref = b.copy()
    ref.code_id[:] = o.load_code(code)
    o.run(ref)
    ref.code_id[:] = 0
    for sw in SWITCHES:
        with _env(**sw):
            gpu_in = b.copy()
            gpu_in.code_id[:] = dev.load_code(code)
            dev.alloc(b.shape, coverage=True)
            dev.upload(gpu_in)
            stats = dev.run_batches(3)
            out = LaneBatch(b.shape)
            dev.download(out)
        assert len({s.lane_steps for s in stats}) == 1 and stats[0].lane_steps == int(ref.steps.sum())
        out.code_id[:] = 0
        assert (out.status != MG_RUNNING).all()
        assert not diff_batches(out, ref), sw
