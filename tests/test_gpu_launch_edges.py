"""Kernel 1's launch prologue and epilogue on an MI355X: lanes reset from the
resident image inside the kernel, the counters the epilogue stores, step
horizons, lanes that are not the concrete stepper's, code staging from the
load-time decode words, and the hook bit a launch adds to them.

Every case is bit-exact against oracle/evm_ref.c through OracleEVM and
diff_batches (parity scalars, stack, memory, storage, records), coverage
included where it is on; the SHA3 / EXP counters, which the oracle does not
keep, are compared with counts worked out from the straight-line program."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.lanes import (MG_ESC_STORAGE, MG_ESCAPE, MG_HALT_STOP, MG_HOOK, MG_LANE_SYMBOLIC, MG_LANE_TAINT,
                               MG_RUNNING, LaneBatch, LaneShape, diff_batches, word_to_limbs)
from oracle.evm_ref import OracleEVM

pytestmark = pytest.mark.gpu

STOP, ADD, MUL, EXP, SHA3, CALLDATALOAD, POP = 0x00, 0x01, 0x02, 0x0A, 0x20, 0x35, 0x50
MLOAD, MSTORE, SLOAD, SSTORE, JUMP, JUMPI, JUMPDEST, PUSH1 = 0x51, 0x52, 0x54, 0x55, 0x56, 0x57, 0x5B, 0x60
GAS = 10 ** 7
N = 300                      # neither a multiple of 64 nor of 256: two blocks, the second partly empty


def push(v, k=None):
    k = k or max(1, (int(v).bit_length() + 7) // 8)
    return bytes([0x5F + k]) + int(v).to_bytes(k, "big")


def asm(*parts):
    return b"".join(bytes([p]) if isinstance(p, int) else p for p in parts)


def cd(k):
    return asm(push(32 * k), CALLDATALOAD)


def words(*ws):
    return b"".join(int(w).to_bytes(32, "big") for w in ws)


# storage[1] = keccak(word 0); storage[2] = 3 ** word 1; mem[32:64] = storage[1] + storage[7]
WORK = asm(cd(0), push(0), MSTORE, push(0x20), push(0), SHA3, push(1), SSTORE,
           cd(1), push(3), EXP, push(2), SSTORE,
           push(1), SLOAD, push(7), SLOAD, ADD, push(0x20), MSTORE, STOP)
OTHER = asm(cd(1), cd(0), MUL, push(0), MSTORE, push(5), push(9), SSTORE, STOP)
# two SHA3 (instructions 2, 11) and two EXP (7, 16) in 19 straight-line instructions
COUNT = asm(push(0x20), push(0), SHA3, POP, cd(1), push(3), EXP, POP,
            push(0x40), push(0), SHA3, POP, cd(1), push(5), EXP, POP, STOP)
COUNT_SHA3, COUNT_EXP = (2, 11), (7, 16)

SHAPE = dict(stack_cap=16, mem_cap=128, calldata_cap=64, storage_cap=4)


def work_batch(n=N, rec_cap=64, code_of=lambda i: 0, **shape_kw):
    """Lanes with 0, 1 and storage_cap storage entries (the last escape at their
    first new slot), and halted and escaped lanes among the running ones."""
    b = LaneBatch(LaneShape(n=n, rec_cap=rec_cap, **{**SHAPE, **shape_kw}))
    for i in range(n):
        st = [{}, {1: 5 + i}, {7: 9}, {10: 1, 11: 2, 12: 3, 13: 4}, {7: 1 << 200, 1: 3}][i % 5]
        b.set_lane(i, code_id=code_of(i), calldata=words(0xC0FFEE + i // 3, i % 9), gas_limit=GAS, storage=st,
                   caller=0xABCD + i)
        if i % 11 == 3:
            b.status[i] = MG_HALT_STOP
        if i % 13 == 5:
            b.status[i], b.aux[i] = MG_ESCAPE, 0xF1 | (1 << 8)
    return b


@contextmanager
def environ(**kw):
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


@pytest.fixture
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


class Case:
    """Codes loaded on both sides, a batch whose code_id indexes `codes`, the
    oracle's copy of it and its coverage."""

    def __init__(self, dev, codes, batch, extra_before=(), coverage=True):
        self.dev, self.o, self.batch = dev, OracleEVM(), batch
        for c in extra_before:                        # codes the batch does not use
            dev.load_code(c)
        self.dids = [dev.load_code(c) for c in codes]
        self.oids = [self.o.load_code(c) for c in codes]
        self.ref = batch.copy()
        self.ref.code_id[:] = np.array(self.oids, dtype=np.uint32)[batch.code_id]
        self.ocov = [np.zeros(len(self.o.code_table(k)[0]), dtype=np.uint8) for k in self.oids]
        dev.alloc(batch.shape, coverage=coverage)
        if coverage:
            dev.coverage_clear()
        self.coverage = coverage
        self.upload()

    def upload(self):
        g = self.batch.copy()
        g.code_id[:] = np.array(self.dids, dtype=np.uint32)[self.batch.code_id]
        self.dev.upload(g)

    def oracle(self, **kw):
        for k, buf in zip(self.oids, self.ocov):
            self.o.set_coverage(k, buf)
        self.o.run(self.ref, **kw)
        for k in self.oids:
            self.o.set_coverage(k, None)

    def fresh_ref(self):
        self.ref = self.batch.copy()
        self.ref.code_id[:] = np.array(self.oids, dtype=np.uint32)[self.batch.code_id]

    def out(self):
        out = LaneBatch(self.batch.shape)
        self.dev.download(out)
        return out

    def check(self, what=""):
        out, ref = self.out(), self.ref.copy()
        out.code_id[:] = ref.code_id[:] = 0
        assert diff_batches(out, ref, limit=20) == [], what
        if self.coverage:
            for d, buf in zip(self.dids, self.ocov):
                assert np.array_equal(self.dev.coverage(d) != 0, buf != 0), what
        return out


# ---- lanes reset inside the kernel ------------------------------------------------------

def test_run_batches_equals_reset_and_step_equals_oracle(dev):
    c = Case(dev, [WORK], work_batch())
    c.oracle()
    ref = c.ref
    assert {int(s) for s in ref.status} >= {MG_HALT_STOP, MG_ESCAPE}
    assert ((ref.status == MG_ESCAPE) & ((ref.aux >> 8) == MG_ESC_STORAGE)).any()
    assert (ref.steps[ref.status == MG_HALT_STOP] == 0).any() and (ref.rec_len > 0).any()
    stats = dev.run_batches(3)
    assert len({(s.lane_steps, s.running, s.halted, s.escaped) for s in stats}) == 1
    assert stats[0].lane_steps == int(ref.steps.sum())
    c.check("run_batches(3)")
    for k in range(3):
        dev.reset()
        st = dev.step()
        assert st.lane_steps == stats[0].lane_steps
        c.check(f"reset + step {k}")


def _counts(steps, at):
    return np.array([sum(1 for k in at if k < s) for s in steps.tolist()], dtype=np.uint32)


def test_counters_across_launches_and_after_a_reset(dev):
    """steps, sha3_count and exp_count accumulate over launches of five
    instructions each and start again from the image after a reset."""
    def make():
        b = LaneBatch(LaneShape(n=200, **SHAPE))
        for i in range(200):
            b.set_lane(i, calldata=words(i, i % 5), gas_limit=GAS)
            if i % 9 == 4:
                b.status[i] = MG_HALT_STOP
        return b

    c = Case(dev, [COUNT], make(), coverage=False)
    live = c.batch.status == MG_RUNNING
    for launch in range(1, 5):
        dev.step(max_steps=5)
        c.oracle(max_steps=5)
        out = c.check(f"launch {launch}")
        assert (out.steps[live] == 5 * launch).all() or launch == 4
        assert (out.steps[~live] == 0).all()
        sha3, exp = dev.event_counts(200)
        assert np.array_equal(sha3, _counts(out.steps, COUNT_SHA3)), launch
        assert np.array_equal(exp, _counts(out.steps, COUNT_EXP)), launch
    assert sha3[live].tolist() == [2] * int(live.sum()) and exp[live].tolist() == [2] * int(live.sum())
    # from the image again: not on top of what the launches above counted
    dev.reset()
    dev.step(max_steps=5)
    c.fresh_ref()
    c.oracle(max_steps=5)
    out = c.check("reset + step")
    sha3, exp = dev.event_counts(200)
    assert np.array_equal(sha3, _counts(out.steps, COUNT_SHA3)) and sha3.max() == 1 and not exp.any()
    dev.run_batches(2, max_steps=12)
    c.fresh_ref()
    c.oracle(max_steps=12)
    out = c.check("run_batches")
    sha3, exp = dev.event_counts(200)
    assert np.array_equal(sha3, _counts(out.steps, COUNT_SHA3)) and sha3.max() == 2
    assert np.array_equal(exp, _counts(out.steps, COUNT_EXP)) and exp.max() == 1


def test_step_until_horizons(dev):
    """Lanes whose images start at different step counts pause at a horizon after
    different numbers of instructions."""
    b = work_batch(rec_cap=0)
    b.steps[:] = np.arange(b.n) % 7
    c = Case(dev, [WORK], b)
    for horizon in (7, 11, 16, 0):
        st = dev.step(horizon=horizon)
        c.oracle(horizon=horizon)
        out = c.check(f"horizon {horizon}")
        run = out.status == MG_RUNNING
        assert st.running == int(run.sum())
        if horizon:
            assert run.any() and (out.steps[run] == horizon).all()
            assert len(set((out.steps - b.steps)[run].tolist())) == 7
    assert not run.any()


def test_symbolic_and_taint_lanes_are_left_alone(dev):
    """Lanes flagged symbolic or taint, in a batch without those planes: the
    concrete stepper counts them as running and changes nothing of theirs."""
    b = work_batch(n=200, rec_cap=0)
    b.status[:] = MG_RUNNING
    sym = np.arange(200) % 4 == 1
    taint = np.arange(200) % 4 == 2
    b.flags[sym] |= MG_LANE_SYMBOLIC
    b.flags[taint] |= MG_LANE_TAINT
    theirs = np.nonzero(sym | taint)[0]
    for i in theirs:                                  # a state a step would change
        b.stack[i, 0] = word_to_limbs(0x20 + i)
        b.sp[i], b.msize[i], b.pc[i], b.steps[i] = 1, 32, 3, i
        b.memory[i, :32] = i % 251
        b.gas_min[i] = b.gas_max[i] = 100 + i
    c = Case(dev, [WORK], b, coverage=False)
    st = dev.step()
    c.oracle()
    out = c.out()
    ref = c.ref.copy()
    out.code_id[:] = ref.code_id[:] = 0
    mine = np.nonzero(~(sym | taint))[0]
    assert diff_batches(out, ref, lanes=mine, limit=20) == []
    given = b.copy()
    given.code_id[:] = 0
    assert diff_batches(out, given, lanes=theirs, limit=20) == []
    assert np.array_equal(out.flags, b.flags) and st.running == theirs.size
    sha3, exp = dev.event_counts(200)
    assert not sha3[theirs].any() and not exp[theirs].any() and sha3[mine].any()


# ---- staging ----------------------------------------------------------------------------

def test_block_with_two_codes_is_not_staged(dev):
    c = Case(dev, [WORK, OTHER], work_batch(code_of=lambda i: (i // 3) % 2))
    dev.step()
    c.oracle()
    c.check()
    assert (c.ref.steps[c.batch.code_id == 1] > 0).any()


def test_three_codes_loaded_one_used(dev):
    c = Case(dev, [WORK], work_batch(), extra_before=[OTHER, COUNT])
    dev.load_code(OTHER + b"\x00")       # and one loaded after it
    assert c.dids == [2]
    dev.step()
    c.oracle()
    c.check("step")
    dev.run_batches(2)
    c.check("run_batches")


def test_block_whose_lanes_are_all_halted(dev):
    b = work_batch(n=600)
    b.status[:256] = MG_HALT_STOP                     # the whole first block
    b.status[256:320] = MG_HALT_STOP                  # and one wave of the second
    c = Case(dev, [WORK], b)
    dev.run_batches(2)
    c.oracle()
    out = c.check()
    assert not out.steps[:320].any() and out.steps[320:].any()


# jumps from inside the staged prefix (7 instructions at MG_K1_PD_CAP=8) out of it and back
FAR = 14
PREFIX = asm(push(FAR), JUMP,                         # 0, 2
             JUMPDEST, push(7), cd(0), ADD,           # 3: back; the prefix ends with ADD
             push(0), MSTORE, STOP,                   # 10, 12, 13
             JUMPDEST, push(5), push(3), MUL, POP, push(3), JUMP)   # 14: far


@pytest.mark.parametrize("env", [{"MG_K1_PD_CAP": "8"}, {"MG_K1_PD_CAP": "4"}, {"MG_K1_RUNENV": "0"},
                                 {"MG_K1_PUSH": "global"}],
                         ids=["pd-cap-8", "pd-cap-4", "runenv-0", "push-global"])
def test_staging_switches(dev, env):
    assert PREFIX[FAR] == JUMPDEST and PREFIX[3] == JUMPDEST
    for code in (PREFIX, WORK):
        c = Case(dev, [code], work_batch())
        c.oracle()
        assert (c.ref.status == MG_HALT_STOP).any()
        with environ(**env):
            dev.step()
            c.check("step")
            dev.run_batches(2)
            c.check("run_batches")


# ---- the hook bit on the load-time decode words -----------------------------------------

def _hook_code():
    head = asm(cd(1), push(0, 1), JUMPI, cd(0), push(0, 1), JUMPI, push(1), push(1), SSTORE, STOP)
    d = len(head)
    tail = asm(JUMPDEST, push(2), push(2), SSTORE, STOP)
    end = d + len(tail)
    code = asm(cd(1), push(end, 1), JUMPI, cd(0), push(d, 1), JUMPI, push(1), push(1), SSTORE, STOP,
               tail, JUMPDEST, STOP)
    assert code[d] == JUMPDEST and code[end] == JUMPDEST
    return code


def test_hook_masks_stop_the_oracles_lanes_and_do_not_stick(dev):
    """Word 1 != 0: the lane ends without an SSTORE; word 0 picks the branch."""
    code = _hook_code()
    b = LaneBatch(LaneShape(n=200, **SHAPE))
    for i in range(200):
        b.set_lane(i, calldata=words(i % 2, 1 if i % 5 == 0 else 0), gas_limit=GAS)
    c = Case(dev, [code], b)
    for op in (PUSH1, JUMPI, SSTORE):
        mask = hook_mask_for([op])
        c.upload()
        c.fresh_ref()
        st = dev.step(mask)
        c.oracle(hook_mask=mask)
        out = c.check(f"hook {op:#x}")
        hooked = out.status == MG_HOOK
        assert st.hooked == int(hooked.sum()) and (out.aux[hooked] == op).all()
        assert int(hooked.sum()) == (160 if op == SSTORE else 200)
        # the same code, no mask: nothing stops
        c.upload()
        c.fresh_ref()
        st = dev.step()
        c.oracle()
        out = c.check(f"no mask after {op:#x}")
        assert st.hooked == 0 and (out.status == MG_HALT_STOP).all()
