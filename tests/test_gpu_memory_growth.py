"""Kernel 1's MLOAD and MSTORE that grow memory (lane_step.cuh mem_fast, the
LDS memory window that is zero past msize), on an MI355X.

Every case is bit-exact against oracle/evm_ref.c through OracleEVM and
diff_batches: status, aux, steps, msize, both gas bounds, the stack and the
memory below msize.  The programs are hand-assembled; each lane takes its
offsets and the stored word from its calldata, so the lanes of one wave grow
to different sizes, at different offsets, or not at all.

OFFSETS holds, for the default window of 160 bytes and for MG_K1_MEMWIN=32, the
last offset whose word still lies in the window, that offset + 1 (the word
straddles the window's edge: the general path) and the first offset outside;
for mem_cap 256 and 128 (smaller than the window) the offset that ends exactly
at mem_cap and one past it (MG_ESC_MEMORY); and ends past 2^32 (out of gas).
The core cases run again with the window off and at 32 bytes, with 32 and 16
lanes per wave, through the loop-bound instantiation and with MSTORE hooked."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.lanes import (MG_ESC_MEMORY, MG_ESCAPE, MG_EXC_OUT_OF_GAS, MG_HALT_STOP, MG_HOOK,
                               MG_MSTATE_GAS_LIMIT, MG_VMEXC, LaneBatch, LaneShape, diff_batches)
from oracle.evm_ref import OracleEVM

pytestmark = pytest.mark.gpu

M = (1 << 256) - 1
STOP, NOT, SHA3, CALLDATALOAD, MLOAD, MSTORE, MSIZE = 0x00, 0x19, 0x20, 0x35, 0x51, 0x52, 0x59
GAS = 10 ** 7
OFFSETS = [0, 1, 31, 32, 33, 0x40, 95, 96, 97, 127, 128, 129, 159, 160, 161, 192, 224, 225, 255, 256,
           2 ** 32 - 32, 2 ** 32, 1 << 255]


def push(v, k=None):
    k = k or max(1, (int(v).bit_length() + 7) // 8)
    return bytes([0x5F + k]) + int(v).to_bytes(k, "big")


def asm(*parts):
    return b"".join(bytes([p]) if isinstance(p, int) else p for p in parts)


def cd(k):
    """push calldata word k"""
    return asm(push(32 * k), CALLDATALOAD)


# calldata words 0..2: offsets, word 3: the value stored
# MSIZE is read inside a straight-line run (MSIZE PUSH1) and as a dispatch of its own
# (between two memory opcodes); the last MLOAD, at msize, is a growth from a non-zero size.
LOADS = asm(cd(0), MLOAD, cd(1), MLOAD, MSIZE, cd(2), MLOAD, MSIZE, MLOAD, STOP)
STORES = asm(cd(3), cd(0), MSTORE, MSIZE, cd(3), NOT, cd(1), MSTORE, cd(2), MLOAD, MSIZE, MLOAD, STOP)
# SHA3 over a range no instruction wrote, then over one that a store touched
SHA = asm(push(0x40), cd(0), SHA3, cd(3), cd(1), MSTORE, push(0x20), cd(2), SHA3, MSIZE, STOP)
PROGRAMS = {"loads": LOADS, "stores": STORES, "sha": SHA}


def words(*ws):
    return b"".join(int(w).to_bytes(32, "big") for w in ws)


def offsets_batch(mem_cap, n=256, trace_cap=0):
    """Lane i's three offsets walk OFFSETS at strides coprime to its length, so
    neighbouring lanes differ in every one of them."""
    b = LaneBatch(LaneShape(n=n, stack_cap=16, mem_cap=mem_cap, calldata_cap=128, storage_cap=1,
                            trace_cap=trace_cap))
    k = len(OFFSETS)
    for i in range(n):
        o1, o2, o3 = OFFSETS[i % k], OFFSETS[(7 * i + i // k) % k], OFFSETS[(3 * i + 5) % k]
        b.set_lane(i, calldata=words(o1, o2, o3, M - i), gas_limit=GAS)
    return b


_REFS = {}


def reference(key, code, make, hook_mask=None, loop_bound=0):
    """The batch of a case and its oracle result (one launch), computed once."""
    if key not in _REFS:
        batch = make()
        o = OracleEVM()
        ref = batch.copy()
        ref.code_id[:] = o.load_code(code)
        kw = {"loop_bound": loop_bound} if loop_bound else {}
        o.run(ref, hook_mask=hook_mask or (0, 0, 0, 0), **kw)
        ref.code_id[:] = 0
        _REFS[key] = (batch, ref)
    return _REFS[key]


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


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def start(d, code, batch):
    gpu_in = batch.copy()
    gpu_in.code_id[:] = d.load_code(code)
    d.alloc(batch.shape)
    d.upload(gpu_in)


def result(d, shape):
    out = LaneBatch(shape)
    d.download(out)
    out.code_id[:] = 0
    return out


def run_once(d, code, batch, hook_mask=None):
    start(d, code, batch)
    d.step(hook_mask)
    return result(d, batch.shape)


# ---- growth offsets, second growths, zeros past the stores, MSIZE, SHA3 -----------------

# name -> (environment, lanes per wave, loop bound, hooked opcodes)
VARIANTS = {
    "default": ({}, 64, 0, None),
    "memwin0": ({"MG_K1_MEMWIN": "0"}, 64, 0, None),
    "memwin32": ({"MG_K1_MEMWIN": "32"}, 64, 0, None),
    "lpw32": ({}, 32, 0, None),
    "lpw16": ({}, 16, 0, None),
    "loop-bound": ({}, 64, 3, None),
    "mstore-hooked": ({}, 64, 0, [MSTORE]),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mem_cap", [256, 128])
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_growth_equals_oracle(dev, name, mem_cap, variant):
    env, lpw, bound, hooked = VARIANTS[variant]
    code = PROGRAMS[name]
    mask = hook_mask_for(hooked) if hooked else None
    batch, ref = reference((name, mem_cap, bound, bool(hooked)), code,
                           lambda: offsets_batch(mem_cap, trace_cap=64 if bound else 0),
                           hook_mask=mask, loop_bound=bound)
    with environ(**env):
        if lpw != 64:
            with environ(MG_LANES_PER_WAVE=str(lpw)):
                d = GpuDevice(0)
        else:
            d = dev
        try:
            d.set_loop_bound(bound)
            out = run_once(d, code, batch, mask)
        finally:
            if lpw != 64:
                d.close()
            else:
                d.set_loop_bound(0)
    assert diff_batches(out, ref, limit=20) == []
    if bound:
        assert np.array_equal(out.trace_len, ref.trace_len)
    # the list reaches every outcome: a stop, the memory escape and out of gas
    if not hooked or name == "loads":
        esc = (ref.status == MG_ESCAPE) & ((ref.aux >> 8) == MG_ESC_MEMORY)
        oog = (ref.status == MG_VMEXC) & (ref.aux == MG_EXC_OUT_OF_GAS)
        assert (ref.status == MG_HALT_STOP).any() and esc.any() and oog.any()
        assert len(set(ref.msize.tolist())) >= 4
    elif name == "stores":
        # stopped before the store: memory untouched
        assert (out.status == MG_HOOK).all() and (out.msize == 0).all() and (out.aux == MSTORE).all()


def test_divergent_wave(dev):
    """One wave: the first store grows to five different sizes at aligned and
    unaligned offsets; the second store lies inside msize for half of the lanes and
    grows for the others; the loads that follow grow again or not."""
    def make():
        b = LaneBatch(LaneShape(n=64, stack_cap=16, mem_cap=256, calldata_cap=128, storage_cap=1))
        for i in range(64):
            o1 = 32 * (i % 5) + (1 if i % 3 == 0 and i % 5 < 4 else 0)
            o2 = 0 if i % 2 else 96 + 32 * (i % 3)
            b.set_lane(i, calldata=words(o1, o2, 32 * (i % 7), M - i), gas_limit=GAS)
        return b

    batch, ref = reference("divergent", STORES, make)
    assert (ref.status == MG_HALT_STOP).all() and len(set(ref.msize.tolist())) >= 4
    for variant in ("default", "memwin32"):
        with environ(**VARIANTS[variant][0]):
            out = run_once(dev, STORES, batch)
        assert diff_batches(out, ref) == [], variant


# ---- memory left by one launch, grown by the next ---------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3])
def test_stepping_k_instructions_a_launch_equals_one_launch(dev, k):
    """Launches of k instructions each enter with a non-zero msize: the window is
    filled from memory below msize and zero beyond it."""
    for name in ("stores", "loads"):
        code = PROGRAMS[name]
        batch, ref = reference((name, 256, 0, False), code, lambda: offsets_batch(256))
        start(dev, code, batch)
        for _ in range(64):
            if dev.step(max_steps=k).running == 0:
                break
        else:
            raise AssertionError("lanes still running")
        assert diff_batches(result(dev, batch.shape), ref, limit=20) == [], name


# words 0, 1: offsets loaded (growth without a write); words 2..6: offsets stored to
TRAP = asm(cd(0), MLOAD, cd(1), MLOAD, MSIZE, *[asm(push(M, 32), cd(k), MSTORE) for k in range(2, 7)], STOP)


def trap_shape(n):
    return LaneShape(n=n, stack_cap=16, mem_cap=256, calldata_cap=224, storage_cap=1)


def fill_batch(n=256):
    """Every lane leaves its whole window (160 bytes) full of 0xff."""
    b = LaneBatch(trap_shape(n))
    for i in range(n):
        b.set_lane(i, calldata=words(128, 0, 0, 32, 64, 96, 128), gas_limit=GAS)
    return b


def short_batch(n=256):
    """Lanes that grow to 32 .. 160 bytes by loading, then overwrite only what lies
    below their own msize: neighbours in a wave end at different sizes."""
    b = LaneBatch(trap_shape(n))
    for i in range(n):
        top = i % 5                                   # the growth reaches word `top`
        o1 = 32 * top - (3 if i % 4 == 1 and top else 0)
        o2 = 32 * (i % (top + 1))
        st = [32 * ((i + k) % (top + 1)) for k in range(5)]
        b.set_lane(i, calldata=words(o1, o2, *st), gas_limit=GAS)
    return b


def test_stale_window_reads_zero_after_a_reset(dev):
    """A launch that leaves 0xff in every window byte, then lanes that grow by
    loading: they read zeros in the first launch after the upload, after
    mg_lanes_reset + step and in both launches of run_batches(2)."""
    fill, fill_ref = reference("trap-fill", TRAP, fill_batch)
    batch, ref = reference("trap-short", TRAP, short_batch)
    assert (ref.status == MG_HALT_STOP).all() and sorted(set(ref.msize.tolist())) == [32, 64, 96, 128, 160]
    for i in range(0, batch.n, 7):
        assert ref.stack_words(i)[:2] == [0, 0]
    assert diff_batches(run_once(dev, TRAP, fill), fill_ref) == []
    assert bytes(fill_ref.memory[5, :160]) == b"\xff" * 160
    assert diff_batches(run_once(dev, TRAP, batch), ref) == []
    dev.reset()
    dev.step()
    assert diff_batches(result(dev, batch.shape), ref) == []
    stats = dev.run_batches(2)
    assert [s.running for s in stats] == [0, 0] and stats[0].lane_steps == stats[1].lane_steps == int(ref.steps.sum())
    assert diff_batches(result(dev, batch.shape), ref) == []


# ---- gas edges --------------------------------------------------------------------------

def fee(nw):
    return 3 * nw + nw * nw // 512


def test_gas_edges_of_a_growth(dev):
    """The gas limit one above, exactly at and below what a growing MLOAD / MSTORE
    needs (memory fee + table gas), for a first and for a second growth, inside the
    window and across its edge; and lanes that start just below the machine-state
    limit of 10^9, where mem_extend's own `> 10^9` test is the one that fires."""
    G1 = asm(cd(0), MLOAD, STOP)                      # 6 gas before the MLOAD
    G2 = asm(cd(0), MLOAD, cd(1), MLOAD, STOP)
    GS = asm(cd(3), cd(0), MSTORE, STOP)              # 12 gas before the MSTORE
    cases = []                                        # (code, calldata, gas_limit, gas at entry)
    for off in (0, 1, 32, 0x40, 96, 128, 129):
        nw = (off + 63) // 32
        for code, pre in ((G1, 6), (GS, 12)):
            need = pre + fee(nw) + 3
            for delta in (-3, -2, -1, 0, 1, 2):
                cases.append((code, words(off, 0, 0, M), need + delta, 0))
            # near the machine-state limit, under a transaction limit above it
            for j in range(-2, 6):
                cases.append((code, words(off, 0, 0, M), 2 * 10 ** 9, MG_MSTATE_GAS_LIMIT - need + j))
    for o1, o2 in ((0, 64), (32, 128), (1, 129), (0x40, 0), (0, 32), (31, 96), (96, 128), (0, 128), (64, 160),
                   (33, 65), (128, 224)):
        n1, n2 = (o1 + 63) // 32, max((o1 + 63) // 32, (o2 + 63) // 32)
        need = 6 + fee(n1) + 3 + 6 + fee(n2) - fee(n1) + 3
        for delta in (-3, -2, -1, 0, 1, 2):
            cases.append((G2, words(o1, o2, 0, M), need + delta, 0))
    codes = [G1, G2, GS]
    seen = set()
    for ci, code in enumerate(codes):
        mine = [c for c in cases if c[0] is code]

        def make():
            b = LaneBatch(LaneShape(n=len(mine), stack_cap=16, mem_cap=256, calldata_cap=128, storage_cap=1))
            for i, (_, data, limit, g0) in enumerate(mine):
                b.set_lane(i, calldata=data, gas_limit=limit)
                b.gas_min[i] = b.gas_max[i] = g0
            return b

        batch, ref = reference(("gas", ci), code, make)
        assert 64 <= batch.n <= 256
        for variant in ("default", "memwin0", "memwin32"):
            with environ(**VARIANTS[variant][0]):
                out = run_once(dev, code, batch)
            assert diff_batches(out, ref, limit=20) == [], (ci, variant)
        oog = (ref.status == MG_VMEXC) & (ref.aux == MG_EXC_OUT_OF_GAS)
        assert ((ref.status == MG_HALT_STOP) | oog).all()
        # each group of limits around one need holds both outcomes
        seen |= {(ci, bool(x)) for x in oog.tolist()}
        near = np.array([c[3] != 0 for c in mine])
        if near.any():
            assert oog[near].any() and (~oog[near]).any()
    assert seen == {(ci, x) for ci in range(3) for x in (False, True)}
