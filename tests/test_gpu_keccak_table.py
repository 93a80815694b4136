"""Kernel 1's per-context Keccak result table (lane_step.cuh K_SHA3, the second
level behind the per-wave LDS cache): a wave whose active lanes all hash the
same 64 aligned bytes publishes the result once, and later launches of the
same context take it from the table instead of running Keccak-f.

Every case is bit-exact against oracle/evm_ref.c (status, the storage that
holds the hashes, records), after the first launch and again after
``run_batches(3)`` on the same image, whose launches 2 and 3 consume what
launch 1 published ("repeat")."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.keccak import keccak_int
from mythril_amd.lanes import MG_HALT_STOP, LaneBatch, LaneShape, diff_batches
from oracle.evm_ref import OracleEVM

pytestmark = pytest.mark.gpu

GAS = 10 ** 7


def _sha3(off, ln, slot):
    # PUSH1 ln PUSH1 off SHA3 PUSH1 slot SSTORE
    return bytes([0x60, ln, 0x60, off, 0x20, 0x60, slot, 0x55])


def _load(words):
    # mem[32k : 32k + 32] = calldata word k
    return b"".join(bytes([0x60, 32 * k, 0x35, 0x60, 32 * k, 0x52]) for k in range(words))


# balances[caller]-style: one 64-byte input hashed twice (the second is an LDS hit)
TWICE = _load(2) + _sha3(0, 64, 0) + _sha3(0, 64, 1) + b"\x00"


def _cd(*words):
    return b"".join(int(w).to_bytes(32, "big") for w in words)


def _batch(cds, rec_cap=0, trace_cap=0):
    b = LaneBatch(LaneShape(n=len(cds), stack_cap=16, mem_cap=256, calldata_cap=96, storage_cap=4,
                            rec_cap=rec_cap, trace_cap=trace_cap))
    for i, cd in enumerate(cds):
        b.set_lane(i, calldata=cd, gas_limit=GAS)
    return b


_REFS = {}


def _reference(key, code, make, hook_mask=None, loop_bound=0):
    """The batch of a case and its oracle result, computed once per key."""
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


def _check(dev, code, batch, ref, hook_mask=None, repeat=True):
    """One launch, then (repeat) three more from the same image; each exact."""
    gpu_in = batch.copy()
    gpu_in.code_id[:] = dev.load_code(code)
    dev.alloc(batch.shape)
    dev.upload(gpu_in)
    dev.step(hook_mask)
    outs = [LaneBatch(batch.shape)]
    dev.download(outs[0])
    if repeat:
        dev.upload(gpu_in)
        stats = dev.run_batches(3, hook_mask)
        assert len({s.lane_steps for s in stats}) == 1
        outs.append(LaneBatch(batch.shape))
        dev.download(outs[1])
    for out in outs:
        out.code_id[:] = 0
        assert not diff_batches(out, ref)
    return outs[-1]


def _uniform_waves(n_waves, salt):
    return lambda: [_cd(0xA11CE + salt, w) for w in range(n_waves) for _ in range(64)]


def _case1(n_waves, rec_cap, salt=0):
    return _reference(("uniform", n_waves, rec_cap, salt), TWICE,
                      lambda: _batch(_uniform_waves(n_waves, salt)(), rec_cap))


@contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.fixture
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def _assert_hashes(out, lanes, salt=0):
    for i in lanes:
        st = out.storage_dict(i, drop_zero=False)
        assert st[0] == st[1] == keccak_int(_cd(0xA11CE + salt, i // 64))


@pytest.mark.parametrize("rec_cap", [0, 512])
def test_many_uniform_inputs_contend_for_the_table(dev, rec_cap):
    """200 waves, wave w hashing input w: 200 publishers for 64 slots (claims,
    collisions, a full table), then launches that read what was published."""
    batch, ref = _case1(200, rec_cap)
    out = _check(dev, TWICE, batch, ref)
    assert (out.status == MG_HALT_STOP).all()
    _assert_hashes(out, (0, 63, 64, 64 * 99 + 5, 64 * 199 + 63))


def test_near_uniform_wave_stays_out_of_the_table(dev):
    """63 equal lanes and one odd lane per wave: not wave-uniform."""
    cds = [_cd(9, 1000 + i if i % 64 == 17 else i // 64) for i in range(64 * 4)]
    batch, ref = _reference("near", TWICE, lambda: _batch(cds, 512))
    out = _check(dev, TWICE, batch, ref)
    assert out.storage_dict(17)[0] == keccak_int(cds[17])
    assert out.storage_dict(18)[0] == keccak_int(cds[18])


def test_uniform_among_the_active_lanes_only(dev):
    """Half of each wave stops before the SHA3 (calldata word 2 == 0); the other
    half hashes one value.  Even waves stop their low half, so the first active
    lane is lane 32; odd waves stop every other lane."""
    # PUSH1 0x40 CALLDATALOAD PUSH1 7 JUMPI STOP JUMPDEST <TWICE>
    code = bytes([0x60, 0x40, 0x35, 0x60, 0x07, 0x57, 0x00, 0x5b]) + TWICE

    def go(i):
        w, l = divmod(i, 64)
        return l >= 32 if w % 2 == 0 else l % 2 == 1

    cds = [_cd(3, i // 64, int(go(i))) for i in range(64 * 6)]
    batch, ref = _reference("active", code, lambda: _batch(cds, 512))
    out = _check(dev, code, batch, ref)
    assert (out.status == MG_HALT_STOP).all()
    assert not out.storage_dict(0) and not out.storage_dict(64)
    assert out.storage_dict(32)[0] == out.storage_dict(63)[1] == keccak_int(_cd(3, 0))
    assert out.storage_dict(65)[0] == keccak_int(_cd(3, 1))


def test_table_is_keyed_by_content_not_address(dev):
    """The same 64 bytes hashed at memory offsets 0 and 32, then other bytes at 0."""
    code = (_load(3) + _sha3(0, 64, 0) + _sha3(32, 64, 1) +
            bytes([0x60, 0x05, 0x60, 0x00, 0x52]) + _sha3(0, 64, 2) + b"\x00")
    cds = [_cd(*([77 + i // 64] * 3)) for i in range(64 * 4)]
    batch, ref = _reference("content", code, lambda: _batch(cds, 512))
    out = _check(dev, code, batch, ref)
    st = out.storage_dict(64)
    assert st[0] == st[1] == keccak_int(_cd(78, 78))
    assert st[2] == keccak_int(_cd(5, 78))


def test_uncacheable_inputs_are_hashed(dev):
    """Length 63 and offset 1 on a uniform wave: neither cache level takes them."""
    code = _load(3) + _sha3(0, 63, 0) + _sha3(1, 64, 1) + _sha3(0, 64, 2) + b"\x00"
    cds = [_cd(11, i // 64, 13) for i in range(64 * 3)]
    batch, ref = _reference("uncacheable", code, lambda: _batch(cds, 512))
    out = _check(dev, code, batch, ref)
    st = out.storage_dict(70)
    assert st[0] == keccak_int(cds[70][:63])
    assert st[1] == keccak_int(cds[70][1:65])
    assert st[2] == keccak_int(cds[70][:64])


@pytest.mark.parametrize("lpw", [32, 16])
def test_narrow_waves(lpw):
    """MG_LANES_PER_WAVE 32 and 16 (read by mg_open): a group of 64 equal lanes
    is then two or four waves, each of them uniform."""
    with _env("MG_LANES_PER_WAVE", str(lpw)):
        d = GpuDevice(0)
    try:
        batch, ref = _case1(16, 512)
        out = _check(d, TWICE, batch, ref)
        _assert_hashes(out, (0, 31, 32, 64 * 15 + 48))
    finally:
        d.close()


def test_switch_off_gives_identical_output(dev):
    batch, ref = _case1(200, 512)
    with _env("MG_K1_KTAB", "0"):
        out = _check(dev, TWICE, batch, ref)
    _assert_hashes(out, (0, 64 * 199))


def test_two_contexts_keep_separate_tables(dev):
    """Two contexts on one GPU, one after the other, whose inputs differ: each
    is exact, so neither reads the other's table."""
    other = GpuDevice(0)
    try:
        for d, salt in ((dev, 0), (other, 1)):
            batch, ref = _case1(200, 512, salt)
            out = _check(d, TWICE, batch, ref)
            _assert_hashes(out, (5, 64 * 150), salt)
    finally:
        other.close()


def test_hooked_launch_reaches_the_table(dev):
    """A launch with a hook mask set (lanes stop at the SSTORE after the SHA3,
    the hash on top of their stacks)."""
    mask = hook_mask_for([0x55])
    cds = _uniform_waves(2, 7)()
    batch, ref = _reference("hooked", TWICE, lambda: _batch(cds, 512), hook_mask=mask)
    out = _check(dev, TWICE, batch, ref, hook_mask=mask)
    assert (out.status != MG_HALT_STOP).all()
    assert out.stack_words(100)[-2] == keccak_int(_cd(0xA11CE + 7, 1))


def test_loop_bound_launch_reaches_the_table(dev):
    """k_lane_step<true> (BoundedLoops on, traces kept) on a uniform batch."""
    cds = _uniform_waves(2, 8)()
    batch, ref = _reference("loop", TWICE, lambda: _batch(cds, 512, trace_cap=64), loop_bound=3)
    dev.set_loop_bound(3)
    out = _check(dev, TWICE, batch, ref)
    assert (out.status == MG_HALT_STOP).all()
    assert np.all(out.trace_len == ref.trace_len)
    _assert_hashes(out, (0, 127), 8)
