"""Kernel 1's SHA3, SLOAD and SSTORE on the fast path and the lane counts it keeps
in registers (lane_step.cuh: the K_SHA3 / K_SLOAD / K_SSTORE cases of the fast
switch, storage_find, kc_lookup / kc_insert, keccak64), on an MI355X.

Every case is bit-exact against oracle/evm_ref.c through OracleEVM and
diff_batches (status, aux, steps, msize, both gas bounds, stack, memory, storage,
record log and its length), plus the storage table entry by entry.  The programs are
hand-assembled; each lane takes its keys, offsets, lengths and data from its calldata,
so the lanes of one wave differ.
Each case asserts from the oracle's result that it holds lanes of every class it
aims at: lanes the fast path takes, lanes it leaves to the general handler, and
lanes that escape or raise."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.lanes import (MG_ESC_MEMORY, MG_ESC_OPCODE, MG_ESC_RECORD, MG_ESC_STORAGE, MG_ESCAPE,
                               MG_EXC_OUT_OF_GAS, MG_EXC_STACK_UNDERFLOW, MG_EXC_WRITE_PROTECTION, MG_HALT_STOP,
                               MG_HOOK, MG_LANE_CREATION, MG_LANE_STATIC, MG_MSTATE_GAS_LIMIT, MG_RUNNING,
                               MG_VMEXC, LaneBatch, LaneShape, diff_batches, word_to_limbs)
from oracle.evm_ref import OracleEVM

pytestmark = pytest.mark.gpu

M = (1 << 256) - 1
STOP, ADD, EXP, SHA3, CALLDATALOAD, CALLDATASIZE, CALLDATACOPY = 0x00, 0x01, 0x0A, 0x20, 0x35, 0x36, 0x37
MLOAD, MSTORE, SLOAD, SSTORE, MSIZE = 0x51, 0x52, 0x54, 0x55, 0x59
GAS = 10 ** 7


def push(v, k=None):
    k = k or max(1, (int(v).bit_length() + 7) // 8)
    return bytes([0x5F + k]) + int(v).to_bytes(k, "big")


def asm(*parts):
    return b"".join(bytes([p]) if isinstance(p, int) else p for p in parts)


def cd(k):
    """push calldata word k"""
    return asm(push(32 * k), CALLDATALOAD)


def words(*ws):
    return b"".join(int(w).to_bytes(32, "big") for w in ws)


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


_REFS = {}


def reference(key, code, make, **run_kw):
    """The batch of a case and its oracle result (one launch), computed once."""
    if key not in _REFS:
        batch = make()
        o = OracleEVM()
        ref = batch.copy()
        ref.code_id[:] = o.load_code(code)
        o.run(ref, **run_kw)
        ref.code_id[:] = 0
        _REFS[key] = (batch, ref)
    return _REFS[key]


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


@contextmanager
def device(dev, lpw=64, **env):
    """The module's device, or one opened with `lpw` lanes per wave, under `env`."""
    with environ(**env):
        if lpw == 64:
            yield dev
        else:
            with environ(MG_LANES_PER_WAVE=str(lpw)):
                d = GpuDevice(0)
            try:
                yield d
            finally:
                d.close()


def start(d, code, batch):
    gpu_in = batch.copy()
    gpu_in.code_id[:] = d.load_code(code)
    d.alloc(batch.shape)
    d.upload(gpu_in)
    return gpu_in


def result(d, shape):
    out = LaneBatch(shape)
    d.download(out)
    out.code_id[:] = 0
    return out


def same(out, ref):
    """diff_batches, and the storage table entry by entry (order included)."""
    diffs = diff_batches(out, ref, limit=20)
    for i in range(ref.n):
        c = int(ref.storage_count[i])
        if not np.array_equal(out.storage[i, :c], ref.storage[i, :c]):
            diffs.append(f"lane {i}: storage entries differ")
    return diffs[:20]


def exc(ref, kind):
    return (ref.status == MG_VMEXC) & (ref.aux == kind)


def esc(ref, op, reason):
    return (ref.status == MG_ESCAPE) & (ref.aux == (op | (reason << 8)))


def step_through(d, k, limit=200):
    for _ in range(limit):
        if d.step(max_steps=k).running == 0:
            return
    raise AssertionError("lanes still running")


# ---- storage ----------------------------------------------------------------------------

CAP = 6
COUNTS = [0, 1, 2, 3, CAP - 1, CAP]
# keys that differ from one another and from ABSENT in one high bit only
KEYS = [(1 << (40 * j + 3)) | 0x55 for j in range(CAP)]
ABSENT, FRESH = 0x55, (1 << 255) | 0x55
# words 0, 1: the keys loaded and stored, word 2: the value.  The store's key is loaded
# right after it; the first key is loaded again behind the store, which may have hit it.
STORAGE = asm(cd(0), SLOAD, cd(2), cd(1), SSTORE, cd(1), SLOAD, cd(0), SLOAD, STOP)


def pick(cnt, which):
    """entry 0, entry 1, the last entry, or no entry of a table of cnt entries"""
    if which == 3 or cnt == 0:
        return ABSENT
    return KEYS[[0, min(1, cnt - 1), cnt - 1][which]]


def storage_batch(n=256, trace_cap=0, static=True):
    b = LaneBatch(LaneShape(n=n, stack_cap=16, mem_cap=64, calldata_cap=96, storage_cap=CAP, trace_cap=trace_cap))
    for i in range(n):
        cnt = COUNTS[i % 6]
        k_load = pick(cnt, (i // 6) % 4)
        k_store = FRESH if (i // 24) % 3 == 2 else pick(cnt, [2, 0][(i // 24) % 3])
        if k_store == ABSENT:
            k_store = FRESH
        b.set_lane(i, calldata=words(k_load, k_store, M - i), gas_limit=GAS,
                   storage={KEYS[j]: (i << 32) | (j + 1) for j in range(cnt)},
                   flags=MG_LANE_STATIC if static and i % 16 == 5 else 0)
    return b


def assert_storage_classes(ref):
    stop = ref.status == MG_HALT_STOP
    full = esc(ref, SSTORE, MG_ESC_STORAGE)
    prot = exc(ref, MG_EXC_WRITE_PROTECTION)
    assert stop.any() and full.any() and prot.any() and (stop | full | prot).all()
    cnt0 = np.array([COUNTS[i % 6] for i in range(ref.n)])
    # a full table: a new key escapes, an existing key stores
    assert (full <= (cnt0 == CAP)).all() and (stop & (cnt0 == CAP)).any()
    # every initial count appears among the lanes that ran to the end, some with a new entry
    assert set(cnt0[stop].tolist()) == set(COUNTS)
    assert (ref.storage_count[stop] == cnt0[stop] + 1).any() and (ref.storage_count[stop] == cnt0[stop]).any()
    # loads that found entry 0, entry 1, a later entry, and nothing
    first = np.array([ref.stack_words(i)[0] if stop[i] else -1 for i in range(ref.n)], dtype=object)
    for j in (1, 2, 3, CAP):
        assert any(v != -1 and (v & 0xFFFFFFFF) == j for v in first), j
    assert any(v == 0 for v in first)


STORAGE_VARIANTS = {
    # name -> (lanes, lanes per wave, loop bound, hooked opcodes)
    "default": (256, 64, 0, None),
    "partial-wave": (130, 64, 0, None),
    "lpw32": (256, 32, 0, None),
    "lpw16": (256, 16, 0, None),
    "loop-bound": (256, 64, 3, None),
    "sload-hooked": (256, 64, 0, [SLOAD]),
    "sstore-hooked": (256, 64, 0, [SSTORE]),
}


@pytest.mark.parametrize("variant", list(STORAGE_VARIANTS))
def test_storage_equals_oracle(dev, variant):
    n, lpw, bound, hooked = STORAGE_VARIANTS[variant]
    mask = hook_mask_for(hooked) if hooked else None
    kw = {"loop_bound": bound} if bound else {}
    batch, ref = reference(("storage", n, bound, tuple(hooked or ())), STORAGE,
                           lambda: storage_batch(n, trace_cap=64 if bound else 0),
                           hook_mask=mask or (0, 0, 0, 0), **kw)
    with device(dev, lpw) as d:
        d.set_loop_bound(bound)
        try:
            start(d, STORAGE, batch)
            d.step(mask)
            out = result(d, batch.shape)
        finally:
            d.set_loop_bound(0)
    assert same(out, ref) == []
    if hooked:
        # stopped before the instruction: the table is the uploaded one
        assert (ref.status == MG_HOOK).all() and (ref.aux == hooked[0]).all()
        assert np.array_equal(out.storage, batch.storage)
    else:
        assert_storage_classes(ref)
        if bound:
            assert np.array_equal(out.trace_len, ref.trace_len)


@pytest.mark.parametrize("k", [1, 3])
def test_storage_paused_and_resumed(dev, k):
    """Launches of k instructions: each enters with the counts the last one left in memory."""
    batch, ref = reference(("storage", 256, 0, ()), STORAGE, storage_batch)
    start(dev, STORAGE, batch)
    assert dev.step(max_steps=k).running > 0
    step_through(dev, k)
    assert same(result(dev, batch.shape), ref) == []


def test_storage_count_comes_from_the_image(dev):
    """run_batches(3) = reset + step, three times: the program adds an entry, so a count kept
    from the launch before (and not the image's) would grow from batch to batch."""
    batch, ref = reference(("storage", 256, 0, ()), STORAGE, storage_batch)
    assert (ref.storage_count > batch.storage_count).any()
    start(dev, STORAGE, batch)
    stats = dev.run_batches(3)
    assert [s.running for s in stats] == [0, 0, 0]
    assert [s.lane_steps for s in stats] == [int(ref.steps.sum())] * 3
    assert same(result(dev, batch.shape), ref) == []
    dev.reset()
    dev.step()
    assert same(result(dev, batch.shape), ref) == []


def test_storage_count_changed_by_the_host_between_launches(dev):
    """step, download, the host drops or adds an entry, upload, step."""
    def edit(b):
        for i in range(b.n):
            c = int(b.storage_count[i])
            if i % 3 == 0 and c >= 1:
                b.storage_count[i] = c - 1
            elif i % 3 == 1 and c < CAP:
                b.storage[i, c, :8] = word_to_limbs(ABSENT)
                b.storage[i, c, 8:] = word_to_limbs(0xABCD00 + i)
                b.storage_count[i] = c + 1

    batch = storage_batch(static=False)
    o = OracleEVM()
    ref = batch.copy()
    ref.code_id[:] = o.load_code(STORAGE)
    o.run(ref, max_steps=5)                   # up to the SSTORE
    assert (ref.status == MG_RUNNING).all()
    edit(ref)
    o.run(ref)
    ref.code_id[:] = 0
    gpu_in = start(dev, STORAGE, batch)
    dev.step(max_steps=5)
    mid = LaneBatch(batch.shape)
    dev.download(mid)
    edit(mid)
    mid.code_id[:] = gpu_in.code_id
    dev.upload(mid)
    dev.step()
    assert same(result(dev, batch.shape), ref) == []
    assert (ref.status == MG_HALT_STOP).any() and esc(ref, SSTORE, MG_ESC_STORAGE).any()


def gas_points(code, make_one, upto):
    """gas_min of one lane after each of its first `upto` instructions"""
    o = OracleEVM()
    cid = o.load_code(code)
    pts = []
    for k in range(1, upto + 1):
        b = make_one()
        b.code_id[:] = cid
        o.run(b, max_steps=k)
        pts.append(int(b.gas_min[0]))
    return pts


def gas_batch(make_one, pts, fill, near_limit=True):
    """Lanes whose gas limit lies one below, at and above every point in `pts`; with
    near_limit also lanes that start that far below the machine-state limit of 10^9
    under a transaction limit above it."""
    cases = [(p + d, 0) for p in sorted(set(pts)) for d in (-1, 0, 1, 2)]
    if near_limit:
        cases += [(2 * 10 ** 9, MG_MSTATE_GAS_LIMIT - p + j) for p in sorted(set(pts)) for j in (-2, -1, 0, 1)]
    one = make_one()
    b = LaneBatch(LaneShape(n=len(cases), stack_cap=one.shape.stack_cap, mem_cap=one.shape.mem_cap,
                            calldata_cap=one.shape.calldata_cap, storage_cap=one.shape.storage_cap,
                            rec_cap=one.shape.rec_cap))
    for i, (limit, g0) in enumerate(cases):
        fill(b, i)
        b.gas_limit[i] = max(limit, 0)
        b.gas_min[i] = b.gas_max[i] = g0
    return b


def test_storage_gas_edges(dev):
    """The gas limit one either side of what each instruction of the storage program needs."""
    def fill(b, i):
        b.set_lane(i, calldata=words(KEYS[1], FRESH if i % 2 else KEYS[0], M - i),
                   storage={KEYS[0]: 5, KEYS[1]: 6})

    def one():
        b = LaneBatch(LaneShape(n=1, stack_cap=16, mem_cap=64, calldata_cap=96, storage_cap=CAP))
        fill(b, 0)
        b.gas_limit[0] = 2 * 10 ** 9
        return b

    pts = gas_points(STORAGE, one, 16)
    batch, ref = reference("storage-gas", STORAGE, lambda: gas_batch(one, pts, fill))
    assert 64 < batch.n <= 256
    oog = exc(ref, MG_EXC_OUT_OF_GAS)
    assert oog.any() and (ref.status == MG_HALT_STOP).any() and (oog | (ref.status == MG_HALT_STOP)).all()
    # out of gas at the first SLOAD (instruction 2) and at the SSTORE (instruction 7), and past both
    assert {2, 7} <= set(ref.pc[oog].tolist())
    start(dev, STORAGE, batch)
    dev.step()
    assert same(result(dev, batch.shape), ref) == []


@pytest.mark.parametrize("code,op", [(asm(SLOAD, STOP), SLOAD), (asm(SSTORE, STOP), SSTORE),
                                     (asm(push(1), SSTORE, STOP), SSTORE)])
def test_storage_stack_underflow(dev, code, op):
    """sp 0 and 1: the general handler raises; 130 lanes, a partial last wave."""
    def make():
        b = LaneBatch(LaneShape(n=130, stack_cap=16, mem_cap=64, calldata_cap=32, storage_cap=CAP))
        for i in range(130):
            b.set_lane(i, gas_limit=GAS, storage={KEYS[0]: 1}, flags=MG_LANE_STATIC if i % 4 == 1 else 0)
        return b

    batch, ref = reference(("underflow", code), code, make)
    # (SSTORE's precheck asks for one word: a static lane with one raises write protection first)
    under, prot = exc(ref, MG_EXC_STACK_UNDERFLOW), exc(ref, MG_EXC_WRITE_PROTECTION)
    assert under.any() and (under | prot).all()
    start(dev, code, batch)
    dev.step()
    assert same(result(dev, batch.shape), ref) == []


# ---- SHA3 -------------------------------------------------------------------------------

# words 0, 1: offset and length of the first SHA3, words 2, 3: the 64 bytes at 0
SHA = asm(cd(2), push(0), MSTORE, cd(3), push(0x20), MSTORE, cd(1), cd(0), SHA3,
          push(0x40), push(0), SHA3, push(3), push(7), EXP, MSIZE, STOP)
# the SHA3 itself grows memory from msize 0
SHA0 = asm(cd(1), cd(0), SHA3, MSIZE, push(0x40), push(0x20), SHA3, STOP)
SHA_PROGRAMS = {"sha": SHA, "sha0": SHA0}
SHA_STEPS = {"sha": 12, "sha0": 4}     # instructions before the first SHA3
WINDOW = 160                           # the default LDS memory window, bytes
# 0, 0x20, the last offset inside the window, one straddling its edge, two in HBM, unaligned
# ones, one past mem_cap 256
OFFS = [0, 0x20, 96, 100, 160, 192, 1, 2, 3, 200, 4, 64, 2 ** 32 - 64]
LENS = [64, 0, 32, 64, 63, 64, 65, 136, 64, 137]


def sha_batch(n=256, mem_cap=256, rec_cap=0, data_mod=5, uniform=False):
    """Lane i's offset and length walk OFFS and LENS at coprime strides; its data is one
    of data_mod values, so a wave's inputs hit its four cache entries partly and evict."""
    b = LaneBatch(LaneShape(n=n, stack_cap=16, mem_cap=mem_cap, calldata_cap=128, storage_cap=1, rec_cap=rec_cap))
    for i in range(n):
        off, ln = (0, 64) if uniform else (OFFS[i % len(OFFS)], LENS[(i + i // len(OFFS)) % len(LENS)])
        key = 0xDEADBEEF if uniform else (0xA11CE << 100) | (i % data_mod)
        b.set_lane(i, calldata=words(off, ln, key, 1), gas_limit=GAS)
    return b


def sha_classes(batch, ref, name):
    """(fast path, general handler, escape) lanes of the first SHA3, from the inputs"""
    ms0 = 64 if name == "sha" else 0
    off = np.array([int.from_bytes(bytes(batch.calldata[i, :32]), "big") for i in range(batch.n)], dtype=object)
    ln = np.array([int.from_bytes(bytes(batch.calldata[i, 32:64]), "big") for i in range(batch.n)], dtype=object)
    lim = min(WINDOW, batch.shape.mem_cap)
    fast = np.array([l == 64 and o % 4 == 0 and (o + 64 <= ms0 or (o + 95) // 32 * 32 <= lim)
                     for o, l in zip(off, ln)])
    escm = esc(ref, SHA3, MG_ESC_MEMORY)
    return fast & ~escm, ~fast & ~escm, escm


SHA_VARIANTS = {
    # name -> (environment, lanes, lanes per wave, loop bound)
    "default": ({}, 256, 64, 0),
    "partial-wave": ({}, 130, 64, 0),
    "ktab0": ({"MG_K1_KTAB": "0"}, 256, 64, 0),
    "memwin0": ({"MG_K1_MEMWIN": "0"}, 256, 64, 0),
    "lpw32": ({}, 256, 32, 0),
    "loop-bound": ({}, 256, 64, 3),
}


@pytest.mark.parametrize("variant", list(SHA_VARIANTS))
@pytest.mark.parametrize("rec_cap", [0, 64, 128])
@pytest.mark.parametrize("name", list(SHA_PROGRAMS))
def test_sha3_equals_oracle(dev, name, rec_cap, variant):
    env, n, lpw, bound = SHA_VARIANTS[variant]
    code = SHA_PROGRAMS[name]
    kw = {"loop_bound": bound} if bound else {}
    batch, ref = reference((name, n, rec_cap, bound), code, lambda: sha_batch(n, rec_cap=rec_cap), **kw)
    with device(dev, lpw, **env) as d:
        d.set_loop_bound(bound)
        try:
            start(d, code, batch)
            d.step()
            out = result(d, batch.shape)
            # a second and a third launch on the same image: the table's entries are usable now
            stats = d.run_batches(2)
            again = result(d, batch.shape)
        finally:
            d.set_loop_bound(0)
    assert same(out, ref) == []
    if not bound:
        # (the image of a batch holds no trace: run_batches is not the loop-bound case)
        assert [s.lane_steps for s in stats] == [int(ref.steps.sum())] * 2
        assert same(again, ref) == []
    fast, slow, escm = sha_classes(batch, ref, name)
    assert fast.any() and slow.any() and escm.any()
    assert exc(ref, MG_EXC_OUT_OF_GAS).any()                 # the offset near 2^32
    if rec_cap == 64:
        # 45 or 46 words of a long first record leave no room for the second SHA3's 27; two
        # records of 27 leave none for the EXP's
        assert esc(ref, SHA3, MG_ESC_RECORD).any()
        assert name != "sha" or esc(ref, EXP, MG_ESC_RECORD)[fast].any()
    else:
        assert (ref.status[fast] == MG_HALT_STOP).all() and (ref.status[slow] == MG_HALT_STOP).any()
    if rec_cap:
        i = int(np.nonzero(fast)[0][0])
        recs = ref.records(i)
        assert recs[0][:2] == (SHA_STEPS[name], "keccak") and len(recs[0][2]) == 64


# the uniform batch: every lane hashes the same 64 bytes twice, then EXP: 27 + 27 + 27 words
@pytest.mark.parametrize("rec_cap,stops_at", [(81, None), (80, EXP), (54, EXP), (53, SHA3), (27, SHA3), (26, SHA3)])
def test_sha3_record_room(dev, rec_cap, stops_at):
    """An exact fit, and one word short for each record: MG_ESC_RECORD with the lane untouched and
    its step count exact.  Every lane's input is the same: the second SHA3 hits the wave's cache."""
    batch, ref = reference(("uniform", rec_cap), SHA, lambda: sha_batch(rec_cap=rec_cap, uniform=True))
    if stops_at is None:
        assert (ref.status == MG_HALT_STOP).all() and (ref.rec_len == rec_cap).all()
    else:
        assert esc(ref, stops_at, MG_ESC_RECORD).all()
        steps = {80: 18, 54: 18, 53: 15, 27: 15, 26: 12}[rec_cap]
        assert (ref.steps == steps).all() and (ref.rec_len == {18: 54, 15: 27, 12: 0}[steps]).all()
    start(dev, SHA, batch)
    dev.step()
    assert same(result(dev, batch.shape), ref) == []


@pytest.mark.parametrize("name,k", [("sha", 1), ("sha", 13), ("sha0", 5)])
def test_sha3_paused_and_resumed(dev, name, k):
    """Launches of k instructions: one ends right behind the first SHA3, so the next enters
    with a non-zero record length and writes its record's step from the steps so far."""
    code = SHA_PROGRAMS[name]
    batch, ref = reference((name, 256, 128, 0), code, lambda: sha_batch(rec_cap=128))
    start(dev, code, batch)
    assert dev.step(max_steps=k).running > 0
    if k > 1:
        mid = result(dev, batch.shape)
        assert ((mid.status == MG_RUNNING) & (mid.rec_len > 0)).any()
    step_through(dev, k)
    assert same(result(dev, batch.shape), ref) == []


@pytest.mark.parametrize("data_mod", [1, 3, 4, 7])
def test_sha3_cache_hits_and_evictions(dev, data_mod):
    """One, three, four and seven distinct inputs in a wave of 64 against a cache of four
    entries: all-hit, partial-hit and evicting dispatches; with the table and without."""
    def make():
        b = sha_batch(rec_cap=96, data_mod=data_mod)
        for i in range(b.n):     # every lane the mapping-slot shape, at 0 or growing to 0x20
            b.calldata[i, :64] = np.frombuffer(words(0x20 if i % 8 == 3 else 0, 64), dtype=np.uint8)
        return b

    batch, ref = reference(("cache", data_mod), SHA, make)
    assert (ref.status == MG_HALT_STOP).all() and (ref.rec_len == 81).all()
    for env in ({}, {"MG_K1_KTAB": "0"}):
        with environ(**env):
            start(dev, SHA, batch)
            dev.step()
            assert same(result(dev, batch.shape), ref) == [], env
            stats = dev.run_batches(2)
            assert [s.running for s in stats] == [0, 0]
            assert same(result(dev, batch.shape), ref) == [], env


def test_sha3_gas_edges(dev):
    """The gas limit one either side of what each instruction needs, for a SHA3 inside msize and
    one that grows memory; and lanes that start just below the machine-state limit, where the
    SHA3's own gas is tested against the limit and its memory fee against 10^9 alone."""
    for off in (0, 0x20, 96):
        def fill(b, i):
            b.set_lane(i, calldata=words(off, 64, 0xFEED00 + (i % 3), 2))

        def one():
            b = LaneBatch(LaneShape(n=1, stack_cap=16, mem_cap=256, calldata_cap=128, storage_cap=1, rec_cap=96))
            fill(b, 0)
            b.gas_limit[0] = 2 * 10 ** 9
            return b

        pts = gas_points(SHA, one, 19)
        batch, ref = reference(("sha-gas", off), SHA, lambda: gas_batch(one, pts, fill))
        assert 64 < batch.n <= 256
        oog = exc(ref, MG_EXC_OUT_OF_GAS)
        assert (oog | (ref.status == MG_HALT_STOP)).all() and (ref.status == MG_HALT_STOP).any()
        # out of gas at the first SHA3 (instruction 12) and at the second (15)
        assert {12, 15} <= set(ref.pc[oog].tolist())
        near = np.asarray(batch.gas_min) != 0
        assert oog[near].any() and (~oog[near]).any()
        start(dev, SHA, batch)
        dev.step()
        assert same(result(dev, batch.shape), ref) == [], off


# ---- calldata ---------------------------------------------------------------------------

# CALLDATASIZE opening a run and as a dispatch of its own (between two CALLDATALOADs);
# CALLDATALOAD at 0 (a dispatch of its own), at 4 and at 36; a CALLDATACOPY of 40 bytes from 2
CALLDATA = asm(CALLDATASIZE, push(0), CALLDATALOAD, CALLDATASIZE, CALLDATALOAD, push(4), CALLDATALOAD,
               push(36), CALLDATALOAD, CALLDATASIZE, push(1), ADD, push(40), push(2), push(0), CALLDATACOPY,
               push(0), MLOAD, push(32), MLOAD, CALLDATASIZE, STOP)
CD_LENS = [0, 31, 32, 36, 68]


def calldata_batch(n=256):
    b = LaneBatch(LaneShape(n=n, stack_cap=16, mem_cap=128, calldata_cap=96, storage_cap=1))
    for i in range(n):
        ln = CD_LENS[(i + i // 5) % 5]
        b.set_lane(i, calldata=bytes((7 * i + 13 * k + 1) & 0xFF for k in range(ln)), gas_limit=GAS,
                   flags=MG_LANE_CREATION if i % 8 == 7 else 0)
    return b


@pytest.mark.parametrize("n,lpw", [(256, 64), (130, 64), (256, 16)])
def test_calldata_length_in_registers(dev, n, lpw):
    batch, ref = reference(("calldata", n), CALLDATA, lambda: calldata_batch(n))
    creation = (batch.flags & MG_LANE_CREATION) != 0
    assert esc(ref, CALLDATASIZE, MG_ESC_OPCODE)[creation].all()           # as before: at the first opcode
    assert (ref.status[~creation] == MG_HALT_STOP).all()
    for ln in CD_LENS:   # every length among the lanes that ran, and pushed by the last CALLDATASIZE
        lanes = np.nonzero(~creation & (batch.calldata_len == ln))[0]
        assert len(lanes) and all(ref.stack_words(i)[-1] == ln for i in lanes)
    # in one wave: loads wholly inside the calldata (the fast path) and partly past its end
    assert {0, 31, 32, 68} <= set(batch.calldata_len[:64].tolist())
    with device(dev, lpw) as d:
        start(d, CALLDATA, batch)
        d.step()
        assert same(result(d, batch.shape), ref) == []
        step_k = 3
        start(d, CALLDATA, batch)
        step_through(d, step_k)
        assert same(result(d, batch.shape), ref) == []
