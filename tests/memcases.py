"""Case lists for kernel 1's memory, copy and SHA3 opcodes (test-only).

One batch per opcode, shared by test_memory_ops_cpu.py (oracle against the
pymem model) and test_gpu_memory_ops.py (device against both).  The device
tests run each batch under LDS memory windows W of 0, 32, 96 and 160 bytes;
the lists enumerate the edges of all four at once, so one batch (and one model
run) serves every window: WINDOWS are the W, MSIZES the initial memory sizes
{0, 32, 64, W, W + 32, 512} over those W, plus mem_cap itself so that the
whole junk-filled page is uploaded.

Lanes are shuffled with a fixed seed: outcome classes mix inside every wave.
"""
import random
from functools import lru_cache

import pymem
import pysem
from mythril_amd.lanes import LaneBatch, LaneShape

WINDOWS = (0, 32, 96, 160)
MEM_CAP = 2048
MSIZES = (0, 32, 64, 96, 128, 160, 192, 512, MEM_CAP)
T32, T256 = 1 << 32, 1 << 256
GAS = 10 ** 7


def edge_offsets():
    """Every byte offset in [0, 8], [W - 40, W + 8] and [M - 40, M + 8]."""
    out = set(range(0, 9))
    for e in WINDOWS + MSIZES:
        out.update(k for k in range(e - 40, e + 9) if k >= 0)
    return sorted(out)


def far_offsets(size):
    """Fits exactly, escapes, the 2^32 edge, and ends that wrap or cannot fit."""
    return [MEM_CAP - size, MEM_CAP - size + 1, T32 - size, T32 - size + 1, T32,
            T256 - 1, T256 - 32]


def dst_offsets(size):
    """Destinations of a `size`-byte range at every alignment across each W and M."""
    out = set(range(0, 4))
    for e in WINDOWS + MSIZES[:-1]:
        for a in range(4):
            out.add(max(0, e - size // 2 - 1 + a))
        out.update(k for k in (e - size, e - 1, e, e + 1) if k >= 0)
    return sorted(out)


def _finish(codes, rows, seed, *, calldata_cap=128, rec_cap=0, fixed=()):
    """rows: dicts for pymem.set_lane; `fixed` rows keep their places in front
    (whole waves with a layout of their own), the rest is shuffled."""
    rows = list(rows)
    random.Random(seed).shuffle(rows)
    rows = list(fixed) + rows
    assert len(rows) <= 8192, len(rows)
    b = LaneBatch(LaneShape(n=len(rows), stack_cap=16, mem_cap=MEM_CAP, calldata_cap=calldata_cap,
                            storage_cap=4, rec_cap=rec_cap))
    pymem.fill_memory(b, seed)
    for i, r in enumerate(rows):
        r = dict(r)
        image = r.pop("image", None)
        pymem.set_lane(b, i, **r)
        if image is not None:
            b.memory[i, : len(image)] = list(image)
    return codes, b


def _values(rng, n):
    sp = pysem.special_words()
    return [sp[k % len(sp)] if k % 3 else rng.getrandbits(256) | (0xA5 << 248) for k in range(n)]


@lru_cache(maxsize=None)
def mload_cases():
    rng = random.Random(0x51)
    rows = []
    offs = edge_offsets()
    for k, off in enumerate(offs):
        for j in range(4):   # each edge offset under four memory sizes, the nearest ones included
            near = [m for m in MSIZES if abs(m - off) <= 48]
            m = near[j % len(near)] if near and j < 2 else MSIZES[(k + 3 * j) % len(MSIZES)]
            rows.append(dict(code_id=0, calldata=pymem.words(off), msize=m))
    for off in far_offsets(32):
        for m in MSIZES:
            rows.append(dict(code_id=0, calldata=pymem.words(off), msize=m))
    for _ in range(400):
        rows.append(dict(code_id=0, calldata=pymem.words(rng.randrange(MEM_CAP - 32)),
                         msize=rng.choice(MSIZES)))
    return _finish([pymem.mload_program()], rows, 0x51)


def _store_cases(program, size, seed):
    rng = random.Random(seed)
    rows = []
    offs = edge_offsets()
    vals = _values(rng, 4 * len(offs) + 1024)
    nv = 0

    def row(off, m):
        nonlocal nv
        v = vals[nv % len(vals)]
        nv += 1
        if size == 1:      # MSTORE8: non-zero upper bytes; reload the word the byte lands in
            v |= 0xC3 << 8 | 0x5A << 200
            second = max(0, off - rng.randrange(32)) if off < T32 else off
        else:
            second = (off - 1) % T256
        return dict(code_id=0, calldata=pymem.words(off, v, second), msize=m)
    for k, off in enumerate(offs):
        near = [m for m in MSIZES if abs(m - off) <= 48]
        for j in range(4):
            m = near[j % len(near)] if near and j < 2 else MSIZES[(k + 3 * j) % len(MSIZES)]
            rows.append(row(off, m))
    for off in far_offsets(size):
        for m in MSIZES:
            rows.append(row(off, m))
    for _ in range(400):
        rows.append(row(rng.randrange(MEM_CAP - 32), rng.choice(MSIZES)))
    return _finish([program], rows, seed)


@lru_cache(maxsize=None)
def mstore_cases():
    return _store_cases(pymem.mstore_program(), 32, 0x52)


@lru_cache(maxsize=None)
def mstore8_cases():
    return _store_cases(pymem.mstore8_program(), 1, 0x53)


CD_LENS = (0, 1, 31, 32, 33, 100)


def _calldata(rng, n):
    return bytes(rng.randrange(1, 256) for _ in range(n))


@lru_cache(maxsize=None)
def calldataload_cases():
    rng = random.Random(0x35)
    pairs = []
    for n in CD_LENS:
        offs = [n + d for d in range(-33, 2) if n + d >= 0]
        offs += list(range(0, max(n - 31, 0), 4))            # aligned and inside: the fast path
        offs += [1, 2, 3, 5, 30, T32 - 1, T32, T32 + 1]
        offs += [T256 - k for k in range(1, 34)]              # bytes wrap round to index 0
        for off in offs:
            pairs.append((n, off))
    rows = []
    for k, (n, off) in enumerate(pairs):
        other = pairs[(7 * k + 3) % len(pairs)][1]
        rows.append(dict(code_id=0, calldata=_calldata(rng, n), stack=(other, off)))
    return _finish([pymem.calldataload_program()], rows, 0x35)


def _sources(n, size):
    """Inside the calldata (or code) of n bytes, straddling its end, at it, past it, wrapping."""
    return [0, max(0, n - size) // 2, max(0, n - size // 2 - 1), n - 1 if n else 0, n, n + 7, T32 - 1, T32,
            T32 + 3, T256 - 1, T256 - max(1, size // 2), T256 - size - 3]


@lru_cache(maxsize=None)
def calldatacopy_cases():
    rng = random.Random(0x37)
    rows = []
    k = 0
    for size in (1, 3, 4, 5, 31, 32, 33, 100):
        for dst in dst_offsets(size):
            for j in range(2):
                n = (100, 100, 33, 100, 0, 100)[k % 6]
                srcs = _sources(n, size)
                rows.append(dict(code_id=0, calldata=_calldata(rng, n),
                                 stack=(size, srcs[k % len(srcs)], dst),
                                 msize=MSIZES[(k + 5 * j) % len(MSIZES)]))
                k += 1
    for m in MSIZES:
        # size 0: nothing at all, whatever the memory offset
        for dst in (T256 - 1, T32, MEM_CAP + 100, m + 64):
            rows.append(dict(code_id=0, calldata=_calldata(rng, 100), stack=(0, 3, dst), msize=m))
        # zeros from past the calldata land on pattern bytes
        rows.append(dict(code_id=0, calldata=_calldata(rng, 33), stack=(33, 20, max(0, m - 40)), msize=m))
        for size in (1, 33, 100):
            for dst in far_offsets(size):
                rows.append(dict(code_id=0, calldata=_calldata(rng, 100), stack=(size, 5, dst), msize=m))
        rows.append(dict(code_id=0, calldata=_calldata(rng, 100), stack=(T32, 0, 0), msize=m))
        rows.append(dict(code_id=0, calldata=_calldata(rng, 100), stack=(T256 - 1, 0, 1), msize=m))
    return _finish([pymem.calldatacopy_program()], rows, 0x37)


@lru_cache(maxsize=None)
def codecopy_cases():
    code = pymem.codecopy_program()
    n = len(code)
    rows = []
    k = 0
    for size in (0, 1, 3, 4, 5, 31, 32, 33, 100):
        for dst in dst_offsets(size):
            srcs = _sources(n, size)
            rows.append(dict(code_id=0, calldata=pymem.words(dst, srcs[k % len(srcs)], size),
                             msize=MSIZES[k % len(MSIZES)]))
            rows.append(dict(code_id=0, calldata=pymem.words(dst, srcs[(k + 5) % len(srcs)], size),
                             msize=MSIZES[(k + 4) % len(MSIZES)]))
            k += 1
    for m in MSIZES:
        for dst in (m + 1, m + 64, MEM_CAP, MEM_CAP + 1):    # size 0 past msize: extends and pays
            rows.append(dict(code_id=0, calldata=pymem.words(dst, 2, 0), msize=m))
        for size in (1, 33, 100):
            for dst in far_offsets(size):
                rows.append(dict(code_id=0, calldata=pymem.words(dst, n - 9, size), msize=m))
        rows.append(dict(code_id=0, calldata=pymem.words(0, 0, T32), msize=m))
    return _finish([code], rows, 0x39)


# 2, 3, 5, 11, 12 and 139 complete the residues modulo 8 (the kernel masks the last
# one to seven bytes of each 8-byte lane and of each 4-byte record word)
SHA3_LENS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 134, 135, 136, 137, 143, 144, 271, 272,
             273, 408, 2, 3, 5, 11, 12, 139)


@lru_cache(maxsize=None)
def sha3_cases(rec_cap):
    rng = random.Random(0x20)
    ranges = []
    sha_m = (64, 160, 512)
    for ln in SHA3_LENS:
        for a in range(4):
            ranges.append((a, ln))
            for w in WINDOWS[1:]:                              # straddles the window's edge
                ranges.append((max(0, w - ln // 2 - 2) + a, ln))
            for m in sha_m:                                    # ends past msize: hashes the zero extension
                ranges.append((max(0, m - ln // 2 - 2) + a, ln))
    rows = []
    for k, (off, ln) in enumerate(ranges):
        off2, ln2 = ranges[(k * 37 + 11) % len(ranges)]
        if k % 2:            # the second hash is a short one for half the lanes (the Python Keccak is slow)
            ln2 = SHA3_LENS[(k // 2) % 10]
        rows.append(dict(code_id=0, calldata=pymem.words(off, ln, off2, ln2),
                         msize=(sha_m + (MEM_CAP,))[k % 4] if k % 8 else 0))
    for m in (0, 64, 512):
        for ln in (T32, T32 + 1, T256 - 1):
            for off in (0, 1):
                rows.append(dict(code_id=0, calldata=pymem.words(off, ln, 0, 0), msize=m, gas_limit=10 ** 9))
        for ln in (1, 33, 137):
            for off in (MEM_CAP - ln, MEM_CAP - ln + 1, MEM_CAP, T32 - ln, T32, T256 - 1):
                rows.append(dict(code_id=0, calldata=pymem.words(off, ln, 2, 9), msize=m))
                rows.append(dict(code_id=0, calldata=pymem.words(3, 5, off, ln), msize=m))
        for lim in (20, 36, 37, 60):                           # SHA3's own gas against the limit
            rows.append(dict(code_id=0, calldata=pymem.words(0, 32, 0, 64), msize=m, gas_limit=lim))
    # whole waves with a layout of their own (the per-wave Keccak result cache)
    fixed = []
    key = bytes(rng.randrange(1, 256) for _ in range(192))
    other = bytes(rng.randrange(1, 256) for _ in range(192))
    same = pymem.words(32, 64, 32, 64)
    for lane in range(64):      # wave 0: every lane hashes the same aligned 64 bytes twice
        fixed.append(dict(code_id=0, calldata=same, msize=192, image=key))
    for lane in range(64):      # wave 1: one lane's bytes differ
        fixed.append(dict(code_id=0, calldata=same, msize=192, image=other if lane == 17 else key))
    for lane in range(64):      # wave 2: cacheable lanes next to other lengths and alignments
        cd = (same, pymem.words(32, 63, 32, 64), pymem.words(33, 64, 32, 65), pymem.words(32, 64, 36, 64),
              pymem.words(32, 137, 32, 64), pymem.words(32, 0, 160, 64))[lane % 6]
        fixed.append(dict(code_id=0, calldata=cd, msize=192, image=key))
    for lane in range(64):      # wave 3: as wave 2, the lowest lane not cacheable, some lanes out of gas
        cd = (pymem.words(34, 64, 32, 64), same, pymem.words(32, 64, 32, 64), pymem.words(96, 64, 32, 64))[lane % 4]
        fixed.append(dict(code_id=0, calldata=cd, msize=(192, 64)[lane % 5 == 0], image=key,
                          gas_limit=GAS if lane % 7 else 70))
    return _finish([pymem.sha3_program()], rows, 0x20, rec_cap=rec_cap, fixed=fixed)


@lru_cache(maxsize=None)
def gas_cases():
    """MSTORE, SHA3 and CALLDATACOPY with the gas limit exactly at, below and
    above what the model says the instruction under test needs; new memory
    sizes of 32, 704, 736 bytes (22 and 23 words: nw * nw / 512 steps) and
    mem_cap, and extensions past mem_cap where the limit decides between out of
    gas and the escape."""
    codes = [pymem.mstore_program(), pymem.sha3_program(), pymem.calldatacopy_program()]
    target_pc = (5, 5, 1)     # instruction index after the opcode under test
    rows = []
    # Past the page only the look-ahead sees the fee.  A page of 64 words is too
    # small to tell the quadratic term's denominator from its neighbours
    # (n * n // 512 == n * n // 511 for every n <= 64); 75, 143 and 150 words
    # are the first sizes where the two differ, and there the limit `need`
    # escapes while `need - 1` is out of gas.
    ends = (32, 704, 736, MEM_CAP, MEM_CAP + 32, MEM_CAP + 64, 75 * 32, 143 * 32, 150 * 32)
    for m in (0, 32, 64, 160, 512, 704):
        for end in ends:
            if end <= m:
                continue
            for slack in (0, 1, 31):
                ln = min(40, end - slack)
                protos = [
                    dict(code_id=1, calldata=pymem.words(end - slack - ln, ln, 0, 0), msize=m),
                    dict(code_id=2, calldata=bytes(range(1, 101)), stack=(ln, 90, end - slack - ln), msize=m),
                ]
                if end - 32 - slack >= 0:
                    protos.append(dict(code_id=0, calldata=pymem.words(end - 32 - slack, 0x1234 << 100, 0),
                                       msize=m))
                for p in protos:
                    need = _need(codes, p, target_pc[p["code_id"]])
                    for lim in (need - 2, need - 1, need, need + 1, need + 2, GAS):
                        rows.append(dict(p, gas_limit=lim))
    return _finish(codes, rows, 0x6A5)


def _need(codes, row, pc_after):
    """The smallest gas limit under which the model, on an unlimited page, gets
    past the instruction under test (found by bisection: passing is monotone)."""
    def passes(limit):
        m = pymem.Model(codes[row["code_id"]], row["calldata"], limit, memory=bytes(row["msize"]),
                        mem_cap=1 << 30, stack=row.get("stack", ()))
        m.ins = m.ins[:pc_after] + [(0x00, None)]
        r = m.run()
        return r.outcome() == "normal" and r.pc == pc_after
    lo, hi = 0, 10 ** 9          # passes(hi), not passes(lo)
    assert passes(hi) and not passes(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if passes(mid):
            hi = mid
        else:
            lo = mid
    return hi


@lru_cache(maxsize=None)
def return_cases():
    codes = [pymem.return_program(0xF3), pymem.return_program(0xFD)]
    rows = []
    for m in MSIZES:
        ranges = [(3, 40), (0, m), (max(0, m - 10), 50), (m, 32), (5, 0), (m + 100, 0), (T32, 0), (T32 + 5, 0),
                  (T256 - 1, 0), (1, 1), (max(0, m - 33), 33), (MEM_CAP - 50, 50), (MEM_CAP - 50, 51)]
        for cid in (0, 1):
            for off, ln in ranges:
                rows.append(dict(code_id=cid, calldata=pymem.words(off, ln), msize=m))
        for off, ln in ((0, T32), (T32 - 1, 2), (T256 - 1, 1), (T256 - 1, 2), (0, MEM_CAP + 1), (MEM_CAP, 1)):
            rows.append(dict(code_id=0, calldata=pymem.words(off, ln), msize=m))
        for lim in (3, 12, 13, 14, 20):       # RETURN's check_gas_usage_limit after four table-gas steps
            rows.append(dict(code_id=0, calldata=pymem.words(0, 32), msize=m, gas_limit=lim))
            rows.append(dict(code_id=0, calldata=pymem.words(m, 64), msize=m, gas_limit=lim + 6))
    return _finish(codes, rows, 0xF3)


CASES = {
    "mload": mload_cases, "mstore": mstore_cases, "mstore8": mstore8_cases,
    "calldataload": calldataload_cases, "calldatacopy": calldatacopy_cases,
    "codecopy": codecopy_cases, "gas": gas_cases, "return": return_cases,
}


@lru_cache(maxsize=None)
def model_results(name, rec_cap=0):
    codes, b = sha3_cases(rec_cap) if name == "sha3" else CASES[name]()
    return [pymem.model_lane(b, codes, i) for i in range(b.n)]
