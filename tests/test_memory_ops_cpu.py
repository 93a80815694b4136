"""The C oracle against the pymem model on the memory, copy and SHA3 opcodes.

Runs every case list of memcases.py (the ones test_gpu_memory_ops.py runs on
the device) through oracle/evm_ref.c and asserts that every lane's status,
exception or escape kind, pc, steps, msize, gas bounds, stack, memory up to
msize, storage, return data and decoded keccak records equal the model's.  It
also checks, with the oracle alone, that the lists are not vacuous: every
outcome class a test names occurs, and classes mix inside single waves.
"""
import numpy as np
import pytest

import memcases
import pymem
from mythril_amd.lanes import MG_ESC_MEMORY, MG_ESCAPE, MG_EXC_OUT_OF_GAS, MG_VMEXC, LaneBatch
from oracle.evm_ref import OracleEVM

# the outcome classes each list must contain ("normal" = STOP, RETURN or REVERT)
CLASSES = {
    "mload": ("normal", "oog", "escape"), "mstore": ("normal", "oog", "escape"),
    "mstore8": ("normal", "oog", "escape"), "calldataload": ("normal",),
    "calldatacopy": ("normal", "oog", "escape"), "codecopy": ("normal", "oog", "escape"),
    "sha3": ("normal", "oog", "escape"), "gas": ("normal", "oog", "escape"),
    "return": ("normal", "oog", "escape"),
}


def cases(name, rec_cap=0):
    return memcases.sha3_cases(rec_cap) if name == "sha3" else memcases.CASES[name]()


def run_oracle(codes, batch: LaneBatch) -> LaneBatch:
    o = OracleEVM()
    ids = np.array([o.load_code(c) for c in codes], dtype=np.uint32)
    ref = batch.copy()
    ref.code_id[:] = ids[batch.code_id]
    o.run(ref)
    ref.code_id[:] = batch.code_id
    return ref


def outcome_classes(b: LaneBatch):
    """Per lane: "normal", "oog" or "escape"; anything else fails the test."""
    out = []
    for i in range(b.n):
        st, aux = int(b.status[i]), int(b.aux[i])
        if st == MG_VMEXC:
            assert aux == MG_EXC_OUT_OF_GAS, (i, aux)
            out.append("oog")
        elif st == MG_ESCAPE:
            assert aux >> 8 == MG_ESC_MEMORY, (i, aux)
            out.append("escape")
        else:
            assert st in (1, 2, 3), (i, st)
            out.append("normal")
    return out


def check_not_vacuous(name, b: LaneBatch):
    cls = outcome_classes(b)
    for c in CLASSES[name]:
        assert c in cls, f"{name}: no lane ends in {c}"
        # the class shares at least one wave with another class
        assert any(c in cls[w: w + 64] and len(set(cls[w: w + 64])) > 1 for w in range(0, b.n, 64)) \
            or len(CLASSES[name]) == 1, f"{name}: {c} never mixes with another class in a wave"
    return {c: cls.count(c) for c in ("normal", "oog", "escape")}


def check_model(name, out: LaneBatch, rec_cap=0):
    want = memcases.model_results(name, rec_cap)
    assert len(want) == out.n                     # the model answers for every lane
    bad = []
    for i, r in enumerate(want):
        bad += pymem.lane_diff(out, i, r)
        if len(bad) > 10:
            break
    assert bad == []


@pytest.mark.parametrize("name", sorted(memcases.CASES))
def test_oracle_equals_model(name):
    codes, b = cases(name)
    ref = run_oracle(codes, b)
    counts = check_not_vacuous(name, ref)
    print(f"{name}: {b.n} lanes, {counts}")
    check_model(name, ref)


@pytest.mark.parametrize("rec_cap", [0, 256])
def test_sha3_oracle_equals_model(rec_cap):
    codes, b = cases("sha3", rec_cap)
    ref = run_oracle(codes, b)
    counts = check_not_vacuous("sha3", ref)
    print(f"sha3 rec_cap={rec_cap}: {b.n} lanes, {counts}")
    check_model("sha3", ref, rec_cap)
    if rec_cap:
        recs = [r for i in range(b.n) for r in ref.records(i)]
        assert {len(r[2]) for r in recs} >= {ln for ln in memcases.SHA3_LENS if ln and ln < (1 << 32)}


def test_sha3_list_has_the_shapes_the_kernel_branches_on():
    """Multi-block inputs, unaligned inputs that straddle each memory window,
    and a wave whose second SHA3 can only hit the per-wave result cache."""
    codes, b = cases("sha3")
    ref = run_oracle(codes, b)
    want = memcases.model_results("sha3")
    hashed = []      # (lane, offset, length) of every SHA3 the model completed
    for i, r in enumerate(want):
        cd = bytes(b.calldata[i, :128])
        ops = [int.from_bytes(cd[32 * k: 32 * k + 32], "big") for k in range(4)]
        done = (r.pc > 4) + (r.pc > 9)
        hashed += [(i, ops[2 * k], ops[2 * k + 1]) for k in range(done)]
    assert any(ln > 136 for _, _, ln in hashed)
    assert any(ln == 136 for _, _, ln in hashed) and any(ln == 135 for _, _, ln in hashed)
    for w in memcases.WINDOWS[1:]:
        assert any(off % 4 and off < w < off + ln for _, off, ln in hashed), w
        assert any(off % 4 and off < w < off + ln and ln > 136 for _, off, ln in hashed), w
    # wave 0: 64 lanes, the same aligned 64 bytes twice, all run to STOP
    first = [(off, ln) for i, off, ln in hashed if i < 64]
    assert first == [(32, 64)] * 128
    assert len({bytes(b.memory[i, 32:96]) for i in range(64)}) == 1
    assert len({bytes(b.memory[i, 32:96]) for i in range(64, 128)}) == 2
    assert (ref.status[:64] == 1).all()
    # waves 2 and 3: a cacheable lane shares its SHA3 with other lengths and alignments
    for w in (2, 3):
        kinds = {(off % 4 == 0 and ln == 64) for i, off, ln in hashed if i // 64 == w}
        assert kinds == {True, False}


def test_gas_list_sits_on_the_edges():
    """Around every limit the model's outcome flips between out of gas and
    passing (or escaping), and the new sizes 32, 704, 736 and mem_cap occur."""
    codes, b = cases("gas")
    want = memcases.model_results("gas")
    sizes = {r.msize for r in want if r.outcome() == "normal"}
    assert {32, 704, 736, memcases.MEM_CAP} <= sizes
    # an extension past the page: out of gas below the need, the escape from it on
    esc = [i for i, r in enumerate(want) if r.outcome() == "escape"]
    assert esc
    by_proto = {}
    for i, r in enumerate(want):
        key = (int(b.code_id[i]), bytes(b.calldata[i, : int(b.calldata_len[i])]), int(b.msize[i]),
               tuple(b.stack_words(i)))
        by_proto.setdefault(key, []).append((int(b.gas_limit[i]), r))
    flips = 0
    for rows in by_proto.values():
        rows.sort(key=lambda t: t[0])
        assert len(rows) == 6
        target = [r.pc for _, r in rows]
        # two limits fail at the instruction under test, the others get past it or escape at it
        assert [r.outcome() for _, r in rows[:2]] == ["oog", "oog"], rows
        assert target[0] == target[1]
        assert all(r.outcome() == "escape" or r.pc > target[0] for _, r in rows[2:]), rows
        flips += 1
    assert flips > 100
