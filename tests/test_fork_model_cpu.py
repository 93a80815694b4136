"""mg_lanes_fork without a GPU: the interface's names, and the NumPy model of its
contract (tests/forkmodel.py) against jumpi_successors.

Symbolic calls into three reference contracts are stepped on the host to their
symbolic JUMPIs, packed, and parked there as MG_FORK by the oracle device; the
model forks them inside the device image (in place and into spare lanes), and
both children, decoded from the image, must be the states jumpi_successors makes
of the decoded parent -- stack, memory, storage, gas, depth, pc -- with the
constraint rebuilt from cond[] (symbolic.fork_conditions) equal to the one each
successor gained.
"""
import ctypes
import dataclasses
import re
from copy import copy

import numpy as np
import pytest

import forkmodel
import symcases
import symcosim
import symref
from mythril_amd import abi, device, lanes, native
from mythril_amd.lanes import (MG_FORK, MG_FORK_BAD_SRC, MG_FORK_MADE_FALL, MG_FORK_MADE_JUMP, MG_FORK_NONE,
                               MG_HALT_STOP, MG_RUNNING, LaneBatch)
from mythril_amd.laser import symbolic as sym
from oracle_device import OracleDevice

CONTRACTS = ("flag_array.sol.o", "symbolic_exec_bytecode.sol.o", "overflow.sol.o")


# ------------------------------------------------------------- the interface
def test_header_declares_the_fork_entry_and_its_constants():
    assert (abi.MG_FORK_NONE, abi.MG_FORK_MADE_FALL, abi.MG_FORK_MADE_JUMP, abi.MG_FORK_BAD_SRC) == \
        (0xFFFFFFFF, 1, 2, 0x80000000)
    for name in ("MG_FORK_NONE", "MG_FORK_MADE_FALL", "MG_FORK_MADE_JUMP", "MG_FORK_BAD_SRC"):
        assert getattr(lanes, name) is getattr(abi, name)
    text = abi.HEADER.read_text()
    assert re.search(r"\bint\s+mg_lanes_fork\s*\(\s*mg_ctx \*ctx,\s*const mg_fork_batch \*forks,", text)
    assert "instructions.py:1558-1636" in text
    assert abi.MG_ABI_VERSION == 15 and re.search(r"additive:[^*]*mg_lanes_fork", text)


def test_binding_has_the_fork_entry():
    res, args = native.SIGNATURES["mg_lanes_fork"]
    assert res is ctypes.c_int and len(args) == 5 and args[1] is ctypes.POINTER(native.MgForkBatch)
    # uint32 n, _pad, then three pointers
    assert ctypes.sizeof(native.MgForkBatch) == 8 + 3 * ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in native.MgForkBatch._fields_] == ["n", "_pad", "src", "dst_fall", "dst_jump"]
    assert hasattr(native.load(), "mg_lanes_fork")
    assert callable(device.GpuDevice.fork) and callable(sym.fork_conditions)


# ------------------------------------------------- the model vs jumpi_successors
def _at_symbolic_jumpi(s) -> bool:
    ins, pc, st = s.environment.code.instruction_list, s.mstate.pc, s.mstate.stack
    return pc < len(ins) and ins[pc]["opcode"] == "JUMPI" and len(st) >= 2 and \
        sym._concrete_value(st[-1]) is not None and sym._concrete_value(st[-2]) is None


def fork_parents(s0, eng, limit: int, budget: int = 4000) -> list:
    """States of the call at JUMPIs on symbolic conditions, breadth first (the
    restatement steps the host side of the exploration)."""
    out, queue = [], [s0]
    while queue and len(out) < limit and budget > 0:
        s = queue.pop(0)
        while budget > 0:
            budget -= 1
            try:
                succ = eng.step(s)
            except symref.Unsupported:
                break
            if _at_symbolic_jumpi(s):
                if sym.lane_eligible(s):
                    out.append(s)
                queue.extend(succ)
                break
            if len(succ) != 1:
                queue.extend(succ)
                break
            s = succ[0]
    return out


def _raws(cs) -> list:
    return [c.raw for c in cs]


@pytest.mark.parametrize("name", CONTRACTS)
def test_model_children_are_jumpi_successors(name):
    dev = OracleDevice()
    ws, addr = symcases.deploy(dev, name)
    parents = fork_parents(symcosim.initial(ws, addr), symref.Engine(), limit=6)
    k = len(parents)
    assert k >= 3, (name, k)
    vm = symcosim.new_vm(dev)
    shape = dataclasses.replace(vm._shape(parents), n=3 * k)
    b = LaneBatch(shape)
    for i, s in enumerate(parents):
        vm._pack(b, i, s)
        b.steps[i] = 0
    b.code_id[k:] = b.code_id[0]
    b.status[k:] = MG_HALT_STOP
    dev.alloc(shape)
    dev.upload(b)
    dev.step()
    dev.download(b)
    assert (b.status[:k] == MG_FORK).all(), b.status[:k]
    # in place and two-destination forms alternate; spare lanes k .. 3k
    src = np.arange(k, dtype=np.uint32)
    dst_fall = np.array([i if i % 2 == 0 else k + 2 * i for i in range(k)], dtype=np.uint32)
    dst_jump = np.array([k + 2 * i + 1 for i in range(k)], dtype=np.uint32)
    codes = {int(b.code_id[i]): forkmodel.CodeTable(s.environment.code.raw) for i, s in enumerate(parents)}
    made, cond = forkmodel.fork(dev._model(), codes, src, dst_fall, dst_jump)
    after = LaneBatch(shape)
    dev.download(after)
    assert not (made & MG_FORK_BAD_SRC).any() and (cond > 0).all()
    checked = 0
    for i, s0 in enumerate(parents):
        parent = vm._materialise(b, i, copy(s0))
        symcosim._replay(b, i, parent)
        want = iter(sym.jumpi_successors(parent))
        negated, condi = sym.fork_conditions(b, i, parent, int(cond[i]))
        for bit, lane, c in ((MG_FORK_MADE_FALL, int(dst_fall[i]), negated), (MG_FORK_MADE_JUMP, int(dst_jump[i]), condi)):
            if not made[i] & bit:
                assert bit == MG_FORK_MADE_JUMP          # only an invalid target makes no lane
                continue
            if c.is_false:
                continue                                  # jumpi_successors drops it: the condition folded
            ref = next(want)
            assert int(after.status[lane]) == MG_RUNNING and int(after.steps[lane]) == 1
            child = vm._materialise(after, lane, copy(s0))
            symcosim._replay(after, lane, child)
            symcosim.assert_same_state(child, ref, (name, i, bit))
            # the same node in the child's copied arena gives the same constraint
            mine = sym.fork_conditions(after, lane, child, int(cond[i]))[0 if bit == MG_FORK_MADE_FALL else 1]
            assert mine.raw == c.raw
            gained = [] if c.value is True else [mine]
            assert _raws(list(child.world_state.constraints) + gained) == _raws(ref.world_state.constraints)
            assert _raws(ref.world_state.constraints)[:len(parent.world_state.constraints)] == \
                _raws(parent.world_state.constraints)
            checked += 1
        assert next(want, None) is None, (name, i, "jumpi_successors made a state the model did not")
    assert checked >= k


def test_model_refuses_what_is_not_a_fork_source():
    """Not MG_FORK, taint, a symbolic target, sp 1: MG_FORK_BAD_SRC and nothing written."""
    from mythril_amd.lanes import MG_LANE_SYMBOLIC, MG_LANE_TAINT, LaneShape
    from xfermodel import DeviceImage, saturated, whole_diff
    shape = LaneShape(n=9, stack_cap=4, mem_cap=32, calldata_cap=4, storage_cap=1, node_cap=2, const_cap=1)
    model = DeviceImage(shape)
    img = saturated(shape, np.random.default_rng(5), 0)
    img.pc[:4] = 2
    img.sp[:4] = 3
    img.status[:4] = MG_FORK
    img.flags[:4] = MG_LANE_SYMBOLIC
    img.stack[:4, 2] = 0
    img.stag[:4, 2] = 0
    img.stag[:4, 1] = 1
    img.status[0] = MG_HALT_STOP
    img.flags[1] |= MG_LANE_TAINT
    img.stag[2, 2] = 2
    img.sp[3] = 1
    model.upload(img, 0, 9)
    before = model.img.copy()
    codes = {0: forkmodel.CodeTable(bytes.fromhex("5b600057"))}
    made, cond = forkmodel.fork(model, codes, [0, 1, 2, 3], [4, 5, 6, 8],
                                 [MG_FORK_NONE, MG_FORK_NONE, 7, MG_FORK_NONE])
    assert made.tolist() == [MG_FORK_BAD_SRC] * 4 and cond.tolist() == [0] * 4
    assert whole_diff(model.img, before) == []
