"""mg_explore without a GPU: the interface's names, the NumPy model of its plan
and path record (tests/exploremodel.py) against hand-worked cases, and the
model's rounds against jumpi_successors applied level by level.

The oracle device has no symbolic stepper, so a level here is what one
mg_explore call of one round is: the restatement (tests/symref.py) steps every
live state to its symbolic JUMPI, the states are packed and parked there as
MG_FORK, the model plans and forks the image, and every successor lane, decoded
with the constraints symbolic.path_constraints reads from its path row, must be
the state jumpi_successors makes of its parent; lanes whose path decodes to None
are the successors the reference never makes.
"""
import ctypes
import dataclasses
import re
from copy import copy

import numpy as np
import pytest

import exploremodel
import forkmodel
import symcases
import symcosim
import symref
from mythril_amd import abi, device, native
from mythril_amd.lanes import (MG_FORK, MG_FORK_NONE, MG_HALT_STOP, MG_LANE_SYMBOLIC, MG_LANE_TAINT, MG_RUNNING,
                               LaneBatch, LaneShape, word_to_limbs)
from mythril_amd.laser import symbolic as sym
from oracle_device import OracleDevice
from test_fork_model_cpu import _at_symbolic_jumpi
from xfermodel import DeviceImage, saturated, whole_diff

NONE = MG_FORK_NONE


# ------------------------------------------------------------- the interface
def test_header_and_binding_have_the_explorer():
    text = abi.HEADER.read_text()
    for fn in ("mg_explore_alloc", "mg_explore", "mg_explore_download"):
        assert re.search(r"\bint\s+%s\s*\(\s*mg_ctx \*ctx," % fn, text), fn
        assert hasattr(native.load(), fn)
    assert "svm.py:293-337" in text and "instructions.py:1558-1636" in text
    assert abi.MG_ABI_VERSION == 15 and re.search(r"additive:[^*]*mg_explore", text)
    res, args = native.SIGNATURES["mg_explore"]
    assert res is ctypes.c_int and len(args) == 8 and args[7] is ctypes.POINTER(native.MgExploreStats)
    # eight uint32, a uint64, two floats
    assert ctypes.sizeof(native.MgExploreStats) == 8 * 4 + 8 + 2 * 4
    assert [f[0] for f in native.MgExploreStats._fields_] == [
        "rounds", "forks", "made_jump", "starved", "path_full", "free_used", "running", "_pad", "lane_steps",
        "kernel_ms", "_padf"]
    for m in ("explore_alloc", "explore", "explore_paths"):
        assert callable(getattr(device.GpuDevice, m))
    assert callable(sym.path_constraints)


# ------------------------------------------------------ the plan, by hand
# index: address  instruction
#  0: 0 JUMPDEST   1: 1 PUSH1 00   2: 3 JUMPI   3: 4 STOP   4: 5 JUMPDEST   5: 6 STOP
CODE = bytes.fromhex("5b" "6000" "57" "00" "5b" "00")
T_VALID, T_INVALID = 5, 4
SHAPE = LaneShape(n=16, stack_cap=4, mem_cap=32, calldata_cap=4, storage_cap=1, node_cap=3, const_cap=1)


def _image(sources, flags=None, sym_target=()):
    """A saturated image with fork sources at `sources`: {lane: jump target}."""
    img = saturated(SHAPE, np.random.default_rng(11), 0)
    for s, target in sources.items():
        img.status[s], img.aux[s], img.pc[s], img.sp[s] = MG_FORK, 0x57, 2, 3
        img.flags[s] = (flags or {}).get(s, MG_LANE_SYMBOLIC)
        img.stack[s, 2] = word_to_limbs(target)
        img.stag[s, 2] = 1 if s in sym_target else 0
        img.stag[s, 1] = 1 + s % 3
        img.n_nodes[s] = 3
        img.gas_min[s] &= np.uint64((1 << 40) - 1)
        img.gas_max[s] &= np.uint64((1 << 40) - 1)
    model = DeviceImage(SHAPE)
    model.upload(img, 0, SHAPE.n)
    return model


CODES = {0: forkmodel.CodeTable(CODE)}


def _plan(model, free, used=0, path_len=None, path_cap=4):
    pl = np.zeros(SHAPE.n, dtype=np.uint32) if path_len is None else path_len
    return [x.tolist() for x in exploremodel.plan(model.img, CODES, free, used, pl, path_cap)]


def test_plan_assigns_free_lanes_in_ascending_order():
    model = _image({2: T_VALID, 5: T_VALID, 9: T_VALID})
    # the free lanes lie between and above the sources: source r takes entry r whatever its lane
    assert _plan(model, [1, 7, 12, 13]) == [[2, 5, 9], [2, 5, 9], [1, 7, 12], [], []]
    # the entries earlier rounds used are skipped
    assert _plan(model, [0, 1, 7, 12, 13], used=1) == [[2, 5, 9], [2, 5, 9], [1, 7, 12], [], []]
    # a lane in the unused part of the free list is no source; a used entry is a lane like any other
    assert _plan(model, [1, 5, 12, 13])[:3] == [[2, 9], [2, 9], [1, 5]]
    src, fall, jump, starved, full = _plan(model, [5, 12, 13], used=1)
    assert (src, jump, starved) == ([2, 5], [12, 13], [9])


def test_plan_invalid_target_takes_no_free_lane():
    model = _image({2: T_VALID, 5: T_INVALID, 9: T_VALID})
    assert _plan(model, [12, 13, 14]) == [[2, 5, 9], [2, 5, 9], [12, NONE, 13], [], []]


def test_plan_shortfall_starves_the_highest_lanes_and_leaves_them():
    model = _image({2: T_VALID, 5: T_INVALID, 9: T_VALID, 10: T_VALID})
    src, fall, jump, starved, full = _plan(model, [12])
    assert (src, fall, jump, starved, full) == ([2, 5], [2, 5], [12, NONE], [9, 10], [])
    before = model.img.copy()
    paths = exploremodel.Paths(SHAPE.n, 4)
    (p_src, _, p_jump, p_starved, _), used = exploremodel.round_(model, CODES, [12], 0, paths)
    assert used == 1 and p_starved.tolist() == [9, 10]
    untouched = [l for l in range(SHAPE.n) if l not in (2, 5, 12)]
    assert whole_diff(model.img, before, lanes=untouched) == []
    assert whole_diff(model.img, before, lanes=[2, 5, 12]) != []
    assert model.img.status[[2, 5, 12]].tolist() == [MG_RUNNING] * 3
    assert model.img.status[[9, 10]].tolist() == [MG_FORK] * 2
    assert paths.path_len.tolist() == [1 if l in (2, 5, 12) else 0 for l in range(SHAPE.n)]
    assert paths.root[12] == 2 and paths.path[12, 0] == (1 + 2 % 3) << 1 | 1 and paths.path[2, 0] == (1 + 2 % 3) << 1
    assert paths.path[5, 0] == (1 + 5 % 3) << 1


def test_plan_path_full_and_empty_free_list():
    model = _image({2: T_VALID, 5: T_INVALID, 9: T_VALID})
    pl = np.zeros(SHAPE.n, dtype=np.uint32)
    pl[2] = 4
    pl[5] = 4
    assert _plan(model, [12, 13], path_len=pl) == [[9], [9], [12], [], [2, 5]]
    # no free lane: every fork with a valid target is starved, the in-place one is made
    assert _plan(model, []) == [[5], [5], [NONE], [2, 9], []]
    # a full path comes before starvation: it is counted once, as path_full
    assert _plan(model, [], path_len=pl) == [[], [], [], [9], [2, 5]]


def test_plan_skips_taint_and_symbolic_target_lanes():
    model = _image({2: T_VALID, 5: T_VALID, 6: T_VALID, 9: T_VALID},
                   flags={5: MG_LANE_SYMBOLIC | MG_LANE_TAINT}, sym_target=(6,))
    assert _plan(model, [12, 13]) == [[2, 9], [2, 9], [12, 13], [], []]


def test_commit_paths_copies_the_row_then_appends():
    paths = exploremodel.Paths(8, 3)
    paths.path[1, :2] = (0x10, 0x21)
    paths.path_len[1] = 2
    paths.root[1] = 6
    paths.path[4] = 0xEE                        # a free lane's stale row
    exploremodel.commit_paths(paths, [1, 2], [4, NONE], [3, 1], [7, 9])
    assert paths.path[4].tolist() == [0x10, 0x21, 7 << 1 | 1] and paths.path[1].tolist() == [0x10, 0x21, 7 << 1]
    assert paths.path_len[[1, 4, 2]].tolist() == [3, 3, 1] and paths.root[[1, 4, 2]].tolist() == [6, 6, 2]
    assert paths.path[2].tolist() == [9 << 1, 0, 0]


# ------------------------------------------- rounds against jumpi_successors
CONTRACTS = ("flag_array.sol.o", "symbolic_exec_bytecode.sol.o", "overflow.sol.o")
LEVELS, WIDTH = 3, 6


def _to_jumpi(s, eng, budget=2000):
    """`s` stepped by the restatement to its next symbolic JUMPI, or None when the
    path ends, forks elsewhere or leaves what a lane carries before one."""
    for _ in range(budget):
        if _at_symbolic_jumpi(s):
            return s if sym.lane_eligible(s) else None
        try:
            succ = eng.step(s)
        except symref.Unsupported:
            return None
        if len(succ) != 1:
            return None
        s = succ[0]
    return None


def _key(s):
    return (s.mstate.pc, s.mstate.depth, s.mstate.min_gas_used, s.mstate.max_gas_used,
            tuple(c.raw for c in s.world_state.constraints))


@pytest.mark.parametrize("name", CONTRACTS)
def test_model_rounds_are_jumpi_successors_level_by_level(name):
    dev = OracleDevice()
    ws, addr = symcases.deploy(dev, name)
    eng = symref.Engine()
    vm = symcosim.new_vm(dev)
    level = [symcosim.initial(ws, addr)]
    forks = dropped = 0
    for depth in range(LEVELS):
        parents = [p for p in (_to_jumpi(s, eng) for s in level) if p is not None][:WIDTH]
        if not parents:
            break
        k = len(parents)
        shape = dataclasses.replace(vm._shape(parents), n=2 * k + 1)
        b = LaneBatch(shape)
        # parents in the odd lanes 1, 3, ..., free lanes between them: 0, 2, ...
        lanes = [2 * i + 1 for i in range(k)]
        b.code_id[:] = 0
        b.status[:] = MG_HALT_STOP
        for lane, s in zip(lanes, parents):
            vm._pack(b, lane, s)
            b.steps[lane] = 0
        b.code_id[:] = b.code_id[1]
        dev.alloc(shape)
        dev.upload(b)
        dev.step()
        dev.download(b)
        assert (b.status[lanes] == MG_FORK).all(), b.status
        codes = {int(b.code_id[1]): forkmodel.CodeTable(parents[0].environment.code.raw)}
        free = list(range(0, 2 * k + 1, 2))
        paths = exploremodel.Paths(shape.n, 16)
        (src, _, dst_jump, starved, full), used = exploremodel.round_(dev._model(), codes, free, 0, paths)
        assert src.tolist() == lanes and starved.size == 0 and full.size == 0
        after = LaneBatch(shape)
        dev.download(after)
        got, want = [], []
        for i, (lane, s0) in enumerate(zip(lanes, parents)):
            parent = vm._materialise(b, lane, copy(s0))
            symcosim._replay(b, lane, parent)
            want += sym.jumpi_successors(parent)
            forks += 1
            for child_lane in [lane] + ([int(dst_jump[i])] if dst_jump[i] != NONE else []):
                assert int(paths.root[child_lane]) == lane and int(paths.path_len[child_lane]) == 1
                child = vm._materialise(after, child_lane, copy(s0))
                symcosim._replay(after, child_lane, child)
                gained = sym.path_constraints(after, child_lane, child, paths.path[child_lane, :1])
                if gained is None:
                    dropped += 1
                    continue
                for c in gained:
                    child.world_state.constraints.append(c)
                got.append(child)
        assert sorted(map(_key, got)) == sorted(map(_key, want)), (name, depth)
        by_key = {_key(s): s for s in want}
        for child in got:
            symcosim.assert_same_state(child, by_key[_key(child)], (name, depth))
        level = got
    assert forks >= 3, (name, forks)
    print(f"{name}: {forks} forks over the levels, {dropped} successors the reference never makes")


def test_path_constraints_decodes_every_entry_from_one_arena():
    """A row of several entries over one lane's arena: each entry gives what
    fork_conditions gives for its node and side, in order; a False one gives None."""
    dev = OracleDevice()
    ws, addr = symcases.deploy(dev, "overflow.sol.o")
    parent = _to_jumpi(symcosim.initial(ws, addr), symref.Engine())
    vm = symcosim.new_vm(dev)
    b = symcosim.pack(vm, [parent])
    n_nodes = int(b.n_nodes[0])
    assert n_nodes >= 1
    state = vm._materialise(b, 0, copy(parent))
    row, want = [], []
    for k in range(min(n_nodes, 4)):
        side = k & 1
        negated, condi = sym.fork_conditions(b, 0, state, k + 1)
        c = condi if side else negated
        if c.is_false:
            continue
        row.append((k + 1) << 1 | side)
        if c.value is not True:
            want.append(c.raw)
    assert row
    got = sym.path_constraints(b, 0, state, np.array(row, dtype=np.uint32))
    assert [c.raw for c in got] == want
    assert sym.path_constraints(b, 0, state, []) == []
