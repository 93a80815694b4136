"""mg_explore on an MI355X: the step-and-fork loop on the device (lane_explore.cuh).
The oracle is the merged fork itself (GpuDevice.fork) plus the NumPy model of the
plan and the path record (tests/exploremodel.py).

a. one round equals dev.step() + a full download + exploremodel.plan + dev.fork on
   a second upload of the same batch, bit for bit, at shapes where the ranking can
   go wrong: three blocks, sources on the wave and block edges, a dense run over a
   block edge, free lanes between and above the sources, an invalid target, a
   taint lane and a symbolic-target lane inside the run, and a free list that is
   exact, one short and empty; at 64 and 32 lanes per wave of kernel 1; and with
   the scan blocks capped at 1 and 2, so that the ranks cross the carry over a
   block's tiles and the block offsets;
b. R rounds in one call equal R calls of one round, each given the unused tail of
   the free list: the image, the paths (composed through root) and the summed stats;
c. co-simulation against the CPU restatement (tests/symref.py), both sides
   exploring exactly R rounds, and a starvation run;
d. path_cap = 1: second-level forks are refused with path_full, their lanes untouched;
e. refusals: every host-side check, with the image unchanged.
"""
import ctypes
import dataclasses
from collections import Counter
from copy import copy

import numpy as np
import pytest

import exploremodel
import forkmodel
import symcases
import symcosim
import symref
from mythril_amd import abi, native
from mythril_amd.device import GpuDevice
from mythril_amd.lanes import (MG_EINVAL, MG_ESCAPE, MG_ESTATE, MG_FORK, MG_FORK_NONE, MG_HALT_DROPPED, MG_HALT_END,
                               MG_HALT_RETURN, MG_HALT_REVERT, MG_HALT_STOP, MG_LANE_SYMBOLIC, MG_LANE_TAINT,
                               MG_RUNNING, MG_VMEXC, LaneBatch)
from mythril_amd.laser import symbolic as sym
from test_gpu_fork import CODE, J_MID, J_NFENT, J_PLAIN, SHAPE, T_DATA, T_DEST, T_ENTRY, T_STOP, _full, make_source
from xfermodel import saturated, whole_diff

pytestmark = pytest.mark.gpu

NONE = MG_FORK_NONE
PATH_CAP = 16


@pytest.fixture(scope="module", params=[64, 32], ids=["lpw64", "lpw32"])
def dev_lpw(request):
    """A context at each kernel-1 wave geometry (MG_LANES_PER_WAVE is read by mg_open)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("MG_LANES_PER_WAVE", str(request.param))
    d = GpuDevice(0)
    mp.undo()
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def _paths(dev, n):
    path, path_len, root = dev.explore_paths(0, n)
    return path, path_len, root


def _same_paths(got, want: exploremodel.Paths):
    path, path_len, root = got
    assert path_len.tolist() == want.path_len.tolist()
    assert root.tolist() == want.root.tolist()
    for l in range(root.size):
        k = int(path_len[l])
        assert path[l, :k].tolist() == want.path[l, :k].tolist(), l
        assert not path[l, k:].any(), l


# ------------------------------------------------ a. one round, hand-made sources
# sources on the edges of waves (63 | 64) and of the plan's blocks (255 | 256, 511 | 512), the
# first and the last lane of the live range, and a dense run across the first block edge
EDGES = (0, 63, 64, 255, 256, 511, 512, 599)
DENSE = tuple(range(250, 261))
SOURCES = tuple(sorted(set(EDGES) | set(DENSE)))
INVALID, TAINT, SYMTARGET = 254, 252, 258          # inside the dense run
VALID = tuple(s for s in SOURCES if s not in (INVALID, TAINT, SYMTARGET))
NEED = len(VALID)


def _layout(layout):
    """(number of lanes, free lanes with at least NEED entries)."""
    if layout == "between":
        # below, between and next to the sources, on both sides of every edge
        free = [1, 2, 62, 65, 66, 200, 249, 261, 262, 300, 400, 510, 513, 514, 550, 597, 598]
        return 600, free
    return 700, list(range(601, 700, 3))           # every free lane above every source


def _hand_image(n, cid, rng):
    shape = dataclasses.replace(SHAPE, n=n)
    host = saturated(shape, rng, cid)
    targets = (T_ENTRY, T_DEST, T_DATA)
    for k, s in enumerate(SOURCES):
        pc = (J_PLAIN, J_MID, J_NFENT)[k % 3]
        make_source(host, s, k, pc, T_STOP if s == INVALID else targets[k % 3],
                    MG_LANE_SYMBOLIC | (MG_LANE_TAINT if s == TAINT else 0))
        if k % 3 == 1 and s not in (TAINT, SYMTARGET):
            host.status[s], host.aux[s] = MG_RUNNING, 0          # the round's own step parks it at the JUMPI
    host.stag[SYMTARGET, int(host.sp[SYMTARGET]) - 1] = 1
    return shape, host


@pytest.mark.parametrize("short", [0, 1, None], ids=["exact", "one-short", "no-free-lane"])
@pytest.mark.parametrize("layout", ["between", "above"])
def test_one_round_equals_step_plus_planned_fork(dev_lpw, layout, short):
    _one_round(dev_lpw, layout, short)


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one-short"])
@pytest.mark.parametrize("blocks", ["1", "2"], ids=["blocks1", "blocks2"])
def test_one_round_across_the_tile_carry_and_the_block_offsets(dev, monkeypatch, blocks, short):
    """The same round with the plan's scan blocks capped (MG_EXPLORE_BLOCKS, read per
    call): the 600 lanes are three tiles, the last partial.  With 1 a single block owns
    all three and both ranked classes carry over its tile edges (the in-place source is
    lane 254, the dense run 250-260 straddles the first edge); with 2 there are a
    two-tile and a one-tile block, so the carry and the block offsets work together.
    The model's plan knows nothing of blocks."""
    monkeypatch.setenv("MG_EXPLORE_BLOCKS", blocks)
    _one_round(dev, "between", short, f"MG_EXPLORE_BLOCKS={blocks}, ")


def _one_round(dev, layout, short, note=""):
    n, free = _layout(layout)
    assert len(free) >= NEED and NEED == 14
    free = [] if short is None else free[:NEED - short]
    cid = dev.load_code(CODE)
    table = {cid: forkmodel.CodeTable(CODE)}
    shape, host = _hand_image(n, cid, np.random.default_rng(0xE1))
    # left: the explorer
    dev.alloc(shape, coverage=True)
    dev.explore_alloc(PATH_CAP)
    dev.coverage_clear()
    dev.upload(host)
    st = dev.explore(free, max_rounds=1)
    left, left_paths, left_cov = _full(dev, shape), _paths(dev, n), dev.coverage(cid)
    # right: step, download, the model's plan, the merged fork
    dev.alloc(shape, coverage=True)
    dev.coverage_clear()
    dev.upload(host)
    stepped = dev.step()
    img = _full(dev, shape)
    assert (img.status[list(SOURCES)] == MG_FORK).all(), img.status[list(SOURCES)]
    paths = exploremodel.Paths(n, PATH_CAP)
    src, dst_fall, dst_jump, starved, full = exploremodel.plan(img, table, free, 0, paths.path_len, PATH_CAP)
    made, cond, _ = dev.fork(src, dst_fall, dst_jump)
    exploremodel.commit_paths(paths, src, dst_jump, made, cond)
    right = _full(dev, shape)
    # the model's plan is the hand-worked one
    n_jump = min(len(free), NEED)
    assert src.tolist() == sorted(list(VALID[:n_jump]) + [INVALID])
    assert dst_jump[src != INVALID].tolist() == free[:n_jump] and starved.tolist() == list(VALID[n_jump:])
    assert int(dst_jump[src.tolist().index(INVALID)]) == NONE and full.size == 0
    assert made.tolist() == [1 if s == INVALID else 3 for s in src]
    # every plane and scalar, the paths, the coverage, the stats
    assert whole_diff(left, right) == []
    _same_paths(left_paths, paths)
    assert left_cov.tolist() == dev.coverage(cid).tolist()
    assert (st.rounds, st.forks, st.made_jump, st.free_used, st.starved, st.path_full) == \
        (1, len(src), n_jump, n_jump, NEED - n_jump, 0)
    assert st.lane_steps == stepped.lane_steps and st.running == stepped.running + len(src) + n_jump
    # the starved, the taint and the symbolic-target lanes are as the step left them
    still = list(starved) + [TAINT, SYMTARGET]
    assert whole_diff(left, img, lanes=still) == [] and (left.status[still] == MG_FORK).all()
    print(f"{note}{layout}, {len(free)} free: {st.forks} forks, {st.made_jump} jump lanes, {st.starved} starved, "
          f"kernel_ms {st.kernel_ms:.4f}")


# ------------------------------------------------------- real states: a root and spare lanes
SPARE_LANES = 383


def _root_image(dev, name, spare=SPARE_LANES, roots=(0,)):
    """The symbolic call into `name` packed into the lanes `roots` of a batch of
    1 + spare lanes, the others halted and free.  A root the device hands to the
    host at once (memjump: a jump target read from memory at a symbolic offset)
    is stepped over by the host first, as LaserEVM's escape handler would."""
    ws, addr = symcases.deploy(dev, name)
    vm = symcosim.new_vm(dev)
    eng = symref.Engine()
    root = symcosim.initial(ws, addr)
    if name == "memjump":
        lanes, _ = symcosim.cosimulate(dev, [root], vm=vm, eng=eng, name=name)
        assert lanes[0].status == MG_ESCAPE
        root = [t for t in eng.step(lanes[0].state) if sym.lane_eligible(t)][0]
    shape = dataclasses.replace(vm._shape([root]), n=1 + spare)
    b = LaneBatch(shape)
    b.status[:] = MG_HALT_STOP
    for lane in roots:
        vm._pack(b, lane, root)
        b.steps[lane] = 0
    b.code_id[:] = b.code_id[roots[0]]
    free = [l for l in range(shape.n) if l not in roots]
    return vm, eng, root, shape, b, free


def _upload_known(dev, shape, b):
    """Upload `b` over an image whose every cell is known (an upload moves only rows
    below the batch's largest counts; what lies above them is compared too)."""
    dev.upload(saturated(shape, np.random.default_rng(0xE2), int(b.code_id[0])))
    dev.upload(b)


def _compose(total: exploremodel.Paths, call) -> exploremodel.Paths:
    """The paths after one more mg_explore call (which restarts root and path_len):
    lane l continues the path its root lane had before the call."""
    path, path_len, root = call
    out = exploremodel.Paths(root.size, total.path_cap)
    for l in range(root.size):
        r, k = int(root[l]), int(path_len[l])
        base = int(total.path_len[r])
        out.path[l, :base] = total.path[r, :base]
        out.path[l, base:base + k] = path[l, :k]
        out.path_len[l] = base + k
        out.root[l] = total.root[r]
    return out


ROUNDS = 4


@pytest.mark.parametrize("name", ["exceptions.sol.o", "overflow.sol.o"])
def test_r_rounds_equal_r_single_rounds(dev, name):
    roots = (0, 70, 300)                       # the same call in three blocks' worth of places
    vm, eng, root, shape, b, free = _root_image(dev, name, roots=roots)
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    _upload_known(dev, shape, b)
    st = dev.explore(free, max_rounds=ROUNDS)
    left, left_paths = _full(dev, shape), _paths(dev, shape.n)
    assert st.rounds == ROUNDS and st.forks >= 3 * 3 and st.starved == 0 and st.path_full == 0
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    _upload_known(dev, shape, b)
    total = exploremodel.Paths(shape.n, PATH_CAP)
    used, sums = 0, Counter()
    for _ in range(ROUNDS):
        one = dev.explore(free[used:], max_rounds=1)
        assert one.rounds == 1
        total = _compose(total, _paths(dev, shape.n))
        used += one.free_used
        for f in ("rounds", "forks", "made_jump", "starved", "path_full", "free_used", "lane_steps"):
            sums[f] += getattr(one, f)
    assert whole_diff(left, _full(dev, shape)) == []
    _same_paths(left_paths, total)
    assert {f: getattr(st, f) for f in sums} == dict(sums) and st.running == one.running
    lineage = left_paths[2]
    assert set(lineage[free[:used]].tolist()) <= set(roots) and lineage[free[used:]].tolist() == free[used:]
    print(f"{name}: {st.forks} forks in {ROUNDS} rounds from {len(roots)} roots, {st.free_used} free lanes used, "
          f"kernel_ms {st.kernel_ms:.3f}")


# ------------------------------------------------ c. co-simulation with the restatement
HALTS = {"stop": MG_HALT_STOP, "return": MG_HALT_RETURN, "revert": MG_HALT_REVERT, "exception": MG_VMEXC,
         "end": MG_HALT_END, "dropped": MG_HALT_DROPPED}
# R per case: the smallest number of rounds at which some path of the restatement has
# forked at least twice and then halted (found on the CPU with restatement_rounds; at most 10)
R = {"flag_array.sol.o": 3, "symbolic_exec_bytecode.sol.o": 3, "overflow.sol.o": 4, "exceptions.sol.o": 4,
     "memjump": 3}


def restatement_rounds(eng, root, rounds: int):
    """The restatement explores `rounds` rounds from `root`: in each, every live
    state is stepped to its stop and, at a JUMPI on a symbolic condition, forked
    with eng.step (no filter).  Returns (stopped, live, forks): stopped = [(kind,
    state at the start of the instruction that stopped it, steps, path forks)],
    live = the successors of the last round's forks."""
    live, stopped, forks = [(root, 0, 0)], [], 0
    for _ in range(rounds):
        nxt = []
        for s, steps, nf in live:
            while True:
                before = len(eng.ended)
                at_fork = _at_symbolic_jumpi(s)
                succ = eng.step(s)
                if at_fork:
                    forks += 1
                    nxt.extend((t, steps + 1, nf + 1) for t in succ)
                    break
                if not succ:
                    kind = eng.ended[-1][0] if len(eng.ended) > before else "dropped"
                    # a halt or an exception counts as a step; running off the code's end does not
                    stopped.append((kind, s, steps + (0 if kind == "end" else 1), nf))
                    break
                assert len(succ) == 1
                s, steps = succ[0], steps + 1
        live = nxt
    return stopped, live, forks


def _at_symbolic_jumpi(s) -> bool:
    ins, pc, st = s.environment.code.instruction_list, s.mstate.pc, s.mstate.stack
    return pc < len(ins) and ins[pc]["opcode"] == "JUMPI" and len(st) >= 2 and \
        sym._concrete_value(st[-1]) is not None and sym._concrete_value(st[-2]) is None


def _exception_aux(s) -> int:
    """MG_EXC_* of the exception the restatement raised at state `s`, from the instruction it stands at."""
    name = s.environment.code.instruction_list[s.mstate.pc]["opcode"]
    if name in ("INVALID", "ASSERT_FAIL"):
        return abi.MG_EXC_INVALID_INSTRUCTION
    if name in ("JUMP", "JUMPI"):
        return abi.MG_EXC_INVALID_JUMP
    raise AssertionError(f"an exception at {name}: this test does not know its MG_EXC_* code")


def _state_key(status, aux, s, steps):
    return (status, aux, s.mstate.pc, s.mstate.depth, s.mstate.min_gas_used, s.mstate.max_gas_used, steps,
            tuple(c.raw for c in s.world_state.constraints))


def _device_lanes(vm, b, paths, root, lanes):
    """[(lane, status, aux, the materialised state with its path's constraints)] of
    the lanes whose path the reference makes too."""
    path, path_len, _ = paths
    out = []
    for lane in lanes:
        s = vm._materialise(b, lane, copy(root))
        symcosim._replay(b, lane, s)
        gained = sym.path_constraints(b, lane, s, path[lane, :int(path_len[lane])])
        if gained is None:
            continue
        for c in gained:
            s.world_state.constraints.append(c)
        out.append((lane, int(b.status[lane]), int(b.aux[lane]), s))
    return out


def _check_against_restatement(name, vm, b, paths, root, lanes, stopped, live):
    got = _device_lanes(vm, b, paths, root, lanes)
    # aux: the exception's code for MG_VMEXC; a halt and a running lane carry 0
    want = [(_state_key(HALTS[kind], _exception_aux(s) if kind == "exception" else 0, s, steps), s)
            for kind, s, steps, _ in stopped] + [(_state_key(MG_RUNNING, 0, s, steps), s) for s, steps, _ in live]
    mine = [(_state_key(status, aux, s, int(b.steps[lane])), s, status, aux) for lane, status, aux, s in got]
    assert Counter(k for k, *_ in mine) == Counter(k for k, _ in want), name
    by_key = {}
    for k, s in want:
        by_key.setdefault(k, []).append(s)
    for k, s, status, aux in mine:
        if status in HALTS.values():
            assert any(_same(s, t, name) for t in by_key[k]), (name, k[:7])
    return got


def _same(got, ref, name) -> bool:
    try:
        symcosim.assert_same_state(got, ref, name)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("name", sorted(R))
def test_cosimulation_explores_r_rounds_like_the_restatement(dev, name):
    vm, eng, root, shape, b, free = _root_image(dev, name)
    stopped, live, forks = restatement_rounds(symref.Engine(), root, R[name])
    # what the reference alone must meet at this R
    assert forks >= (2 if name == "memjump" else 3), (name, forks)
    assert any(nf >= 2 and kind in HALTS for kind, _, _, nf in stopped), (name, "no path forked twice and halted")
    assert forks <= SPARE_LANES and max(nf for _, _, nf in live + [(0, 0, 0)]) <= PATH_CAP   # starved == path_full == 0
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    _upload_known(dev, shape, b)
    st = dev.explore(free, max_rounds=R[name])
    assert (st.rounds, st.starved, st.path_full) == (R[name], 0, 0)
    out = LaneBatch(shape)
    dev.download(out)
    paths = _paths(dev, shape.n)
    lanes = [0] + free[:st.free_used]
    assert (paths[2][lanes] == 0).all()
    got = _check_against_restatement(name, vm, out, paths, root, lanes, stopped, live)
    print(f"{name}: R = {R[name]}, {st.forks} device forks ({forks} in the restatement), {len(got)} of "
          f"{len(lanes)} lanes on paths the reference makes")


def test_starvation_leaves_lanes_for_the_host_route(dev):
    name, spare = "exceptions.sol.o", 5
    vm, eng, root, shape, b, free = _root_image(dev, name, spare=spare)
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    _upload_known(dev, shape, b)
    total, used, starved_lanes, st = exploremodel.Paths(shape.n, PATH_CAP), 0, [], None
    for _ in range(10):
        # round by round, so that the image a plain step leaves is at hand
        before = _full(dev, shape)
        st = dev.explore(free[used:], max_rounds=1)
        total = _compose(total, _paths(dev, shape.n))
        used += st.free_used
        if st.starved:
            after = _full(dev, shape)
            # the same image stepped plainly: the starved lanes are bit-identical to it
            dev.upload(before)
            dev.step()
            stepped = _full(dev, shape)
            p = exploremodel.plan(stepped, {int(b.code_id[0]): forkmodel.CodeTable(root.environment.code.raw)},
                                  free[used - st.free_used:], 0, np.zeros(shape.n, dtype=np.uint32), PATH_CAP)
            starved_lanes = p[3].tolist()
            assert len(starved_lanes) == st.starved >= 1
            assert whole_diff(after, stepped, lanes=starved_lanes) == []
            assert (after.status[starved_lanes] == MG_FORK).all()
            dev.upload(after)
            break
    assert st is not None and st.starved >= 1 and used == spare
    # everything that did fork is still right: each lane against the restatement along its own path
    out = LaneBatch(shape)
    dev.download(out)
    checked = 0
    for lane in range(shape.n):
        if int(total.root[lane]) != 0 or (lane != 0 and int(total.path_len[lane]) == 0):
            continue
        s = vm._materialise(out, lane, copy(root))
        symcosim._replay(out, lane, s)
        gained = sym.path_constraints(out, lane, s, total.path[lane, :int(total.path_len[lane])])
        if gained is None:
            continue
        ref, k, steps = root, 0, int(out.steps[lane]) - (1 if int(out.status[lane]) in symcosim.EXECUTED_HALTS else 0)
        for _ in range(steps):
            if _at_symbolic_jumpi(ref):
                side = int(total.path[lane, k]) & 1
                k += 1
                pc = ref.mstate.pc
                succ = [t for t in eng.step(ref) if (t.mstate.pc == pc + 1) == (side == 0)]
                assert len(succ) == 1, (lane, k)
                ref = succ[0]
            else:
                succ = eng.step(ref)
                assert len(succ) == 1
                ref = succ[0]
        assert k == int(total.path_len[lane])
        symcosim.assert_same_state(s, ref, (name, lane))
        assert [c.raw for c in list(s.world_state.constraints) + gained] == [c.raw for c in ref.world_state.constraints]
        checked += 1
    assert checked >= 3
    print(f"{name} with {spare} spare lanes: {st.starved} starved {starved_lanes}, {checked} lanes checked")


# ----------------------------------------------------------------- d. path_cap = 1
def test_path_cap_one_refuses_second_level_forks(dev):
    vm, eng, root, shape, b, free = _root_image(dev, "exceptions.sol.o")
    dev.alloc(shape)
    dev.explore_alloc(1)
    _upload_known(dev, shape, b)
    st = dev.explore(free, max_rounds=5)
    left, (path, path_len, path_root) = _full(dev, shape), _paths(dev, shape.n)
    # round 1 forks the root; round 2 steps its children to their JUMPIs and plans nothing
    assert (st.rounds, st.forks, st.made_jump, st.free_used, st.starved) == (2, 1, 1, 1, 0) and st.path_full >= 1
    assert path_len.tolist() == [1, 1] + [0] * (shape.n - 2) and path_root[:2].tolist() == [0, 0]
    assert path[0, 0] >> 1 == path[1, 0] >> 1 and (int(path[0, 0]) & 1, int(path[1, 0]) & 1) == (0, 1)
    # the same batch with room in the path, one round and a plain step: the refused lanes are untouched
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    _upload_known(dev, shape, b)
    one = dev.explore(free, max_rounds=1)
    dev.step()
    right = _full(dev, shape)
    assert one.forks == 1 and whole_diff(left, right) == []
    assert st.path_full == int((right.status[:2] == MG_FORK).sum())


# ------------------------------------------------------------------ e. refusals
def _rc(dev, free, max_rounds=1, null=False):
    arr = np.ascontiguousarray(np.asarray(free, dtype=np.uint32))
    st = native.MgExploreStats()
    rc = dev.lib.mg_explore(dev.ctx, None, 1 << 30, 0, max_rounds, None if null or not arr.size else arr.ctypes.data,
                            arr.size, ctypes.byref(st))
    return rc, dev.lib.mg_last_error(dev.ctx).decode()


def test_host_side_checks_refuse_and_leave_the_image(dev):
    rng = np.random.default_rng(0xE5)
    cid = dev.load_code(CODE)
    n = SHAPE.n
    fresh = GpuDevice(0)
    try:
        rc, msg = _rc(fresh, [1])
        assert rc == MG_ESTATE and "mg_lanes_alloc" in msg, (rc, msg)
    finally:
        fresh.close()
    # a batch without symbolic planes
    plain = dataclasses.replace(SHAPE, node_cap=0, const_cap=0)
    dev.alloc(plain)
    host = saturated(plain, rng, cid)
    dev.upload(host)
    before = _full(dev, plain)
    rc, msg = _rc(dev, [1])
    assert rc == MG_ESTATE and "symbolic" in msg, (rc, msg)
    assert dev.lib.mg_explore_alloc(dev.ctx, 4) == MG_ESTATE
    assert whole_diff(_full(dev, plain), before) == []
    # symbolic planes, no explore planes; then explore planes, nothing uploaded
    dev.alloc(SHAPE)
    host = saturated(SHAPE, rng, cid)
    for k in range(8):
        make_source(host, k, k, J_PLAIN, T_ENTRY)
    dev.upload(host)
    before = _full(dev, SHAPE)
    rc, msg = _rc(dev, [100])
    assert rc == MG_ESTATE and "mg_explore_alloc" in msg, (rc, msg)
    assert whole_diff(_full(dev, SHAPE), before) == []
    dev.alloc(SHAPE)
    dev.explore_alloc(4)
    rc, msg = _rc(dev, [100])
    assert rc == MG_ESTATE and "upload" in msg, (rc, msg)
    assert dev.lib.mg_explore_alloc(dev.ctx, 4) == MG_ESTATE          # twice for one batch
    dev.upload(host)
    before = _full(dev, SHAPE)
    bad = {
        "max_rounds == 0": (dict(free=[100, 101], max_rounds=0), "max_rounds"),
        "equal neighbours": (dict(free=[100, 101, 101]), "free_lanes[2]"),
        "descending": (dict(free=[100, 99]), "free_lanes[1]"),
        "outside the batch": (dict(free=[100, n]), "free_lanes[1]"),
        "far outside the batch": (dict(free=[0xFFFFFFFE]), "free_lanes[0]"),
    }
    for what, (kw, named) in bad.items():
        rc, msg = _rc(dev, **kw)
        assert rc == MG_EINVAL and named in msg, (what, rc, msg)
        assert whole_diff(_full(dev, SHAPE), before) == [], what
        assert not dev.explore_paths(0, n)[1].any(), what
    st = native.MgExploreStats()
    rc = dev.lib.mg_explore(dev.ctx, None, 1 << 30, 0, 1, None, 3, ctypes.byref(st))
    assert rc == MG_EINVAL and whole_diff(_full(dev, SHAPE), before) == []
    assert dev.lib.mg_explore_alloc(dev.ctx, 0) == MG_ESTATE          # already allocated comes first
    # the context is usable.  No free lane: all eight are starved and nothing is written;
    # then three free lanes: the three lowest sources fork
    got = dev.explore([], max_rounds=1)
    assert (got.forks, got.starved, got.free_used, got.running) == (0, 8, 0, 0)
    assert whole_diff(_full(dev, SHAPE), before) == []
    got = dev.explore([100, 101, 102], max_rounds=1)
    assert (got.forks, got.made_jump, got.starved, got.running) == (3, 3, 5, 6)
    after = _full(dev, SHAPE)
    assert whole_diff(after, before) != [] and whole_diff(after, before, lanes=[3, 4, 5, 6, 7, 103]) == []
