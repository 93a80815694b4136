"""mg_lanes_fork on an MI355X: the JUMPI fork of symbolic lanes inside the device
image (lane_fork.cuh), pinned three ways.

a. bit for bit against the NumPy model of the contract (tests/forkmodel.py) on
   the transfer tests' ragged shape: live counts on the tile edges of every
   field, placements across tiles, in place, one-sided, and every kind of jump
   target; a whole download of all lanes, sentinels above the live bounds and
   unnamed lanes included;
b. against the stepper's own concrete JUMPI: the children equal the parent
   stepped one instruction with the condition made 0 and 1;
c. co-simulation past forks with no re-packing: the symbolic co-simulation of
   tests/test_gpu_symbolic.py with the successors made by GpuDevice.fork and
   resumed on the device without an upload;
d. refusals: every host-side check, and every non-forkable source.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import forkmodel
import symcases
import symcosim
import symref
from mythril_amd import native, workloads
from mythril_amd.device import GpuDevice
from mythril_amd.lanes import (_ALL_FIELDS, _SYM_FIELDS, MG_EINVAL, MG_ESCAPE, MG_ESTATE, MG_FORK, MG_FORK_BAD_SRC,
                               MG_FORK_MADE_FALL, MG_FORK_MADE_JUMP, MG_FORK_NONE, MG_HALT_RETURN, MG_HALT_REVERT,
                               MG_HALT_STOP, MG_LANE_HOOK_ACK, MG_LANE_SYMBOLIC, MG_LANE_SYMCD, MG_LANE_TAINT,
                               MG_RUNNING, MG_SYM_CDSIZE, MG_VMEXC, LaneBatch, LaneShape, word_to_limbs)
from mythril_amd.laser import BreadthFirstSearchStrategy, LaserEVM
from mythril_amd.laser import symbolic as sym
from xfermodel import DeviceImage, saturated, sentinel_filled, whole_diff

pytestmark = pytest.mark.gpu

N = 200
SHAPE = LaneShape(n=N, stack_cap=20, mem_cap=288, calldata_cap=68, storage_cap=6, trace_cap=70, rec_cap=130,
                  node_cap=35, const_cap=9)
NONE = MG_FORK_NONE

# index: address  instruction
#  0:  0  JUMPDEST          entry (address 0)
#  1:  1  DUP1
#  2:  2  PUSH4 aabbccdd
#  3:  7  EQ
#  4:  8  PUSH2 0014        the dispatcher's target: address 20
#  5: 11  JUMPI             <- J_PLAIN (fall-through 6 is no entry)
#  6: 12  PUSH2 5b5b        address 13 lies in its data: resolves to index 7
#  7: 15  JUMPDEST          no entry
#  8: 16  PUSH1 00
#  9: 18  JUMPI             <- J_MID
# 10: 19  STOP
# 11: 20  JUMPDEST          entry (_function_0xaabbccdd)
# 12: 21  PUSH1 01
# 13: 23  EQ
# 14: 24  PUSH1 1b          a dispatcher entry at address 27, right after its own JUMPI
# 15: 26  JUMPI             <- J_NFENT (fall-through 16 is an entry)
# 16: 27  JUMPDEST          entry
# 17: 28  STOP              last address 28
CODE = bytes.fromhex("5b" "80" "63aabbccdd" "14" "610014" "57" "615b5b" "5b" "6000" "57" "00" "5b" "6001" "14" "601b"
                     "57" "5b" "00")
J_PLAIN, J_MID, J_NFENT = 5, 9, 15
# jump targets: a JUMPDEST that is an entry, a plain JUMPDEST, a non-JUMPDEST, push data before a
# JUMPDEST (valid by the ">=" table), the last address + 1, a word with limb 1 set
T_ENTRY, T_DEST, T_STOP, T_DATA, T_PAST, T_WIDE = 20, 15, 28, 13, 29, (1 << 32) | 15

SP = (2, 3, 9, 10, 17, 20)
MSIZE = (0, 32, 256, 288)
STORAGE = (0, 1, 5, 6)
NODES = (1, 16, 17, 35)
CONSTS = (0, 1, 8, 9)
REC = (0, 64, 65, 130)
TRACE = (0, 63, 64, 70)


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def _full(dev, shape):
    out = sentinel_filled(shape)
    dev.download(out)
    return out


def _expected_full(model):
    out = sentinel_filled(model.shape)
    model.download(out, 0, model.shape.n)
    return out


def make_source(b, i, k, pc, target, flags=MG_LANE_SYMBOLIC):
    """Lane i of a saturated image becomes a fork source: the k-th combination of
    live counts, at the JUMPI `pc`, jump target `target`, condition tag in the arena."""
    b.status[i], b.aux[i], b.flags[i], b.pc[i] = MG_FORK, 0x57, flags, pc
    sp = SP[k % len(SP)]
    b.sp[i] = sp
    b.msize[i] = MSIZE[(k + k // 6) % len(MSIZE)]
    b.storage_count[i] = STORAGE[(k + k // 5) % len(STORAGE)]
    b.n_nodes[i] = NODES[(k + k // 7) % len(NODES)]
    b.n_consts[i] = CONSTS[(k + k // 3) % len(CONSTS)]
    b.rec_len[i] = REC[(k + k // 9) % len(REC)]
    b.trace_len[i] = TRACE[(k + k // 11) % len(TRACE)]
    b.stack[i, sp - 1] = word_to_limbs(target)
    b.stag[i, sp - 1] = 0
    b.stag[i, sp - 2] = 1 + k % int(b.n_nodes[i])
    b.gas_min[i] &= np.uint64((1 << 40) - 1)
    b.gas_max[i] &= np.uint64((1 << 40) - 1)


# ------------------------------------------------------------- a. the model
def _placements():
    """(src, dst_fall, dst_jump, pc, target)"""
    t = [T_ENTRY, T_DEST, T_STOP, T_DATA, T_PAST, T_WIDE]
    out = [(3, 192, 199, J_PLAIN, T_ENTRY),          # tile 0 -> the last tile (8 lanes)
           (195, 0, 1, J_NFENT, T_DEST),             # the last tile -> tile 0, adjacent destinations
           (10, 10, 11, J_MID, T_DATA),              # in place, with a jump child
           (12, 12, 13, J_NFENT, T_STOP),            # in place, the jump invalid
           (14, 14, NONE, J_PLAIN, T_ENTRY),         # in place, fall only
           (20, 21, NONE, J_NFENT, T_ENTRY),         # fall only
           (30, NONE, 31, J_PLAIN, T_ENTRY),         # jump only
           (32, NONE, 33, J_PLAIN, T_PAST),          # jump only, invalid: nothing made
           (40, NONE, NONE, J_MID, T_DEST),          # neither
           (63, 64, 127, J_MID, T_WIDE),             # across a tile edge
           (128, 191, 65, J_PLAIN, T_DATA)]
    # a run of adjacent destinations (two tiles' worth of neighbours), every target and JUMPI
    for j in range(12):
        out.append((70 + j, 130 + 2 * j, 131 + 2 * j, (J_PLAIN, J_MID, J_NFENT)[j % 3], t[j % 6]))
    return out


def test_fork_equals_the_model_bit_for_bit(dev):
    rng = np.random.default_rng(0xF02C)
    cid = dev.load_code(CODE)
    table = forkmodel.CodeTable(CODE)
    assert [k for k, e in enumerate(table.entry) if e] == [0, 11, 16] and table.addrs[-1] == 28
    assert (dev.code_fentries(cid) & 1).tolist() == [int(e) for e in table.entry]
    dev.alloc(SHAPE, coverage=True)
    dev.coverage_clear()
    host = saturated(SHAPE, rng, cid)
    forks = _placements()
    for k, (s, _, _, pc, target) in enumerate(forks):
        make_source(host, s, k, pc, target,
                    MG_LANE_SYMBOLIC | (MG_LANE_HOOK_ACK if k % 2 else 0) | (MG_LANE_SYMCD if k % 3 else 0))
    for count, values in (("sp", SP), ("msize", MSIZE), ("storage_count", STORAGE), ("n_nodes", NODES),
                          ("rec_len", REC), ("trace_len", TRACE)):
        assert {int(getattr(host, count)[f[0]]) for f in forks} == set(values), count
    model = DeviceImage(SHAPE)
    dev.upload(host)
    model.upload(host, 0, N)
    assert whole_diff(_full(dev, SHAPE), _expected_full(model)) == []
    src, dst_fall, dst_jump = (np.array([f[j] for f in forks], dtype=np.uint32) for j in range(3))
    cov = {cid: np.zeros(table.n, dtype=np.uint8)}
    want_made, want_cond = forkmodel.fork(model, {cid: table}, src, dst_fall, dst_jump, coverage=cov)
    made, cond, ms = dev.fork(src, dst_fall, dst_jump)
    print(f"fork of {len(forks)} lanes: kernel_ms {ms:.4f}")
    assert made.tolist() == want_made.tolist() and cond.tolist() == want_cond.tolist()
    assert whole_diff(_full(dev, SHAPE), _expected_full(model)) == []
    # the model made what the placements are there for
    by_src = {int(s): int(m) for s, m in zip(src, made)}
    assert by_src[3] == by_src[10] == 3 and by_src[12] == 1 and by_src[30] == 2 and by_src[32] == 0 and by_src[40] == 0
    assert {int(m) for m in made} == {0, 1, 2, 3} and not (made & MG_FORK_BAD_SRC).any()
    assert dev.coverage(cid).tolist() == cov[cid].tolist() and cov[cid][[J_PLAIN, J_MID, J_NFENT]].tolist() == [1, 1, 1]
    assert int(cov[cid].sum()) == 3
    # n == 0 is a successful no-op
    e = np.zeros(0, dtype=np.uint32)
    made0, cond0, _ = dev.fork(e, e, e)
    assert made0.size == 0 and cond0.size == 0
    assert whole_diff(_full(dev, SHAPE), _expected_full(model)) == []


# ------------------------------------------------ b. the stepper's own JUMPI
def _dispatcher_jumpi(code: bytes):
    """(JUMPI index, target address) of a dispatcher JUMPI whose target is a function entry."""
    table = forkmodel.CodeTable(code)
    from mythril_amd.laser import Disassembly
    ins = Disassembly(code).instruction_list
    for j in range(1, len(ins)):
        if ins[j]["opcode"] == "JUMPI" and ins[j - 1]["opcode"].startswith("PUSH"):
            arg = ins[j - 1]["argument"]
            target = int(arg, 16) if isinstance(arg, str) else int.from_bytes(bytes(arg), "big")
            idx = table.resolve(target)
            if idx is not None and idx != 0 and table.entry[idx]:
                return j, target
    raise AssertionError("no dispatcher JUMPI")


STEPPER_FIELDS = ("pc", "sp", "depth", "gas_min", "gas_max", "steps", "status", "aux", "flags", "fent")


def test_children_equal_the_steppers_concrete_jumpi(dev):
    over = workloads.bytecode("overflow.sol.o")
    cases = [(dev.load_code(over),) + _dispatcher_jumpi(over), (dev.load_code(CODE), J_NFENT, T_DEST)]
    assert dev.code_fentries(cases[1][0])[J_NFENT] & 2
    shape = LaneShape(n=10, stack_cap=8, mem_cap=64, calldata_cap=36, storage_cap=2, rec_cap=32, node_cap=4, const_cap=4)
    b = LaneBatch(shape)
    b.status[:] = MG_HALT_STOP
    for c, (cid, pc, target) in enumerate(cases):
        base = 5 * c                      # parent, condition 0, condition 1, two spare lanes
        b.code_id[base:base + 5] = cid
        for i in range(base, base + 3):
            b.pc[i], b.sp[i], b.depth[i], b.steps[i] = pc, 3, 4, 7
            b.gas_min[i], b.gas_max[i], b.gas_limit[i] = 1000, 2000, 8_000_000
            b.flags[i] = MG_LANE_SYMBOLIC | MG_LANE_SYMCD | MG_LANE_HOOK_ACK
            b.fent[i] = 2
            b.stack[i, 0] = word_to_limbs(0x1234)
            b.stack[i, 2] = word_to_limbs(target)
            b.node[i, 0] = (MG_SYM_CDSIZE | (256 << 8), 0, 0, 0)
            b.n_nodes[i] = 1
            b.status[i] = MG_RUNNING
        b.status[base], b.aux[base], b.stag[base, 1] = MG_FORK, 0x57, 1
        b.stack[base + 2, 1] = word_to_limbs(1)
    dev.alloc(shape)
    dev.upload(b)
    st = dev.step(max_steps=1)
    assert st.lane_steps == 4
    ref = LaneBatch(shape)
    dev.download(ref)
    made, cond, _ = dev.fork([0, 5], [3, 8], [4, 9])
    assert made.tolist() == [3, 3] and cond.tolist() == [1, 1]
    got = LaneBatch(shape)
    dev.download(got)
    for base in (0, 5):
        for child, stepped in ((base + 3, base + 1), (base + 4, base + 2)):
            for f in STEPPER_FIELDS:
                assert int(getattr(got, f)[child]) == int(getattr(ref, f)[stepped]), (base, child, f)
            assert int(got.status[child]) == MG_RUNNING and not int(got.flags[child]) & MG_LANE_HOOK_ACK
            assert int(got.steps[child]) == 8 and int(got.depth[child]) == 5 and int(got.sp[child]) == 1
    # the entries: the dispatcher's jump lands on one, the directed fall-through is one
    assert int(got.fent[4]) == int(got.pc[4]) != 2 and int(got.fent[3]) == 2
    assert int(got.fent[8]) == J_NFENT + 1 == int(got.pc[8]) and int(got.fent[9]) == 2


# --------------------------------------------------- c. co-simulation past forks
SPARE_LANES = 383
HALTS = (MG_HALT_STOP, MG_HALT_RETURN, MG_HALT_REVERT, MG_VMEXC)


def _min_forks(name: str) -> int:
    return 2 if name == "memjump" else 3      # tests/test_gpu_symbolic.py's bound for these cases


def _view(b, lane, base_steps, base_rec):
    """Lane `lane` of the downloaded image as a batch of one, its step count and
    its records rebased to the state the lane's path is checked from."""
    v = LaneBatch(dataclasses.replace(b.shape, n=1))
    for f in _ALL_FIELDS + _SYM_FIELDS:
        getattr(v, f)[0] = getattr(b, f)[lane]
    v.steps[0] -= base_steps
    rl = int(b.rec_len[lane])
    v.rec[0] = 0
    v.rec[0, :rl - base_rec] = b.rec[lane, base_rec:rl]
    v.rec_len[0] = rl - base_rec
    return v


# (case, spare lanes): every case with lanes to spare, and one with so few that
# forks go the host route too
@pytest.mark.parametrize("name,spare", [("flag_array.sol.o", SPARE_LANES), ("symbolic_exec_bytecode.sol.o", SPARE_LANES),
                                        ("overflow.sol.o", SPARE_LANES), ("exceptions.sol.o", SPARE_LANES),
                                        ("memjump", SPARE_LANES), ("exceptions.sol.o", 5)])
def test_cosimulation_forks_on_the_device_without_repacking(dev, name, spare):
    ws, addr = symcases.deploy(dev, name)
    vm = LaserEVM(requires_statespace=False, device=dev, strategy=BreadthFirstSearchStrategy)
    eng = symref.Engine()
    root = symcosim.initial(ws, addr)
    shape = dataclasses.replace(vm._shape([root]), n=1 + spare)
    b = LaneBatch(shape)
    vm._pack(b, 0, root)
    b.steps[0] = 0
    b.code_id[1:] = b.code_id[0]
    b.status[1:] = MG_HALT_STOP
    dev.alloc(shape)
    dev.upload(b)
    free = list(range(shape.n - 1, 0, -1))            # pop() hands out lanes 1, 2, ...
    # lane -> (the state its steps and records count from, steps and rec_len there, device forks on its path)
    live = {0: (root, 0, 0, 0)}
    host_queue = []
    device_forks = host_forks = launches = checked = twice_then_halted = uploads = 0
    while live:
        dev.step()
        launches += 1
        dev.download_range(b, 0, max(live) + 1)
        todo = []                                     # (lane, successors, want_fall, want_jump, tag, path forks)
        for lane in sorted(live):
            s0, base_steps, base_rec, nf = live.pop(lane)
            ln = symcosim.check_lanes(vm, eng, _view(b, lane, base_steps, base_rec), [s0], name)[0]
            checked += 1
            if ln.status == MG_FORK:
                mine = sym.jumpi_successors(ln.state)
                theirs = eng.step(ln.ref)
                assert [(t.mstate.pc, tuple(c.raw for c in t.world_state.constraints)) for t in mine] == \
                    [(t.mstate.pc, tuple(c.raw for c in t.world_state.constraints)) for t in theirs]
                tag = int(b.stag[lane, int(b.sp[lane]) - 2])
                negated, condi = sym.fork_conditions(b, lane, ln.state, tag)
                for t in mine:
                    t._arena_prefix = getattr(s0, "_arena_prefix", None)     # the arena's prefix is the parent's
                todo.append((lane, mine, not negated.is_false, not condi.is_false, tag, nf))
            elif ln.status == MG_ESCAPE and name == "memjump":
                # the host takes the jump (as LaserEVM's escape handler would) and the
                # path goes back into its lane: an upload of one lane, not a fork
                for t in [t for t in eng.step(ln.state) if sym.lane_eligible(t)][:1]:
                    vm._pack(b, lane, t)
                    b.steps[lane] = 0
                    dev.upload_range(b, lane, 1)
                    uploads += 1
                    live[lane] = (t, 0, 0, 0)
            else:
                free.append(lane)
                if ln.status in HALTS and nf >= 2:
                    twice_then_halted += 1
        # every fork of this launch in one call, in place and two-destination forms in turn
        src, dst_fall, dst_jump, plan = [], [], [], []
        for lane, mine, want_fall, want_jump, tag, nf in todo:
            in_place = want_fall and (device_forks + len(src)) % 2 == 0
            need = (1 if want_fall and not in_place else 0) + (1 if want_jump else 0)
            if len(free) < need:
                host_forks += 1
                host_queue.extend(t for t in mine if sym.lane_eligible(t))
                free.append(lane)
                continue
            df = lane if in_place else free.pop() if want_fall else NONE
            dj = free.pop() if want_jump else NONE
            src.append(lane), dst_fall.append(df), dst_jump.append(dj)
            plan.append((lane, mine, want_fall, tag, nf, in_place))
        if src:
            made, cond, _ = dev.fork(src, dst_fall, dst_jump)
            for i, (lane, mine, want_fall, tag, nf, in_place) in enumerate(plan):
                assert not int(made[i]) & MG_FORK_BAD_SRC and int(cond[i]) == tag
                assert bool(int(made[i]) & MG_FORK_MADE_FALL) == want_fall
                succ = iter(mine)
                base = (int(b.steps[lane]) + 1, int(b.rec_len[lane]), nf + 1)
                if want_fall:
                    live[dst_fall[i]] = (next(succ),) + base
                if int(made[i]) & MG_FORK_MADE_JUMP:
                    live[dst_jump[i]] = (next(succ),) + base
                elif dst_jump[i] != NONE:
                    free.append(dst_jump[i])             # an invalid target: no lane was written
                assert next(succ, None) is None, (name, lane, "jumpi_successors made a state the device did not")
                if not in_place:
                    free.append(lane)
                device_forks += 1
    # what found no spare lane goes the host route: re-encoded, in batches of its own
    while host_queue:
        states, host_queue = host_queue[:256], host_queue[256:]
        lanes, _ = symcosim.cosimulate(dev, states, vm=vm, eng=eng, name=name)
        for ln in lanes:
            if ln.status == MG_FORK:
                host_forks += 1
                host_queue.extend(t for t in sym.jumpi_successors(ln.state) if sym.lane_eligible(t))
    print(f"{name}: {device_forks} device forks, {host_forks} host-route forks, {launches} launches, "
          f"{checked} lane checks, {uploads} lane uploads after the first, {twice_then_halted} paths forked twice "
          f"on the device and halted")
    assert device_forks >= _min_forks(name), (device_forks, host_forks)
    if spare == SPARE_LANES:
        assert twice_then_halted >= 1 and host_forks == 0
    else:
        assert host_forks >= 1
    assert uploads == (0 if name != "memjump" else uploads)


# ------------------------------------------------------------------ d. refusals
def _refusal_image(dev, rng):
    cid = dev.load_code(CODE)
    dev.alloc(SHAPE)
    host = saturated(SHAPE, rng, cid)
    for k, s in enumerate(range(8)):
        make_source(host, s, k, J_PLAIN, T_ENTRY)
    dev.upload(host)
    return cid, host


def _rc(dev, src, dst_fall, dst_jump, made=True, cond=True):
    arrs = [np.asarray(a, dtype=np.uint32) for a in (src, dst_fall, dst_jump)]
    n = arrs[0].size
    m, c = np.full(max(n, 1), 0xEE, dtype=np.uint32), np.full(max(n, 1), 0xEE, dtype=np.uint32)
    batch = native.MgForkBatch(n, 0, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data)
    rc = dev.lib.mg_lanes_fork(dev.ctx, ctypes.byref(batch), m.ctypes.data if made else None,
                               c.ctypes.data if cond else None, None)
    return rc, dev.lib.mg_last_error(dev.ctx).decode()


def test_host_side_checks_refuse_and_leave_the_image(dev):
    rng = np.random.default_rng(0xD1)
    _refusal_image(dev, rng)
    before = _full(dev, SHAPE)
    bad = {
        "duplicate src": ([0, 1, 0], [100, 101, 102], [NONE] * 3, "src[2]"),
        "destination twice": ([0, 1], [100, 101], [102, 100], "dst_jump[1]"),
        "fall and jump in one lane": ([0], [100], [100], "dst_jump[0]"),
        "destination is another source": ([0, 1], [100, 0], [NONE, NONE], "dst_fall[1]"),
        "jump destination is another source": ([0, 1], [NONE, NONE], [1, 100], "dst_jump[0]"),
        "dst_jump == src": ([0], [NONE], [0], "dst_jump[0]"),
        "src out of range": ([0, N], [100, 101], [NONE, NONE], "src[1]"),
        "dst_fall out of range": ([0], [N], [NONE], "dst_fall[0]"),
        "dst_jump out of range": ([0], [NONE], [0xFFFFFFFE], "dst_jump[0]"),
    }
    for what, (src, df, dj, named) in bad.items():
        rc, msg = _rc(dev, src, df, dj)
        assert rc == MG_EINVAL and named in msg, (what, rc, msg)
        assert whole_diff(_full(dev, SHAPE), before) == [], what
    for made, cond in ((False, True), (True, False)):
        rc, msg = _rc(dev, [0], [100], [101], made=made, cond=cond)
        assert rc == MG_EINVAL, msg
        assert whole_diff(_full(dev, SHAPE), before) == []
    # the context is usable: the next valid call succeeds
    made, cond, _ = dev.fork([0, 1], [0, 100], [101, NONE])
    assert made.tolist() == [3, 1]
    assert whole_diff(_full(dev, SHAPE), before) != []


def test_fork_needs_an_upload_and_symbolic_planes(dev):
    rng = np.random.default_rng(0xD2)
    cid = dev.load_code(CODE)
    plain = dataclasses.replace(SHAPE, node_cap=0, const_cap=0)
    dev.alloc(plain)
    host = saturated(plain, rng, cid)
    dev.upload(host)
    before = _full(dev, plain)
    rc, msg = _rc(dev, [0], [1], [2])
    assert rc == MG_ESTATE and "symbolic" in msg, (rc, msg)
    assert whole_diff(_full(dev, plain), before) == []
    dev.alloc(SHAPE)                                   # symbolic planes, nothing uploaded
    rc, msg = _rc(dev, [0], [1], [2])
    assert rc == MG_ESTATE and "upload" in msg, (rc, msg)
    host = saturated(SHAPE, rng, cid)
    make_source(host, 0, 2, J_MID, T_DEST)
    dev.upload(host)
    made, cond, _ = dev.fork([0], [1], [2])
    assert made.tolist() == [3] and int(cond[0]) == int(host.stag[0, int(host.sp[0]) - 2])


def test_sources_that_cannot_fork_answer_bad_src(dev):
    rng = np.random.default_rng(0xD3)
    cid = dev.load_code(CODE)
    dev.alloc(SHAPE)
    host = saturated(SHAPE, rng, cid)
    for k in range(5):
        make_source(host, k, k + 1, J_PLAIN, T_ENTRY)
    host.status[0] = MG_HALT_STOP                                  # a halted lane
    host.flags[1] |= MG_LANE_TAINT                                 # a taint lane
    host.stag[2, int(host.sp[2]) - 1] = 1                          # a symbolic target
    host.sp[3] = 1                                                 # sp 1
    host.stag[3, 0] = 1
    dev.upload(host)
    before = _full(dev, SHAPE)
    src, df, dj = [0, 1, 2, 3], [0, 101, 102, 103], [110, 111, 112, 113]
    made, cond, _ = dev.fork(src, df, dj)
    assert made.tolist() == [MG_FORK_BAD_SRC] * 4 and cond.tolist() == [0] * 4
    assert whole_diff(_full(dev, SHAPE), before) == []
    # beside a source that can: only that one's lanes change, as the model says
    model = DeviceImage(SHAPE)
    model.upload(host, 0, N)
    table = forkmodel.CodeTable(CODE)
    want = forkmodel.fork(model, {cid: table}, src + [4], df + [104], dj + [114])
    made, cond, _ = dev.fork(src + [4], df + [104], dj + [114])
    assert made.tolist() == want[0].tolist() == [MG_FORK_BAD_SRC] * 4 + [3] and cond.tolist() == want[1].tolist()
    assert whole_diff(_full(dev, SHAPE), _expected_full(model)) == []
