"""Directed cases for the symbolic stepper on an MI355X (tests/symdirect.py):
each program is co-simulated against the restatement (tests/symcosim.py) and
must end where its case says -- instruction count, status, aux, arena node
kinds, records -- so a lane that escapes early cannot pass by doing nothing.

* one parametrised test per case list (memparts, taghygiene, chain, aluquirks,
  the stack limit, static calls, LOGs, the resource program and a fork);
* capacity sweeps: the resource program under every node, constant, record,
  storage and stack capacity from the legal minimum to one past what it needs.
  A lane that stops for a capacity must have left nothing behind: its counts
  are the uncapped run's after as many steps, and resumed under the uncapped
  shape it ends as the uncapped run does, plane for plane;
* gas sweeps: one lane per limit c - 1, c, c + 1 around every cumulative gas
  value the restatement reaches;
* slices: every program whole, in launches of 1, 2 and 3 instructions, and as
  MG_LANE_STEP1 lanes;
* hooks: a hook mask on SLOAD, SHA3, MLOAD and JUMPI stops a lane before the
  opcode with nothing changed; acknowledged, it ends as the unhooked run does."""
from collections import Counter

import numpy as np
import pytest

import symcosim
import symdirect
import symref
from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.lanes import (MG_ESC_ARENA, MG_ESC_RECORD, MG_ESC_STACK, MG_ESC_STORAGE, MG_ESCAPE, MG_HOOK,
                               MG_LANE_HOOK_ACK, MG_LANE_STEP1, MG_RUNNING)
from xfermodel import live_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def vm(dev):
    # one LaserEVM for the module: it loads each code once, so images of the same
    # program carry the same code id and can be compared plane for plane
    return symcosim.new_vm(dev)


def _assert_case(case, ln):
    assert (ln.steps, ln.status) == (case.steps, case.status), (case.name, ln.steps, ln.status, hex(ln.aux), ln.pc)
    if case.aux is not None:
        assert ln.aux == case.aux, (case.name, hex(ln.aux), hex(case.aux))
    for kind, width in case.kinds:
        have = ln.kinds[kind] if width is None else ln.kind_widths[(kind, width)]
        assert have > 0, (case.name, "no arena node of kind", kind, "width", width, sorted(ln.kind_widths))
    for r in case.records:
        assert any(rec[1] == r for rec in ln.records), (case.name, "no record", r, ln.records)


def _run_case(dev, vm, name, every_step=True):
    """Co-simulate one case.  With `every_step`, one instruction a launch with the
    lane compared against the restatement after each, so a value the program pops
    again is checked while it is on the stack."""
    case = symdirect.BY_NAME[name]
    eng, s0 = symref.Engine(), symdirect.initial_state(case)
    if not every_step:
        lanes, _ = symcosim.cosimulate(dev, [s0], caps=case.caps, vm=vm, eng=eng, name=name, constraints=True)
        ln = lanes[0]
    else:
        b = symcosim.pack(vm, [s0], case.caps)
        dev.alloc(b.shape)
        dev.upload(b)
        trail = []
        for _ in range(case.steps + 2):
            dev.step(max_steps=1)
            dev.download(b)
            ln = symcosim.check_lanes(vm, eng, b, [s0], name, constraints=True, trail=trail)[0]
            if ln.status != MG_RUNNING:
                break
    print(name, "steps", ln.steps, "status", ln.status, "aux", hex(ln.aux), "nodes", ln.n_nodes, "consts",
          ln.n_consts, "rec", ln.rec_len, "chain", ln.storage_count)
    _assert_case(case, ln)
    return case, ln, eng


def _names(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("name", _names(symdirect.MEMPARTS))
def test_memparts(dev, vm, name):
    _run_case(dev, vm, name)


@pytest.mark.parametrize("name", _names(symdirect.TAGHYGIENE))
def test_taghygiene(dev, vm, name):
    _run_case(dev, vm, name)


@pytest.mark.parametrize("name", _names(symdirect.CHAIN))
def test_chain(dev, vm, name):
    _run_case(dev, vm, name)


def _step_outcome(eng, state):
    try:
        return [(t.mstate.pc, [x.raw for x in t.mstate.stack], t.mstate.min_gas_used) for t in eng.step(state)]
    except symref.Unsupported:
        return "unsupported"


@pytest.mark.parametrize("name", _names(symdirect.ALUQUIRKS))
def test_aluquirks(dev, vm, name):
    case, ln, eng = _run_case(dev, vm, name)
    if case.status == MG_ESCAPE:
        # the host's step of the escaped instruction, from the decoded lane, is the
        # restatement's from its own state: the successor's pc, stack terms and gas.
        # That says something only where the restatement has semantics (the Bool
        # operands, which its stack holds as If(b, 1, 0)); for the rest the device's
        # stop before the instruction, asserted above, is all there is to check
        want = _step_outcome(eng, ln.ref)
        assert (want == "unsupported") == (name in symdirect.NO_RESTATEMENT), (name, want)
        if want != "unsupported":
            assert len(want) == 1 and _step_outcome(eng, ln.state) == want


@pytest.mark.parametrize("name", _names(symdirect.STACK_LIMIT))
def test_stack_limit(dev, vm, name):
    # a thousand-word stack: decoded once, at the end
    _run_case(dev, vm, name, every_step=False)


@pytest.mark.parametrize("name", _names(symdirect.STATIC + symdirect.LOGS))
def test_static_calls_and_logs(dev, vm, name):
    _run_case(dev, vm, name)


@pytest.mark.parametrize("name", ["consume", "fork", "gas_tail"])
def test_resource_program_and_fork(dev, vm, name):
    _run_case(dev, vm, name)


# ---- (a) capacity sweeps --------------------------------------------------------------
COUNT_OF = {"node_cap": "n_nodes", "const_cap": "n_consts", "rec_cap": "rec_len", "storage_cap": "storage_count",
            "stack_cap": "sp"}
REASON_OF = {"node_cap": MG_ESC_ARENA, "const_cap": MG_ESC_ARENA, "rec_cap": MG_ESC_RECORD,
             "storage_cap": MG_ESC_STORAGE, "stack_cap": MG_ESC_STACK}
LEGAL_MIN = {"node_cap": 1, "const_cap": 1, "rec_cap": 1, "storage_cap": 1, "stack_cap": 16}


@pytest.fixture(scope="module")
def uncapped(dev, vm):
    """The resource program under the default shape, one instruction a launch:
    (its first state, the image at the end, the counts after every step)."""
    s0 = symdirect.initial_state(symdirect.CONSUME)
    b = symcosim.pack(vm, [s0])
    dev.alloc(b.shape)
    dev.upload(b)
    after = []
    for _ in range(symdirect.CONSUME.steps + 2):
        dev.download(b)
        after.append({f: int(getattr(b, f)[0]) for f in COUNT_OF.values()})
        assert int(b.steps[0]) == len(after) - 1 or int(b.status[0]) != MG_RUNNING
        if int(b.status[0]) != MG_RUNNING:
            break
        dev.step(max_steps=1)
    assert (int(b.steps[0]), int(b.status[0])) == (symdirect.CONSUME.steps, symdirect.CONSUME.status)
    return s0, b, after


@pytest.mark.parametrize("cap", list(COUNT_OF))
def test_capacity_sweep(dev, vm, uncapped, cap):
    case = symdirect.CONSUME
    s0, full, after = uncapped
    count = COUNT_OF[cap]
    need = max(a[count] for a in after)          # the smallest capacity the program fits in
    assert need >= LEGAL_MIN[cap] + 4, (cap, need)
    eng, trail = symref.Engine(), []
    stops, last = [], -1
    for c in range(LEGAL_MIN[cap], need + 2):
        b = symcosim.launch(dev, symcosim.pack(vm, [s0], {cap: c}))
        ln = symcosim.check_lanes(vm, eng, b, [s0], f"{cap}={c}", constraints=True, trail=trail)[0]
        assert ln.steps >= last, (cap, c, ln.steps, last)        # non-decreasing in the capacity
        last = ln.steps
        if c >= need:
            _assert_case(case, ln)
            assert not live_diff(b.regrown(full.shape), full), (cap, c)
            continue
        # stopped before an instruction, for this capacity, with nothing left behind
        assert (ln.status, ln.reason) == (MG_ESCAPE, REASON_OF[cap]), (cap, c, ln.status, hex(ln.aux), ln.steps)
        assert ln.steps < case.steps
        got = {f: int(getattr(b, f)[0]) for f in COUNT_OF.values()}
        assert got == after[ln.steps], (cap, c, ln.steps, got, after[ln.steps])
        stops.append(ln.steps)
        # resumed under the uncapped shape it ends exactly as the uncapped run does
        r = symcosim.launch(dev, symcosim.resumed(b, full.shape))
        assert not live_diff(r, full), (cap, c, live_diff(r, full))
    print(cap, "capacities", LEGAL_MIN[cap], "..", need + 1, "distinct stop points", len(set(stops)))
    assert len(set(stops)) >= 4, (cap, stops)


# ---- (b) gas sweeps -------------------------------------------------------------------
@pytest.mark.parametrize("name", _names(symdirect.GAS_SWEPT))
def test_gas_sweep(dev, vm, name):
    case = symdirect.BY_NAME[name]
    limits = symdirect.gas_limits(case)
    assert 3 <= len(limits) <= 256
    states = [symdirect.initial_state(case, gas_limit=g) for g in limits]
    lanes, _ = symcosim.cosimulate(dev, states, vm=vm, name=name, constraints=True)
    ends = Counter()
    for g, ln in zip(limits, lanes):
        want = symdirect.expected_under_gas(case, g)
        got = (ln.steps, ln.status, None if want[2] is None else ln.aux)
        assert got == want, (name, g, got, hex(ln.aux), want)
        ends[got[1:]] += 1
    print(name, len(limits), "limits", dict(ends))
    assert len(ends) >= 2


# ---- slices ---------------------------------------------------------------------------
# every program, in one batch per set of capacity overrides (a batch has one shape)
SLICED = {}
for _c in symdirect.ALL:
    SLICED.setdefault(tuple(sorted((_c.caps or {}).items())), []).append(_c)


def _sliced_batches(vm):
    return {caps: symcosim.pack(vm, [symdirect.initial_state(c) for c in cases], dict(caps))
            for caps, cases in SLICED.items()}


@pytest.fixture(scope="module")
def whole(dev, vm):
    out = {caps: symcosim.launch(dev, b) for caps, b in _sliced_batches(vm).items()}
    for caps, b in out.items():
        assert [int(x) for x in b.steps] == [c.steps for c in SLICED[caps]], caps
    return out


@pytest.mark.parametrize("k", [1, 2, 3])
def test_slices_of_k_instructions_equal_one_run(dev, vm, whole, k):
    assert sum(len(v) for v in SLICED.values()) == len(symdirect.ALL) and len(SLICED) >= 3
    for caps, b in _sliced_batches(vm).items():
        b = symcosim.launch(dev, b, max_steps=k)
        assert not live_diff(b, whole[caps]), (caps, live_diff(b, whole[caps]))


def test_step1_lanes_equal_one_run(dev, vm, whole):
    # MG_LANE_STEP1: at most one instruction a launch, whatever max_steps says
    for caps, b in _sliced_batches(vm).items():
        b.flags[:] = b.flags | np.uint32(MG_LANE_STEP1)
        b = symcosim.launch(dev, b, max_steps=5)
        b.flags[:] = b.flags & ~np.uint32(MG_LANE_STEP1)
        assert not live_diff(b, whole[caps]), (caps, live_diff(b, whole[caps]))


# ---- hooks ----------------------------------------------------------------------------
HOOKED_OPS = {"SLOAD": 0x54, "SHA3": 0x20, "MLOAD": 0x51, "JUMPI": 0x57}
HOOKED = ["chain_symbolic_base", "sha3_mixed_lengths", "mload_sweep_0_21", "fork", "consume"]


def test_hooked_lanes_stop_unchanged_and_resume_to_the_unhooked_end(dev, vm):
    cases = [symdirect.BY_NAME[n] for n in HOOKED]
    states = [symdirect.initial_state(c) for c in cases]
    eng = symref.Engine()
    plain = symcosim.launch(dev, symcosim.pack(vm, states))
    mask = hook_mask_for(HOOKED_OPS.values())
    b = symcosim.launch(dev, symcosim.pack(vm, states), hook_mask=mask)
    hooks = Counter()
    for _ in range(200):
        hooked = [i for i in range(b.n) if int(b.status[i]) == MG_HOOK]
        if not hooked:
            break
        # stopped before the opcode: the state is the restatement's after as many steps
        lanes = symcosim.check_lanes(vm, eng, b, states, "hooked", constraints=True)
        for i in hooked:
            ins = states[i].environment.code.instruction_list[lanes[i].pc]["opcode"]
            assert lanes[i].aux == HOOKED_OPS[ins], (HOOKED[i], ins, hex(lanes[i].aux))
            hooks[ins] += 1
        b = symcosim.launch(dev, symcosim.resumed(b, ack=True), hook_mask=mask)
    else:
        raise AssertionError("lanes still hooked after 200 rounds")
    assert all(hooks[ins] >= 1 for ins in HOOKED_OPS), hooks
    assert sum(hooks.values()) == sum(c.src.split().count(ins) for c in cases for ins in HOOKED_OPS)
    # a lane whose acknowledged instruction did not run (the JUMPI that forks) keeps the flag
    b.flags[:] = b.flags & ~np.uint32(MG_LANE_HOOK_ACK)
    assert not live_diff(b, plain), live_diff(b, plain)
