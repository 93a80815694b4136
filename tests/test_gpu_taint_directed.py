"""The directed taint cases (tests/taintdirect.py) on an MI355X: k_sym_step's taint
lanes against the restatement (tests/taintref.py over the C oracle) AND against
each case's hand-written outcome.

* geometry: every family's cases are laid out over 600 lanes (three 256-thread
  blocks, the last one partial), placed and repeated at the block and wave edges,
  interleaved with plain concrete lanes (which must equal oracle/evm_ref.c's run)
  and with lanes already halted (which must be untouched);
* slices: whole, in launches of 1, 2 and 3 instructions, and as MG_LANE_STEP1
  lanes: the same planes at the end (partitions, not handle numbers);
* hooks: a real hook mask on ADD, SSTORE, JUMPI and ORIGIN stops each lane before
  the opcode as the restatement says; acknowledged, the instruction runs with no
  atom and no record;
* capacity sweeps: one lane per rec_cap around every cumulative record length;
  a lane that escapes has left nothing behind and, resumed under the uncapped
  shape, ends as the uncapped run;
* compaction: the cases end in the same partition at obj_cap 64, where no
  compaction happens, and the device's n_obj shows that it did happen at 16.

All comparisons are bit-exact.
"""
import numpy as np
import pytest

import taintdirect as td
from mythril_amd.device import GpuDevice, hook_mask_for
from mythril_amd.lanes import (MG_ESC_RECORD, MG_ESCAPE, MG_HALT_STOP, MG_HOOK, MG_LANE_HOOK_ACK, MG_LANE_STEP1,
                               MG_RUNNING, LaneBatch)
from mythril_amd.laser.opcodes import OPCODES
from oracle_device import OracleDevice
from symdirect import asm

pytestmark = pytest.mark.gpu

N = 600
EDGES = (0, 63, 64, 255, 256, 511, 512, 599)
SCALARS = ("pc", "sp", "msize", "status", "aux", "steps", "gas_min", "gas_max", "rec_len", "storage_count",
           "n_atoms", "sink", "ymask", "tflags")
PLAIN = asm(td.PLAIN_SRC)


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    d.cids = {}
    yield d
    d.close()


def _cid(d, code, force=None):
    """One code id per (code, force table) on a device."""
    key = (bytes(code), None if force is None else force.tobytes())
    if key not in d.cids:
        d.cids[key] = d.load_code(code)
        if force is not None:
            d.set_taint_force(d.cids[key], force)
    return d.cids[key]


def layout(n_cases):
    """What each of the 600 lanes holds: a case (by index), a plain concrete lane
    or a halted lane.  The block and wave edges hold cases that appear elsewhere
    too."""
    plan = [None] * N
    for j, lane in enumerate(EDGES):
        plan[lane] = j % n_cases
    k = 0
    for i in range(N):
        if plan[i] is None:
            if i % 4 == 1:
                plan[i] = "plain"
            elif i % 4 == 3:
                plan[i] = "halted"
            else:
                plan[i] = k % n_cases
                k += 1
    assert k >= n_cases
    return plan


def _set_halted(b, i, cid):
    td.set_case_lane(b, i, td.BY_NAME["gc_acked_full"], cid)      # six objects on the stack
    b.status[i], b.aux[i], b.steps[i], b.pc[i] = MG_HALT_STOP, 0, 5, 1


def _used(b, i):
    """Everything of lane i that a step reads or writes, as comparable values."""
    out = {f: int(getattr(b, f)[i]) for f in SCALARS + ("flags", "n_obj", "n_fixed")}
    out["stack"] = b.stack[i, : int(b.sp[i])].tobytes()
    out["sobj"] = b.sobj[i, : int(b.sp[i])].tobytes()
    out["omask"] = b.omask[i, : int(b.n_obj[i])].tobytes()
    out["rec"] = b.rec[i, : int(b.rec_len[i])].tobytes()
    out["memory"] = b.memory[i, : int(b.msize[i])].tobytes()
    out["storage"] = b.storage[i, : int(b.storage_count[i])].tobytes()
    return out


def _same(b, i, r, j, what, taint=True):
    """Lane i of b equals lane j of r: scalars, stack, memory, storage and the
    record log word for word; the partition of the stack into objects."""
    for f in SCALARS[:10] + (SCALARS[10:] if taint else ()):
        assert int(getattr(b, f)[i]) == int(getattr(r, f)[j]), (what, i, f, int(getattr(b, f)[i]),
                                                                 int(getattr(r, f)[j]))
    assert np.array_equal(b.stack[i, : int(b.sp[i])], r.stack[j, : int(r.sp[j])]), (what, i, "stack")
    assert np.array_equal(b.rec[i, : int(b.rec_len[i])], r.rec[j, : int(r.rec_len[j])]), (what, i, "records")
    assert np.array_equal(b.memory[i, : int(b.msize[i])], r.memory[j, : int(r.msize[j])]), (what, i, "memory")
    assert b.storage_dict(i, drop_zero=False) == r.storage_dict(j, drop_zero=False), (what, i, "storage")
    if taint:
        assert td.partition(b, i) == td.partition(r, j), (what, i, td.partition(b, i), td.partition(r, j))


class Group:
    """One group of cases (one shape, one action table): the 600-lane device batch
    and the restatement's batch (one lane per case, then the plain lane)."""

    def __init__(self, dev, cases, **caps):
        self.dev, self.cases, self.caps = dev, cases, caps
        self.plan = layout(len(cases))
        self.ora = None
        self.actions = td.action_words(dict(cases[0].actions))

    def device_batch(self, flags=0):
        b = LaneBatch(td.shape_of(self.cases[0], N, **self.caps))
        for i, what in enumerate(self.plan):
            if what == "plain":
                b.set_lane(i, code_id=_cid(self.dev, PLAIN), caller=td.CALLER, address=td.ADDRESS)
            elif what == "halted":
                _set_halted(b, i, _cid(self.dev, PLAIN))
            else:
                c = self.cases[what]
                td.set_case_lane(b, i, c, _cid(self.dev, c.code, td.force_flags(c)))
                b.flags[i] |= flags
        return b

    def ref_batch(self):
        # a new OracleDevice starts the C oracle's code table afresh: one at a time
        n = len(self.cases)
        self.ora = OracleDevice()
        self.ocid = [self.ora.load_code(c.code) for c in self.cases] + [self.ora.load_code(PLAIN)]
        for c, cid in zip(self.cases, self.ocid):
            if c.force:
                self.ora.set_taint_force(cid, td.force_flags(c))
        r = LaneBatch(td.shape_of(self.cases[0], n + 1, **self.caps))
        for j, c in enumerate(self.cases):
            td.set_case_lane(r, j, c, self.ocid[j])
        r.set_lane(n, code_id=self.ocid[n], caller=td.CALLER, address=td.ADDRESS)
        return r

    def start(self, b, r=None):
        self.dev.alloc(b.shape)
        self.dev.set_taint_program(self.actions)
        self.dev.upload(b)
        if r is not None:
            self.ora.alloc(r.shape)
            self.ora.set_taint_program(self.actions)
            self.ora.upload(r)

    def launches(self):
        return max((c.out_uncapped or c.out).steps for c in self.cases) + len(td.PLAIN_SRC.split()) + 2

    def run_device(self, b, max_steps=1 << 20, launches=1, hook=None):
        self.start(b)
        for _ in range(launches):
            self.dev.step(hook, max_steps=max_steps)
        self.dev.download(b)
        return b

    def check_others(self, b, b0, r):
        """The plain lanes ran as the C oracle's; the halted lanes are untouched."""
        for i, what in enumerate(self.plan):
            if what == "plain":
                _same(b, i, r, len(self.cases), "plain", taint=False)
            elif what == "halted":
                assert _used(b, i) == _used(b0, i), ("halted", i)

    def outcome(self, c):
        return (c.out_uncapped or c.out) if self.caps.get("obj_cap") else c.out


def _groups(dev, family, **caps):
    for cases in td.groups(td.FAMILIES[family]):
        yield Group(dev, cases, **caps)


def _whole(g):
    """One launch of the group on the device and in the restatement, compared."""
    b0 = g.device_batch()
    b, r = b0.copy(), g.ref_batch()
    g.start(b, r)
    g.dev.step(None, max_steps=1 << 20)
    g.ora.step(None, max_steps=1 << 20)
    g.dev.download(b)
    g.ora.download(r)
    for i, what in enumerate(g.plan):
        if isinstance(what, int):
            c = g.cases[what]
            want = g.outcome(c)
            got = td.observe(b, i, c, want)
            assert got == want, (c.name, i, got, want)                     # device = hand-written outcome
            _same(b, i, r, what, c.name)                                   # device = restatement
            td.check_pins(b, i, c)
            if c.dev_n_obj is not None and not g.caps:
                assert int(b.n_obj[i]) == c.dev_n_obj, (c.name, i, int(b.n_obj[i]), c.dev_n_obj)
    g.check_others(b, b0, r)
    return b, r


@pytest.mark.parametrize("family", list(td.FAMILIES))
def test_family_whole_and_in_slices(dev, family):
    n = 0
    for g in _groups(dev, family):
        whole, r = _whole(g)
        n += len(g.cases)
        ways = [("1", 1, 0), ("2", 2, 0), ("3", 3, 0), ("step1", 5, MG_LANE_STEP1)]
        for name, k, flag in ways:
            b0 = g.device_batch(flags=flag)
            b = g.run_device(b0.copy(), max_steps=k, launches=g.launches() if flag else -(-g.launches() // k))
            assert not (b.status == MG_RUNNING).any(), (family, name, np.nonzero(b.status == MG_RUNNING)[0][:8])
            if flag:
                b.flags[:] = b.flags & ~np.uint32(flag)
            for i, what in enumerate(g.plan):
                if isinstance(what, int):
                    _same(b, i, whole, i, (g.cases[what].name, "slices of", name))
                    assert int(b.flags[i]) == int(whole.flags[i]), (g.cases[what].name, name)
            g.check_others(b, b0, r)
    assert n == len(td.FAMILIES[family])


def test_compaction_cases_without_compaction(dev):
    # obj_cap 64: no compaction; the same partitions (and for the two that escape at
    # a full table, the uncapped outcome)
    for g in _groups(dev, "compaction", obj_cap=64):
        b, _ = _whole(g)
        small = Group(dev, g.cases)
        s = small.run_device(small.device_batch())
        for i, what in enumerate(g.plan):
            if isinstance(what, int):
                c = g.cases[what]
                assert int(s.n_obj[i]) == c.dev_n_obj, (c.name, int(s.n_obj[i]))
                if c.name not in td.GC_ESCAPES:
                    assert int(s.n_obj[i]) < int(b.n_obj[i]), (c.name, int(s.n_obj[i]), int(b.n_obj[i]))
                    assert td.partition(s, i) == td.partition(b, i), c.name


def test_full_table_escape_changes_nothing_and_resumes(dev):
    """gc_all_live: MG_ESC_TAINT with every plane as before the instruction (the
    same lane stopped one instruction earlier by its budget); resumed under
    obj_cap 64 it ends plane for plane as the uncapped run."""
    c = td.BY_NAME["gc_all_live"]
    g = Group(dev, [c])
    esc = g.run_device(g.device_batch())
    short = g.run_device(g.device_batch(), max_steps=c.out.steps)
    big = Group(dev, [c], obj_cap=64)
    full = big.run_device(big.device_batch())
    res = esc.regrown(full.shape)
    res.status[:] = np.where(res.status == MG_ESCAPE, MG_RUNNING, res.status)
    res.aux[res.status == MG_RUNNING] = 0
    res = big.run_device(res)
    for i, what in enumerate(g.plan):
        if isinstance(what, int):
            assert (int(esc.status[i]), int(esc.aux[i])) == (c.out.status, c.out.aux)
            assert (int(short.status[i]), int(short.steps[i])) == (MG_RUNNING, c.out.steps)
            for f in SCALARS[:3] + SCALARS[5:]:
                assert int(getattr(esc, f)[i]) == int(getattr(short, f)[i]), f
            assert td.partition(esc, i) == td.partition(short, i)
            assert np.array_equal(esc.rec[i, : int(esc.rec_len[i])], short.rec[i, : int(short.rec_len[i])])
            _same(res, i, full, i, "resumed")
            assert td.observe(res, i, c, c.out_uncapped) == c.out_uncapped


HOOKED = ("ADD", "SSTORE", "JUMPI", "ORIGIN")


@pytest.mark.parametrize("family", ["identity", "fresh", "compaction", "capacity", "yield"])
def test_hooked_lanes_stop_unchanged_and_run_acknowledged_without_actions(dev, family):
    mask = hook_mask_for([OPCODES[o] for o in HOOKED])
    stops = 0
    for g in _groups(dev, family):
        b, r = g.device_batch(), g.ref_batch()
        g.start(b, r)
        for _ in range(64):
            g.dev.step(mask, max_steps=1 << 20)
            g.ora.step(mask, max_steps=1 << 20)
            g.dev.download(b)
            g.ora.download(r)
            hooked = 0
            for i, what in enumerate(g.plan):
                if isinstance(what, int):
                    # stopped before the opcode with nothing changed: the restatement's
                    # planes after as many instructions
                    _same(b, i, r, what, (g.cases[what].name, "hooked"))
                    if int(b.status[i]) == MG_HOOK:
                        assert int(b.aux[i]) in [OPCODES[o] for o in HOOKED] + [OPCODES["SLOAD"]]
                        hooked += 1
            if not hooked:
                break
            stops += hooked
            for x in (b, r):
                h = x.status == MG_HOOK
                x.flags[h] |= np.uint32(MG_LANE_HOOK_ACK)
                x.status[h], x.aux[h] = MG_RUNNING, 0
            g.dev.upload(b)
            g.ora.upload(r)
        else:
            raise AssertionError("lanes still hooked after 64 rounds")
        for i, what in enumerate(g.plan):
            if isinstance(what, int):
                c = g.cases[what]
                if all(dict(c.actions).get(o, 0) == 0 or o in HOOKED for o in set(c.src.split()) & set(OPCODES)):
                    # every action of the program was the host's: no atom, no record of the device's
                    assert int(b.n_atoms[i]) == c.n_atoms, (c.name, int(b.n_atoms[i]))
                    assert not [k for k in td.record_kinds(b, i, c.rec_len) if k[0] in ("pre", "post")], c.name
    assert stops > 0


# ---- (h) capacity sweeps ---------------------------------------------------------------
def _stepwise(g):
    """The group under its own shape, one instruction a launch: the images after
    every step."""
    b = g.device_batch()
    g.start(b)
    after = [b.copy()]
    for _ in range(g.launches()):
        g.dev.step(None, max_steps=1)
        g.dev.download(b)
        after.append(b.copy())
    return after


def test_record_capacity_sweep(dev):
    cases = [td.BY_NAME[n] for n in td.SWEPT]
    assert len({c.shape_key for c in cases}) == 1
    full_g = Group(dev, cases)
    after = _stepwise(full_g)
    full = after[-1]
    assert not (full.status == MG_RUNNING).any()
    lens = sorted({int(a.rec_len[i]) for a in after for i, w in enumerate(full_g.plan) if isinstance(w, int)} - {0})
    assert set(w for w, _ in td.CAPREC_STOPS) <= set(lens)
    stops = set()
    for cap in sorted({c for w in lens for c in (w - 1, w, w + 1)}):
        g = Group(dev, cases, rec_cap=cap)
        b0 = g.device_batch()
        b, r = b0.copy(), g.ref_batch()
        g.start(b, r)
        g.dev.step(None, max_steps=1 << 20)
        g.ora.step(None, max_steps=1 << 20)
        g.dev.download(b)
        g.ora.download(r)
        res = b.regrown(full.shape)
        res.aux[res.status == MG_ESCAPE] = 0
        res.status[res.status == MG_ESCAPE] = MG_RUNNING
        res = full_g.run_device(res)
        for i, what in enumerate(g.plan):
            if not isinstance(what, int):
                continue
            c = cases[what]
            _same(b, i, r, what, (c.name, "rec_cap", cap))
            steps = int(b.steps[i])
            if c is td.CAPREC:
                assert steps == td.caprec_steps(cap), (cap, steps)
            if int(b.status[i]) == MG_ESCAPE:
                # before an instruction, with nothing left behind: the uncapped run's
                # planes after as many steps
                assert int(b.aux[i]) >> 8 == MG_ESC_RECORD and steps < c.out.steps, (c.name, cap, hex(int(b.aux[i])))
                a = after[steps]
                for f in SCALARS[:3] + SCALARS[5:]:
                    assert int(getattr(b, f)[i]) == int(getattr(a, f)[i]), (c.name, cap, f)
                assert td.partition(b, i) == td.partition(a, i), (c.name, cap)
                assert np.array_equal(b.rec[i, : int(b.rec_len[i])], a.rec[i, : int(a.rec_len[i])])
                stops.add((c.name, steps))
            else:
                assert td.observe(b, i, c) == c.out, (c.name, cap)
            # resumed under the uncapped shape it ends as the uncapped run does
            _same(res, i, full, i, (c.name, "resumed from rec_cap", cap))
        g.check_others(b, b0, r)
    assert len({s for n, s in stops if n == td.CAPREC.name}) == len(td.CAPREC_STOPS), stops
