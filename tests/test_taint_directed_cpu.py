"""The directed taint cases (tests/taintdirect.py) without a GPU: the restatement
over the C oracle (tests/taintref.py through tests/oracle_device.py) must end
every case in its hand-written outcome, and the table must cover what it says it
covers.  tests/test_gpu_taint_directed.py runs the same table on the device."""
import numpy as np
import pytest

import taintdirect as td
from mythril_amd.lanes import MG_ESC_RECORD, MG_ESCAPE, MG_RUNNING, MG_TAINT_OBJ0
from mythril_amd.laser.opcodes import OPCODES
from taintref import UNION2, ZERODIV


@pytest.mark.parametrize("family", list(td.FAMILIES))
def test_restatement_ends_in_the_hand_written_outcome(family):
    for cases in td.groups(td.FAMILIES[family]):
        watch = {}
        b = td.restated(cases, watch=watch)
        for i, c in enumerate(cases):
            assert td.observe(b, i, c) == c.out, (c.name, td.observe(b, i, c), c.out)
            td.check_pins(b, i, c)
            # no case passes by doing nothing: it reaches an opcode with an action
            # word, or an object table that has to be compacted
            w = watch.get(i, {})
            assert w.get("reached", 0) > 0 or w.get("nobj_peak", 0) + 4 > c.obj_cap, (c.name, w)


def test_compaction_cases_compact_and_end_alike_without_it():
    cases = td.FAMILIES["compaction"]
    assert all(MG_TAINT_OBJ0 + 5 <= c.obj_cap <= 16 for c in cases)
    watch = {}
    b = td.restated(cases, watch=watch, obj_cap=64)
    for i, c in enumerate(cases):
        want = c.out_uncapped or c.out
        assert (c.out_uncapped is not None) == (c.name in td.GC_ESCAPES)
        assert td.observe(b, i, c, want) == want, (c.name, td.observe(b, i, c, want), want)
        td.check_pins(b, i, c)
        # handles the device takes without compaction: past what the small table allows
        assert watch[i]["nobj_peak"] > c.obj_cap - 4, (c.name, watch[i])


def test_the_table_covers_every_result_rule():
    ops = {tok for c in td.FAMILIES["result"] for tok in c.src.split()}
    for b in sorted(UNION2 | ZERODIV | {0x08, 0x09, 0x15, 0x19, 0x1A}):
        name = next(n for n, v in OPCODES.items() if v == b)
        assert name in ops, name
    names = set(td.BY_NAME)
    for n in ("none", "0", "1", "0_1"):
        assert f"u2_gt_{n}" in names and f"div0_sdiv_{n}" in names and f"div3_smod_{n}" in names
    assert {"mod0_addmod_2", "mod5_mulmod_2", "mod0_mulmod_none", "idx100000000_byte_1",
            "idx10000000000000005_byte_1", "exp_100000000_1", "exp_100000001_100000000"} <= names
    for c in td.FAMILIES["result"]:
        if c.name.endswith("_none"):
            assert c.out.stack == ((0, 0),) and c.dev_n_obj == MG_TAINT_OBJ0 + 1, c.name


def test_the_default_actions_are_those_of_the_taint_test():
    import test_gpu_taint
    assert np.array_equal(td.action_words(td.DEFAULT_ACTIONS), test_gpu_taint.ACTIONS)


def test_record_capacity_sweep_of_the_restatement():
    """Around every cumulative record length: the lane stops before the first
    instruction whose records do not fit all at once, with nothing written."""
    case = td.CAPREC
    lens = sorted({w for w, _ in td.CAPREC_STOPS})
    for cap in sorted({c for w in lens for c in (w - 1, w, w + 1)}):
        b = td.restated([case], rec_cap=cap)
        steps = td.caprec_steps(cap)
        assert int(b.steps[0]) == steps, (cap, int(b.steps[0]), steps)
        if steps == case.out.steps:
            assert td.observe(b, 0, case) == case.out
        else:
            assert (int(b.status[0]), int(b.aux[0]) >> 8) == (MG_ESCAPE, MG_ESC_RECORD), cap
            k = [s for _, s in td.CAPREC_STOPS].index(steps)
            assert int(b.rec_len[0]) == ([0] + lens)[k], (cap, int(b.rec_len[0]))
            assert td.record_kinds(b, 0) == case.out.records[:len(td.record_kinds(b, 0))]


def test_slices_of_the_restatement_equal_one_run():
    # one instruction a launch ends every case as one launch does
    for family, all_cases in td.FAMILIES.items():
        if family in ("result", "fresh"):
            all_cases = all_cases[::7]
        for cases in td.groups(all_cases):
            b = td.restated(cases, max_steps=1, launches=max(c.out.steps for c in cases) + 2)
            for i, c in enumerate(cases):
                assert int(b.status[i]) != MG_RUNNING
                assert td.observe(b, i, c) == c.out, (c.name, td.observe(b, i, c), c.out)
