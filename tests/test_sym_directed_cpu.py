"""The directed symbolic-lane cases (tests/symdirect.py) pinned without a GPU:
every program disassembles into its source, the restatement (tests/symref.py)
runs it to the stated instruction count and outcome, the stated arena node
kinds follow from the terms the restatement builds, the gas sweep's limits are
the restatement's own cumulative values, and four cases carry hand-worked
expected terms with the reference lines that justify them."""
import pytest

import symdirect
from mythril_amd.lanes import (MG_ESC_SYMBOLIC, MG_ESCAPE, MG_EXC_OUT_OF_GAS, MG_FORK, MG_HALT_RETURN, MG_HALT_STOP,
                               MG_VMEXC)
from mythril_amd.laser import Disassembly
from mythril_amd.laser.symbolic import (MG_SYM_CDBYTE, MG_SYM_CDBYTEX, MG_SYM_CDLOAD, MG_SYM_CDSIZE, MG_SYM_CONCAT,
                                        MG_SYM_ENV, MG_SYM_EXTRACT, MG_SYM_KECCAK, MG_SYM_SLOAD)
from mythril_amd.smt.expr import Node, const, var

NAMES = [c.name for c in symdirect.ALL]


@pytest.fixture(scope="module")
def runs():
    """name -> (states before each instruction, how the restatement ended)."""
    return {c.name: symdirect.restate(c) for c in symdirect.ALL}


@pytest.mark.parametrize("name", NAMES)
def test_every_program_disassembles_into_its_source(name):
    case = symdirect.BY_NAME[name]
    toks = case.src.split()
    want, k = [], 0
    while k < len(toks):
        want.append((toks[k], int(toks[k + 1], 0)) if toks[k].startswith("PUSH") else (toks[k], None))
        k += 2 if toks[k].startswith("PUSH") else 1
    got = [(i["opcode"], int(i["argument"], 16) if "argument" in i else None)
           for i in Disassembly(case.code).instruction_list]
    assert got == want
    assert len(got) == symdirect.n_instructions(case.src) >= case.steps - 1


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_runs_the_case_to_its_stated_outcome(runs, name):
    case = symdirect.BY_NAME[name]
    states, end = runs[name]
    n = len(states) - 1
    if case.status in (MG_HALT_STOP, MG_HALT_RETURN):
        # the halt counts as a device step and leaves the state at its start
        assert (n, end) == (case.steps - 1, "stop" if case.status == MG_HALT_STOP else "return")
    elif case.status == MG_VMEXC:
        assert (n, end) == (case.steps - 1, "exception")
    elif case.status == MG_FORK:
        assert (n, end) == (case.steps, "fork")
    else:
        # an escape: the device stops before an instruction that is the host's.  The
        # restatement has no semantics for it, or runs it (a Bool operand: the
        # reference's stack holds If(b, 1, 0), machine_state.py:29-56, and only the
        # device tells the two apart); a smaller stack plane is no limit of the reference
        assert case.status == MG_ESCAPE
        assert n >= case.steps and (n > case.steps or end == "unsupported")
        assert (n == case.steps and end == "unsupported") == (name in symdirect.NO_RESTATEMENT)
        op = states[case.steps].environment.code.instruction_list[states[case.steps].mstate.pc]["opcode"]
        assert symdirect._BYTE_OF[op] == case.aux & 0xFF


def _terms(states):
    """Every term node the run shows: each instruction's new top of stack, the
    symbolic memory bytes and the storage chain of every state."""
    seen, work = set(), []
    for s in states:
        if s.mstate.stack:
            work.append(s.mstate.stack[-1].raw)
        work.extend(e.raw for e in s.mstate.memory.symbolic_bytes().values())
        st = s.environment.active_account.storage
        if st.is_chain:
            for k, v in st.chain():
                work += [k.raw, v.raw]
    while work:
        n = work.pop()
        if n in seen:
            continue
        seen.add(n)
        work.extend(n.args)
    return seen


# what an arena node kind looks like in the host's terms (the others -- BIN, UN,
# BALANCE, the MSTOREK / MLOADK events -- have no one shape there)
_SHAPE = {
    MG_SYM_EXTRACT: lambda n, w: n.op == "extract" and n.width == w,
    MG_SYM_CONCAT: lambda n, w: n.op == "concat" and n.width == w,
    MG_SYM_KECCAK: lambda n, w: n.op == "uf" and n.param[0].startswith("keccak256_"),
    MG_SYM_SLOAD: lambda n, w: n.op == "select" and n.width == 256,
    MG_SYM_CDBYTE: lambda n, w: n.op == "select" and n.width == 8,
    MG_SYM_CDBYTEX: lambda n, w: n.op == "select" and n.width == 8 and n.args[1].op != "const",
    MG_SYM_CDLOAD: lambda n, w: n.op == "select" and n.width == 8,
    MG_SYM_CDSIZE: lambda n, w: n.op == "var" and n.param.endswith("calldatasize"),
    MG_SYM_ENV: lambda n, w: n.op == "var",
}


@pytest.mark.parametrize("name", NAMES)
def test_the_stated_node_kinds_follow_from_the_restatements_terms(runs, name):
    case = symdirect.BY_NAME[name]
    terms = _terms(runs[name][0])
    device_only = symdirect.DEVICE_ONLY.get(name, [])
    for kind, width in case.kinds:
        if (kind, width) in device_only or kind not in _SHAPE:
            continue
        assert any(_SHAPE[kind](n, width) for n in terms), (name, kind, width)
    # the records: a SHA3 of symbolic data, a symbolic EXP, a symbolic SHA3 length
    if "symkeccak" in case.records:
        assert any(n.op == "uf" and n.param[0].startswith("keccak256_") for n in terms)
    if "symexp" in case.records:
        assert any(n.op == "uf" and n.param[0] == "Power" for n in terms)
    if "cdsize" in case.records:
        cons = runs[name][0][-1].world_state.constraints
        assert any(c.raw.op == "eq" and any(a.op == "var" and a.param.endswith("calldatasize") for a in c.raw.args)
                   for c in cons)
    if "symlen" in case.records:
        cons = runs[name][0][-1].world_state.constraints
        assert any(c.raw.op == "eq" and const(64, 256) in c.raw.args for c in cons)


@pytest.mark.parametrize("name", [c.name for c in symdirect.GAS_SWEPT])
def test_the_gas_limits_are_the_restatements_cumulative_values(runs, name):
    case = symdirect.BY_NAME[name]
    states, _ = runs[name]
    limits = symdirect.gas_limits(case)
    reached = sorted({s.mstate.min_gas_used for s in states} - {0})
    assert set(limits) == {c + d for c in reached for d in (-1, 0, 1)} - {0}
    # an instruction that takes the gas to c runs out at the limits c - 1 and c
    # (`min_gas_used >= gas_limit`, machine_state.py check_gas) and runs at c + 1
    for k in range(1, len(states)):
        c = states[k].mstate.min_gas_used
        if c == states[k - 1].mstate.min_gas_used:
            continue
        # ... but for a JUMPI to a symbolic target, whose gas jumpi_ adds by hand with no
        # check (instructions.py:1572-1579): the next instruction's check raises
        ins = states[k - 1].environment.code.instruction_list[states[k - 1].mstate.pc]["opcode"]
        late = 1 if ins == "JUMPI" else 0
        assert len(symdirect.restate(case, c)[0]) == k + late, (name, k, c)
        assert len(symdirect.restate(case, c + 1)[0]) > k, (name, k, c)
        steps, status, aux = symdirect.expected_under_gas(case, c)
        assert (steps, status, aux) in ((k + late, MG_VMEXC, MG_EXC_OUT_OF_GAS),
                                        (k - 1, MG_ESCAPE, 0x20 | MG_ESC_SYMBOLIC << 8))
    assert symdirect.expected_under_gas(case, 8_000_000) == (case.steps, case.status, case.aux)


# ---- hand-worked terms ----------------------------------------------------------------
def _top_after(src: str, n: int, **kw):
    """The top of the stack after n instructions of the program."""
    states, _ = symdirect.restate(symdirect.Case("hand", src, 0, MG_HALT_STOP, **kw))
    return states[n].mstate.stack[-1].raw


SENDER, VALUE = var("sender_50", 256), var("call_value50", 256)


def test_mload_at_5_over_a_word_stored_at_0():
    # memory.py:56-82 get_word_at: simplify(Concat(bytes 5..36)); bytes 5..31 are
    # Extract(255 - 8j, 248 - 8j, caller), j = 5..31 (write_word_at, :102-115), which
    # simplify joins into Extract(215, 0, caller); bytes 32..36 are zeros
    got = _top_after("CALLER PUSH1 0 MSTORE PUSH1 5 MLOAD STOP", 5)
    want = Node("concat", 256, (Node("extract", 216, (SENDER,), (215, 0)), const(0, 40)))
    assert got is want


def test_sload_after_a_symbolic_and_a_constant_store():
    # account.py:75 Storage.__getitem__: simplify(Select(Store(Store(base, x, v), k, w), .)):
    # at k the newest store answers w; at x the store at the constant k neither equals
    # nor provably differs from x, so the Select stays over the whole chain
    src = "PUSH1 0 CALLDATALOAD CALLVALUE DUP2 SSTORE PUSH1 9 PUSH1 3 SSTORE PUSH1 3 SLOAD DUP2 SLOAD STOP"
    x = _top_after(src, 2)
    assert _top_after(src, 10) is const(9, 256)
    got = _top_after(src, 12)
    assert got.op == "select" and got.args[1] is x
    outer = got.args[0]
    assert outer.op == "store" and outer.args[1] is const(3, 256) and outer.args[2] is const(9, 256)
    inner = outer.args[0]
    assert inner.op == "store" and inner.args[1] is x and inner.args[2] is VALUE and inner.args[0].op == "array"


def test_x_eq_x_folds_to_one():
    # eq_ (instructions.py:721-745) pushes the Bool op1 == op2; z3 builds x == x as True,
    # and the stack holds If(True, 1, 0) = 1 (machine_state.py:29-56)
    assert _top_after("CALLVALUE DUP1 EQ STOP", 3) is const(1, 256)
    assert _top_after("CALLVALUE CALLVALUE EQ STOP", 3) is const(1, 256)
    assert _top_after("CALLER CALLVALUE EQ STOP", 3).op == "ite"


def test_div_by_a_concrete_zero_is_zero():
    # div_ (instructions.py:505-519): `if op1 == 0: push 0`, for a concrete divisor only
    assert _top_after("PUSH1 0 CALLVALUE DIV STOP", 3) is const(0, 256)
    assert _top_after("CALLER CALLVALUE DIV STOP", 3).op != "const"
