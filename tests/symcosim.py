"""The co-simulation of symbolic lanes against the CPU restatement, as one
function (tests/test_gpu_symbolic.py and tests/test_gpu_sym_directed.py).

`cosimulate` packs states into one batch (LaserEVM._shape / _pack, with optional
capacity overrides), uploads, steps, downloads, and `check_lanes` decodes every
lane (LaserEVM._materialise), replays its records, steps the restatement
(tests/symref.py) the same number of instructions from the same state and
compares the two: pc, stack node for node, gas, depth, memory bytes (concrete,
symbolic, at symbolic keys) and storage.  What each lane ended as comes back as
a `Lane`, so a caller can assert where and why it stopped."""
from __future__ import annotations

import dataclasses
from collections import Counter
from copy import copy
from typing import Dict, List, Optional

import numpy as np

import symref
from mythril_amd.lanes import (MG_ESCAPE, MG_HALT_RETURN, MG_HALT_REVERT, MG_HALT_STOP, MG_HOOK, MG_LANE_HOOK_ACK,
                               MG_RUNNING, MG_VMEXC, LaneBatch, LaneShape)
from mythril_amd.laser import (Account, BreadthFirstSearchStrategy, ContractCreationTransaction, Disassembly, LaserEVM,
                               MessageCallTransaction, SymbolicCalldata, WorldState)
from mythril_amd.laser import symbolic as sym
from mythril_amd.laser.transaction import ACTORS
from mythril_amd.smt.exponent_manager import exponent_function_manager
from mythril_amd.smt.expr import Or, symbol_factory
from mythril_amd import workloads

CAPS = ("node_cap", "const_cap", "rec_cap", "stack_cap", "storage_cap", "mem_cap")
# a halt or a VmException counts as an executed step but leaves the state at the
# instruction's start (MG_HALT_STOP, _RETURN, _REVERT, _DROPPED, MG_VMEXC)
EXECUTED_HALTS = (1, 2, 3, 5, 6)
_ENDED_AS = {MG_HALT_STOP: "stop", MG_HALT_RETURN: "return", MG_HALT_REVERT: "revert", MG_VMEXC: "exception"}


@dataclasses.dataclass
class Lane:
    status: int
    aux: int
    steps: int
    pc: int
    n_nodes: int
    n_consts: int
    rec_len: int
    storage_count: int
    kinds: Counter            # arena node kind -> count
    kind_widths: Counter      # (arena node kind, width) -> count
    records: list             # LaneBatch.records(i)
    state: object             # the decoded device lane (a GlobalState)
    ref: object               # the restatement's state after the same instructions

    @property
    def reason(self) -> int:
        return self.aux >> 8

    @property
    def op(self) -> int:
        return self.aux & 0xFF


def deploy_code(code: bytes, concrete_storage: bool = False):
    """An account holding `code` at the fixed address (symcases.deploy's RUNTIME
    form): symbolic storage, or concrete (empty: every slot reads 0)."""
    ws = WorldState()
    ws.put_account(Account(ACTORS["CREATOR"], balances=None))
    ws.put_account(Account(workloads.CONTRACT, code=Disassembly(code), concrete_storage=concrete_storage))
    return ws, workloads.CONTRACT


def initial(ws, addr, txid: str = "50", gas_limit: int = 8_000_000, static: bool = False, calldata=None):
    """The first state of a symbolic message call (transaction/symbolic.py:105-150):
    symbolic calldata, caller and call value.  With `calldata` (bytes), the calldata
    is concrete and only the caller and the call value are symbolic."""
    sender = symbol_factory.BitVecSym(f"sender_{txid}", 256)
    tx = MessageCallTransaction(world_state=ws, identifier=txid,
                                gas_price=symbol_factory.BitVecSym(f"gas_price{txid}", 256),
                                gas_limit=gas_limit, origin=sender, caller=sender,
                                callee_account=ws[addr],
                                call_data=SymbolicCalldata(txid) if calldata is None else bytes(calldata),
                                call_value=symbol_factory.BitVecSym(f"call_value{txid}", 256), static=static)
    gs = tx.initial_global_state()
    gs.transaction_stack.append((tx, None))
    gs.world_state.constraints.append(
        Or(*[tx.caller == symbol_factory.BitVecVal(a, 256) for a in ACTORS.values()]))
    return gs


def initial_creation(code: bytes, txid: str = "50", gas_limit: int = 8_000_000):
    """The first state of a symbolic creation of `code` (transaction/symbolic.py:154-219):
    symbolic calldata and call value, the creator as caller."""
    ws = WorldState()
    ws.put_account(Account(ACTORS["CREATOR"], balances=None))
    tx = ContractCreationTransaction(
        world_state=ws, identifier=txid, gas_price=symbol_factory.BitVecSym(f"gas_price{txid}", 256),
        gas_limit=gas_limit, origin=ACTORS["CREATOR"], code=Disassembly(code), caller=ACTORS["CREATOR"],
        call_data=SymbolicCalldata(txid), call_value=symbol_factory.BitVecSym(f"call_value{txid}", 256))
    gs = tx.initial_global_state()
    gs.transaction_stack.append((tx, None))
    gs.world_state.transaction_sequence.append(tx)
    gs.world_state.constraints.append(
        Or(*[tx.caller == symbol_factory.BitVecVal(a, 256) for a in ACTORS.values()]))
    return gs


def new_vm(dev) -> LaserEVM:
    return LaserEVM(requires_statespace=False, device=dev, strategy=BreadthFirstSearchStrategy)


def shape_for(vm, states, caps: Optional[Dict[str, int]] = None) -> LaneShape:
    """LaserEVM._shape's shape with `caps` in place of its capacities.  An override
    below what a packed state already holds would be a refused upload, which is
    not what any test here is about: a ValueError."""
    shape = vm._shape(states)
    if not caps:
        return shape
    bad = set(caps) - set(CAPS)
    if bad:
        raise ValueError(f"not a capacity: {sorted(bad)}")
    shape = dataclasses.replace(shape, **caps)
    for s in states:
        le = vm._encodings.get(id(s))
        need = {"stack_cap": len(s.mstate.stack), "mem_cap": len(s.mstate.memory),
                "storage_cap": s.environment.active_account.storage.n_entries(),
                "node_cap": len(le.enc.nodes) if le is not None else 0,
                "const_cap": len(le.enc.consts) if le is not None else 0}
        for f, n in need.items():
            if getattr(shape, f) < n:
                raise ValueError(f"{f} = {getattr(shape, f)} is below what the packed state holds ({n})")
    return shape


def launch(dev, b: LaneBatch, max_steps: Optional[int] = None, hook_mask=None) -> LaneBatch:
    """Upload `b`, step it and download it.  With `max_steps`, launches of at
    most that many instructions a lane until no lane is left running."""
    dev.alloc(b.shape)
    dev.upload(b)
    if max_steps is None:
        dev.step(hook_mask=hook_mask)
    else:
        for _ in range(1 << 16):
            st = dev.step(hook_mask=hook_mask, max_steps=max_steps)
            if not st.running:
                break
        else:
            raise AssertionError("lanes still running after 65536 launches")
    dev.download(b)
    return b


def pack(vm, states, caps: Optional[Dict[str, int]] = None) -> LaneBatch:
    shape = shape_for(vm, states, caps)
    b = LaneBatch(shape)
    for i, s in enumerate(states):
        vm._pack(b, i, s)
        b.steps[i] = 0
    return b


def resumed(b: LaneBatch, shape: Optional[LaneShape] = None, ack: bool = False) -> LaneBatch:
    """The stopped lanes of a downloaded image set running again, under `shape`
    (larger capacities: LaneBatch.regrown) and, with `ack`, with MG_LANE_HOOK_ACK
    (the host has run the hooks of the instruction at pc)."""
    out = b.regrown(shape) if shape is not None and shape != b.shape else b.copy()
    for i in range(out.n):
        if int(out.status[i]) in (MG_ESCAPE, MG_HOOK):
            if ack and int(out.status[i]) == MG_HOOK:
                out.flags[i] |= MG_LANE_HOOK_ACK
            out.status[i] = MG_RUNNING
            out.aux[i] = 0
    return out


def _replay(b, i, got) -> None:
    # the path constraints LaserEVM's record replay appends (EXP: the
    # exponent manager's condition, instructions.py:624-638), in order
    for r in b.records(i):
        if r[1] == "symexp":
            _, cond = exponent_function_manager.create_condition(*sym.exp_operands(b, i, got, r[2]))
            got.world_state.constraints.append(cond)
        elif r[1] == "exp":
            _, cond = exponent_function_manager.create_condition(
                symbol_factory.BitVecVal(r[2], 256), symbol_factory.BitVecVal(r[3], 256))
            got.world_state.constraints.append(cond)
        elif r[1] == "symlen":          # sha3_ of a symbolic length (:1023-1028)
            got.world_state.constraints.append(sym.decode_node(b, i, got, r[2]) == r[3])
        elif r[1] == "cdsize":          # codesize_ of a creation (:989-997)
            got.world_state.constraints.append(
                got.environment.calldata.size == symbol_factory.BitVecVal(r[2], 256))


def assert_same_state(got, ref, name="") -> None:
    assert got.mstate.pc == ref.mstate.pc, (name, got.mstate.pc, ref.mstate.pc)
    assert [x.raw for x in got.mstate.stack] == [x.raw for x in ref.mstate.stack], (name, got.mstate.pc)
    assert [type(x) for x in got.mstate.stack] == [type(x) for x in ref.mstate.stack]
    assert (got.mstate.min_gas_used, got.mstate.max_gas_used, got.mstate.depth) == \
        (ref.mstate.min_gas_used, ref.mstate.max_gas_used, ref.mstate.depth)
    assert got.mstate.memory.raw() == ref.mstate.memory.raw()
    assert {p: e.raw for p, e in got.mstate.memory.symbolic_bytes().items()} == \
        {p: e.raw for p, e in ref.mstate.memory.symbolic_bytes().items()}
    # bytes at symbolic keys (MG_SYM_MSTOREK events), values and write order
    assert [(k, v if isinstance(v, int) else v.raw)
            for k, v in got.mstate.memory.symbolic_key_bytes().items()] == \
        [(k, v if isinstance(v, int) else v.raw) for k, v in ref.mstate.memory.symbolic_key_bytes().items()]
    gst, rst = got.environment.active_account.storage, ref.environment.active_account.storage
    if rst.is_chain:
        assert [(k.raw, v.raw) for k, v in gst.chain()] == [(k.raw, v.raw) for k, v in rst.chain()]
    else:
        assert gst.slots() == rst.slots()


def check_lanes(vm, eng, b: LaneBatch, states, name="", constraints: bool = False,
                trail: Optional[list] = None) -> List[Lane]:
    """Decode every lane of the downloaded image `b` (packed from `states`), step
    the restatement as many instructions from the same state, compare them, and
    return what each lane ended as.  With `constraints`, the path constraints
    the records replay to must be the restatement's too, and a lane that halted
    or raised must be at an instruction where the restatement ends the same way.
    `trail` (for batches of one state run again and again): the restatement's
    states so far, trail[k] after k instructions, extended as needed."""
    out = []
    if trail is not None:
        assert len(states) == 1
        if not trail:
            trail.append(states[0])
        assert trail[0] is states[0]
    for i, s0 in enumerate(states):
        n = int(b.steps[i])
        st = int(b.status[i])
        got = vm._materialise(b, i, copy(s0))
        _replay(b, i, got)
        # the restatement: the same state, the same number of instructions (a
        # halt or VmException counts as a step but leaves the state at its start)
        n_ref = n - (1 if st in EXECUTED_HALTS else 0)
        ref = s0 if trail is None else trail[min(n_ref, len(trail) - 1)]
        for _ in range(n_ref if trail is None else n_ref - (len(trail) - 1)):
            succ = eng.step(ref)
            assert len(succ) == 1, (name, "the restatement forked or ended inside a device run")
            ref = succ[0]
            if trail is not None:
                trail.append(ref)
        assert_same_state(got, ref, name)
        if constraints:
            assert [c.raw for c in got.world_state.constraints] == [c.raw for c in ref.world_state.constraints], name
            if st in _ENDED_AS:
                before = len(eng.ended)
                assert eng.step(ref) == [] and len(eng.ended) == before + 1 and \
                    eng.ended[-1][0] == _ENDED_AS[st], (name, st, eng.ended[before:])
        nn = int(b.n_nodes[i]) if b.symbolic else 0
        heads = np.asarray(b.node[i, :nn, 0]) if nn else np.zeros(0, dtype=np.uint32)
        out.append(Lane(status=st, aux=int(b.aux[i]), steps=n, pc=int(b.pc[i]), n_nodes=nn,
                        n_consts=int(b.n_consts[i]) if b.symbolic else 0, rec_len=int(b.rec_len[i]),
                        storage_count=int(b.storage_count[i]),
                        kinds=Counter((heads & 0xFF).tolist()),
                        kind_widths=Counter(zip((heads & 0xFF).tolist(), (heads >> 8).tolist())),
                        records=b.records(i), state=got, ref=ref))
    return out


def cosimulate(dev, states, caps: Optional[Dict[str, int]] = None, max_steps: Optional[int] = None, hook_mask=None,
               vm=None, eng=None, name="", constraints: bool = False):
    """One batch of `states` through the device and the restatement.  Returns
    (the lanes, the downloaded image)."""
    vm = vm or new_vm(dev)
    eng = eng or symref.Engine()
    b = launch(dev, pack(vm, states, caps), max_steps, hook_mask)
    return check_lanes(vm, eng, b, states, name, constraints), b
