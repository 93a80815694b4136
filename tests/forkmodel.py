"""A plain NumPy model of mg_lanes_fork's contract (include/mythgpu.h; jumpi_,
instructions.py:1558-1636) over xfermodel.DeviceImage.

`fork` restates the contract with indexing only: per fork, the forkability test,
the jump's ">=" resolution over the host's own disassembly, then the successor
lanes as slices of the source's live rows plus the scalar updates.  It shares no
code with the library: the code tables come from mythril_amd.laser.Disassembly.
Sources are read from a snapshot taken before anything is written, which is the
contract's "as if every source were read first" (the in-place form).
"""
from __future__ import annotations

import numpy as np

from mythril_amd.lanes import (MG_FORK, MG_FORK_BAD_SRC, MG_FORK_MADE_FALL, MG_FORK_MADE_JUMP,
                               MG_FORK_NONE, MG_LANE_HOOK_ACK, MG_LANE_SYMBOLIC, MG_LANE_TAINT, MG_RUNNING)
from mythril_amd.laser import Disassembly
from xfermodel import SCALARS, DeviceImage

JUMPI_GAS = 10
# scalars a successor takes from its source unchanged (the updated ones are written after)
SYM_COUNTS = ("n_nodes", "n_consts")


class CodeTable:
    """What the model needs of a loaded code, from the host's disassembly: the
    byte address and the JUMPDEST-ness of every instruction, and the function
    entries (Disassembly.function_entries)."""

    def __init__(self, code: bytes):
        d = Disassembly(bytes(code))
        self.addrs = [int(ins["address"]) for ins in d.instruction_list]
        self.jumpdest = [ins["opcode"] == "JUMPDEST" for ins in d.instruction_list]
        self.entry = [bool(x) for x in d.function_entries()]
        self.n = len(self.addrs)

    def resolve(self, target: int):
        """The instruction index a jump to byte address `target` lands on when it
        is valid, else None: the first instruction at or past the address (targets
        past the last address resolve to nothing), which must be a JUMPDEST."""
        if self.n == 0 or target > self.addrs[-1]:
            return None
        idx = next(k for k, a in enumerate(self.addrs) if a >= target)
        return idx if self.jumpdest[idx] else None


def forkable(img, s: int, codes) -> bool:
    sp, flags = int(img.sp[s]), int(img.flags[s])
    if int(img.status[s]) != MG_FORK or not flags & MG_LANE_SYMBOLIC or flags & MG_LANE_TAINT:
        return False
    if sp < 2 or sp > img.shape.stack_cap:
        return False
    code = codes.get(int(img.code_id[s]))
    if code is None or int(img.pc[s]) >= code.n:
        return False
    return int(img.stag[s, sp - 1]) == 0 and int(img.stag[s, sp - 2]) != 0


def _successor(img, snap, s: int, d: int, pc: int, fent: int):
    """Lane d of `img` becomes the successor of lane s of `snap` at `pc`."""
    sh = img.shape
    sp = int(snap.sp[s])
    if d != s:
        for f in SCALARS + SYM_COUNTS + (("trace_len",) if sh.trace_cap else ()) + (("rec_len",) if sh.rec_cap else ()):
            getattr(img, f)[d] = getattr(snap, f)[s]
        live = (("stack", sp - 2), ("stag", sp - 2), ("memory", int(snap.msize[s])), ("mtag", int(snap.msize[s])),
                ("storage", int(snap.storage_count[s])), ("sttag", int(snap.storage_count[s])),
                ("node", int(snap.n_nodes[s])), ("cval", int(snap.n_consts[s])))
        live += (("trace", int(snap.trace_len[s])),) if sh.trace_cap else ()
        live += (("rec", int(snap.rec_len[s])),) if sh.rec_cap else ()
        for f, k in live:
            getattr(img, f)[d, :k] = getattr(snap, f)[s, :k]
        img.calldata[d] = snap.calldata[s]
        img.env[d] = snap.env[s]
    img.pc[d] = pc
    img.sp[d] = sp - 2
    img.depth[d] = int(snap.depth[s]) + 1
    img.gas_min[d] = int(snap.gas_min[s]) + JUMPI_GAS
    img.gas_max[d] = int(snap.gas_max[s]) + JUMPI_GAS
    img.steps[d] = int(snap.steps[s]) + 1
    img.status[d] = MG_RUNNING
    img.aux[d] = 0
    img.flags[d] = int(snap.flags[s]) & ~MG_LANE_HOOK_ACK
    img.fent[d] = fent


def fork(model: DeviceImage, codes, src, dst_fall, dst_jump, coverage=None):
    """Apply one mg_lanes_fork to the model's image.  `codes`: code_id -> CodeTable;
    `coverage`: code_id -> uint8 array per instruction, marked when given.
    Returns (made, cond) as the library does.  The arguments must pass the
    library's host-side checks (this is the model of an accepted call)."""
    img = model.img
    snap = img.copy()
    n = len(src)
    made = np.zeros(n, dtype=np.uint32)
    cond = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        s, df, dj = int(src[i]), int(dst_fall[i]), int(dst_jump[i])
        if not forkable(snap, s, codes):
            made[i] = MG_FORK_BAD_SRC
            continue
        code = codes[int(snap.code_id[s])]
        sp, pc, fent = int(snap.sp[s]), int(snap.pc[s]), int(snap.fent[s])
        cond[i] = snap.stag[s, sp - 2]
        if dj != MG_FORK_NONE:
            limbs = [int(x) for x in snap.stack[s, sp - 1]]
            idx = code.resolve(limbs[0]) if not any(limbs[1:]) else None
            if idx is not None:
                _successor(img, snap, s, dj, idx, idx if code.entry[idx] else fent)
                made[i] |= MG_FORK_MADE_JUMP
        if df != MG_FORK_NONE:
            nfent = pc + 1 if pc + 1 < code.n and code.entry[pc + 1] else fent
            _successor(img, snap, s, df, pc + 1, nfent)
            made[i] |= MG_FORK_MADE_FALL
        if coverage is not None and made[i]:
            coverage[int(snap.code_id[s])][pc] = 1
    return made, cond


def live_bytes(img, s: int) -> int:
    """Bytes of lane s a fork copies into one successor in another lane: its
    live rows, calldata, environment words and scalars."""
    sh = img.shape
    sp, ms, sc = int(img.sp[s]) - 2, int(img.msize[s]), int(img.storage_count[s])
    rows = sp * (32 + 4) + ms * (1 + 4) + sc * (64 + 8) + int(img.n_nodes[s]) * 16 + int(img.n_consts[s]) * 32
    rows += (int(img.trace_len[s]) * 4 if sh.trace_cap else 0) + (int(img.rec_len[s]) * 4 if sh.rec_cap else 0)
    return rows + sh.calldata_cap + 5 * 32 + 4 * 22 + 8 * 3

