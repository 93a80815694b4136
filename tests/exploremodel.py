"""A plain NumPy model of mg_explore's plan and path record (include/mythgpu.h)
over xfermodel.DeviceImage, on top of forkmodel (mg_lanes_fork's model, which it
imports and does not change).

`plan` restates the contract's plan of one round with loops over lanes in
ascending order: no ranks, no scans.  `commit_paths` restates the path record.
`round_` puts a round's fork together: plan, forkmodel.fork, commit_paths (the
stepping is the device's or the caller's).
"""
from __future__ import annotations

import numpy as np

import forkmodel
from mythril_amd.lanes import MG_FORK_MADE_JUMP, MG_FORK_NONE


class Paths:
    """The path planes: path[lane, entry], path_len[lane], root[lane], as
    mg_explore leaves them at its start."""

    def __init__(self, n: int, path_cap: int):
        self.path_cap = path_cap
        self.path = np.zeros((n, path_cap), dtype=np.uint32)
        self.path_len = np.zeros(n, dtype=np.uint32)
        self.root = np.arange(n, dtype=np.uint32)

    def copy(self):
        p = Paths(self.root.size, self.path_cap)
        p.path, p.path_len, p.root = self.path.copy(), self.path_len.copy(), self.root.copy()
        return p


def jump_valid(img, s: int, codes) -> bool:
    code = codes[int(img.code_id[s])]
    limbs = [int(x) for x in img.stack[s, int(img.sp[s]) - 1]]
    return not any(limbs[1:]) and code.resolve(limbs[0]) is not None


def plan(img, codes, free, used: int, path_len, path_cap: int):
    """The plan of one round over image `img`: (src, dst_fall, dst_jump, starved,
    path_full); the first three are mg_lanes_fork's arguments, the last two the
    lanes left untouched for want of a free lane / of room in their path."""
    free = [int(x) for x in free]
    unused = set(free[used:])
    nxt = used
    src, dst_jump, starved, path_full = [], [], [], []
    for s in range(img.shape.n):
        if s in unused or not forkmodel.forkable(img, s, codes):
            continue
        if int(path_len[s]) >= path_cap:
            path_full.append(s)
        elif not jump_valid(img, s, codes):
            src.append(s), dst_jump.append(MG_FORK_NONE)
        elif nxt < len(free):
            src.append(s), dst_jump.append(free[nxt])
            nxt += 1
        else:
            starved.append(s)
    u32 = lambda xs: np.array(xs, dtype=np.uint32)
    return u32(src), u32(src), u32(dst_jump), u32(starved), u32(path_full)


def commit_paths(paths: Paths, src, dst_jump, made, cond) -> None:
    """The path record of the forks a round made (made / cond: mg_lanes_fork's answers)."""
    for s, dj, m, c in zip(src, dst_jump, made, cond):
        s, dj, m, c = int(s), int(dj), int(m), int(c)
        k = int(paths.path_len[s])
        if m & MG_FORK_MADE_JUMP:
            paths.path[dj] = 0
            paths.path[dj, :k] = paths.path[s, :k]
            paths.path[dj, k] = c << 1 | 1
            paths.path_len[dj] = k + 1
            paths.root[dj] = paths.root[s]
        paths.path[s, k] = c << 1
        paths.path_len[s] = k + 1


def round_(model, codes, free, used: int, paths: Paths, coverage=None):
    """Plan and fork the stepped image of `model` (a DeviceImage).  Returns the
    plan and the number of free lanes used after it."""
    p = plan(model.img, codes, free, used, paths.path_len, paths.path_cap)
    src, dst_fall, dst_jump = p[:3]
    made, cond = forkmodel.fork(model, codes, src, dst_fall, dst_jump, coverage=coverage)
    commit_paths(paths, src, dst_jump, made, cond)
    return p, used + int((dst_jump != MG_FORK_NONE).sum())
