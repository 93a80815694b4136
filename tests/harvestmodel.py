"""A plain NumPy model of mg_harvest_select, mg_harvest_download and
mg_explore_resume (include/mythgpu.h), written from the header's text with
slicing and fancy indexing only: no ranks, no scans, no tiles.

`select` restates which lanes match and the eight maxima over a full-capacity
image (xfermodel.DeviceImage's `img`).  `download` restates which host cells
take which device cells.  `explore` is exploremodel's round in a loop, with the
path reset of mg_explore or, for mg_explore_resume, without it; the stepping is
the caller's.
"""
from __future__ import annotations

import numpy as np

import exploremodel
from mythril_amd.lanes import MG_RUNNING
from xfermodel import LANE_ROWS, SCALARS, SYM_ROWS, SYM_SCALARS

FIELDS = ("sp", "msize", "storage_count", "trace_len", "rec_len", "n_nodes", "n_consts", "path_len")
NEVER_UPLOADED = 0xFFFFFFFF


class Info:
    """mg_harvest_info without kernel_ms."""

    def __init__(self, n=0, matched=0, **maxima):
        self.n, self.matched = n, matched
        for f in FIELDS:
            setattr(self, f, int(maxima.get(f, 0)))

    def key(self):
        return (self.n, self.matched) + tuple(getattr(self, f) for f in FIELDS)


def select(img, status_mask: int, skip=(), max_lanes=None, path_len=None):
    """(lanes, Info) of one mg_harvest_select over the image `img`; path_len: the
    path_len plane, or None without explore planes."""
    sh = img.shape
    skipped = set(int(x) for x in skip)
    matching = [l for l in range(sh.n)
                if int(img.status[l]) < 32 and status_mask >> int(img.status[l]) & 1 and l not in skipped]
    cap = sh.n if max_lanes is None else min(int(max_lanes), sh.n)
    lanes = np.array(matching[:cap], dtype=np.uint32)
    present = {"sp": img.sp, "msize": img.msize, "storage_count": img.storage_count,
               "trace_len": img.trace_len if sh.trace_cap else None, "rec_len": img.rec_len if sh.rec_cap else None,
               "n_nodes": img.n_nodes if sh.node_cap else None, "n_consts": img.n_consts if sh.node_cap else None,
               "path_len": path_len}
    maxima = {f: int(a[lanes].max()) if a is not None and lanes.size else 0 for f, a in present.items()}
    return lanes, Info(len(lanes), len(matching), **maxima)


def download(model, lanes, info: Info, host, paths=None):
    """One mg_harvest_download from the DeviceImage `model` into the host image
    `host` (host.n == info.n; symbolic planes when it has them); paths: an
    exploremodel.Paths, or None.  Returns (path, path_len, root) or None."""
    d, hs = model.img, host.shape
    idx = np.asarray(lanes, dtype=np.int64)
    assert host.n == info.n == idx.size
    if idx.size == 0:
        return None
    for f in SCALARS:
        getattr(host, f)[:] = getattr(d, f)[idx]
    if host.fent is not None:
        host.fent[:] = d.fent[idx]
    host.env[:] = d.env[idx]
    host.calldata[:] = d.calldata[idx, :hs.calldata_cap]
    bound = {"sp": info.sp, "storage_count": info.storage_count, "msize": info.msize, "trace_len": info.trace_len,
             "rec_len": info.rec_len, "n_nodes": info.n_nodes, "n_consts": info.n_consts}
    for rows, count, cap in LANE_ROWS:
        hcap = getattr(hs, cap)
        if rows in ("trace", "rec"):
            if not hcap:
                continue
            getattr(host, count)[:] = getattr(d, count)[idx]
        k = min(bound[count], hcap)
        getattr(host, rows)[:, :k] = getattr(d, rows)[idx, :k]
    if host.symbolic:
        for f in SYM_SCALARS:
            getattr(host, f)[:] = getattr(d, f)[idx]
        for rows, count, cap in SYM_ROWS + (("stag", "sp", "stack_cap"), ("mtag", "msize", "mem_cap"),
                                            ("sttag", "storage_count", "storage_cap")):
            k = min(bound[count], getattr(hs, cap))
            getattr(host, rows)[:, :k] = getattr(d, rows)[idx, :k]
    if paths is None:
        return None
    path = np.zeros((idx.size, paths.path_cap), dtype=np.uint32)
    for i, l in enumerate(idx):
        k = int(paths.path_len[l])
        path[i, :k] = paths.path[l, :k]
    return path, paths.path_len[idx].copy(), paths.root[idx].copy()


def explore(model, codes, free, paths: exploremodel.Paths, max_rounds: int, step, resume: bool):
    """mg_explore (resume=False: every lane's root and path restart) or
    mg_explore_resume (they stay) over the DeviceImage `model`: up to max_rounds
    rounds of step(model.img) -- the caller's stepping rule -- and exploremodel's
    planned fork.  Returns (rounds, forks, free_used, starved of the last round)."""
    if not resume:
        paths.path[...] = 0
        paths.path_len[:] = 0
        paths.root[:] = np.arange(paths.root.size, dtype=np.uint32)
    used = rounds = forks = 0
    starved = np.zeros(0, dtype=np.uint32)
    for _ in range(max_rounds):
        step(model.img)
        running = int((model.img.status == MG_RUNNING).sum())
        (src, _, dst_jump, starved, _), used = exploremodel.round_(model, codes, free, used, paths)
        rounds += 1
        forks += len(src)
        if not len(src) and not running:
            break
    return rounds, forks, used, starved


def merge_free(free, lanes):
    """The caller's free list after it took the harvested lanes: ascending."""
    return sorted(set(int(x) for x in free) | set(int(x) for x in lanes))

