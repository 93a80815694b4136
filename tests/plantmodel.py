"""A plain NumPy model of mg_harvest_upload (include/mythgpu.h), the mirror of
harvestmodel.download, written from the header's text with fancy indexing only:
no lists on a device, no tiles, no tables.

`upload` restates which device cells take which host cells over a full-capacity
image (xfermodel.DeviceImage) and, with `paths`, over the path planes
(exploremodel.Paths).  Everything it does not assign is what the call must leave.
`reset` restates what mg_lanes_reset restores from the resident image, which the
call does not write.
"""
from __future__ import annotations

import numpy as np

from mythril_amd.lanes import MG_FENT_NONE
from xfermodel import LANE_ROWS, SCALARS, SYM_ROWS, SYM_SCALARS

SYM_LIVE = SYM_ROWS + (("stag", "sp", "stack_cap"), ("mtag", "msize", "mem_cap"), ("sttag", "storage_count", "storage_cap"))
# what the resident reset image holds per lane (mg_lanes_upload's second destinations)
RESET_SCALARS = ("pc", "depth", "status", "aux", "steps", "gas_min", "gas_max", "storage_count")


def _max(a) -> int:
    return int(a.max()) if a.size else 0


def upload(model, lanes, host, paths=None, path_rows=None):
    """One mg_harvest_upload of the host image `host` (symbolic planes when it has
    them) into lanes `lanes` of the DeviceImage `model`.  paths: the device's
    exploremodel.Paths and path_rows = (path [n, path_cap], path_len, root), the
    host's; or both None."""
    d, hs = model.img, host.shape
    idx = np.asarray(lanes, dtype=np.int64)
    assert host.n == idx.size and (np.diff(idx) > 0).all() and (idx.size == 0 or idx[-1] < model.shape.n)
    if idx.size == 0:
        return
    for f in SCALARS:
        getattr(d, f)[idx] = getattr(host, f)
    d.fent[idx] = MG_FENT_NONE if host.fent is None else host.fent
    d.env[idx] = host.env
    d.calldata[idx, :hs.calldata_cap] = host.calldata
    for rows, count, cap in LANE_ROWS:
        hcap = getattr(hs, cap)
        if rows in ("trace", "rec"):
            if not getattr(model.shape, cap):
                continue
            if not hcap:                          # the host keeps no trace / records: none so far
                getattr(d, count)[idx] = 0
                continue
            getattr(d, count)[idx] = getattr(host, count)
        k = min(_max(getattr(host, count)), hcap)
        getattr(d, rows)[idx, :k] = getattr(host, rows)[:, :k]
    if host.symbolic:
        for f in SYM_SCALARS:
            getattr(d, f)[idx] = getattr(host, f)
        for rows, count, cap in SYM_LIVE:
            k = min(_max(getattr(host, count)), getattr(hs, cap))
            getattr(d, rows)[idx, :k] = getattr(host, rows)[:, :k]
    if paths is None:
        return
    path, path_len, root = path_rows
    paths.path_len[idx] = path_len
    paths.root[idx] = root
    k = _max(np.asarray(path_len))
    below = np.arange(k)[None, :] < np.asarray(path_len, dtype=np.int64)[:, None]
    paths.path[idx, :k] = np.where(below, np.asarray(path)[:, :k], 0)


def reset(model, initial):
    """mg_lanes_reset over the DeviceImage `model` whose resident image was left by a
    whole upload of `initial` (empty stacks and memory): the image's scalars and
    storage rows below its counts come back, sp, msize, trace_len and rec_len are
    0 and fent is none; everything else stays."""
    d, n = model.img, initial.n
    for f in RESET_SCALARS:
        getattr(d, f)[:n] = getattr(initial, f)
    d.sp[:n] = 0
    d.msize[:n] = 0
    d.trace_len[:n] = 0
    d.rec_len[:n] = 0
    d.fent[:n] = MG_FENT_NONE
    k = min(_max(initial.storage_count), initial.shape.storage_cap)
    keep = np.arange(k)[None, :] < initial.storage_count.astype(np.int64)[:, None]
    d.storage[:n, :k] = np.where(keep[:, :, None], initial.storage[:, :k], d.storage[:n, :k])
