"""A plain NumPy model of the lane-transfer contract (include/mythgpu.h:
mg_lanes_upload / _upload_live / _download / _download_live, mg_sym_* and
mg_taint_* transfers; DESIGN.md §3.3 "only live rows cross PCIe").

`DeviceImage` holds what the device holds: one full-capacity lane-major array
per field of the allocated shape.  `upload` and `download` restate the
documented contract with slicing only -- no tiles, no transposes, no byte
swaps -- so a transfer kernel that drops `first`, mishandles a tile edge, takes
a bound from the wrong array or writes a slim host image at the wrong stride
differs from it in some cell.

Host images are LaneBatch objects of any capacities up to the device's.  A
host image "passes no fent" when its `fent` attribute is None.
"""
from __future__ import annotations

import numpy as np

from mythril_amd.lanes import (_SYM_FIELDS, _TAINT_FIELDS, _U32_FIELDS, _U64_FIELDS, MG_FENT_NONE,
                               MG_HALT_STOP, MG_TAINT_MAX_ATOMS, MG_TAINT_OBJ0, LaneBatch, LaneShape)

# scalars every lane transfer moves (trace_len / rec_len / fent have rules of their own)
SCALARS = tuple(f for f in _U32_FIELDS + _U64_FIELDS if f not in ("trace_len", "rec_len", "fent"))
# row fields bounded by a count: (rows, count, capacity attribute of the shape)
LANE_ROWS = (("stack", "sp", "stack_cap"), ("storage", "storage_count", "storage_cap"),
             ("memory", "msize", "mem_cap"), ("trace", "trace_len", "trace_cap"), ("rec", "rec_len", "rec_cap"))
SYM_SCALARS = ("n_nodes", "n_consts")
SYM_ROWS = (("node", "n_nodes", "node_cap"), ("cval", "n_consts", "const_cap"))
SYM_WHOLE = (("stag", "stack_cap"), ("mtag", "mem_cap"), ("sttag", "storage_cap"))
TAINT_SCALARS = ("n_obj", "n_fixed", "n_atoms", "tflags", "sink", "ymask")
TAINT_ROWS = (("omask", "n_obj", "obj_cap"),)
TAINT_WHOLE = (("sobj", "stack_cap"),)


def fields_of(shape: LaneShape) -> tuple:
    """Every array of an image of this shape that a transfer can move."""
    out = list(SCALARS) + ["fent", "env", "calldata", "stack", "storage", "memory"]
    if shape.trace_cap:
        out += ["trace_len", "trace"]
    if shape.rec_cap:
        out += ["rec_len", "rec"]
    if shape.node_cap:
        out += list(_SYM_FIELDS)
    if shape.obj_cap:
        out += list(_TAINT_FIELDS)
    return tuple(out)


def _max(counts) -> int:
    return int(counts.max()) if counts.size else 0


class DeviceImage:
    def __init__(self, shape: LaneShape):
        self.shape = shape
        self.img = LaneBatch(shape)

    # ------------------------------------------------------------------ upload
    def upload(self, host: LaneBatch, first: int, n: int, host_first=None, live: bool = False):
        """Host lanes [host_first, host_first + n) to device lanes [first, first + n).
        `live` makes no difference: every upload is bounded by the range's counts."""
        hf = first if host_first is None else host_first
        d, h, hs = self.img, slice(hf, hf + n), host.shape
        dl = slice(first, first + n)
        if n == 0:
            return
        for f in SCALARS:
            getattr(d, f)[dl] = getattr(host, f)[h]
        d.fent[dl] = MG_FENT_NONE if host.fent is None else host.fent[h]
        d.env[dl] = host.env[h]
        d.calldata[dl, :hs.calldata_cap] = host.calldata[h]
        for rows, count, cap in LANE_ROWS:
            hcap = getattr(hs, cap)
            if rows in ("trace", "rec"):
                if not getattr(self.shape, cap):
                    continue
                if not hcap:                      # the host keeps no trace / records: none so far
                    getattr(d, count)[dl] = 0
                    continue
                getattr(d, count)[dl] = getattr(host, count)[h]
            k = min(_max(getattr(host, count)[h]), hcap)
            getattr(d, rows)[dl, :k] = getattr(host, rows)[h, :k]
        if self.shape.node_cap and host.symbolic:
            self._planes_up(host, h, dl, SYM_SCALARS, SYM_ROWS, SYM_WHOLE)
        if self.shape.obj_cap and host.taint:
            self._planes_up(host, h, dl, TAINT_SCALARS, TAINT_ROWS, TAINT_WHOLE)

    def _planes_up(self, host, h, dl, scalars, bounded, whole):
        d, hs = self.img, host.shape
        for f in scalars:
            getattr(d, f)[dl] = getattr(host, f)[h]
        for rows, count, cap in bounded:
            k = min(_max(getattr(host, count)[h]), getattr(hs, cap))
            getattr(d, rows)[dl, :k] = getattr(host, rows)[h, :k]
        for rows, cap in whole:
            k = getattr(hs, cap)
            getattr(d, rows)[dl, :k] = getattr(host, rows)[h, :k]

    # ---------------------------------------------------------------- download
    def download(self, host: LaneBatch, first: int, n: int, host_first=None, live: bool = False):
        """Device lanes [first, first + n) into host lanes [host_first, host_first + n).
        Non-live: every row up to the host's capacities, env and calldata.  Live:
        rows below the range's largest device count (clipped to the host's
        capacity); the host's cells above it, its env and calldata stay."""
        hf = first if host_first is None else host_first
        d, h, hs = self.img, slice(hf, hf + n), host.shape
        dl = slice(first, first + n)
        if n == 0:
            return
        for f in SCALARS:
            getattr(host, f)[h] = getattr(d, f)[dl]
        if host.fent is not None:
            host.fent[h] = d.fent[dl]
        if not live:
            host.env[h] = d.env[dl]
            host.calldata[h] = d.calldata[dl, :hs.calldata_cap]
        for rows, count, cap in LANE_ROWS:
            hcap = getattr(hs, cap)
            if rows in ("trace", "rec"):
                if not hcap:
                    continue
                getattr(host, count)[h] = getattr(d, count)[dl]
            k = min(_max(getattr(d, count)[dl]), hcap) if live else hcap
            getattr(host, rows)[h, :k] = getattr(d, rows)[dl, :k]
        # the arena and the object table are always bounded by the device's counts
        if self.shape.node_cap and host.symbolic:
            self._planes_down(host, h, dl, SYM_SCALARS, SYM_ROWS, SYM_WHOLE)
        if self.shape.obj_cap and host.taint:
            self._planes_down(host, h, dl, TAINT_SCALARS, TAINT_ROWS, TAINT_WHOLE)

    def _planes_down(self, host, h, dl, scalars, bounded, whole):
        d, hs = self.img, host.shape
        for f in scalars:
            getattr(host, f)[h] = getattr(d, f)[dl]
        for rows, count, cap in bounded:
            k = min(_max(getattr(d, count)[dl]), getattr(hs, cap))
            getattr(host, rows)[h, :k] = getattr(d, rows)[dl, :k]
        for rows, cap in whole:
            k = getattr(hs, cap)
            getattr(host, rows)[h, :k] = getattr(d, rows)[dl, :k]


# ------------------------------------------------------------------- helpers
def _random(rng, arr):
    if arr.dtype == np.uint8:
        arr[...] = rng.integers(0, 256, size=arr.shape, dtype=np.uint8)
    elif arr.dtype == np.uint32:
        arr[...] = rng.integers(0, 1 << 32, size=arr.shape, dtype=np.uint32)
    else:
        arr[...] = rng.integers(0, 1 << 64, size=arr.shape, dtype=np.uint64)


def saturated(shape: LaneShape, rng, code_id: int) -> LaneBatch:
    """A batch that makes the whole device image known and dirty: every lane
    halted (MG_HALT_STOP), every count at its capacity, every row random."""
    b = LaneBatch(shape)
    for f in ("pc", "depth", "aux", "steps", "ret_offset", "ret_len", "fent", "gas_min", "gas_max", "gas_limit",
              "calldata", "env", "stack", "memory", "storage"):
        _random(rng, getattr(b, f))
    b.code_id[:] = code_id
    b.status[:] = MG_HALT_STOP
    b.flags[:] = 0
    b.sp[:] = shape.stack_cap
    b.msize[:] = shape.mem_cap
    b.storage_count[:] = shape.storage_cap
    b.calldata_len[:] = shape.calldata_cap
    b.trace_len[:] = shape.trace_cap
    b.rec_len[:] = shape.rec_cap
    if shape.trace_cap:
        _random(rng, b.trace)
    if shape.rec_cap:
        _random(rng, b.rec)
    if shape.node_cap:
        for f in ("stag", "node", "cval", "mtag", "sttag"):
            _random(rng, getattr(b, f))
        b.n_nodes[:] = shape.node_cap
        b.n_consts[:] = shape.const_cap
    if shape.obj_cap:
        b.sobj[...] = rng.integers(0, shape.obj_cap, size=b.sobj.shape, dtype=np.uint32)   # upload validates handles
        for f in ("omask", "sink", "ymask"):
            _random(rng, getattr(b, f))
        b.tflags[:] = rng.integers(0, 4, size=shape.n, dtype=np.uint32)
        b.n_obj[:] = shape.obj_cap
        b.n_fixed[:] = MG_TAINT_OBJ0
        b.n_atoms[:] = MG_TAINT_MAX_ATOMS
    return b


def sentinel_filled(shape: LaneShape, byte: int = 0xA5) -> LaneBatch:
    """A host image whose every cell holds the sentinel byte pattern."""
    b = LaneBatch(shape)
    for f in _U32_FIELDS + _U64_FIELDS + ("calldata", "env", "stack", "memory", "storage", "trace", "rec") + (
            _SYM_FIELDS if b.symbolic else ()) + (_TAINT_FIELDS if b.taint else ()):
        getattr(b, f).view(np.uint8)[...] = byte
    return b


def whole_diff(a: LaneBatch, b: LaneBatch, lanes=None, limit: int = 8) -> list:
    """Cell-for-cell differences of two images of one shape over whole capacities."""
    assert a.shape == b.shape
    idx = slice(None) if lanes is None else np.asarray(list(lanes), dtype=np.int64)
    out = []
    for f in fields_of(a.shape):
        x, y = getattr(a, f), getattr(b, f)
        if x is None or y is None:
            continue
        x, y = x[idx], y[idx]
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            where = [tuple(int(v) for v in r) for r in bad[:3]]
            out.append(f"{f}: {len(bad)} cells differ, first (index within the compared lanes) {where}")
            if len(out) >= limit:
                break
    return out


def live_diff(a: LaneBatch, b: LaneBatch, limit: int = 8) -> list:
    """Differences of two images in what is live: the scalars, env, calldata below
    calldata_len and every row below each lane's own count.  [] when equal."""
    assert a.shape == b.shape
    sh, out = a.shape, []
    scalars = list(SCALARS) + ["fent"] + (["trace_len"] if sh.trace_cap else []) + (["rec_len"] if sh.rec_cap else [])
    scalars += (list(SYM_SCALARS) if sh.node_cap else []) + (list(TAINT_SCALARS) if sh.obj_cap else [])
    for f in scalars:
        bad = np.nonzero(getattr(a, f) != getattr(b, f))[0]
        if bad.size:
            out.append(f"{f}: lanes {bad[:4].tolist()} differ")
    if out:
        return out[:limit]
    rows = [("stack", "sp"), ("storage", "storage_count"), ("memory", "msize"), ("calldata", "calldata_len")]
    rows += ([("trace", "trace_len")] if sh.trace_cap else []) + ([("rec", "rec_len")] if sh.rec_cap else [])
    if sh.node_cap:
        rows += [("stag", "sp"), ("node", "n_nodes"), ("cval", "n_consts"), ("mtag", "msize"),
                 ("sttag", "storage_count")]
    if sh.obj_cap:
        rows += [("sobj", "sp"), ("omask", "n_obj")]
    if not np.array_equal(a.env, b.env):
        out.append("env differs")
    for f, count in rows:
        x, y, c = getattr(a, f), getattr(b, f), getattr(a, count)
        for i in range(sh.n):
            k = min(int(c[i]), x.shape[1])
            if not np.array_equal(x[i, :k], y[i, :k]):
                out.append(f"lane {i}: {f} differs below {count} = {k}")
                if len(out) >= limit:
                    return out
    return out


def live_equal(a: LaneBatch, b: LaneBatch) -> bool:
    """Equal scalars, and equal rows below each lane's own counts."""
    return not live_diff(a, b, limit=1)
