"""One MI355X context: codes, a resident lane batch, stepping and evaluation.

Thin object wrapper over the C-ABI (native.py).  One ``GpuDevice`` per GPU and
per process (contexts are single-threaded; multi-GPU = one
process per GPU).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import native
from .lanes import LaneBatch, LaneShape


@dataclass
class StepStats:
    lane_steps: int
    running: int
    halted: int
    hooked: int
    escaped: int
    kernel_ms: float


@dataclass
class ExploreStats:
    rounds: int
    forks: int
    made_jump: int
    starved: int
    path_full: int
    free_used: int
    running: int
    lane_steps: int
    kernel_ms: float


@dataclass
class HarvestInfo:
    """mg_harvest_info: n lanes selected of `matched`, and the largest counts among
    the selected lanes (the bounds of harvest_download)."""
    n: int
    matched: int
    sp: int
    msize: int
    storage_count: int
    trace_len: int
    rec_len: int
    n_nodes: int
    n_consts: int
    path_len: int
    kernel_ms: float


def _mask_array(hook_mask: Optional[Sequence[int]]):
    m = list(hook_mask) if hook_mask is not None else [0, 0, 0, 0]
    return (ctypes.c_uint64 * 4)(*[int(x) & ((1 << 64) - 1) for x in m])


def hook_mask_for(opcodes) -> list:
    """256-bit mask (4 x u64) with the given opcode bytes set."""
    m = [0, 0, 0, 0]
    for b in opcodes:
        m[b >> 6] |= 1 << (b & 63)
    return m


class GpuDevice:
    def __init__(self, device: int = 0):
        self.lib = native.load()
        self.ctx = ctypes.c_void_p()
        rc = self.lib.mg_open(device, ctypes.byref(self.ctx))
        if rc != native.MG_OK:
            raise native.MythGpuError(f"mg_open({device}) failed with {rc}")
        self.device = device
        self.shape: Optional[LaneShape] = None
        self.path_cap = 0                  # explore planes of the current batch (explore_alloc)
        self.codes = []

    # -- errors --------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc != native.MG_OK:
            msg = self.lib.mg_last_error(self.ctx)
            raise native.MythGpuError(f"{what}: rc={rc}: {msg.decode() if msg else ''}")

    def close(self):
        if self.ctx:
            self.lib.mg_close(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- codes ---------------------------------------------------------------
    def load_code(self, code: bytes) -> int:
        cid = ctypes.c_uint32()
        self._check(self.lib.mg_load_code(self.ctx, bytes(code), len(code), ctypes.byref(cid)),
                    "mg_load_code")
        self.codes.append(bytes(code))
        return cid.value

    def n_instr(self, code_id: int) -> int:
        n = ctypes.c_uint32()
        self._check(self.lib.mg_code_info(self.ctx, code_id, ctypes.byref(n)), "mg_code_info")
        return n.value

    def code_fentries(self, code_id: int) -> np.ndarray:
        """mg_code_fentries: uint8[n_instr], bit 0 = a JUMP / JUMPI landing here
        switches active_function_name, bit 1 = the same for the next index."""
        out = np.zeros(self.n_instr(code_id), dtype=np.uint8)
        self._check(self.lib.mg_code_fentries(self.ctx, code_id, out.ctypes.data, out.size), "mg_code_fentries")
        return out

    def code_table(self, code_id: int):
        """mg_code_table: (opcode byte per instruction, byte address per instruction)."""
        n = self.n_instr(code_id)
        ops = np.zeros(n, dtype=np.uint8)
        addrs = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.mg_code_table(self.ctx, code_id, ops.ctypes.data, addrs.ctypes.data, n),
                    "mg_code_table")
        return ops, addrs

    # -- lanes ---------------------------------------------------------------
    def alloc(self, shape: LaneShape, coverage: bool = False):
        cfg = native.MgBatchCfg(shape.n, shape.stack_cap, shape.mem_cap, shape.calldata_cap,
                                shape.storage_cap, 1 if coverage else 0, shape.trace_cap,
                                shape.rec_cap)
        self._check(self.lib.mg_lanes_alloc(self.ctx, ctypes.byref(cfg)), "mg_lanes_alloc")
        if shape.node_cap:
            self._check(self.lib.mg_sym_alloc(self.ctx, shape.node_cap, max(shape.const_cap, 1)),
                        "mg_sym_alloc")
        if shape.obj_cap:
            self._check(self.lib.mg_taint_alloc(self.ctx, shape.obj_cap), "mg_taint_alloc")
        self.shape = shape
        self.path_cap = 0

    def set_taint_program(self, actions) -> None:
        """mg_taint_program: the per-opcode action words of the batch-safe hooks
        (256 x uint32, mythril_amd/laser/taint.py)."""
        arr = np.ascontiguousarray(np.asarray(actions, dtype=np.uint32).reshape(256))
        self._check(self.lib.mg_taint_program(self.ctx, arr.ctypes.data), "mg_taint_program")

    def set_taint_force(self, code_id: int, flags) -> None:
        """mg_taint_force: instructions of a code where taint lanes stop for the
        host instead of applying the batch-safe actions."""
        arr = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8))
        self._check(self.lib.mg_taint_force(self.ctx, int(code_id), arr.ctypes.data, arr.size),
                    "mg_taint_force")

    def _planes(self, batch: LaneBatch, first: int, n: int, up: bool, dev_first: Optional[int] = None):
        """Symbolic / taint planes of host lanes [first, first + n) to or from
        device lanes [dev_first, dev_first + n) (dev_first defaults to first)."""
        d = first if dev_first is None else dev_first
        if batch.symbolic:
            s = batch.sym_soa_range(first, n)
            fn = self.lib.mg_sym_upload if up else self.lib.mg_sym_download
            self._check(fn(self.ctx, ctypes.addressof(s), d, n), "mg_sym_upload" if up else "mg_sym_download")
        if batch.taint:
            t = batch.taint_soa_range(first, n)
            fn = self.lib.mg_taint_upload if up else self.lib.mg_taint_download
            self._check(fn(self.ctx, ctypes.addressof(t), d, n),
                        "mg_taint_upload" if up else "mg_taint_download")

    def upload(self, batch: LaneBatch, first: int = 0):
        soa = batch.soa()
        self._check(self.lib.mg_lanes_upload(self.ctx, ctypes.addressof(soa), first, batch.n),
                    "mg_lanes_upload")
        self._planes(batch, 0, batch.n, True, first)

    def download(self, batch: LaneBatch, first: int = 0):
        soa = batch.soa()
        self._check(self.lib.mg_lanes_download(self.ctx, ctypes.addressof(soa), first, batch.n),
                    "mg_lanes_download")
        self._planes(batch, 0, batch.n, False, first)

    def upload_range(self, batch: LaneBatch, first: int, n: int, live: bool = False):
        """Upload lanes [first, first + n) of `batch` to the same device lanes.
        Every upload moves only what a step reads, below the range's largest sp /
        msize / storage count / record and trace length; live=True says so by
        name (mg_lanes_upload_live, the same transfer as mg_lanes_upload)."""
        soa = batch.soa_range(first, n)
        fn = self.lib.mg_lanes_upload_live if live else self.lib.mg_lanes_upload
        self._check(fn(self.ctx, ctypes.addressof(soa), first, n),
                    "mg_lanes_upload_live" if live else "mg_lanes_upload")
        self._planes(batch, first, n, True)

    def download_range(self, batch: LaneBatch, first: int, n: int, live: bool = False):
        """Download lanes [first, first + n).  live=True (the host image was
        uploaded from `batch`): only what a step can have changed, below the
        range's largest sp / msize / storage count / record length
        (mg_lanes_download_live)."""
        soa = batch.soa_range(first, n)
        fn = self.lib.mg_lanes_download_live if live else self.lib.mg_lanes_download
        self._check(fn(self.ctx, ctypes.addressof(soa), first, n),
                    "mg_lanes_download_live" if live else "mg_lanes_download")
        self._planes(batch, first, n, False)

    def set_loop_bound(self, bound: int):
        """BoundedLoopsStrategy on the device (0 = off); needs trace_cap > 0."""
        self._check(self.lib.mg_set_loop_bound(self.ctx, int(bound)), "mg_set_loop_bound")

    def reset(self):
        self._check(self.lib.mg_lanes_reset(self.ctx), "mg_lanes_reset")

    def fork(self, src, dst_fall, dst_jump):
        """mg_lanes_fork: make the JUMPI successors of the lanes `src` (stopped with
        MG_FORK) in the lanes `dst_fall` / `dst_jump` on the device (MG_FORK_NONE:
        not this one; dst_fall[i] == src[i]: in place).  uint32 arrays in;
        returns (made uint32[n] of MG_FORK_MADE_* / MG_FORK_BAD_SRC, cond uint32[n] =
        1 + the condition's arena node, kernel_ms)."""
        arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1)) for a in (src, dst_fall, dst_jump)]
        n = arrs[0].size
        if arrs[1].size != n or arrs[2].size != n:
            raise ValueError("fork: src, dst_fall and dst_jump must have one entry per fork")
        made = np.zeros(n, dtype=np.uint32)
        cond = np.zeros(n, dtype=np.uint32)
        batch = native.MgForkBatch(n, 0, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data)
        ms = ctypes.c_float()
        self._check(self.lib.mg_lanes_fork(self.ctx, ctypes.byref(batch), made.ctypes.data, cond.ctypes.data,
                                           ctypes.byref(ms)), "mg_lanes_fork")
        return made, cond, ms.value

    def explore_alloc(self, path_cap: int):
        """mg_explore_alloc: the path planes of mg_explore, `path_cap` entries per
        lane; after alloc() of a shape with symbolic planes, once per batch."""
        self._check(self.lib.mg_explore_alloc(self.ctx, int(path_cap)), "mg_explore_alloc")
        self.path_cap = int(path_cap)

    def explore(self, free, hook_mask=None, max_steps: int = 1 << 30, max_depth: int = 0,
                max_rounds: int = 64, resume: bool = False) -> ExploreStats:
        """mg_explore: up to `max_rounds` rounds of step + fork on the device.  `free`:
        the lanes that may be overwritten with jump successors, strictly ascending;
        they are handed out from the front, stats.free_used of them.  resume=True
        (mg_explore_resume): root, path_len and path continue from the last call."""
        arr = np.ascontiguousarray(np.asarray(free, dtype=np.uint32).reshape(-1))
        st = native.MgExploreStats()
        fn, name = (self.lib.mg_explore_resume, "mg_explore_resume") if resume else (self.lib.mg_explore, "mg_explore")
        self._check(fn(self.ctx, _mask_array(hook_mask), max_steps, max_depth, int(max_rounds),
                       arr.ctypes.data if arr.size else None, arr.size, ctypes.byref(st)), name)
        return ExploreStats(st.rounds, st.forks, st.made_jump, st.starved, st.path_full, st.free_used, st.running,
                            st.lane_steps, st.kernel_ms)

    def explore_paths(self, first: int, n: int):
        """mg_explore_download: (path uint32[n, path_cap] of cond_tag << 1 | side,
        zero at and above path_len; path_len uint32[n]; root uint32[n])."""
        path = np.zeros((n, self.path_cap), dtype=np.uint32)
        path_len = np.zeros(n, dtype=np.uint32)
        root = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.mg_explore_download(self.ctx, path.ctypes.data, path_len.ctypes.data, root.ctypes.data,
                                                 first, n), "mg_explore_download")
        return path, path_len, root

    def explore_upload_paths(self, path, path_len, root, first: int = 0):
        """mg_explore_upload: the inverse of explore_paths for lanes [first, first + n),
        n = len(path_len); path uint32[n, path_cap]."""
        path_len = np.ascontiguousarray(np.asarray(path_len, dtype=np.uint32).reshape(-1))
        root = np.ascontiguousarray(np.asarray(root, dtype=np.uint32).reshape(-1))
        n = path_len.size
        path = np.ascontiguousarray(np.asarray(path, dtype=np.uint32))
        if root.size != n or path.shape != (n, self.path_cap):
            raise ValueError("explore_upload_paths: path is [n, path_cap], path_len and root are [n]")
        self._check(self.lib.mg_explore_upload(self.ctx, path.ctypes.data, path_len.ctypes.data, root.ctypes.data,
                                               first, n), "mg_explore_upload")

    def harvest_select(self, status_mask: int, skip=(), max_lanes: Optional[int] = None) -> HarvestInfo:
        """mg_harvest_select: choose on the device the lanes whose status bit is set in
        `status_mask` and that are not in `skip` (the caller's free list, strictly
        ascending), the lowest `max_lanes` of them (None: all).  The list stays on
        the device for harvest_download."""
        arr = np.ascontiguousarray(np.asarray(skip, dtype=np.uint32).reshape(-1))
        info = native.MgHarvestInfo()
        cap = 0xFFFFFFFF if max_lanes is None else int(max_lanes)
        self._check(self.lib.mg_harvest_select(self.ctx, int(status_mask) & 0xFFFFFFFF,
                                               arr.ctypes.data if arr.size else None, arr.size, cap,
                                               ctypes.byref(info)), "mg_harvest_select")
        return HarvestInfo(info.n, info.matched, info.sp, info.msize, info.storage_count, info.trace_len,
                           info.rec_len, info.n_nodes, info.n_consts, info.path_len, info.kernel_ms)

    def harvest_shape(self, info: HarvestInfo) -> LaneShape:
        """The slim shape harvest_download builds by default: info's maxima as the
        capacities (mem_cap rounded up to 32, stack_cap at least 1), the device's
        calldata capacity, symbolic planes when the batch has them."""
        d = self.shape
        return LaneShape(n=info.n, stack_cap=max(info.sp, 1), mem_cap=(info.msize + 31) // 32 * 32,
                         calldata_cap=d.calldata_cap, storage_cap=info.storage_count,
                         trace_cap=info.trace_len if d.trace_cap else 0, rec_cap=info.rec_len if d.rec_cap else 0,
                         node_cap=max(info.n_nodes, 1) if d.node_cap else 0,
                         const_cap=max(info.n_consts, 1) if d.node_cap else 0)

    def harvest_download(self, info: HarvestInfo, shape: Optional[LaneShape] = None, batch: Optional[LaneBatch] = None):
        """mg_harvest_download of the last harvest_select: (lanes uint32[n], LaneBatch of
        n lanes, path uint32[n, path_cap], path_len, root); row i is device lane
        lanes[i].  The image is `batch` when given (its cells above the bounds are
        kept), else a new one of `shape` (default: harvest_shape(info)).  path,
        path_len and root are None without explore planes."""
        n = info.n
        if batch is None:
            batch = LaneBatch(shape if shape is not None else self.harvest_shape(info))
        if batch.n != n:
            raise ValueError("harvest_download: the host image has one lane per selected lane")
        lanes = np.zeros(n, dtype=np.uint32)
        path = path_len = root = None
        if self.path_cap:
            path = np.zeros((n, self.path_cap), dtype=np.uint32)
            path_len = np.zeros(n, dtype=np.uint32)
            root = np.zeros(n, dtype=np.uint32)
        soa = batch.soa()
        sym = batch.sym_soa_range(0, n) if batch.symbolic else None
        self._check(self.lib.mg_harvest_download(
            self.ctx, lanes.ctypes.data, ctypes.addressof(soa), ctypes.addressof(sym) if sym is not None else None,
            path.ctypes.data if path is not None else None, path_len.ctypes.data if path is not None else None,
            root.ctypes.data if path is not None else None), "mg_harvest_download")
        return lanes, batch, path, path_len, root

    def harvest_upload(self, lanes, batch: LaneBatch, path=None, path_len=None, root=None):
        """mg_harvest_upload, the inverse of harvest_download: row i of `batch` (and of
        path uint32[n, path_cap], path_len, root when given, all three or none) goes
        to device lane lanes[i]; lanes strictly ascending, or None for the resident
        list of the last harvest_select.  Only rows below the largest count among
        the n rows cross PCIe; the symbolic planes go when the batch has them."""
        n = batch.n
        if lanes is not None:
            lanes = np.ascontiguousarray(np.asarray(lanes, dtype=np.uint32).reshape(-1))
            if lanes.size != n:
                raise ValueError("harvest_upload: the host image has one lane per listed lane")
        given = [a is not None for a in (path, path_len, root)]
        if any(given) != all(given):
            raise ValueError("harvest_upload: path, path_len and root go together")
        if all(given):
            path = np.ascontiguousarray(np.asarray(path, dtype=np.uint32))
            path_len = np.ascontiguousarray(np.asarray(path_len, dtype=np.uint32).reshape(-1))
            root = np.ascontiguousarray(np.asarray(root, dtype=np.uint32).reshape(-1))
            if path.shape != (n, self.path_cap) or path_len.size != n or root.size != n:
                raise ValueError("harvest_upload: path is [n, path_cap], path_len and root are [n]")
        soa = batch.soa()
        sym = batch.sym_soa_range(0, n) if batch.symbolic else None
        self._check(self.lib.mg_harvest_upload(
            self.ctx, lanes.ctypes.data if lanes is not None else None, ctypes.addressof(soa),
            ctypes.addressof(sym) if sym is not None else None,
            path.ctypes.data if path is not None else None, path_len.ctypes.data if path is not None else None,
            root.ctypes.data if path is not None else None), "mg_harvest_upload")

    def harvest(self, status_mask: int, skip=(), max_lanes: Optional[int] = None, shape: Optional[LaneShape] = None):
        """harvest_select + harvest_download: (info, lanes, LaneBatch, path, path_len, root)."""
        info = self.harvest_select(status_mask, skip, max_lanes)
        return (info,) + self.harvest_download(info, shape)

    def explore_check(self, pool, bindings, lane_binding, allowed=None, first: int = 0, n: Optional[int] = None,
                      bits: bool = False, functions=None):
        """mg_explore_check: which candidate model satisfies each lane's recorded path,
        evaluated from the arenas on the device.  pool: a ModelPool, or None for the
        one the last eval_upload left resident; bindings: native.MgPathBinding per
        lineage; lane_binding: uint32[n_lanes], indexed by root[lane], an index into
        bindings or MG_PATH_UNBOUND; allowed: uint64[len(bindings), ceil(n_models / 64)]
        or None (every model); functions: a native.MgPathFunctions
        (symbolic.path_functions) naming the pool's Power and keccak256_<bits> tables
        (mg_explore_check_fn), or None: mg_explore_check, under which a KECCAK or Power
        node makes its lane unknown.  Returns (first_sat uint32[n] -- a model index,
        MG_BV_NO_MODEL or MG_PATH_UNKNOWN --, sat_bits uint64[n, words] or None,
        kernel_ms)."""
        n_lanes = self.shape.n
        n = n_lanes - first if n is None else int(n)
        bindings = list(bindings)
        barr = (native.MgPathBinding * max(len(bindings), 1))(*bindings)
        lb = np.ascontiguousarray(np.asarray(lane_binding, dtype=np.uint32).reshape(-1))
        if lb.size != n_lanes:
            raise ValueError("explore_check: lane_binding has one entry per lane of the batch")
        mods = pool.c_struct() if pool is not None else None
        n_models = pool.n_models if pool is not None else self._models.n_models
        words = (n_models + 63) // 64
        if allowed is not None:
            allowed = np.ascontiguousarray(np.asarray(allowed, dtype=np.uint64))
            if allowed.shape != (len(bindings), words):
                raise ValueError("explore_check: allowed is [len(bindings), ceil(n_models / 64)]")
        fs = np.zeros(max(n, 1), dtype=np.uint32)
        sb = np.zeros((max(n, 1), words), dtype=np.uint64) if bits else None
        ms = ctypes.c_float()
        head = (self.ctx, ctypes.byref(mods) if mods is not None else None, barr, len(bindings), lb.ctypes.data,
                allowed.ctypes.data if allowed is not None else None)
        tail = (first, n, fs.ctypes.data, sb.ctypes.data if bits else None, ctypes.byref(ms))
        if functions is None:
            self._check(self.lib.mg_explore_check(*head, *tail), "mg_explore_check")
        else:
            self._check(self.lib.mg_explore_check_fn(*head, ctypes.byref(functions), *tail), "mg_explore_check_fn")
        if mods is not None:
            self._models = mods             # the resident pool now
        return fs[:n], (sb[:n] if bits else None), ms.value

    def step(self, hook_mask=None, max_steps: int = 1 << 30, max_depth: int = 0,
             horizon: int = 0) -> StepStats:
        """mg_step (horizon 0) or mg_step_until: lanes also pause once their
        cumulative steps reach `horizon`."""
        st = native.MgStepStats()
        if horizon:
            rc = self.lib.mg_step_until(self.ctx, _mask_array(hook_mask), max_steps, max_depth,
                                        horizon, ctypes.byref(st))
        else:
            rc = self.lib.mg_step(self.ctx, _mask_array(hook_mask), max_steps, max_depth,
                                  ctypes.byref(st))
        self._check(rc, "mg_step")
        return StepStats(st.lane_steps, st.running, st.halted, st.hooked, st.escaped, st.kernel_ms)

    def run_batches(self, n_batches: int, hook_mask=None, max_steps: int = 1 << 30,
                    max_depth: int = 0):
        """mg_run_batches: n_batches x (reset from the resident image + one
        stepping launch) enqueued back to back, one host wait; per-batch stats."""
        st = (native.MgStepStats * n_batches)()
        self._check(self.lib.mg_run_batches(self.ctx, _mask_array(hook_mask), max_steps, max_depth,
                                            n_batches, st), "mg_run_batches")
        return [StepStats(s.lane_steps, s.running, s.halted, s.hooked, s.escaped, s.kernel_ms)
                for s in st]

    def step_profile(self, hook_mask=None, max_steps: int = 1 << 30, max_depth: int = 0):
        """Step with per-opcode counters; returns (op_counts[256], extra[4])."""
        ops = np.zeros(256, dtype=np.uint64)
        extra = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.mg_step_profile(self.ctx, _mask_array(hook_mask), max_steps, max_depth,
                                             ops.ctypes.data, extra.ctypes.data), "mg_step_profile")
        return ops, extra

    def step_async(self, hook_mask=None, max_steps: int = 1 << 30, max_depth: int = 0):
        self._check(self.lib.mg_step_async(self.ctx, _mask_array(hook_mask), max_steps, max_depth),
                    "mg_step_async")

    def sync(self):
        self._check(self.lib.mg_sync(self.ctx), "mg_sync")

    def coverage(self, code_id: int) -> np.ndarray:
        n = self.n_instr(code_id)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.mg_coverage(self.ctx, code_id, out.ctypes.data, out.size), "mg_coverage")
        return out[:n]

    def coverage_clear(self):
        self._check(self.lib.mg_coverage_clear(self.ctx), "mg_coverage_clear")

    def event_counts(self, n: int, first: int = 0):
        sha3 = np.zeros(n, dtype=np.uint32)
        exp = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.mg_event_counts(self.ctx, sha3.ctypes.data, exp.ctypes.data, first, n),
                    "mg_event_counts")
        return sha3, exp

    # -- kernel 2 ------------------------------------------------------------
    def eval_upload(self, program, models):
        """program: mythril_amd.smt.program.ProgramBatch; models: ModelPool."""
        self._dags = program.c_struct()
        self._models = models.c_struct()
        self._check(self.lib.mg_eval_upload(self.ctx, ctypes.byref(self._dags),
                                            ctypes.byref(self._models)), "mg_eval_upload")
        self._n_dags = program.n_dags

    def eval_run(self, first: int = 0, count: Optional[int] = None) -> float:
        count = self._n_dags - first if count is None else count
        ms = ctypes.c_float()
        self._check(self.lib.mg_eval_run(self.ctx, first, count, ctypes.byref(ms)), "mg_eval_run")
        return ms.value

    def eval_download(self, first: int = 0, count: Optional[int] = None):
        count = self._n_dags - first if count is None else count
        fs = np.zeros(count, dtype=np.uint32)
        sc = np.zeros(count, dtype=np.uint32)
        self._check(self.lib.mg_eval_download(self.ctx, fs.ctypes.data, sc.ctypes.data, first, count),
                    "mg_eval_download")
        return fs, sc

    def eval_bits(self, program, models):
        """(first_sat, sat_count, sat_bits[n_dags, ceil(n_models/64)] uint64, ms)."""
        dags, mods = program.c_struct(), models.c_struct()
        n, words = program.n_dags, (models.n_models + 63) // 64
        fs = np.zeros(n, dtype=np.uint32)
        sc = np.zeros(n, dtype=np.uint32)
        bits = np.zeros((n, words), dtype=np.uint64)
        ms = ctypes.c_float()
        self._check(self.lib.mg_eval_bits(self.ctx, ctypes.byref(dags), ctypes.byref(mods),
                                          fs.ctypes.data, sc.ctypes.data, bits.ctypes.data,
                                          ctypes.byref(ms)), "mg_eval_bits")
        return fs, sc, bits, ms.value

    def eval(self, program, models):
        self.eval_upload(program, models)
        ms = self.eval_run()
        fs, sc = self.eval_download()
        return fs, sc, ms

    def eval_terms(self, program, models):
        """mg_eval_terms: (values uint32[n_dags, n_models, 8], ms) -- the value of
        every program's final accumulator under every model, little-endian limbs."""
        dags, mods = program.c_struct(), models.c_struct()
        out = np.zeros((program.n_dags, models.n_models, 8), dtype=np.uint32)
        ms = ctypes.c_float()
        self._check(self.lib.mg_eval_terms(self.ctx, ctypes.byref(dags), ctypes.byref(mods), out.ctypes.data,
                                           ctypes.byref(ms)), "mg_eval_terms")
        return out, ms.value

    def eval_min(self, program, models, cons, objs):
        """mg_eval_min.  cons[q] / objs[q]: the program indices that must hold /
        that are minimised (most significant first) for query q.  Returns
        (best_model uint32[n_queries], best_values: per query uint32[len(objs[q]), 8],
        cand_count uint32[n_queries], ms); best_model 0xFFFFFFFF = no candidate."""
        if len(cons) != len(objs):
            raise ValueError("eval_min: one constraint list and one objective list per query")
        nq = len(cons)

        def lists(xs):
            off = np.zeros(nq + 1, dtype=np.uint32)
            off[1:] = np.cumsum([len(x) for x in xs], dtype=np.int64)
            flat = np.array([int(i) for x in xs for i in x] or [0], dtype=np.uint32)
            return off, flat

        c_off, c_dag = lists(cons)
        o_off, o_dag = lists(objs)
        dags, mods = program.c_struct(), models.c_struct()
        batch = native.MgMinBatch(nq, 0, c_off.ctypes.data, c_dag.ctypes.data, o_off.ctypes.data, o_dag.ctypes.data)
        best = np.zeros(max(nq, 1), dtype=np.uint32)
        count = np.zeros(max(nq, 1), dtype=np.uint32)
        vals = np.zeros((max(int(o_off[-1]), 1), 8), dtype=np.uint32)
        ms = ctypes.c_float()
        self._check(self.lib.mg_eval_min(self.ctx, ctypes.byref(dags), ctypes.byref(mods), ctypes.byref(batch),
                                         best.ctypes.data, vals.ctypes.data, count.ctypes.data, ctypes.byref(ms)),
                    "mg_eval_min")
        per_query = [vals[int(o_off[q]):int(o_off[q + 1])] for q in range(nq)]
        return best[:nq], per_query, count[:nq], ms.value
