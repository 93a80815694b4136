#!/usr/bin/env python
"""mg_harvest_select + mg_harvest_download against the transfers the library offered
before, on scripts/explore_bench.py's batch.

Run by hand on the MI355X (under a timeout); bench.py does not call it.

The batch: `--lanes` lanes (65,536), the first half the start of a symbolic message
call into each of the 18 reference contracts (bench.symbolic_lane_batch), the rest
spare, after the mg_explore rounds that fit (`--rounds`; the spare lanes are used up
by the first).  The finished lanes are those whose status is neither MG_RUNNING nor
MG_FORK and that are not left in the free list.  At two densities -- every finished
lane, and max_lanes = 1/16 of them (the lowest) -- three routes fetch them:

  device      harvest_select + harvest_download into a slim image of the selection's
              maxima: the lanes are chosen and gathered on the device, one transfer.
  host (a)    what a caller must do today: the scalars of the whole batch (the
              statuses), then download_range(live=True) with mg_sym_download, and
              mg_explore_download, over [0, n), then NumPy indexing of the chosen lanes.
  host (b)    the same transfers once per run of consecutive chosen lanes.

Repetitions alternate between the routes.  All three must give the same host image
of the chosen lanes: every scalar, the paths, and every row below the lane's own
count (env and calldata are not compared: the live download does not move them); the
script asserts it.  Prints one JSON object with the range of every figure; --out
also writes it to a file.  --device-only runs the device route alone (for a kernel
trace of the gathers).
"""
import argparse
import ctypes
import json
import sys
import time
from dataclasses import replace
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bench  # noqa: E402
from mythril_amd.device import GpuDevice  # noqa: E402
from mythril_amd.lanes import (_ALL_FIELDS, _SYM_FIELDS, _U32_FIELDS, _U64_FIELDS, MG_ENV_WORDS, MG_FORK,  # noqa: E402
                               MG_HALT_STOP, MG_RUNNING, LaneBatch)

PATH_CAP = 16
FINISHED = 0xFFFFFFFF & ~(1 << MG_RUNNING) & ~(1 << MG_FORK)
INFO_BYTES = 40
ROWS = (("stack", "sp", 32), ("storage", "storage_count", 64), ("memory", "msize", 1), ("rec", "rec_len", 4),
        ("trace", "trace_len", 4), ("stag", "sp", 4), ("node", "n_nodes", 16), ("cval", "n_consts", 32),
        ("mtag", "msize", 4), ("sttag", "storage_count", 8))
SCALAR_FIELDS = tuple(f for f in _U32_FIELDS + _U64_FIELDS) + ("n_nodes", "n_consts")


def scalars(dev, b):
    """The lanes' scalars only (NULL row pointers are skipped by mg_lanes_download)."""
    soa = b.soa()
    for f in ("calldata", "env", "stack", "memory", "storage", "trace", "rec"):
        setattr(soa, f, None)
    dev._check(dev.lib.mg_lanes_download(dev.ctx, ctypes.addressof(soa), 0, b.n), "mg_lanes_download")


def span(xs):
    return {"min": float(min(xs)), "max": float(max(xs)), "all": [float(x) for x in xs]}


def runs_of(lanes):
    """[(first, n)] of the runs of consecutive lanes in an ascending list."""
    if not len(lanes):
        return []
    cut = np.flatnonzero(np.diff(lanes) != 1) + 1
    return [(int(r[0]), int(r.size)) for r in np.split(lanes, cut)]


def row_bytes(shape, bounds, n):
    """Bytes of the row fields of n lanes under per-field unit bounds (clipped to the shape)."""
    caps = {"stack": shape.stack_cap, "storage": shape.storage_cap, "memory": shape.mem_cap, "rec": shape.rec_cap,
            "trace": shape.trace_cap, "stag": shape.stack_cap, "node": shape.node_cap, "cval": shape.const_cap,
            "mtag": shape.mem_cap, "sttag": shape.storage_cap}
    return {f: n * min(bounds[f], caps[f]) * unit for f, _, unit in ROWS}


def same_live(a, pa, b, pb):
    """Differences of two images of the same lanes in what is live: scalars, paths, rows below each lane's count."""
    out = []
    for f in SCALAR_FIELDS:
        if not np.array_equal(getattr(a, f), getattr(b, f)):
            out.append(f)
    for f, count, _ in ROWS:
        x, y, c = getattr(a, f), getattr(b, f), getattr(a, count).astype(np.int64)
        k = min(x.shape[1], y.shape[1])
        if int(c.max(initial=0)) > k:
            out.append(f + ": a count above both images' capacity")
            continue
        if k == 0:
            continue
        live = np.arange(k)[None, :] < c[:, None]
        eq = x[:, :k] == y[:, :k]
        eq = eq.reshape(eq.shape[0], k, -1).all(axis=2)
        if not (eq | ~live).all():
            out.append(f)
    for x, y, what in zip(pa, pb, ("path", "path_len", "root")):
        if not np.array_equal(x, y):
            out.append(what)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=2, help="mg_explore rounds before the harvest")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    half = args.lanes // 2
    dev = GpuDevice(0)
    _, live = bench.symbolic_lane_batch(dev, half)
    shape = replace(live.shape, n=args.lanes)
    b = LaneBatch(shape)
    for f in _ALL_FIELDS + _SYM_FIELDS:
        getattr(b, f)[:half] = getattr(live, f)
    b.code_id[half:] = b.code_id[0]
    b.status[half:] = MG_HALT_STOP
    free = np.arange(half, args.lanes, dtype=np.uint32)
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    dev.upload(b)
    st = dev.explore(free, max_rounds=args.rounds)
    skip = free[st.free_used:]
    cur = LaneBatch(shape)                          # the host routes' image of the whole batch
    scalar_bytes = sum(getattr(cur, f).nbytes for f in SCALAR_FIELDS) // args.lanes
    path_bytes = (PATH_CAP + 2) * 4
    print(f"batch: {args.lanes} lanes, {st.rounds} rounds, {st.forks} forks, {st.starved} starved", file=sys.stderr, flush=True)

    def device_route(cap):
        dev.sync()
        t0 = time.perf_counter()
        info = dev.harvest_select(FINISHED, skip, cap)
        t1 = time.perf_counter()
        lanes, img, path, path_len, root = dev.harvest_download(info)
        t2 = time.perf_counter()
        bounds = {"stack": info.sp, "stag": info.sp, "storage": info.storage_count, "sttag": info.storage_count,
                  "memory": info.msize, "mtag": info.msize, "rec": info.rec_len, "trace": info.trace_len,
                  "node": info.n_nodes, "cval": info.n_consts}
        rows = row_bytes(shape, bounds, info.n)
        whole = info.n * (scalar_bytes + 4 + 8 + shape.calldata_cap + MG_ENV_WORDS * 32 + info.path_len * 4)
        rec = {"wall_ms": (t2 - t0) * 1e3, "select_wall_ms": (t1 - t0) * 1e3, "download_wall_ms": (t2 - t1) * 1e3,
               "select_kernel_ms": info.kernel_ms, "pcie_bytes": skip.nbytes + INFO_BYTES + whole + sum(rows.values()),
               "n": info.n, "matched": info.matched, "row_bytes": rows}
        return rec, (lanes, img, (path, path_len, root))

    def pick(lanes):
        """NumPy indexing of the chosen lanes out of the whole-batch image."""
        out = LaneBatch(replace(shape, n=int(lanes.size)))
        for f in _ALL_FIELDS + _SYM_FIELDS:
            getattr(out, f)[...] = getattr(cur, f)[lanes]
        return out

    def host_route(cap, per_run):
        dev.sync()
        t0 = time.perf_counter()
        scalars(dev, cur)
        ok = ((np.uint32(1) << np.minimum(cur.status, 31)) & np.uint32(FINISHED)).astype(bool) & (cur.status < 32)
        ok[skip] = False
        lanes = np.flatnonzero(ok).astype(np.uint32)
        lanes = lanes if cap is None else lanes[:cap]
        t1 = time.perf_counter()
        ranges = runs_of(lanes) if per_run else [(0, args.lanes)]
        path = np.zeros((args.lanes, PATH_CAP), dtype=np.uint32)
        path_len = np.zeros(args.lanes, dtype=np.uint32)
        root = np.zeros(args.lanes, dtype=np.uint32)
        pcie = args.lanes * scalar_bytes
        for first, n in ranges:
            dev.download_range(cur, first, n, live=True)
            path[first:first + n], path_len[first:first + n], root[first:first + n] = dev.explore_paths(first, n)
            r = slice(first, first + n)
            bounds = {"stack": int(cur.sp[r].max()), "storage": int(cur.storage_count[r].max()),
                      "memory": int(cur.msize[r].max()), "rec": int(cur.rec_len[r].max()),
                      "trace": int(cur.trace_len[r].max()), "node": int(cur.n_nodes[r].max()),
                      "cval": int(cur.n_consts[r].max()), "stag": shape.stack_cap, "mtag": shape.mem_cap,
                      "sttag": shape.storage_cap}
            pcie += n * (scalar_bytes + path_bytes) + sum(row_bytes(shape, bounds, n).values())
        t2 = time.perf_counter()
        img = pick(lanes)
        t3 = time.perf_counter()
        rec = {"wall_ms": (t3 - t0) * 1e3, "scalars_wall_ms": (t1 - t0) * 1e3, "download_wall_ms": (t2 - t1) * 1e3,
               "index_wall_ms": (t3 - t2) * 1e3, "pcie_bytes": pcie, "n": int(lanes.size), "transfers": len(ranges)}
        return rec, (lanes, img, (path[lanes], path_len[lanes], root[lanes]))

    out = {"lanes": args.lanes, "live_lanes": half, "explore_rounds": st.rounds, "forks": st.forks,
           "starved": st.starved, "path_cap": PATH_CAP, "reps": args.reps, "density": {}}
    matched = dev.harvest_select(FINISHED, skip, 0).matched
    out["finished_lanes"] = matched
    for label, cap in (("every_finished_lane", None), ("one_sixteenth", max(matched // 16, 1))):
        routes = {"device": lambda: device_route(cap)}
        if not args.device_only:
            routes["host_a"] = lambda: host_route(cap, False)
            routes["host_b"] = lambda: host_route(cap, True)
        for fn in routes.values():                  # warm-up: pinned buffers, page faults of the host images
            fn()
        runs, last = {k: [] for k in routes}, {}
        for rep in range(args.reps):                # alternating
            for k, fn in routes.items():
                rec, last[k] = fn()
                runs[k].append(rec)
            print(f"{label}: repetition {rep + 1} of {args.reps}", file=sys.stderr, flush=True)
        rec = {"max_lanes": cap, "n": runs["device"][-1]["n"], "runs_of_consecutive_lanes": len(runs_of(last["device"][0]))}
        for k, rs in runs.items():
            rec[k] = {f: span([r[f] for r in rs]) for f in rs[0] if f.endswith("_ms") or f == "pcie_bytes"}
            rec[k]["transfers"] = rs[-1].get("transfers", 1)
        rec["device"]["row_bytes"] = runs["device"][-1]["row_bytes"]
        for k in ("host_a", "host_b"):
            if k in last:
                assert np.array_equal(last[k][0], last["device"][0]), k
                diffs = same_live(last["device"][1], last["device"][2], last[k][1], last[k][2])
                assert diffs == [], (k, diffs)
                rec["same_image_" + k] = True
                rec["device_slowest_is_faster_than_%s_fastest" % k] = \
                    rec["device"]["wall_ms"]["max"] < rec[k]["wall_ms"]["min"]
        out["density"][label] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
