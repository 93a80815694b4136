#!/usr/bin/env python
"""mg_harvest_upload against the range uploads the library offered before, on
scripts/harvest_bench.py's batch in the state that script reaches.

Run by hand on the MI355X (under a timeout); bench.py does not call it.

The finished lanes of the batch are harvested once (harvest_select +
harvest_download, a slim image).  At two densities -- every harvested lane, and
every 16th of them, which lie spread over the batch as the lanes a host resolves
do -- three routes put the rows back into the lanes they came from:

  device      harvest_upload with the list: one stage, one H2D copy, the indexed
              placement and scatters on the device.
  host (a)    the rows written into a full host image of the batch with NumPy, then
              one range upload over [0, n): upload_range + mg_sym_upload +
              mg_explore_upload.
  host (b)    the same three calls once per run of consecutive lanes.

Repetitions alternate between the routes.  After its last repetition each route's
image of the whole batch is downloaded, and all three must hold the same live image
(every scalar, the paths, every row below the lane's own count); the script asserts
it.  Prints one JSON object with the range of every figure; --out also writes it to
a file.  --device-only runs the device route alone (for a kernel trace).
"""
import argparse
import json
import sys
import time
from dataclasses import replace
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

import bench  # noqa: E402
from harvest_bench import FINISHED, PATH_CAP, SCALAR_FIELDS, row_bytes, runs_of, same_live, span  # noqa: E402
from mythril_amd.device import GpuDevice  # noqa: E402
from mythril_amd.lanes import _ALL_FIELDS, _SYM_FIELDS, MG_ENV_WORDS, MG_HALT_STOP, LaneBatch  # noqa: E402


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
    info = dev.harvest_select(FINISHED, skip)
    all_lanes, taken, tpath, tlen, troot = dev.harvest_download(info)
    cur = LaneBatch(shape)                          # the host routes' image of the whole batch
    dev.download(cur)
    cpath, clen, croot = dev.explore_paths(0, args.lanes)
    scalar_bytes = sum(getattr(cur, f).nbytes for f in SCALAR_FIELDS) // args.lanes
    per_lane = scalar_bytes + shape.calldata_cap + MG_ENV_WORDS * 32 + 8
    print(f"batch: {args.lanes} lanes, {st.rounds} rounds, {st.forks} forks, {info.n} harvested", file=sys.stderr, flush=True)

    def subset(rows):
        """Rows `rows` of the harvested image, as the host would hand them back."""
        out = LaneBatch(replace(taken.shape, n=int(rows.size)))
        for f in _ALL_FIELDS + _SYM_FIELDS:
            getattr(out, f)[...] = getattr(taken, f)[rows]
        return out, np.ascontiguousarray(tpath[rows]), np.ascontiguousarray(tlen[rows]), np.ascontiguousarray(troot[rows])

    def bounds_of(img, plen):
        top = lambda a: int(a.max(initial=0))
        return {"stack": top(img.sp), "stag": top(img.sp), "storage": top(img.storage_count),
                "sttag": top(img.storage_count), "memory": top(img.msize), "mtag": top(img.msize), "rec": top(img.rec_len),
                "trace": top(img.trace_len), "node": top(img.n_nodes), "cval": top(img.n_consts)}, top(plen)

    def device_route(lanes, img, path, plen, root):
        dev.sync()
        t0 = time.perf_counter()
        dev.harvest_upload(lanes, img, path, plen, root)
        t1 = time.perf_counter()
        bounds, ptop = bounds_of(img, plen)
        rows = row_bytes(img.shape, bounds, img.n)
        pcie = img.n * (4 + per_lane + ptop * 4) + sum(rows.values())
        return {"wall_ms": (t1 - t0) * 1e3, "pcie_bytes": pcie, "n": img.n, "transfers": 1, "row_bytes": rows}

    def host_route(lanes, img, path, plen, root, per_run):
        dev.sync()
        t0 = time.perf_counter()
        for f in _ALL_FIELDS + _SYM_FIELDS:         # the rows into the whole-batch image
            dst, src = getattr(cur, f), getattr(img, f)
            if src.ndim == 1:
                dst[lanes] = src
            else:
                dst[lanes, :src.shape[1]] = src
        cpath[lanes], clen[lanes], croot[lanes] = path, plen, root
        t1 = time.perf_counter()
        ranges = runs_of(lanes) if per_run else [(0, args.lanes)]
        pcie = 0
        for first, n in ranges:
            r = slice(first, first + n)
            dev.upload_range(cur, first, n)
            dev.explore_upload_paths(cpath[r], clen[r], croot[r], first)
            top = lambda a: int(a[r].max(initial=0))
            bounds = {"stack": top(cur.sp), "storage": top(cur.storage_count), "memory": top(cur.msize),
                      "rec": top(cur.rec_len), "trace": top(cur.trace_len), "node": top(cur.n_nodes),
                      "cval": top(cur.n_consts), "stag": shape.stack_cap, "mtag": shape.mem_cap,
                      "sttag": shape.storage_cap}
            pcie += n * (per_lane + PATH_CAP * 4) + sum(row_bytes(shape, bounds, n).values())
        t2 = time.perf_counter()
        return {"wall_ms": (t2 - t0) * 1e3, "index_wall_ms": (t1 - t0) * 1e3, "upload_wall_ms": (t2 - t1) * 1e3,
                "pcie_bytes": pcie, "n": int(lanes.size), "transfers": 3 * len(ranges)}

    def image():
        whole = LaneBatch(shape)
        dev.download(whole)
        return whole, dev.explore_paths(0, args.lanes)

    out = {"lanes": args.lanes, "live_lanes": half, "explore_rounds": st.rounds, "forks": st.forks,
           "harvested_lanes": info.n, "path_cap": PATH_CAP, "reps": args.reps, "density": {}}
    for label, rows in (("every_harvested_lane", np.arange(info.n)), ("one_sixteenth", np.arange(0, info.n, 16))):
        lanes = np.ascontiguousarray(all_lanes[rows])
        given = (lanes,) + subset(rows)
        routes = {"device": lambda: device_route(*given)}
        if not args.device_only:
            routes["host_a"] = lambda: host_route(*given, False)
            routes["host_b"] = lambda: host_route(*given, True)
        for fn in routes.values():                  # warm-up: pinned buffers, page faults of the host images
            fn()
        runs, left = {k: [] for k in routes}, {}
        for rep in range(args.reps):                # alternating
            for k, fn in routes.items():
                runs[k].append(fn())
                if rep == args.reps - 1:
                    left[k] = image()
            print(f"{label}: repetition {rep + 1} of {args.reps}", file=sys.stderr, flush=True)
        rec = {"n": int(lanes.size), "runs_of_consecutive_lanes": len(runs_of(lanes))}
        for k, rs in runs.items():
            rec[k] = {f: span([r[f] for r in rs]) for f in rs[0] if f.endswith("_ms") or f == "pcie_bytes"}
            rec[k]["transfers"] = rs[-1]["transfers"]
        rec["device"]["row_bytes"] = runs["device"][-1]["row_bytes"]
        for k in ("host_a", "host_b"):
            if k in left:
                diffs = same_live(left["device"][0], left["device"][1], left[k][0], left[k][1])
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
