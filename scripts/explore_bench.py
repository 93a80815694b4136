#!/usr/bin/env python
"""mg_explore against the host-driven fork rounds, on scripts/fork_bench.py's batch.

Run by hand on the MI355X (under a timeout); bench.py does not call it.

The batch: `--lanes` lanes (65,536), the first `--live` (half of them by default)
the start of a symbolic message call into each of the 18 reference contracts
(bench.symbolic_lane_batch), the rest spare.  With half of the lanes live the spare
lanes are used up by the first fork round; `--live 8192` leaves room for three.
From the same upload, R rounds (1 and 3) go two ways:

  explorer     one mg_explore call of R rounds: the plan is made on the device, the
               host reads one counter block per round.
  host route   what the library offered before: per round dev.step(), a download of
               the lanes' scalars (the statuses), the plan on the host (NumPy: the
               MG_FORK lanes in ascending order, the next free lanes as jump lanes,
               the fall-through in place), dev.fork().  The table of which lane
               descends from which, which the host must also keep, is not timed.

Both must leave the same device image (every live cell of every lane); the
script asserts it.  The host cannot know from the scalars whether a jump target
is valid; it hands a free lane to every source.  The two plans therefore agree
only while every jump is made, which the script checks and reports.

Repetitions alternate between the two routes.  Prints one JSON object with the
range of every figure; --out also writes it to a file.
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
from mythril_amd.lanes import (_ALL_FIELDS, _SYM_FIELDS, _U32_FIELDS, _U64_FIELDS, MG_FORK, MG_FORK_MADE_FALL,  # noqa: E402
                               MG_FORK_MADE_JUMP, MG_HALT_STOP, MG_LANE_SYMBOLIC, MG_LANE_TAINT, LaneBatch)
from xfermodel import live_diff  # noqa: E402

PATH_CAP = 16
CTR_BYTES = 32        # the counter block the explorer reads back per round


def scalars(dev, b):
    """The lanes' scalars only (NULL row pointers are skipped by mg_lanes_download)."""
    soa = b.soa()
    for f in ("calldata", "env", "stack", "memory", "storage", "trace", "rec"):
        setattr(soa, f, None)
    dev._check(dev.lib.mg_lanes_download(dev.ctx, ctypes.addressof(soa), 0, b.n), "mg_lanes_download")


def whole_image(dev, shape):
    out = LaneBatch(shape)
    dev.download(out)
    return out


def span(xs):
    return {"min": float(min(xs)), "max": float(max(xs)), "all": [float(x) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--live", type=int, default=0, help="live lanes (default: half of --lanes); the rest are spare")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    half = args.live or args.lanes // 2
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
    cur = LaneBatch(shape)
    scalar_bytes = sum(getattr(cur, f).nbytes for f in _U32_FIELDS + _U64_FIELDS if getattr(cur, f) is not None)

    def explorer(rounds):
        dev.upload(b)
        dev.sync()
        t0 = time.perf_counter()
        st = dev.explore(free, max_rounds=rounds)
        wall = (time.perf_counter() - t0) * 1e3
        return {"wall_ms": wall / st.rounds, "kernel_ms": st.kernel_ms / st.rounds,
                "pcie_bytes": (free.nbytes + st.rounds * CTR_BYTES) / st.rounds,
                "rounds": st.rounds, "forks": st.forks, "made_jump": st.made_jump, "starved": st.starved,
                "path_full": st.path_full, "lane_steps": st.lane_steps}

    def host_route(rounds):
        dev.upload(b)
        dev.sync()
        used = forks = jumps = pcie = 0
        kernel = 0.0
        all_made = True
        t0 = time.perf_counter()
        for _ in range(rounds):
            st = dev.step()
            scalars(dev, cur)
            src = np.nonzero((cur.status == MG_FORK) & ((cur.flags & MG_LANE_SYMBOLIC) != 0) &
                             ((cur.flags & MG_LANE_TAINT) == 0))[0].astype(np.uint32)
            src = src[:free.size - used]
            dst_jump = free[used:used + src.size]
            made, _, ms = dev.fork(src, src, dst_jump)
            used += int(src.size)
            forks += int(src.size)
            jumps += int(((made & MG_FORK_MADE_JUMP) != 0).sum())
            all_made &= bool((made == (MG_FORK_MADE_FALL | MG_FORK_MADE_JUMP)).all())
            kernel += st.kernel_ms + ms
            pcie += scalar_bytes + (5 * int(src.size) + 2 * int(src.size)) * 4
        wall = (time.perf_counter() - t0) * 1e3
        return {"wall_ms": wall / rounds, "kernel_ms": kernel / rounds, "pcie_bytes": pcie / rounds, "rounds": rounds,
                "forks": forks, "made_jump": jumps, "every_jump_made": all_made}

    out = {"lanes": args.lanes, "live_lanes": half, "spare_lanes": int(free.size), "path_cap": PATH_CAP,
           "reps": args.reps, "rounds": {}}
    explorer(1), host_route(1)                      # warm-up
    for rounds in (1, 3):
        ex, ho = [], []
        for _ in range(args.reps):                  # alternating
            ex.append(explorer(rounds))
            image_ex = whole_image(dev, shape) if len(ex) == args.reps else None
            ho.append(host_route(rounds))
        image_ho = whole_image(dev, shape)
        # the host hands out free lanes in the same order; it plans the same forks while every jump is made
        same_plan = all(h["every_jump_made"] for h in ho) and ex[-1]["path_full"] == 0
        diffs = live_diff(image_ex, image_ho)
        if same_plan:
            assert diffs == [], diffs
            assert ex[-1]["forks"] == ho[-1]["forks"] and ex[-1]["made_jump"] == ho[-1]["made_jump"]
        rec = {"same_plan": same_plan, "same_image": diffs == [],
               "forks": ex[-1]["forks"], "made_jump": ex[-1]["made_jump"], "lane_steps": ex[-1]["lane_steps"],
               "starved": ex[-1]["starved"], "rounds_run": ex[-1]["rounds"]}
        for what, runs in (("explorer", ex), ("host_route", ho)):
            rec[what] = {k + "_per_round": span([r[k] for r in runs]) for k in ("wall_ms", "kernel_ms", "pcie_bytes")}
        rec["explorer_slowest_is_faster_than_host_fastest"] = \
            rec["explorer"]["wall_ms_per_round"]["max"] < rec["host_route"]["wall_ms_per_round"]["min"]
        out["rounds"][str(rounds)] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
