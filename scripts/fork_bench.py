#!/usr/bin/env python
"""mg_lanes_fork against the host image route, on bench.py's symbolic_lanes batch.

Run by hand on the MI355X (under a timeout); bench.py does not call it.

The batch: `--lanes` lanes (65,536), the first half the start of a symbolic
message call into each of the 18 reference contracts (bench.symbolic_lane_batch),
the second half spare.  One launch takes every live lane to its first stop;
those that stopped with MG_FORK are forked two ways, from the same device image:

  device route      one mg_lanes_fork call: in place for the fall-through, the
                    jump child into a spare lane.  kernel_ms (HIP events around the
                    three launches) and the wall time of the call.
  host image route  the parent commit's way of moving a lane image: a live
                    download of the sources, the NumPy model of the fork
                    (tests/forkmodel.py) on the host, a live upload of the children.

Both routes must leave the same device image (every live cell of every lane).
Then fork and step alternate with no lane state crossing PCIe until the spare
lanes run out: lane-steps per started path between host round trips of lane
state, against 7 with host forks.

Prints one JSON object; --out also writes it to a file.
"""
import argparse
import ctypes
import json
import sys
import time
import types
from dataclasses import replace
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bench  # noqa: E402
import forkmodel  # noqa: E402
from mythril_amd.device import GpuDevice  # noqa: E402
from mythril_amd.lanes import (_ALL_FIELDS, _SYM_FIELDS, MG_FORK, MG_FORK_MADE_FALL, MG_FORK_MADE_JUMP,  # noqa: E402
                               MG_HALT_STOP, LaneBatch)
from xfermodel import DeviceImage, live_diff  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
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
    codes = {int(c): forkmodel.CodeTable(dev.codes[int(c)]) for c in np.unique(b.code_id)}
    dev.alloc(shape)

    def to_first_stop():
        dev.upload(b)
        return dev.step()

    st0 = to_first_stop()
    at = LaneBatch(shape)
    scalars(dev, at)
    src = np.nonzero(at.status[:half] == MG_FORK)[0].astype(np.uint32)
    n = int(src.size)
    if n == 0:
        raise SystemExit("no lane stopped with MG_FORK")
    dst_fall = src.copy()
    dst_jump = (half + np.arange(n)).astype(np.uint32)

    # ---- device route: warm-up, then reps from the same image
    dev.fork(src, dst_fall, dst_jump)
    kms, wall = [], []
    for _ in range(args.reps):
        to_first_stop()
        dev.sync()
        t0 = time.perf_counter()
        made, cond, ms = dev.fork(src, dst_fall, dst_jump)
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(ms)
    image_dev = whole_image(dev, shape)
    n_jump = int(((made & MG_FORK_MADE_JUMP) != 0).sum())
    assert int(((made & MG_FORK_MADE_FALL) != 0).sum()) == n

    # ---- host image route: download_range(live), the model, upload_range(live)
    host_ms = []
    hb, at_stop = LaneBatch(shape), None
    for _ in range(args.host_reps):
        to_first_stop()
        dev.sync()
        hb = b.copy()                       # env and calldata: a live download leaves the host's
        t0 = time.perf_counter()
        dev.download_range(hb, 0, half, live=True)
        t1 = time.perf_counter()
        if at_stop is None:
            at_stop = types.SimpleNamespace(shape=shape, **{f: getattr(hb, f)[:half].copy() for f in (
                "sp", "msize", "storage_count", "n_nodes", "n_consts", "trace_len", "rec_len")})
        model = DeviceImage.__new__(DeviceImage)
        model.shape, model.img = shape, hb
        want_made, want_cond = forkmodel.fork(model, codes, src, dst_fall, dst_jump)
        t2 = time.perf_counter()
        dev.upload_range(hb, 0, shape.n, live=True)
        dev.sync()
        t3 = time.perf_counter()
        host_ms.append({"download_ms": (t1 - t0) * 1e3, "model_ms": (t2 - t1) * 1e3, "upload_ms": (t3 - t2) * 1e3,
                        "total_ms": (t3 - t0) * 1e3})
    assert want_made.tolist() == made.tolist() and want_cond.tolist() == cond.tolist()
    image_host = whole_image(dev, shape)
    diffs = live_diff(image_dev, image_host)
    assert diffs == [], diffs

    # ---- bytes per fork: what crosses PCIe on the device route, what a successor's live image holds
    live_b = float(np.mean([forkmodel.live_bytes(at_stop, int(s)) for s in src[:4096]]))
    pcie_dev = (3 * n + 2 * n_jump + 2 * n) * 4 / max(n, 1)

    # ---- fork and step in turn, no lane state through the host, until the spare lanes run out
    to_first_stop()
    free = list(range(shape.n - 1, half - 1, -1))
    lane_steps, visits, forks_done = int(st0.lane_steps), 1, 0
    cur = LaneBatch(shape)
    while True:
        scalars(dev, cur)
        f = np.nonzero(cur.status == MG_FORK)[0]
        f = f[:len(free)]
        if f.size == 0:
            break
        dj = np.array([free.pop() for _ in range(f.size)], dtype=np.uint32)
        made_k, _, _ = dev.fork(f.astype(np.uint32), f.astype(np.uint32), dj)
        forks_done += int(f.size)
        free.extend(int(x) for x in dj[(made_k & MG_FORK_MADE_JUMP) == 0])
        st = dev.step()
        visits += 1
        lane_steps += int(st.lane_steps)
        if st.lane_steps == 0:
            break
    out = {
        "lanes": args.lanes, "live_lanes": half, "forks": n, "jump_children": n_jump,
        "first_launch_lane_steps_per_lane": st0.lane_steps / half,
        "device_route": {"kernel_ms": float(np.median(kms)), "kernel_ms_all": kms,
                         "wall_ms": float(np.median(wall)), "wall_ms_all": wall,
                         "pcie_bytes_per_fork": pcie_dev},
        "host_image_route": {"total_ms": float(np.median([h["total_ms"] for h in host_ms])), "all": host_ms},
        "same_image": True,
        "live_bytes_per_fork_model": live_b,
        "alternating": {"launches": visits, "device_forks": forks_done, "lane_steps": lane_steps,
                        "lane_steps_per_started_path_without_lane_state_on_pcie": lane_steps / half,
                        "with_host_forks": st0.lane_steps / half},
    }
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
