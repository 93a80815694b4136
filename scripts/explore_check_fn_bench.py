#!/usr/bin/env python
"""mg_explore_check_fn: what binding the models' function tables buys, and what it costs.

Run by hand on the MI355X (under a timeout); bench.py does not call it.  The batches
are scripts/explore_check_bench.py's (bench.symbolic_lane_batch: the start of a
symbolic message call into each of the 18 reference contracts), whose root states and
candidate models this script takes as they are.

  --mode share   `--live` live lanes (8,192) in `--lanes` lanes (65,536: room for three
                 rounds of forks).  After 1, 2 and 3 explore rounds (--round-list), each from
                 a fresh upload: the share of successors the device answers MG_PATH_UNKNOWN with
                 nothing bound and with symbolic.path_functions bound, on the same
                 build, and what remains unknown by cause (tests/pathfnmodel.py's cone
                 pass over a strided sample of the unknown lanes).
  --mode cost    the one-round batch (every lane forks once, no function cones) at 64,
                 1,024 and 4,096 models: kernel ms and wall of mg_explore_check with the
                 pool resident.  One process measures one library (MYTHGPU_LIB); the
                 caller alternates the parent's and this one's and compares ranges.
  --mode cones   the `--live` batch after `--rounds` rounds: the device route with the
                 tables bound against the host route (download, decode, flatten, pool,
                 eval_bits, the last four over a strided sample), alternating; the two
                 routes must agree on first_sat over the sample (asserted).

Prints one JSON object; --out also writes it to a file.
"""
import argparse
import json
import sys
import time
from collections import Counter
from dataclasses import replace
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

import bench  # noqa: E402
import pathfnmodel  # noqa: E402
from explore_check_bench import PATH_CAP, model_dicts, root_states, span  # noqa: E402
from mythril_amd import abi  # noqa: E402
from mythril_amd.device import GpuDevice  # noqa: E402
from mythril_amd.lanes import _ALL_FIELDS, _SYM_FIELDS, MG_HALT_STOP, LaneBatch  # noqa: E402
from mythril_amd.laser import symbolic as sym  # noqa: E402
from mythril_amd.smt import flatten  # noqa: E402
from mythril_amd.smt.lower import TableSig  # noqa: E402
from mythril_amd.smt.program import ModelPool  # noqa: E402

UNKNOWN = abi.MG_PATH_UNKNOWN


class Batch:
    """`live` root lanes in `lanes` lanes, uploaded afresh by explore(rounds)."""

    def __init__(self, dev, live: int, lanes: int):
        self.dev, self.live, self.lanes = dev, live, lanes
        _, packed = bench.symbolic_lane_batch(dev, live)
        self.states = root_states()
        self.shape = replace(packed.shape, n=lanes)
        b = self.b = LaneBatch(self.shape)
        for f in _ALL_FIELDS + _SYM_FIELDS:
            getattr(b, f)[:live] = getattr(packed, f)
        b.code_id[live:] = b.code_id[0]
        b.status[live:] = MG_HALT_STOP
        self.contract = np.arange(live) * len(self.states) // live
        self.lane_binding = np.full(lanes, abi.MG_PATH_UNBOUND, dtype=np.uint32)
        self.lane_binding[:live] = self.contract
        n = len(self.states)
        self.var_names = [v for k in range(n) for v in (f"{k + 1}_calldatasize", f"sender_{k + 1}",
                                                        f"call_value{k + 1}", f"gas_price{k + 1}")]
        storage = self.states[0].environment.active_account.storage.base_raw.param[0]
        self.base_tables = [TableSig(f"{k + 1}_calldata", "array", (256,), 8) for k in range(n)] + \
                           [TableSig(storage, "array", (256,), 256)]

    def explore(self, rounds: int):
        dev = self.dev
        dev.alloc(self.shape)
        dev.explore_alloc(PATH_CAP)
        dev.upload(self.b)
        st = dev.explore(np.arange(self.live, self.lanes, dtype=np.uint32), max_rounds=rounds)
        self.paths = dev.explore_paths(0, self.lanes)
        _, path_len, root = self.paths
        self.successors = np.nonzero((root < self.live) & (path_len > 0))[0]
        return st

    def image(self):
        out = LaneBatch(self.shape)
        self.dev.download(out)
        return out

    def tables(self, image):
        """The pool's tables: the arrays, Power, and keccak256_<w> for every input width the image holds."""
        kinds, imm = image.node[:, :, 0] & 0xFF, image.node[:, :, 3]
        used = np.arange(image.node.shape[1])[None, :] < image.n_nodes[:, None]
        widths = sorted(int(w) for w in np.unique(imm[(kinds == abi.MG_SYM_KECCAK) & used]))
        return self.base_tables + [TableSig("Power", "uf", (256, 256), 256)] + \
            [TableSig(f"keccak256_{w}", "uf", (w,), 256) for w in widths if 1 <= w <= 4096], widths

    def pool(self, tables, count):
        ms = model_dicts(self.states, count)
        return ms, ModelPool.from_dicts(ms, self.var_names, [256] * len(self.var_names), tables)


def cause(image, l, row, root, bindings, lane_binding, fn) -> str:
    """Why the cone pass of tests/pathfnmodel.py calls lane l unknown."""
    try:
        pathfnmodel._cone_of(image, l, row, root, bindings, lane_binding, fn)
    except pathfnmodel._Unknown as e:
        what = str(e)
        if not what.startswith("node "):
            return "keccak input: " + what if "part" in what or "leaves" in what or "wide" in what else what
        x, _, _, w = pathfnmodel._Lane(image, l).rows[int(what[5:])]
        kind = x & 0xFF
        if kind == abi.MG_SYM_MLOADK:
            return "MLOADK"
        if kind == abi.MG_SYM_TERM:
            return "TERM"
        if kind == abi.MG_SYM_ENV:
            return "fresh environment word" if w >= abi.MG_ENV_WORDS else "environment word unbound"
        if kind == abi.MG_SYM_KECCAK:
            return "KECCAK input above 512 bits" if w > 512 else "KECCAK width unbound"
        if kind == abi.MG_SYM_BIN:
            return f"BIN opcode {w:#x}"
        return f"kind {kind}"
    return "known"


def mode_share(dev, args):
    bt = Batch(dev, args.live, args.lanes)
    out = {"mode": "share", "live_lanes": args.live, "lanes": args.lanes, "models": args.models[0], "rounds": {}}
    for rounds in args.round_list:
        st = bt.explore(rounds)
        image = bt.image()
        tables, widths = bt.tables(image)
        _, pool = bt.pool(tables, args.models[0])
        bindings = [sym.path_binding(s, bt.var_names, tables) for s in bt.states]
        fn = sym.path_functions(tables)
        bare, _, bare_ms = dev.explore_check(pool, bindings, bt.lane_binding)
        bound, _, bound_ms = dev.explore_check(None, bindings, bt.lane_binding, functions=fn)
        succ = bt.successors
        unk_bare, unk_bound = succ[bare[succ] == UNKNOWN], succ[bound[succ] == UNKNOWN]
        assert set(unk_bound.tolist()) <= set(unk_bare.tolist())
        path, path_len, root = bt.paths
        sample = unk_bound[::max(1, unk_bound.size // args.sample)][:args.sample]
        F = pathfnmodel.Functions(fn)
        causes = Counter(cause(image, int(l), [int(e) for e in path[l, :int(path_len[l])]], int(root[l]), bindings,
                               bt.lane_binding, F) for l in sample)
        assert "known" not in causes, "the device calls a lane unknown that the model evaluates"
        out["rounds"][str(rounds)] = {
            "rounds_run": st.rounds, "forks": st.forks, "starved": st.starved, "path_full": st.path_full,
            "successors": int(succ.size), "keccak_widths_in_image": widths,
            "keccak_widths_bound": [int(fn.keccak_bits[j]) for j in range(fn.n_keccak)],
            "unknown_nothing_bound": int(unk_bare.size), "unknown_share_nothing_bound": unk_bare.size / max(succ.size, 1),
            "unknown_functions_bound": int(unk_bound.size), "unknown_share_functions_bound": unk_bound.size / max(succ.size, 1),
            "kernel_ms_nothing_bound": bare_ms, "kernel_ms_functions_bound": bound_ms,
            "remaining_unknown_sample": int(sample.size), "remaining_unknown_by_cause": dict(causes)}
    return out


def mode_cost(dev, args):
    bt = Batch(dev, args.lanes // 2, args.lanes)
    st = bt.explore(1)
    bindings = [sym.path_binding(s, bt.var_names, bt.base_tables) for s in bt.states]
    out = {"mode": "cost", "lanes": args.lanes, "forks": st.forks, "successors": int(bt.successors.size),
           "reps": args.reps, "models": {}}
    for count in args.models:
        _, pool = bt.pool(bt.base_tables, count)
        fs, _, _ = dev.explore_check(pool, bindings, bt.lane_binding)
        wall, kernel = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got, _, ms = dev.explore_check(None, bindings, bt.lane_binding)
            wall.append((time.perf_counter() - t0) * 1e3)
            kernel.append(ms)
            assert got.tolist() == fs.tolist()
        out["models"][str(count)] = {"wall_ms": span(wall), "kernel_ms": span(kernel),
                                     "unknown": int((fs[bt.successors] == UNKNOWN).sum())}
    return out


def mode_cones(dev, args):
    bt = Batch(dev, args.live, args.lanes)
    st = bt.explore(args.rounds)
    image = bt.image()
    tables, _ = bt.tables(image)
    bindings = [sym.path_binding(s, bt.var_names, tables) for s in bt.states]
    fn = sym.path_functions(tables)
    path, path_len, root = bt.paths
    succ = bt.successors
    out = {"mode": "cones", "live_lanes": args.live, "lanes": args.lanes, "rounds": st.rounds, "forks": st.forks,
           "successors": int(succ.size), "reps": args.reps, "models": {}}
    for count in args.models:
        ms, pool = bt.pool(tables, count)
        fs, _, _ = dev.explore_check(pool, bindings, bt.lane_binding, functions=fn)
        bare, _, _ = dev.explore_check(None, bindings, bt.lane_binding)
        # the lanes the tables decide: unknown with nothing bound, answered with them
        decided = succ[(bare[succ] == UNKNOWN) & (fs[succ] != UNKNOWN)]
        sample = decided[::max(1, decided.size // args.sample)][:args.sample]
        if sample.size == 0:                            # no cone of this image reads a function
            out["models"][str(count)] = {"decided_by_the_tables": 0}
            continue
        dev_runs, host_runs = [], []
        for _ in range(args.reps):                      # alternating
            t0 = time.perf_counter()
            got, _, kernel = dev.explore_check(None, bindings, bt.lane_binding, functions=fn)
            dev_runs.append({"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": kernel})
            assert got.tolist() == fs.tolist()
            t0 = time.perf_counter()
            dev.download(image)
            t1 = time.perf_counter()
            sets = [sym.path_constraints(image, int(l), bt.states[int(bt.contract[root[l]])], path[l, :int(path_len[l])])
                    for l in sample]
            t2 = time.perf_counter()
            alive = [k for k, s in enumerate(sets) if s is not None]
            prog, kept = flatten.compile_sets([sets[k] for k in alive])
            t3 = time.perf_counter()
            k2_pool = ModelPool.from_dicts(ms, prog.var_names, prog.var_widths, prog.tables)
            t4 = time.perf_counter()
            k2_fs, _, _, k2_ms = dev.eval_bits(prog, k2_pool)
            t5 = time.perf_counter()
            host_runs.append({"download_ms": (t1 - t0) * 1e3, "decode_ms": (t2 - t1) * 1e3, "flatten_ms": (t3 - t2) * 1e3,
                              "pool_ms": (t4 - t3) * 1e3, "eval_bits_ms": (t5 - t4) * 1e3, "eval_kernel_ms": k2_ms})
            dev.explore_check(pool, bindings, bt.lane_binding, functions=fn)    # eval_bits replaced the pool
            verdict = np.full(sample.size, abi.MG_BV_NO_MODEL, dtype=np.uint32)
            verdict[[alive[k] for k in kept]] = k2_fs
            compared = set(alive[k] for k in kept) | set(k for k, s in enumerate(sets) if s is None)
            for k, l in enumerate(sample):
                if k in compared:
                    assert int(got[l]) == int(verdict[k]), (count, int(l), int(got[l]), int(verdict[k]))
        scale = decided.size / max(sample.size, 1)      # the host route takes only the lanes the device leaves
        host_total = [r["download_ms"] + scale * (r["decode_ms"] + r["flatten_ms"] + r["pool_ms"] + r["eval_bits_ms"])
                      for r in host_runs]
        out["models"][str(count)] = {
            "decided_by_the_tables": int(decided.size), "sample": int(sample.size), "compared": len(compared),
            "unknown_functions_bound": int((fs[succ] == UNKNOWN).sum()), "unknown_nothing_bound": int((bare[succ] == UNKNOWN).sum()),
            "device": {k: span([r[k] for r in dev_runs]) for k in ("wall_ms", "kernel_ms")},
            "host_sample": {k: span([r[k] for r in host_runs]) for k in host_runs[0]},
            "host_total_ms_for_the_decided_lanes": span(host_total)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("share", "cost", "cones"), required=True)
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--live", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--round-list", type=int, nargs="*", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--models", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = GpuDevice(0)
    out = {"share": mode_share, "cost": mode_cost, "cones": mode_cones}[args.mode](dev, args)
    dev.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
