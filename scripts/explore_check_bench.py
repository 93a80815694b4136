#!/usr/bin/env python
"""mg_explore_check against the host's fork-filter route, on scripts/explore_bench.py's batch.

Run by hand on the MI355X (under a timeout); bench.py does not call it.

The batch: `--lanes` lanes (65,536), the first half the start of a symbolic message
call into each of the 18 reference contracts (bench.symbolic_lane_batch), the rest
spare; one mg_explore round forks every live lane.  Then, for 64, 1,024 and 4,096
candidate models (per transaction id: a dispatcher selector of its contract with 36
bytes of calldata, empty calldata, or nothing), "which model satisfies each
successor's path" goes two ways:

  device route  GpuDevice.explore_check over every lane, the pool resident: kernel ms
                and wall.
  host route    what the fork filter does today, each stage timed: the download of the
                lanes; symbolic.path_constraints (decode); flatten.compile_sets; the
                model pool for the compiled programs; GpuDevice.eval_bits.  Decode,
                flatten, pool and eval_bits run over a strided sample of `--sample`
                successors (the whole batch takes minutes in Python); the record
                holds the sample's figures and, marked as such, their scaling to all
                successors.  The download is always the whole batch.

On the sample the two routes' verdicts must agree wherever the device does not answer
MG_PATH_UNKNOWN (asserted).  tests/pathmodel.py counts the unknown lanes of the whole
batch once.  Repetitions alternate between the routes.  Prints one JSON object with
the range of every figure; --out also writes it to a file.
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

import bench  # noqa: E402
import pathmodel  # noqa: E402
from mythril_amd import abi, workloads  # noqa: E402
from mythril_amd.device import GpuDevice  # noqa: E402
from mythril_amd.lanes import _ALL_FIELDS, _SYM_FIELDS, MG_HALT_STOP, LaneBatch  # noqa: E402
from mythril_amd.laser import (Account, Disassembly, MessageCallTransaction, SymbolicCalldata,  # noqa: E402
                               WorldState)
from mythril_amd.laser import symbolic as sym  # noqa: E402
from mythril_amd.laser.transaction import ACTORS  # noqa: E402
from mythril_amd.smt import flatten  # noqa: E402
from mythril_amd.smt.expr import symbol_factory  # noqa: E402
from mythril_amd.smt.lower import TableSig  # noqa: E402
from mythril_amd.smt.program import ArrayInterp, ModelPool  # noqa: E402

PATH_CAP = 16


def root_states():
    """The states bench.symbolic_lane_batch packs, by the same recipe (transaction ids 1..18)."""
    codes = json.loads((ROOT / "tests" / "golden" / "bytecodes.json").read_text())
    out = []
    for k, name in enumerate(sorted(codes)):
        ws = WorldState()
        ws.put_account(Account(ACTORS["CREATOR"]))
        acct = Account(workloads.CONTRACT, code=Disassembly(workloads.bytecode(name)), concrete_storage=False)
        ws.put_account(acct)
        t = str(k + 1)
        sender = symbol_factory.BitVecSym(f"sender_{t}", 256)
        tx = MessageCallTransaction(world_state=ws, identifier=t, gas_price=symbol_factory.BitVecSym(f"gas_price{t}", 256),
                                    gas_limit=8_000_000, origin=sender, caller=sender, callee_account=acct,
                                    call_data=SymbolicCalldata(t), call_value=symbol_factory.BitVecSym(f"call_value{t}", 256))
        gs = tx.initial_global_state()
        gs.transaction_stack.append((tx, None))
        out.append(gs)
    return out


def model_dicts(states, count: int):
    rng = np.random.default_rng(0xC4EC)
    actors = list(ACTORS.values())
    out = []
    for m in range(count):
        d = {}
        for k, s in enumerate(states):
            t = str(k + 1)
            sels = sorted({int(h, 16) for h in s.environment.code.func_hashes}) or [0]
            how = int(rng.integers(0, 8))
            if how == 0:
                continue                                    # nothing for this transaction: all zero
            d[f"sender_{t}"] = actors[int(rng.integers(0, len(actors)))]
            if how == 1:
                d[f"{t}_calldata"] = ArrayInterp(0xFF)      # empty calldata
                continue
            sel = sels[int(rng.integers(0, len(sels)))]
            cd = {j: (sel >> (8 * (3 - j))) & 0xFF for j in range(4)}
            cd[35] = int(rng.integers(0, 256))
            d[f"{t}_calldatasize"] = 36
            d[f"{t}_calldata"] = ArrayInterp(0, cd)
            if how == 2:
                d[f"call_value{t}"] = 1
        out.append(d)
    return out


def span(xs):
    return {"min": float(min(xs)), "max": float(max(xs)), "all": [float(x) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1024)
    ap.add_argument("--models", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    half = args.lanes // 2
    dev = GpuDevice(0)
    _, live = bench.symbolic_lane_batch(dev, half)
    states = root_states()
    shape = replace(live.shape, n=args.lanes)
    b = LaneBatch(shape)
    for f in _ALL_FIELDS + _SYM_FIELDS:
        getattr(b, f)[:half] = getattr(live, f)
    b.code_id[half:] = b.code_id[0]
    b.status[half:] = MG_HALT_STOP
    dev.alloc(shape)
    dev.explore_alloc(PATH_CAP)
    dev.upload(b)
    st = dev.explore(np.arange(half, args.lanes, dtype=np.uint32), max_rounds=1)
    paths = dev.explore_paths(0, args.lanes)
    path, path_len, root = paths
    # lineage of root lane l: the contract it was packed from (symbolic_lane_batch's "code" order)
    contract = np.arange(half) * len(states) // half
    lane_binding = np.full(args.lanes, abi.MG_PATH_UNBOUND, dtype=np.uint32)
    lane_binding[:half] = contract
    var_names = [n for k in range(len(states)) for n in (f"{k + 1}_calldatasize", f"sender_{k + 1}",
                                                         f"call_value{k + 1}", f"gas_price{k + 1}")]
    storage = states[0].environment.active_account.storage.base_raw.param[0]
    tables = [TableSig(f"{k + 1}_calldata", "array", (256,), 8) for k in range(len(states))] + \
             [TableSig(storage, "array", (256,), 256)]
    bindings = [sym.path_binding(s, var_names, tables) for s in states]
    successors = np.nonzero((root < half) & (path_len > 0))[0]
    sample = successors[::max(1, successors.size // args.sample)][:args.sample]
    image = LaneBatch(shape)
    dev.download(image)
    t0 = time.perf_counter()
    unknown_model = sum(pathmodel.lane_unknown(image, int(l), path[l, :int(path_len[l])], int(root[l]), bindings,
                                               lane_binding) for l in successors)
    model_s = time.perf_counter() - t0
    out = {"lanes": args.lanes, "live_lanes": half, "forks": st.forks, "successors": int(successors.size),
           "explore_kernel_ms": st.kernel_ms, "sample": int(sample.size), "reps": args.reps,
           "unknown_lanes_by_model": int(unknown_model), "unknown_share": unknown_model / max(successors.size, 1),
           "model_cone_pass_s": model_s, "models": {}}

    for count in args.models:
        ms = model_dicts(states, count)
        pool = ModelPool.from_dicts(ms, var_names, [256] * len(var_names), tables)
        t0 = time.perf_counter()
        fs, _, first_kernel = dev.explore_check(pool, bindings, lane_binding)
        first_wall = (time.perf_counter() - t0) * 1e3

        def device_route():
            t0 = time.perf_counter()
            got, _, kernel = dev.explore_check(None, bindings, lane_binding)
            return {"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": kernel}, got

        def host_route():
            r = {}
            t0 = time.perf_counter()
            dev.download(image)
            t1 = time.perf_counter()
            sets = [sym.path_constraints(image, int(l), states[int(contract[root[l]])], path[l, :int(path_len[l])])
                    for l in sample]
            t2 = time.perf_counter()
            alive = [k for k, s in enumerate(sets) if s is not None]
            prog, kept = flatten.compile_sets([sets[k] for k in alive])
            t3 = time.perf_counter()
            k2_pool = ModelPool.from_dicts(ms, prog.var_names, prog.var_widths, prog.tables)
            t4 = time.perf_counter()
            k2_fs, _, _, k2_ms = dev.eval_bits(prog, k2_pool)
            t5 = time.perf_counter()
            r.update(download_ms=(t1 - t0) * 1e3, decode_ms=(t2 - t1) * 1e3, flatten_ms=(t3 - t2) * 1e3,
                     pool_ms=(t4 - t3) * 1e3, eval_bits_ms=(t5 - t4) * 1e3, eval_kernel_ms=k2_ms)
            verdict = np.full(sample.size, abi.MG_BV_NO_MODEL, dtype=np.uint32)
            verdict[[alive[k] for k in kept]] = k2_fs
            undecided = set(range(sample.size)) - set(alive[k] for k in kept) - \
                set(k for k, s in enumerate(sets) if s is None)
            return r, verdict, undecided

        dev_runs, host_runs = [], []
        for _ in range(args.reps):                      # alternating
            d, got = device_route()
            assert got.tolist() == fs.tolist()
            h, verdict, undecided = host_route()
            dev.explore_check(pool, bindings, lane_binding)     # eval_bits replaced the pool: make it resident again
            for k, l in enumerate(sample):
                if got[l] != abi.MG_PATH_UNKNOWN and k not in undecided:
                    assert int(got[l]) == int(verdict[k]), (count, int(l), int(got[l]), int(verdict[k]))
            dev_runs.append(d)
            host_runs.append(h)
        scale = successors.size / max(sample.size, 1)
        rec = {"first_call_with_upload": {"wall_ms": first_wall, "kernel_ms": first_kernel},
               "device": {k: span([r[k] for r in dev_runs]) for k in ("wall_ms", "kernel_ms")},
               "host_sample": {k: span([r[k] for r in host_runs]) for k in host_runs[0]},
               "satisfied": int((fs[successors] < count).sum()),
               "no_model": int((fs[successors] == abi.MG_BV_NO_MODEL).sum()),
               "unknown": int((fs[successors] == abi.MG_PATH_UNKNOWN).sum())}
        # the host route over every successor: the whole download as measured, the sampled stages scaled
        host_total = [r["download_ms"] + scale * (r["decode_ms"] + r["flatten_ms"] + r["pool_ms"] + r["eval_bits_ms"])
                      for r in host_runs]
        host_sample_total = [sum(r[k] for k in ("download_ms", "decode_ms", "flatten_ms", "pool_ms", "eval_bits_ms"))
                             for r in host_runs]
        rec["host_total_ms_scaled_from_sample"] = span(host_total)
        rec["host_total_ms_sample_only"] = span(host_sample_total)
        rec["device_slowest_is_faster_than_host_fastest"] = rec["device"]["wall_ms"]["max"] < min(host_total)
        rec["device_slowest_is_faster_than_host_sample_fastest"] = rec["device"]["wall_ms"]["max"] < min(host_sample_total)
        assert rec["unknown"] == unknown_model
        out["models"][str(count)] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
