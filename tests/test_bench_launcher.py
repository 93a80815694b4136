"""bench.py --gpus N starts N ranks itself (bench.launch_ranks) when WORLD_SIZE is
unset.  On CPU: 2 gloo ranks with the oracle device; the one JSON line reports
n_gpus == 2, weak scaling, and the whole-job lane-steps of both ranks."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


def test_two_ranks_from_the_bench_entry(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    code = ("import sys; sys.path.insert(0, %r); import bench; "
            "sys.exit(bench.launch_ranks(2, sys.argv[1:], script=%r))" %
            (str(ROOT), str(HERE / "bench_rank_cpu.py")))
    argv = ["--gpus", "2", "--steps", "2", "--warmup", "1", "--lanes", "128", "--full", "--no-c4",
            "--no-cpu-baseline", "--no-roofline", "--rec-cap", "0", "--full-record", str(tmp_path / "full.json")]
    p = subprocess.run([sys.executable, "-c", code] + argv, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak"
    per_rank = out["config"]["lane_steps_per_batch"]
    # whole-job value = both ranks' lane-steps / the slower rank's time
    assert out["value"] > 0 and out["value"] * out["ms_per_step"] / 1e3 > 1.5 * per_rank


def test_launcher_returns_worst_status(tmp_path):
    import bench
    bad = tmp_path / "fail_rank.py"
    bad.write_text("import os, sys; sys.exit(3 if os.environ['RANK'] == '1' else 0)\n")
    assert bench.launch_ranks(2, [], script=str(bad)) == 3


def test_compact_line_fits_the_driver(tmp_path):
    """the driver keeps ~12 KB of output, so the one JSON
    line stays <= 4 KB with every contract key, the roofline and the CPU
    baseline -- checked on round 5's full record (23 KB, every field), and on a
    line bench.py prints on the oracle device."""
    import bench
    full = json.loads((HERE / "golden" / "bench_full_r05.json").read_text())
    line = bench.compact_line(full, "profiles/x.json")
    text = json.dumps(line)
    assert len(text) <= bench.LINE_LIMIT
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert line["fields"]["c4"]["roofline"]["frac"] > 0
    assert line["fields"]["myth_analyze"]["totals"]["issues"] == 26
    assert json.loads(text)["value"] == line["value"]


def _plain_run(tmp_path, dump, steps):
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    code = ("import sys; sys.path.insert(0, %r); import bench; "
            "sys.exit(bench.launch_ranks(1, sys.argv[1:], script=%r))" %
            (str(ROOT), str(HERE / "bench_rank_cpu.py")))
    argv = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--lanes", "192", "--dump-outputs", str(dump)]
    p = subprocess.run([sys.executable, "-c", code] + argv, env=env, capture_output=True, text=True,
                       timeout=300, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096
    return json.loads(lines[0]), {f.stem: np.load(f) for f in sorted(dump.glob("*.npy"))}, p.stderr


def test_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    """Without --full the benchmark runs the warm-up and the timed steps only:
    no secondary field, baseline, roofline or full record.  --dump-outputs
    writes the last timed step's lanes (float32 / float64, within 64 MB); the
    inputs are seeded, so a second run writes the same arrays, and they agree
    with the result line."""
    import numpy as np
    line, a, err = _plain_run(tmp_path, tmp_path / "a", 3)
    line2, b, _ = _plain_run(tmp_path, tmp_path / "b", 2)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line2["steps"] == 2 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(
        line["config"]["lane_steps_per_batch"] / (line["ms_per_step"] / 1e3), rel=1e-2)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["fields"] == {}
    assert line["full_record"] is None
    assert [p.name for p in tmp_path.iterdir()] in (["a", "b"], ["b", "a"])      # nothing else written
    for gone in ("unbucketed", "two streams", "3,523", "roofline", "hooked", "taint", "symbolic", "C3", "C4",
                 "CPU baseline"):
        assert gone not in err, gone
    assert set(a) == set(b) and {"step_stats", "coverage", "status", "pc", "sp", "steps", "gas_min", "gas_max",
                                 "sample_lanes", "stack", "memory", "storage", "rec"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["steps"].shape == (192,) and a["steps"].sum() == a["step_stats"][0]
    # the line carries 4 significant digits (bench._r)
    assert line["config"]["lane_steps_per_batch"] == pytest.approx(a["step_stats"][0], rel=1e-3)
    assert a["step_stats"][1] == 0 and 0 < a["coverage"].sum() <= a["coverage"].size
    # the sampled rows are the lanes' results: nothing at or past sp / msize / the record length
    idx = a["sample_lanes"].astype(int)
    assert len(set(idx)) == len(idx) == 192
    sp, msize, rl = a["sp"][idx], a["msize"][idx], a["rec_len"][idx]
    assert not (a["stack"] * (np.arange(a["stack"].shape[1])[None, :, None] >= sp[:, None, None])).any()
    assert not (a["memory"] * (np.arange(a["memory"].shape[1])[None, :] >= msize[:, None])).any()
    assert not (a["rec"] * (np.arange(a["rec"].shape[1])[None, :] >= rl[:, None])).any()
    assert a["memory"].any() and a["storage"].any() and a["rec"].any()
    # and they are what the oracle computes for the benchmark's lanes
    from mythril_amd import workloads
    from mythril_amd.lanes import bucket_order, permuted
    from oracle.evm_ref import OracleEVM
    o = OracleEVM()
    ref = workloads.c2_batch(192, code_id=o.load_code(workloads.bytecode("overflow.sol.o")),
                             stack_cap=1024, mem_cap=1024, rec_cap=128)
    ref = permuted(ref, bucket_order(ref))
    o.run(ref)
    for f in ("status", "pc", "sp", "msize", "steps", "gas_min", "gas_max", "storage_count", "rec_len"):
        assert np.array_equal(a[f], getattr(ref, f).astype(np.float64)), f
    for j, i in enumerate(idx):
        assert np.array_equal(a["stack"][j, :int(sp[j])], ref.stack[i, :int(sp[j])])
        assert np.array_equal(a["memory"][j, :int(msize[j])], ref.memory[i, :int(msize[j])])
        assert np.array_equal(a["storage"][j, :int(ref.storage_count[i])], ref.storage[i, :int(ref.storage_count[i])])
        assert np.array_equal(a["rec"][j, :int(rl[j])], ref.rec[i, :int(rl[j])])


def test_bench_prints_one_compact_line_on_the_oracle_device(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    rec = tmp_path / "full.json"
    code = ("import sys; sys.path.insert(0, %r); import bench; "
            "sys.exit(bench.launch_ranks(1, sys.argv[1:], script=%r))" %
            (str(ROOT), str(HERE / "bench_rank_cpu.py")))
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--lanes", "128", "--full", "--no-c4",
            "--cpu-seconds", "0.2", "--rec-cap", "0", "--no-roofline", "--full-record", str(rec)]
    p = subprocess.run([sys.executable, "-c", code] + argv, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096
    out = json.loads(lines[0])
    assert out["cpu_baseline"]["value"] > 0 and out["full_record"] == str(rec)
    assert json.loads(rec.read_text())["value"] == out["value"] or abs(
        json.loads(rec.read_text())["value"] / out["value"] - 1) < 1e-3
