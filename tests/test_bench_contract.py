"""bench.py's output contract (the driver parses its one JSON line) and the PMC traffic summary
that feeds `roofline.traffic`."""
import csv
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_counters(path, counter, rows):
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["Kernel_Name", "Counter_Name", "Counter_Value"])
        w.writeheader()
        for name, value in rows:
            w.writerow({"Kernel_Name": name, "Counter_Name": counter, "Counter_Value": value})


def test_pmc_summary_tags_workload_and_doubles_fetch(tmp_path):
    """FETCH_SIZE is doubled (gfx950 correction), WRITE_SIZE taken as is, both KB -> bytes per
    launch averaged over dispatches, and the output names the workload it was measured on."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import pmc_summary

    k = "void vx::(anonymous namespace)::k_landmark_solve(vx::BAArgs, int)"
    _write_counters(tmp_path / "f.csv", "FETCH_SIZE", [(k, 100.0), (k, 300.0)])
    _write_counters(tmp_path / "w.csv", "WRITE_SIZE", [(k, 10.0), (k, 30.0)])
    out = tmp_path / "t.json"
    pmc_summary.main(str(tmp_path / "f.csv"), str(tmp_path / "w.csv"), str(out), "C4", "2")
    d = json.load(open(out))
    assert d["config"] == "C4" and d["n_gpus"] == 2
    assert d["bytes_per_launch"]["ba_landmark"] == int(2 * 200.0 * 1024 + 20.0 * 1024)


def test_committed_traffic_is_tagged():
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    # (the dominant kernel of the default bench: the fused LocalBA iteration, bench.py's "ba_iter")
    assert d["config"] == "C3" and d["n_gpus"] == 1 and d["bytes_per_launch"]["ba_iter"] > 0


def test_bench_help_runs_without_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--steps" in r.stdout and "--grid-share" in r.stdout


@pytest.mark.gpu
def test_bench_json_line():
    """A short bench run prints exactly one JSON line with the fields the driver reads (--full: the
    roofline comes from the profiling passes)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2",
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["higher_is_better"] is False
    assert d["value"] > 0 and d["unit"] == "ms/frame" and d["config"]["workload"].startswith("C3")
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4
    # frac follows from the bytes and the profiling pass's per-dispatch average (stages_us)
    assert abs(rf["avg_launch_us"] - d["stages_us"][rf["kernel"]]) <= 0.01
    assert abs(rf["frac"] - rf["bytes_per_launch"] / (rf["avg_launch_us"] * 1e-6) / 8e12) <= 2e-4


def test_committed_bench_roofline_matches_committed_profile():
    """The committed C3 bench line of this round (the default command, unprofiled) and the rocprofv3
    --kernel-trace --stats summary of the same command in the same session (profiles/r06): the
    line's roofline fraction is within 5 % of the algorithmic bytes / rocprof's average duration of
    that kernel / 8 TB/s (session r06s2, the final tree).  (The line the profiled process prints itself,
    bench_c3_under_rocprof_r06s2.json,
    is not compared: under the tracer the bench's own event-timed pass runs ~25 % longer.)"""
    d = json.loads(open(os.path.join(ROOT, "profiles", "r06", "bench_c3_r06s2.json")).read().strip().splitlines()[-1])
    rf = d["roofline"]
    assert rf["hip_kernel"] in ("k_ba_iter", "k_ba_win")
    # k_ba_iter: the iteration launches (k_ba_iter<false, ...>; the prologue k_ba_iter<true, ...> is its
    # own stage); k_ba_win: the whole window
    key = "k_ba_iter<false" if rf["hip_kernel"] == "k_ba_iter" else "k_ba_win<"
    with open(os.path.join(ROOT, "profiles", "r06", "kernel_stats_bench_c3_r06s2.csv")) as f:
        rows = [r for r in csv.DictReader(f) if key in r["Name"]]
    assert len(rows) == 1
    avg_us = float(rows[0]["AverageNs"]) / 1e3
    frac_prof = rf["bytes_per_launch"] / (avg_us * 1e-6) / 8e12
    assert abs(rf["frac"] - frac_prof) <= 0.05 * frac_prof, (rf["frac"], frac_prof, avg_us, rf["avg_launch_us"])


def test_cpu_baseline_mt_small():
    """The multi-threaded CPU leg (SURVEY.md §8(d) best-effort CPU) on a tiny workload."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "visionx-slam_amd", "python"))
    import bench
    from vxslam import synth

    h, w, nf, nk, nl = 120, 160, 200, 5, 300
    frames = synth.make_frames(7, 2, h, w)
    m = synth.make_ba_map(7, nk, nl)
    d = bench.cpu_baseline_mt((h, w, nf, nk, nl), frames, m, 2)
    assert d["value"] > 0 and d["cores"] >= 1 and d["unit"] == "ms/frame" and d["kind"] == "port"


def test_ba_flags_reference_names(tmp_path):
    """bench.py takes the reference runner's LocalBA flags (apps/main.cpp:42-47) on the command line
    and from a key=value --config file (the reference's LoadConfig format, default.cfg's keys);
    command-line flags win over the file, the file over the workload's defaults."""
    sys.path.insert(0, ROOT)
    import argparse

    import bench

    cfg = tmp_path / "run.cfg"
    cfg.write_text("# Local BA\nenable_local_ba=false\nba_window_size=7\n ba_iterations = 3 \n"
                   "ba_huber_delta=2.5\nsequence=rgbd_dataset_freiburg1_desk\n")
    ns = argparse.Namespace(config_file=str(cfg), **{k: None for k in bench.BA_FLAGS})
    ns.ba_iterations = 4
    v = bench.resolve_ba_flags(ns, 50)
    assert v == {"ba_window_size": 7, "ba_iterations": 4, "ba_min_pose_observations": 20,
                 "ba_min_point_observations": 2, "ba_huber_delta": 2.5, "ba_max_reproj_error": 5.0}
    ns = argparse.Namespace(config_file=None, **{k: None for k in bench.BA_FLAGS})
    assert bench.resolve_ba_flags(ns, 50)["ba_window_size"] == 50
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    for k in bench.BA_FLAGS:
        assert f"--{k}" in r.stdout


def _json_line(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_c4_strong_scaling_line():
    """--config C4 --scaling strong: BASELINE configs[3]'s fixed 100 KF / 50k window (at N = 1 the
    same work as the default C4 line), the mode echoed in the line."""
    d = _json_line(["--config", "C4", "--scaling", "strong", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"])
    assert d["scaling"] == "strong" and d["config"]["scaling"] == "strong"
    assert d["config"]["ba_window_kf"] == 100 and d["config"]["ba_landmarks"] == 50000
    assert d["config"]["workload"].startswith("C4") and d["value"] > 0


@pytest.mark.gpu
def test_bench_c5_line():
    """--config C5: 8 cameras + the Schur BA of the 200 KF / 100k window; the MFMA roofline of the dense
    pose solve (FP64 flops of the symbolic tile factorisation) when it dominates."""
    d = _json_line(["--config", "C5", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert d["config"]["workload"].startswith("C5") and d["config"]["frames_per_step"] == 8
    assert d["config"]["ba_window_kf"] == 200 and d["config"]["ba_landmarks"] == 100000
    assert d["unit"] == "ms/frame" and d["value"] > 0 and d["work_per_step"]["sba_iterations"] >= 2
    rf = d["roofline"]
    assert rf is not None
    if rf["bound"] == "mfma":
        assert rf["unit"] == "TFLOP/s" and 0 < rf["frac"] < 1 and rf["flops_per_factorisation"] > 0


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) times the steps only: the line keeps its headline fields, the other
    passes' fields are null; --dump-outputs writes the last step's arrays as float .npy files."""
    import numpy as np

    d = _json_line(["--config", "C2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")])
    assert d["full"] is False and d["steps"] == 3 and d["value"] > 0 and d["unit"] == "ms/frame"
    F = d["config"]["frames_per_step"]
    # one step is F frames; both figures are rounded to 4 decimals
    assert abs(d["ms_per_step"] - d["value"] * F) <= (F + 1) * 5e-5 + 1e-9
    for key in ("roofline", "cpu_baseline", "per_keyframe_ms", "latency_ms_per_frame", "ba_plan_build_ms"):
        assert d[key] is None, key
    assert d["stages_us"] == {}
    files = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 10 ** 6
    kp, desc, ma = (files[f"frame{F - 1:02d}_{x}.npy"] for x in ("keypoints", "descriptors", "matches"))
    assert kp.shape == (d["work_per_step"]["keypoints"], 5) and desc.shape == (len(kp), 32)
    assert ma.shape == (d["work_per_step"]["matches"], 3)
    from vxslam import synth

    m = synth.make_ba_map(0x5EED0003, 10, 2000, n_streams=1, n_old_kf=2)  # C2's window before LocalBA ran
    for key in ("kf_pose", "lm_pos"):
        after = files[f"ba_{key}.npy"]
        assert after.shape == m[key].shape and np.isfinite(after).all() and not np.array_equal(after, m[key])


def test_dump_outputs_floats_and_cap(tmp_path, monkeypatch):
    """bench.dump_outputs: record arrays become float64 columns, bytes float32; over the cap every
    array keeps the same seeded rows from run to run."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    rec = np.zeros(4, [("a", "<i4"), ("b", "<f4")])
    rec["a"], rec["b"] = [3, 1, 2, 7], [0.5, 1.5, 2.5, 3.5]
    arrays = {"rec": rec, "u8": np.arange(64, dtype=np.uint8).reshape(2, 32), "f64": np.arange(3000.0).reshape(-1, 3)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    assert got["rec"].dtype == np.float64 and got["rec"].tolist() == [[3, 0.5], [1, 1.5], [2, 2.5], [7, 3.5]]
    assert got["u8"].dtype == np.float32 and np.array_equal(got["u8"], arrays["u8"])
    assert got["f64"].dtype == np.float64 and np.array_equal(got["f64"], arrays["f64"])
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 6000)
    arrays = {"u8": np.zeros((40, 32), np.uint8), "f64": arrays["f64"]}
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    b, c = (np.load(tmp_path / d / "f64.npy") for d in ("b", "c"))
    total = sum(np.load(p).nbytes for p in (tmp_path / "b").iterdir())
    assert total <= 6000 and 0 < len(b) < 1000 and np.array_equal(b, c)
    assert np.all(np.diff(b[:, 0]) > 0) and np.all(b[:, 1] == b[:, 0] + 1)  # whole rows, in order


def test_sba_parity_field_logic():
    """bench.py's C5 N > 1 gate on made-up shard results: a correct split passes; a shard off by
    1e-3, a missing landmark, ranks disagreeing bitwise or a different LM decision fail."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    rng = np.random.default_rng(3)
    pose = rng.normal(size=(6, 7))
    pos = rng.normal(size=(10, 3)) + 5
    ref = {"pose": pose, "lm_idx": np.arange(10), "lm_pos": pos, "iterations": 4, "accepted": 3,
           "steps": [2, 1, 1, 0], "cost": [10.0, 8.0, 7.0, 7.5]}
    own = [np.array([0, 2, 4, 6, 8]), np.array([1, 3, 5, 7, 9])]
    shards = [dict(ref, lm_idx=o, lm_pos=pos[o]) for o in own]
    assert bench.sba_parity_vs_unsharded(shards, ref)["ok"]
    bad = [dict(s) for s in shards]
    bad[1]["lm_pos"] = bad[1]["lm_pos"] * (1 + 1e-3)
    assert not bench.sba_parity_vs_unsharded(bad, ref)["ok"]
    bad = [dict(s) for s in shards]
    bad[0]["lm_idx"], bad[0]["lm_pos"] = bad[0]["lm_idx"][1:], bad[0]["lm_pos"][1:]
    assert not bench.sba_parity_vs_unsharded(bad, ref)["shards_partition"]
    bad = [dict(s) for s in shards]
    bad[1]["pose"] = pose.copy()
    bad[1]["pose"][0, 4] += 1e-12
    assert not bench.sba_parity_vs_unsharded(bad, ref)["ranks_agree"]
    bad = [dict(s) for s in shards]
    bad[0]["steps"] = [2, 1, 0, 0]
    assert not bench.sba_parity_vs_unsharded(bad, ref)["same_lm_decisions"]
