"""The recorded bench lines (profiles/r02_bench_*.json, written by bench.py on the GPU box) carry every field the driver's
contract names, and the figures inside them are mutually consistent."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALG = {"c2": (2963001, 2234734), "c5": (17023027, 12838642)}       # pyramid+FAST, blur (bytes per frame)


@pytest.mark.parametrize("cfg", ["c2", "c5", "c3", "c4"])
def test_recorded_bench_line_has_the_contract_fields(cfg):
    d = json.load(open(os.path.join(ROOT, "profiles", "r02_bench_%s.json" % cfg)))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "u8" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    # achieved = algorithmic bytes per launch group / live span of those launches
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["launch_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    if cfg in ALG:                                                   # the blur is scheduled inside the pass
        assert r["algorithmic_bytes_per_frame"] == sum(ALG[cfg]) and "blur" in r["kernel"]
        assert r["traffic"] is not None and 1.0 <= r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.3
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["unit"] == "frames/s" and c["cores"] == (1 if cfg in ("c2", "c5") else 2)
    frames = d["config"]["frames_per_step_per_gpu"] * d["n_gpus"]
    assert abs(d["value"] - frames / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    # value counts the results-to-host copy; the device-resident figure can only be higher, and the host must not be the bound
    assert d["value_device_resident"] >= 0.98 * d["value"] and d["host_copy_matches_device"] is True
    assert d["host_enqueue_ms_per_step"] < 0.5 * d["ms_per_step"]
    assert abs(d["gpu_wall_ms_per_step"] - d["ms_per_step"]) < 0.1 * d["ms_per_step"]        # wall within 10 % of the GPU-side time
    if cfg == "c3":
        assert d["stereo_and_triangulation_match_oracle"] is True


def _run_bench(args, env=None, timeout=300):
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """`--steps` sets the timed steps, the line carries the headline fields, `--dump-outputs` writes float .npy files
    (ORB_BENCH_STUB=1: the workload is a sleep, so this runs without a GPU)."""
    import numpy as np
    env = dict(os.environ, ORB_BENCH_STUB="1", ORB_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    d = _run_bench(["--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", "3", "--dump-outputs", str(tmp_path / "out")], env)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - 3 * 7 / (d["ms_per_step"] * 7e-3)) < 1e-6 * d["value"]
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["counts.npy"]
    a = np.load(tmp_path / "out" / "counts.npy")
    assert a.dtype == np.float64 and a.tolist() == [1000.0] * 3


@pytest.mark.gpu
def test_plain_run_dumps_what_the_oracle_computes(tmp_path, synth, oracle):
    """A plain run is lean (no roofline, no CPU baseline) and its --dump-outputs hold the last timed step's results: counts,
    keypoints and descriptors of the sampled frames bit-exact against the oracle on the same seeded frames."""
    import numpy as np
    B, nd = 8, 4
    d = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--distinct", str(nd),
                    "--dump-outputs", str(tmp_path)], timeout=600)
    assert d["steps"] == 2 and d["config"]["frames_per_step_per_gpu"] == B
    assert "roofline" not in d and "cpu_baseline" not in d and "value_device_resident" not in d
    out = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    base = [synth.gen_image(752, 480, 1 + i, "textured") for i in range(nd)]
    ref = {i: oracle.Extractor(1000, 1.2, 8, 20, 7)(base[i], (0, 1000)) for i in range(nd)}
    assert out["counts"].tolist() == [float(ref[i % nd][0]) for i in range(B)]
    assert out["monos"].tolist() == [float(ref[i % nd][3]) for i in range(B)]
    sel = out["sample"].astype(int)
    assert len(sel) == B and sorted(set(sel.tolist())) == list(range(B))
    kps = np.concatenate([np.stack([ref[i % nd][1][f].astype(np.float64) for f in ref[i % nd][1].dtype.names], axis=-1) for i in sel])
    desc = np.concatenate([ref[i % nd][2] for i in sel]).astype(np.float32)
    assert np.array_equal(out["keypoints"], kps) and np.array_equal(out["descriptors"], desc)
    assert len(out["matches"]) == sum(ref[i % nd][0] for i in sel if i < B - 1) and len(out["matches_per_frame"]) == B - 1
