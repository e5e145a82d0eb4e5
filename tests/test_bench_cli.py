"""bench.py's command line: a plain run times the steps and prints the headline figures only,
--full adds the measurements that take runs of their own, --dump-outputs DIR writes what the last
timed step computed as DIR/<name>.npy (float32 / float64, at most 64 MB, reproducible)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import art
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def _bench(*args):
    p = subprocess.run([sys.executable, "bench.py", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def _load(d):
    arrs = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}
    assert arrs and all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
    return arrs


def test_write_outputs_samples_rows_above_the_cap(tmp_path, monkeypatch):
    """Above the cap every array keeps a fixed, seeded sample of its rows (the same rows in every
    run) and <name>_rows.npy names them; below it the arrays are written whole."""
    sys.path.insert(0, ROOT)
    import bench
    a = np.arange(1000 * 8, dtype=np.float32).reshape(1000, 8)
    b = np.arange(1000, dtype=np.float64)
    bench.write_outputs(str(tmp_path / "whole"), {"a": a, "b": b})
    whole = _load(str(tmp_path / "whole"))
    assert set(whole) == {"a", "b"} and np.array_equal(whole["a"], a) and np.array_equal(whole["b"], b)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4000)
    for d in ("s1", "s2"):
        bench.write_outputs(str(tmp_path / d), {"a": a, "b": b})
    s1, s2 = _load(str(tmp_path / "s1")), _load(str(tmp_path / "s2"))
    assert set(s1) == {"a", "a_rows", "b", "b_rows"}
    assert sum(v.nbytes for v in s1.values()) <= 4000
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    for k, src in (("a", a), ("b", b)):
        rows = s1[k + "_rows"].astype(np.int64)
        assert 0 < rows.size < 1000 and np.all(np.diff(rows) > 0)
        assert np.array_equal(s1[k], src[rows])


def test_cpu_path_plain_full_and_dump(tmp_path):
    """--path cpu (config 1 through the C ABI's CPU backend; needs no GPU): a plain run measures the
    N-thread leg only, --full the one-thread leg too; the dumped arrays equal the oracle's frame."""
    d = str(tmp_path / "out")
    plain = _bench("--path", "cpu", "--cpu-seconds", "0.2", "--dump-outputs", d)
    assert all(k in plain for k in HEADLINE) and plain["full"] is False and plain["threads_1"] is None
    assert plain["ms_per_step"] > 0 and plain["value"] > 0
    full = _bench("--path", "cpu", "--cpu-seconds", "0.2", "--full")
    assert full["full"] is True and full["threads_1"]["threads"] == 1
    assert full["metric"] == plain["metric"] and full["unit"] == plain["unit"]
    got = _load(d)
    cfg = art.CONFIGS[1]
    scene, org, params = art.synth(cfg)
    ref = art.FanOutputs(cfg.S, cfg.R, cfg.H, cfg.T, 1, hits=True)
    oracle.run(scene, params, org, ref, threads=4)
    assert np.array_equal(got["echo"], ref.echo.view(np.float16).astype(np.float32))
    assert np.array_equal(got["muffle"], ref.muffle.astype(np.float32))
    assert np.array_equal(got["perm"], ref.perm)
    assert np.array_equal(got["hit_ids"], ref.hit_ids.astype(np.float64))
    assert np.array_equal(got["settings_reverb_volume"], ref.settings["reverb_volume"])
    assert (got["echo"] != 0).any()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_path(tmp_path):
    """The flagship path, plain: exactly --steps timed steps, the headline fields, none of the
    figures that need runs of their own; the dump of two runs is identical, and its fans equal the
    oracle's frame of the same seeded scene (config 2's fans and rays, 5 % of its colliders)."""
    args = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0", "--collider-scale", "0.05")
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    r = _bench(*args, "--dump-outputs", d1)
    _bench(*args, "--dump-outputs", d2)
    assert all(k in r for k in HEADLINE) and r["steps"] == 3 and r["warmup"] == 1 and r["full"] is False
    assert r["ms_per_step"] > 0 and r["value"] > 0 and r["higher_is_better"] is True and r["dtype"] == "f32"
    for moved in ("roofline", "kernel_ms", "cpu_baseline", "dynamic", "p50_frame_ms", "allgather_ms"):
        assert moved not in r, moved
    a, b = _load(d1), _load(d2)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    cfg = art.CONFIGS[2]
    scene, org, params = art.synth(cfg, C_scale=0.05)
    assert a["echo"].shape == (cfg.S, cfg.R * cfg.H) and a["muffle"].shape == (cfg.S, cfg.T)
    sub = np.arange(0, cfg.S, 16)
    ref = art.FanOutputs(len(sub), cfg.R, cfg.H, cfg.T, 1)
    oracle.run(scene, params, np.ascontiguousarray(org[sub]), ref, threads=16)
    assert np.array_equal(a["echo"][sub], ref.echo.view(np.float16).astype(np.float32), equal_nan=True)
    assert np.array_equal(a["muffle"][sub], ref.muffle.astype(np.float32))
    for f in ref.settings.dtype.names:
        assert np.array_equal(a[f"settings_{f}"][sub], ref.settings[f], equal_nan=True), f
    assert (a["echo"] != 0).any() and (a["muffle"] != 0).any()
