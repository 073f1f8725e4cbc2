"""bench.py's plain run (the headline only, exactly --steps timed steps) and --dump-outputs (what the last timed step returned,
seeded inputs: two runs with the same arguments write the same arrays)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_dump_outputs_types_and_seeded_sample(tmp_path, monkeypatch):
    """float32 maps, int64 indices as exact float64; over the size limit a fixed sample of images, the same in every array."""
    import torch
    B, K = 10, 7
    rng = np.random.default_rng(5)
    out = {"dets": torch.from_numpy(rng.random((B, K, 6), dtype=np.float32)), "lms": torch.from_numpy(rng.random((B, K, 10), dtype=np.float32)),
           "inds": torch.from_numpy(rng.integers(0, 1 << 40, (B, K))), "all": torch.from_numpy(rng.random((B, K, 16), dtype=np.float32))}
    bench.dump_outputs(str(tmp_path / "a"), out, "none")
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("dets", "lms", "inds")}
    assert sorted(os.listdir(tmp_path / "a")) == ["dets.npy", "inds.npy", "lms.npy"]
    assert got["dets"].dtype == np.float32 and np.array_equal(got["dets"], out["dets"].numpy())
    assert got["inds"].dtype == np.float64 and np.array_equal(got["inds"].astype(np.int64), out["inds"].numpy())
    bench.dump_outputs(str(tmp_path / "r"), out, "cf")
    assert os.listdir(tmp_path / "r") == ["records.npy"] and np.array_equal(np.load(tmp_path / "r" / "records.npy"), out["all"].numpy())
    full = sum(a.nbytes for a in got.values())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", full // 2)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), out, "none")
    s1 = {n: np.load(tmp_path / "s1" / (n + ".npy")) for n in got}
    s2 = {n: np.load(tmp_path / "s2" / (n + ".npy")) for n in got}
    assert sum(a.nbytes for a in s1.values()) <= full // 2 and len(s1["dets"]) == B // 2
    rows = [int(np.flatnonzero((got["dets"] == r).all(axis=(1, 2)))[0]) for r in s1["dets"]]
    for n in got:
        assert np.array_equal(s1[n], s2[n]) and np.array_equal(s1[n], got[n][rows])


def _plain(tmp_path, tag):
    d = tmp_path / tag
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--batch", "4", "--size", "160", "--topk", "20", "--dump-outputs", str(d)],
                         capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(d / (n + ".npy")) for n in ("dets", "lms", "inds")}


@pytest.mark.gpu
def test_plain_run_times_exactly_steps_and_dumps_reproducible_outputs(tmp_path):
    """A plain run: one window of exactly --steps steps, the headline fields and none of the --full blocks; the dumped outputs are the
    top-K decode of the last step's batch and are identical in a second run with the same arguments."""
    d, a = _plain(tmp_path, "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "windows"):
        assert k in d, k
    for k in ("roofline", "cpu_baseline", "parity", "tolerance_mode", "exact_fp32_mode", "value_with_h2d", "other_configs"):
        assert k not in d, k
    assert d["steps"] == 5 and d["warmup"] == 2 and d["windows"]["n"] == 1 and d["windows"]["steps_each"] == 5
    assert abs(d["ms_per_step"] - d["windows"]["median_ms"] / 5) < 1e-3
    assert abs(d["value"] - 4 * 5 / (d["windows"]["median_ms"] * 1e-3)) / d["value"] < 1e-3
    assert a["dets"].shape == (4, 20, 6) and a["lms"].shape == (4, 20, 10) and a["inds"].shape == (4, 20)
    assert a["dets"].dtype == np.float32 and a["inds"].dtype == np.float64
    assert np.all(np.diff(a["dets"][..., 4], axis=1) <= 0) and np.all((a["inds"] >= 0) & (a["inds"] < 40 * 40))
    _, b = _plain(tmp_path, "b")
    for n in a:
        assert np.array_equal(a[n], b[n]), n
