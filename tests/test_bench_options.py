"""bench.py's own options: --steps is validated, --dump-outputs writes the last timed step's outputs (dtypes, the 64 MB cap with a
seeded row sample, the same outputs run to run), and a plain run leaves the --full measurements out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


def test_steps_must_be_at_least_one():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    a = bench.parse(["--steps", "3", "--warmup", "0"])
    assert a.steps == 3 and a.warmup == 0 and not a.full and a.dump_outputs is None


def test_write_outputs_samples_what_does_not_fit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 10_000)
    small = np.arange(12, dtype=np.float64)
    big = np.arange(4000, dtype=np.float32).reshape(1000, 4)          # 16 000 bytes: more than is left
    bench.write_outputs(str(tmp_path / "a"), [("small", small), ("big", big)])
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    got, idx = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big_sample_rows.npy")
    assert got.dtype == np.float32 and idx.dtype == np.float64 and (np.diff(idx) > 0).all()
    assert np.array_equal(got, big[idx.astype(np.int64)])
    assert small.nbytes + idx.nbytes + got.nbytes <= 10_000 and len(idx) > 0
    bench.write_outputs(str(tmp_path / "b"), [("small", small), ("big", big)])      # a fixed seed: the same sample every time
    assert np.array_equal(np.load(tmp_path / "b" / "big_sample_rows.npy"), idx)
    assert not os.path.exists(tmp_path / "a" / "small_sample_rows.npy")


def _plain_run(out_dir, steps=2, warmup=1):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--ring", "32",
           "--batch", "8", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(gpu, tmp_path):
    out = _plain_run(tmp_path / "a")
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 64 / (out["ms_per_step"] / 1e3)) / out["value"] < 1e-3
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["config"]["plugin_loop"] is None     # --full only
    names = ("track_counts", "detection_counts", "track_rows", "reid_crops_per_frame_last_group", "reid_embeddings_last_group")
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    nt, rows = a["track_counts"], a["track_rows"]
    assert nt.shape == (64,) and a["detection_counts"].shape == (64,) and rows.shape == (64, 32, 6)
    assert round(float(nt.mean()), 2) == out["config"]["confirmed_tracks_per_frame"] == 30.0
    live = np.arange(32)[None, :] < nt[:, None]
    assert (rows[live][:, 4] > 0).all() and (rows[~live] == 0).all()         # live rows carry a track id, the rest are zeroed
    emb = a["reid_embeddings_last_group"]
    assert emb.shape == (int(a["reid_crops_per_frame_last_group"].sum()), 512) and len(emb) > 0 and np.isfinite(emb).all()
    _plain_run(tmp_path / "b")                                               # the same arguments: the same inputs, the same outputs
    for d in ("b",):
        for n in names:
            assert np.array_equal(np.load(tmp_path / d / (n + ".npy")), a[n]), (d, n)
