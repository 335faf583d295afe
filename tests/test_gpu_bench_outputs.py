"""bench.py as every change is measured: a plain run prints the headline line and does nothing it does not time, and
--dump-outputs writes what the last timed step computed — the same bits from one run to the next."""
import json
import subprocess
import sys

import numpy as np
import pytest

from __graft_entry__ import ROOT

pytestmark = pytest.mark.gpu


def _bench(*flags):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _same_files(a, b):
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    total = 0
    for nm in names:
        x, y = np.load(a / nm), np.load(b / nm)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, nm
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), nm
        total += x.nbytes
    assert total <= 64 << 20
    return set(names)


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    flags = ("--steps", "4", "--warmup", "2", "--preroll", "10", "--particles", "8192")
    outs = [_bench(*flags, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for out in outs:
        assert out["steps"] == 4 and out["unit"] == "particle-updates/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert out["value"] == pytest.approx(8192 / (out["ms_per_step"] * 1e-3), rel=1e-9)
        assert out["cpu_baseline"] is None
        assert not {"stage_avg_ms", "north_star", "end_to_end_obs32", "north_star_strong"} & set(out)
    names = _same_files(tmp_path / "a", tmp_path / "b")
    assert {"poses.npy", "best_pose.npy", "best_logw_index.npy", "mean_pose.npy", "map_rows.npy", "map_rows_index.npy"} <= names
    poses, rows = np.load(tmp_path / "a" / "poses.npy"), np.load(tmp_path / "a" / "map_rows.npy")
    assert poses.shape == (3, 8192) and np.isfinite(poses).all()
    assert rows.shape == (256, 5, 500) and np.isfinite(rows).all()


def test_score_mode_dumps_scores_and_counts(tmp_path):
    flags = ("--mode", "score", "--steps", "3", "--warmup", "1", "--particles", "4096")
    for d in ("a", "b"):
        _bench(*flags, "--dump-outputs", str(tmp_path / d))
    assert _same_files(tmp_path / "a", tmp_path / "b") == {"score.npy", "count.npy"}
    count = np.load(tmp_path / "a" / "count.npy")
    assert count.shape == (4096,) and count.max() > 0
