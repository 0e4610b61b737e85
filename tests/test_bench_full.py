"""bench.py: a plain run does only what its headline needs; everything measured beside the headline runs with --full.

The CPU test pins the defaults the option decides; the GPU test runs a small workload both ways and checks that the extras
appear only with --full, and that --full changes nothing of what the timed steps computed (--dump-outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("long_run", "opening_phase", "roofline", "roofline_step", "roofline_select_wide_synthetic", "cpu_baseline")


def _parse(monkeypatch, *argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_leaves_the_extra_legs_to_full(monkeypatch):
    plain = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "3")
    assert not plain.full and plain.long_run_steps == 0 and plain.opening_steps == 0
    full = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "3", "--full")
    assert full.full and full.long_run_steps == 2000 and full.opening_steps == 20
    # the timed workload itself does not depend on the option
    keep = ("games", "sims", "net", "net_dtype", "preroll", "cohorts", "steps", "warmup", "max_game_moves", "batch")
    assert {k: getattr(plain, k) for k in keep} == {k: getattr(full, k) for k in keep}
    # legs asked for by name run without --full; the defaults stay off where they were off before
    named = _parse(monkeypatch, "--long-run-steps", "50", "--opening-steps", "5")
    assert named.long_run_steps == 50 and named.opening_steps == 5
    assert _parse(monkeypatch, "--full", "--games", "128").long_run_steps == 0
    assert _parse(monkeypatch, "--full", "--no-roofline").long_run_steps == 0
    assert _parse(monkeypatch, "--full", "--fast").opening_steps == 0
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--fast", "--select-sweep")


def _bench(out_dir, extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--games", "64", "--sims", "64",
           "--preroll", "24", "--max-game-moves", "16", "--dump-outputs", str(out_dir)] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_full_adds_the_extra_legs_and_changes_nothing_the_steps_compute(tmp_path):
    plain = _bench(tmp_path / "plain", [])
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0
    assert not [k for k in EXTRAS if k in plain]
    full = _bench(tmp_path / "full", ["--full", "--long-run-steps", "4", "--wide-trees", "1024", "--cpu-seconds", "1", "--cpu-cores", "2"])
    assert all(k in full for k in HEADLINE) and full["value"] > 0
    assert full["long_run"]["steps"] == 4 and full["opening_phase"]["steps"] == 20
    assert full["roofline"]["kernel"].startswith("bo_k_tower_s") and full["roofline"]["launches_timed"] > 0
    assert full["roofline_select_wide_synthetic"]["levels_per_launch"] > 0 and full["roofline_step"]["levels"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["cores"] == 2
    for name in ("game_id", "ply", "pi"):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.shape == b.shape and np.array_equal(a, b), name
