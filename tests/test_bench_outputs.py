"""bench.py's plain run: the headline leg alone, one result line whose ms_per_step belongs to the --steps it was given, and
--dump-outputs: the results of the headline job, the same from run to run (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--a5-reads", "4096", "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(built, tmp_path):
    a = _bench(tmp_path / "a", 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["unit"] == "cells/s" and a["higher_is_better"] is True and a["dtype"] == "f64"
    assert a["steps"] == 3 and a["ms_per_step"] > 0 and a["value"] > 0
    assert "cpu_baseline" not in a and "e2e" not in a and "loci_per_s" not in a   # (the other legs: --full)
    names = ("n_candidate_alignments", "max_score", "is_realigned", "realign_pos", "n_indel_scores", "ref_lnp", "indel_lnp")
    got = {k: np.load(tmp_path / "a" / ("a5_%s.npy" % k)) for k in names}
    assert all(v.dtype == np.float64 for v in got.values())
    n_cals = got["n_candidate_alignments"]
    assert len(n_cals) == a["a5"]["reads"] and n_cals.sum() > 0 and np.isfinite(got["max_score"][n_cals > 0]).all()
    assert len(got["ref_lnp"]) == len(got["indel_lnp"]) == got["n_indel_scores"].sum()
    b = _bench(tmp_path / "b", 5)
    assert b["steps"] == 5
    for k in names:
        assert np.array_equal(np.load(tmp_path / "b" / ("a5_%s.npy" % k)).view(np.uint64), got[k].view(np.uint64)), k


def test_full_side_legs_do_not_scale_with_a_large_step_count(monkeypatch):
    """--steps is sized by the ~1 ms headline; the other --full legs (60 .. 400 ms a step) time at most --leg-steps"""
    import bench
    for argv, want in ((["--steps", "8000"], 20), (["--steps", "5"], 5), (["--steps", "8000", "--leg-steps", "40"], 40)):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--full"] + argv)
        args = bench.parse()
        assert bench.side_leg_steps(args) == want and args.steps == int(argv[1])
