"""GPU (-m gpu): `main.py -m swa` end to end on a reference-style config (tests/configs/av_synthetic_swa.py, three epochs): training writes one checkpoint per epoch,
swa averages them, refreshes the BatchNorm statistics and writes checkpoints_swa-equal-1-3.ckpt, and evaluation loads that file.  Three fresh child processes, one
optimisation step per epoch: sized like tests/test_entry_point.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.gpu
def test_main_training_swa_evaluation(tmp_path):
    env = dict(os.environ, AVEC_TEST_CALLBACKS=str(tmp_path), PYTHONPATH=ROOT)
    cfg = os.path.join("tests", "configs", "av_synthetic_swa.py")
    out = _run(["-c", cfg, "-m", "training", "--steps_per_epoch", "1", "--step_log_period", "1", "--eval_steps", "1"], env)
    assert "Mode: training" in out
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".ckpt")) == ["checkpoints_epoch_%d_step_%d.ckpt" % (e, e) for e in (1, 2, 3)]
    out = _run(["-c", cfg, "-m", "swa", "--swa_epochs", "1", "3", "--steps_per_epoch", "2"], env)
    assert "Mode: swa" in out and "Updating Batch Normalization Statistics" in out
    assert os.path.exists(os.path.join(str(tmp_path), "checkpoints_swa-equal-1-3.ckpt"))
    out = _run(["-c", cfg, "-m", "evaluation", "-i", "checkpoints_swa-equal-1-3.ckpt", "--eval_steps", "1"], env)
    m = re.search(r"Evaluation: \{.*'loss': ([0-9.eE+-]+|nan|inf)", out)
    assert m is not None, out[-2000:]
    loss = float(m.group(1))
    assert loss == loss and 0.0 < loss < float("inf"), out[-2000:]
