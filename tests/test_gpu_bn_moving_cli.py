"""train.py --bn_moving and evaluate.py --bn moving end to end on the GPU
(synthetic TFRecords, 107^2, one epoch of one step: 24 records in a batch of
64): only the flagged run writes <model>.bnstats and the .meta entry;
evaluate.py --bn moving runs on it (x8 in place of x6h, the statistics line
printed), refuses the checkpoint without statistics by name, and takes it
with --bn_calibrate_dir."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu


def _train(tmp_path, data, name, extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "-t", str(data / "train"),
                        "-v", str(data / "val"),
                        "-sm", str(out / "model"), "-ss", str(out / "logs"), "-so", str(out / "op.csv"),
                        "--image_size", "107", "--num_epochs", "1", "--max_steps_per_epoch", "2", "--shuffle_seed", "1"]
                       + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(str(out / "model") + ".meta"), "no checkpoint was written"
    return str(out / "model"), r.stdout


def _evaluate(tmp_path, data, model, extra):
    return subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "-o", "--data_dir", str(data / "val"),
                           "-lm", model, "-b", "8", "-so", str(tmp_path / "test_op.csv")] + extra,
                          cwd=str(tmp_path), capture_output=True, text=True, timeout=600)


def test_bn_moving_flags_end_to_end(tmp_path):
    from jr import checkpoint, synth_records
    from jr.inception import build_inception_v3
    d = tmp_path / "data"
    synth_records.write_split(str(d / "train"), 24, size=107, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 12, size=107, start=100, num_shards=1, name="validation")
    with_stats, log_on = _train(tmp_path, d, "on", ["--bn_moving"])
    plain, log_off = _train(tmp_path, d, "off", [])
    # only the flagged run writes the statistics; the training itself is the same
    assert os.path.exists(with_stats + ".bnstats") and not os.path.exists(plain + ".bnstats")
    meta_on, meta_off = json.load(open(with_stats + ".meta")), json.load(open(plain + ".meta"))
    assert "bn_moving" not in meta_off
    assert meta_on["bn_moving"]["momentum"] == 0.99 and meta_on["bn_moving"]["updates"] == 1
    assert open(with_stats + checkpoint.DATA_SUFFIX, "rb").read() == open(plain + checkpoint.DATA_SUFFIX, "rb").read()
    assert log_on == log_off.replace(str(tmp_path / "off"), str(tmp_path / "on"))
    st = checkpoint.load_bn_moving(with_stats, build_inception_v3(107, 107))
    assert all(np.all(np.isfinite(v)) for v in st.values())
    var = st["batch_normalization_1/moving_variance"]
    assert np.all(var >= 0) and np.all(var < 1.0)           # the update moved it off the initial 1
    assert checkpoint.load_bn_moving(plain, build_inception_v3(107, 107)) is None

    r = _evaluate(tmp_path, d, with_stats, ["--bn", "moving"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("BN statistics: moving (momentum 0.99, 1 updates)") == 1
    assert r.stdout.count("conv_math x8 is used instead of x6h") == 1
    assert "Brier score:" in r.stdout and "AUC:" in r.stdout
    p = _evaluate(tmp_path, d, with_stats, ["--bn", "moving", "--per_member"])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert [ln for ln in p.stdout.splitlines() if ln.startswith(("Brier", "Spec"))] == \
        [ln for ln in r.stdout.splitlines() if ln.startswith(("Brier", "Spec"))]      # grouped = per-member engines

    r = _evaluate(tmp_path, d, plain, ["--bn", "moving"])
    assert r.returncode != 0
    assert plain in r.stderr and "--bn_calibrate_dir" in r.stderr
    r = _evaluate(tmp_path, d, plain, ["--bn", "moving", "--bn_calibrate_dir", str(d / "train"),
                                       "--bn_calibrate_batches", "2"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("BN statistics: moving (calibrated on 2 batches") == 1
    assert "Brier score:" in r.stdout
