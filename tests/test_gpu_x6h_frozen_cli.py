"""evaluate.py --bn moving --x6h_frozen end to end on the GPU (synthetic
TFRecords, two checkpoints trained two steps with --bn_moving at 107^2): the
run keeps x6h (no fallback line) and writes its CSV; with --attribution
gradient it writes maps and leaves stdout and the CSV byte-equal to the
flagged run without it; and its ensemble predictions stay within 3x the
x8-vs-f32 difference of the x8 predictions the unflagged run computes:
max |p_x6h - p_x8| <= 3 max |p_f32 - p_x8|.

Where that inequality is taken.  On the SAVED statistics of this fixture (one
update at momentum 0.99: mean ~ 0, variance ~ 1) every logit is ~1e-3, all
predictions lie in [0.49977, 0.49988], and float32 resolves them to 3e-8 --
1.2e-7 in the logit, a hundred times the arithmetic differences.  p_f32 and
p_x8 are then equal bit for bit (envelope exactly 0) and p_x6h differs from
them by 0 or by one ulp as rounding falls (measured on an MI355X: 0 on one
box, 2.98e-8 on another, against 3 x 0): that comparison decides nothing, so
its figures are printed and the inequality is asserted on the same records and
members under --bn_calibrate_dir, where the statistics fit the activations,
logits are O(1) and the arithmetics differ by many ulps."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

RES, BATCH = 107, 8
FALLBACK = "conv_math x8 is used instead of x6h"


def _train(tmp_path, data, name, seed):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "-t", str(data / "train"),
                        "-v", str(data / "val"),
                        "-sm", str(out / "model"), "-ss", str(out / "logs"), "-so", str(out / "op.csv"),
                        "--image_size", str(RES), "--num_epochs", "1", "--max_steps_per_epoch", "2",
                        "--shuffle_seed", str(seed), "--bn_moving"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return str(out / "model")


def _evaluate(tmp_path, data, models, csv_name, extra):
    return subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "-o", "--data_dir", str(data / "val"),
                           "-lm", ",".join(models), "-b", str(BATCH), "-so", str(tmp_path / csv_name)] + extra,
                          cwd=str(tmp_path), capture_output=True, text=True, timeout=600)


def _predictions(models, data, conv_math, calibrate=False):
    """The ensemble predictions evaluate.py computes under --bn moving (calibrate: --bn_calibrate_dir train,
    2 batches) with this conv_math, through its own functions."""
    import evaluate
    from jr import checkpoint
    meta = checkpoint.read_meta(models[0])
    engines = evaluate.make_engines(models, meta, BATCH, conv_math=conv_math, grouped=True)
    if calibrate:
        assert evaluate.freeze_engines(engines, None, str(data / "train"), 2, BATCH) == 2
    else:
        stats, _ = evaluate.load_bn_stats(models, engines.g)
        evaluate.freeze_engines(engines, stats)
    preds, labels, _ = evaluate.predict_all(engines, str(data / "val"), BATCH, bn="frozen")
    return np.mean(np.array(preds), axis=0), labels


def test_x6h_frozen_flag_end_to_end(tmp_path):
    from jr import synth_records
    sys.path.insert(0, PKG)
    d = tmp_path / "data"
    synth_records.write_split(str(d / "train"), 24, size=RES, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 12, size=RES, start=100, num_shards=1, name="validation")
    models = [_train(tmp_path, d, "a", 1), _train(tmp_path, d, "b", 2)]

    flagged = _evaluate(tmp_path, d, models, "op.csv", ["--bn", "moving", "--x6h_frozen"])
    assert flagged.returncode == 0, flagged.stdout[-3000:] + flagged.stderr[-3000:]
    assert FALLBACK not in flagged.stdout and "Brier score:" in flagged.stdout
    assert flagged.stdout.count("BN statistics: moving (momentum 0.99, 1 updates)") == 1
    op = open(tmp_path / "op.csv", "rb").read()
    assert len(op.splitlines()) == 201

    maps_dir = tmp_path / "maps"
    attr = _evaluate(tmp_path, d, models, "op.csv", ["--bn", "moving", "--x6h_frozen", "--attribution", "gradient",
                                                     "--attribution_dir", str(maps_dir)])
    assert attr.returncode == 0, attr.stdout[-3000:] + attr.stderr[-3000:]
    assert attr.stdout == flagged.stdout                       # grouped and per-member x6h engines: the same bits
    assert open(tmp_path / "op.csv", "rb").read() == op
    assert sorted(os.listdir(maps_dir)) == ["index.csv", "maps_000000.npy", "maps_000001.npy"]
    for name, n in (("maps_000000.npy", 8), ("maps_000001.npy", 4)):
        m = np.load(maps_dir / name)
        assert m.dtype == np.float32 and m.shape == (n, RES, RES) and np.all(np.isfinite(m)) and np.any(m > 0)

    def compare(index, calibrate):
        """(max |p_x6h - p_x8|, max |p_f32 - p_x8|): p_x6h from the flagged run's index.csv (9 digits: exact
        float32), p_x8 what the run without the flag computes, p_f32 what --conv_math f32 computes."""
        rows = list(csv.reader(open(index)))
        assert rows[0] == ["batch", "row", "label", "prediction"] and len(rows) == 13
        p_x6h = np.array([np.float32(r[3]) for r in rows[1:]], np.float32).reshape(-1, 1)
        p_x8, labels = _predictions(models, d, "x8", calibrate)
        p_f32, _ = _predictions(models, d, "f32", calibrate)
        assert [int(r[2]) for r in rows[1:]] == [int(v) for v in labels[:, 0]]
        moved = float(np.max(np.abs(p_x6h.astype(np.float64) - p_x8)))
        envelope = float(np.max(np.abs(p_f32.astype(np.float64) - p_x8)))
        print(f"\n--x6h_frozen ({'calibrated' if calibrate else 'saved'} statistics): max |p_x6h - p_x8| {moved:.3g}; "
              f"max |p_f32 - p_x8| {envelope:.3g}; p_x8 in [{float(p_x8.min()):.9g}, {float(p_x8.max()):.9g}]")
        return moved, envelope

    compare(maps_dir / "index.csv", False)      # below float32's resolution of p here (module docstring): printed
    cal_dir = tmp_path / "maps_cal"
    cal = _evaluate(tmp_path, d, models, "op_cal.csv",
                    ["--bn", "moving", "--x6h_frozen", "--bn_calibrate_dir", str(d / "train"),
                     "--bn_calibrate_batches", "2", "--attribution", "gradient", "--attribution_dir", str(cal_dir)])
    assert cal.returncode == 0, cal.stdout[-3000:] + cal.stderr[-3000:]
    assert FALLBACK not in cal.stdout and cal.stdout.count("BN statistics: moving (calibrated on 2 batches") == 1
    moved, envelope = compare(cal_dir / "index.csv", True)
    assert envelope > 1e-7, envelope            # (many ulps of p: a degenerate envelope cannot hide a failure)
    assert moved <= 3 * envelope, (moved, envelope)
