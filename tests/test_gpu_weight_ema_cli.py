"""train.py --optimizer rmsprop --weight_ema and evaluate.py --weights averaged
end to end on the GPU (synthetic TFRecords, 107^2, one epoch of two steps):
the checkpoint carries the trained weights and <model>.ema with its .meta
entries; evaluate.py runs on either and the averaged predictions are those of
the .ema file; two ranks on one device finish with identical digests of the
weights and of their average."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

RES = 107
FLAGS = ["--optimizer", "rmsprop", "--weight_ema", "0.5", "--weight_decay", "4e-5", "--clip_norm", "2"]


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    from jr import synth_records
    d = tmp_path_factory.mktemp("ema_records")
    synth_records.write_split(str(d / "train"), 128, size=RES, num_shards=2, name="train")
    # (48 validation images: enough of both classes that the first epoch's AUC clears the 0.01 a checkpoint needs)
    synth_records.write_split(str(d / "val"), 48, size=RES, start=100, num_shards=1, name="validation")
    return d


def _train_args(d, out):
    return [os.path.join(PKG, "train.py"), "-t", str(d / "train"), "-v", str(d / "val"), "-sm", str(out / "model"),
            "-ss", str(out / "logs"), "-so", str(out / "op.csv"), "--image_size", str(RES), "--num_epochs", "1",
            "--max_steps_per_epoch", "2", "--shuffle_seed", "1"] + FLAGS


def _evaluate(tmp_path, d, model, extra):
    return subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "-o", "--data_dir", str(d / "val"),
                           "-lm", model, "-b", "8", "-so", str(tmp_path / "test_op.csv")] + extra,
                          cwd=str(tmp_path), capture_output=True, text=True, timeout=600)


def _brier_line(labels, pred):
    import lib.metrics
    value, update, reset = lib.metrics.create_reset_metric(lib.metrics.mean_squared_error, scope="brier")
    reset()
    update(labels, pred)
    return f"Brier score: {value():6.4}"


def test_train_writes_the_average_and_evaluate_reads_it(records, tmp_path):
    import evaluate
    from jr import checkpoint
    from jr.inception import build_inception_v3
    d, out = records, tmp_path / "run"
    r = subprocess.run([sys.executable] + _train_args(d, out), cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    model = str(out / "model")
    assert os.path.exists(model + ".meta"), "no checkpoint was written:\n" + r.stdout[-3000:]
    assert "Learning rate:" in r.stdout and "Brier score:" in r.stdout          # the printed lines keep their format
    meta = json.load(open(model + ".meta"))
    assert meta["optimizer"] == {"learning_rate": 3e-3, "lr_decay": None, "lr_warmup": 0, "weight_decay": 4e-5,
                                 "clip_norm": 2.0, "name": "rmsprop",
                                 "rmsprop": {"rho": 0.9, "momentum": 0.9, "epsilon": 1.0},
                                 "weight_ema": {"decay": 0.5, "warm": True}}
    assert meta["weight_ema"]["decay"] == 0.5 and meta["weight_ema"]["warm"] is True
    assert meta["weight_ema"]["updates"] == 2
    g = build_inception_v3(RES, RES)
    trained = checkpoint.load(model, g)[0]
    ema, info = checkpoint.load_ema(model, g)
    assert os.path.getsize(model + ".ema") == os.path.getsize(model + checkpoint.DATA_SUFFIX)
    assert np.all(np.isfinite(ema)) and np.all(np.isfinite(trained)) and not np.array_equal(ema, trained)

    # evaluate.py on either set of weights; the averaged run says so
    rt = _evaluate(tmp_path, d, model, [])
    ra = _evaluate(tmp_path, d, model, ["--weights", "averaged"])
    for run in (rt, ra):
        assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert ra.stdout.count("Weights: averaged") == 1 and "Weights:" not in rt.stdout
    # the same engines in this process: averaged predictions differ from the trained ones, are those of an
    # engine loaded with the .ema file, and give the Brier score the command printed
    kw = dict(device=0, conv_math="x6h", dtype="f32", grouped=True)
    val = str(d / "val")
    e = evaluate.make_engines([model], meta, 8, flats=evaluate.load_averaged([model], g), **kw)
    p_avg, labels, _ = evaluate.predict_all(e, val, 8)
    e = evaluate.make_engines([model], meta, 8, **kw)
    p_trained, _, _ = evaluate.predict_all(e, val, 8)
    raw = np.fromfile(model + ".ema", dtype="<f4")
    e = evaluate.make_engines([model], meta, 8, flats=[raw], **kw)
    p_raw, _, _ = evaluate.predict_all(e, val, 8)
    assert p_avg[0].shape == (48, 1) and np.array_equal(p_avg[0], p_raw[0])
    assert not np.array_equal(p_avg[0], p_trained[0])
    assert _brier_line(labels, p_avg[0]) in ra.stdout and _brier_line(labels, p_trained[0]) in rt.stdout


def test_two_ranks_agree_on_weights_and_average(records, tmp_path):
    d, out, logs = records, tmp_path / "out", tmp_path / "torchrun_logs"
    port = 29600 + (os.getpid() + 13) % 1000
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]), JR_DIST_BACKEND="gloo", JR_ONE_DEVICE="1")
    args = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", str(port), "--log-dir", str(logs), "--redirects", "3"]
    r = subprocess.run(args + _train_args(d, out), capture_output=True, text=True, env=env, cwd=str(tmp_path),
                       timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])      # check_replicas raises when digests differ
    f = list(logs.glob("*/attempt_*/0/stdout.log"))
    assert len(f) == 1 and "End of epoch 0!" in f[0].read_text()
    meta = json.load(open(str(out / "model") + ".meta"))
    assert meta["weight_ema"]["updates"] == 1 and os.path.exists(str(out / "model") + ".ema")
