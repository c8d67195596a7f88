"""train.py --accum_steps end to end on the GPU (synthetic TFRecords, 107^2, one
epoch of seven batches, K = 3 with the device recipe flags): the start-up line,
three updates (3, 3 and the flushed 1), the .meta entry, and a checkpoint that
is byte for byte the one the same batches give when driven through Session /
Engine by hand -- and again on a second run."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

RES, K, BATCHES = 107, 3, 7
FLAGS = ["--optimizer", "rmsprop", "--weight_decay", "4e-5", "--clip_norm", "2", "--lr_decay", "0.94,1",
         "--lr_warmup", "2", "--weight_ema", "0.5"]


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    from jr import synth_records
    d = tmp_path_factory.mktemp("accum_records")
    # seven batches of train.py's 64: six full ones and one of 8
    synth_records.write_split(str(d / "train"), 6 * 64 + 8, size=RES, num_shards=2, name="train")
    # (48 validation images: enough of both classes that the first epoch's AUC clears the 0.01 a checkpoint needs)
    synth_records.write_split(str(d / "val"), 48, size=RES, start=1000, num_shards=1, name="validation")
    return d


def _argv(d, out):
    return ["-t", str(d / "train"), "-v", str(d / "val"), "-sm", str(out / "model"), "-ss", str(out / "logs"),
            "-so", str(out / "op.csv"), "--image_size", str(RES), "--num_epochs", "1", "--shuffle_seed", "1",
            "--replica_dump_dir", str(out / "dump"), "--accum_steps", str(K), "--max_steps_per_epoch", str(BATCHES)
            ] + FLAGS


def _run(d, out, cwd):
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py")] + _argv(d, out), cwd=str(cwd),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(str(out / "model") + ".meta"), "no checkpoint was written:\n" + r.stdout[-3000:]
    return r.stdout


def _by_hand(d):
    """The same seven batches through Session / Engine: what train.py's loop does, spelled out."""
    import lib.dataset
    import train
    from jr.engine import Engine
    from jr.schedule import accum_groups, learning_rate
    from jr.session import Session
    args = train.build_parser().parse_args(_argv(d, d / "unused"))
    ds = lib.dataset.initialize_dataset(
        args.train_dir, train.TRAIN_BATCH_SIZE, num_workers=train.NUM_WORKERS,
        prefetch_buffer_size=2 * train.TRAIN_BATCH_SIZE, shuffle_buffer_size=train.SHUFFLE_BUFFER_SIZE,
        image_data_format="channels_last", num_channels=train.NUM_CHANNELS, image_dim=[RES, RES],
        seed=args.shuffle_seed, decode_dtype="uint8", shard=None)
    eng = Engine(train.TRAIN_BATCH_SIZE, RES, RES, device=0, optimizer="rmsprop", lr=train.LEARNING_RATE,
                 momentum=train.MOMENTUM, seed=0, dtype="f32", conv_math="x6h", tiles="pinned",
                 weight_decay=4e-5, clip_norm=2.0, device_lr=True, weight_ema=0.5, weight_ema_warm=True,
                 accum_steps=K)
    sess = Session(eng, [0.5])
    sizes, per_epoch = accum_groups(BATCHES, K)
    assert (sizes, per_epoch) == ([3, 3, 1], 3)
    steps, it = [], iter(ds)
    try:
        for b, (images, labels) in enumerate(it):
            if b >= BATCHES:
                break
            eng.set_lr(float(learning_rate(sess.global_step, train.LEARNING_RATE, (0.94, 1 * per_epoch), 2)))
            steps.append(sess.train_batch(images, labels)[0])
    finally:
        lib.dataset.close_iterator(it)
    assert eng.accum_pending() == 1 and sess.accum_flush() is True
    assert sess.global_step == 3 and eng.ema_updates() == 3 and eng.opt_step()[2:] == (0, 0)
    flat = eng.params_numpy()
    eng.close()
    return steps, flat


def test_accum_steps_trains_and_reproduces_the_hand_driven_run(records, tmp_path):
    from jr import checkpoint
    d = records
    out = [tmp_path / "run1", tmp_path / "run2"]
    stdout = _run(d, out[0], tmp_path)
    model = str(out[0] / "model")
    # the start-up line: K, the batch per update (64 * K * world) and the updates per epoch
    assert stdout.count("Gradient accumulation: 3 batches of 64 per update, 192 images per update, "
                        "3 updates per epoch\n") == 1, stdout[-3000:]
    # one status line per batch; Step: counts updates -- groups of 3, 3 and 1
    status = [(int(b), int(s)) for b, s in re.findall(r"Batch:\s+(\d+), Xent:[^,]*, Step:\s+(\d+)", stdout)]
    assert status == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 1), (6, 2)], status
    m = re.search(r"^Learning rate: (\S+), median gradient norm: (\S+), clipped steps: (\d+), skipped steps: (\d+)$",
                  stdout, re.M)
    assert m and 0 <= int(m.group(3)) <= 3 and int(m.group(4)) == 0, stdout[-3000:]
    from jr.schedule import learning_rate
    want_lr = float(learning_rate(2, 3e-3, (0.94, 3), 2))                 # the third update's rate: epoch 0, warm
    assert abs(float(m.group(1)) - want_lr) <= 1e-5 * want_lr, (m.group(1), want_lr)
    meta = json.load(open(model + ".meta"))
    assert meta["accum_steps"] == K
    assert meta["weight_ema"]["updates"] == 3                             # the average counts updates: 3, 3, 1
    # ... and the same batches by hand
    steps, flat = _by_hand(d)
    assert steps == [s for _, s in status]
    raw = open(model + checkpoint.DATA_SUFFIX, "rb").read()
    assert raw == np.ascontiguousarray(flat, dtype="<f4").tobytes()
    assert np.load(out[0] / "dump" / "params_e0_r0.npy").tobytes() == flat.tobytes()
    # a second run reproduces it
    _run(d, out[1], tmp_path)
    assert open(str(out[1] / "model") + checkpoint.DATA_SUFFIX, "rb").read() == raw
    assert open(str(out[1] / "model") + checkpoint.EMA_SUFFIX, "rb").read() == open(model + checkpoint.EMA_SUFFIX,
                                                                                      "rb").read()
