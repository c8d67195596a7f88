"""Images per second of the hand-driven Session loop over synthetic records, 299^2, B = 64, 40 batches,
loader included: A (every batch waits: train.py --status_every 1) against B (Session(device_metrics=True),
the step log read every 50 batches), interleaved A/B/A/B in one process, f32 (x6h) and bf16 (DESIGN.md
§15).  `python tools/train_loop_bench.py [OUT.txt]` prints its table and, with OUT, keeps it there as it
grows (profiles/train_loop_runahead.txt)."""
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jama16-retina-replication_amd")
sys.path[:0] = [ROOT, PKG]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lib.dataset  # noqa: E402
import train  # noqa: E402
from jr import synth_records  # noqa: E402
from jr.engine import Engine  # noqa: E402
from jr.schedule import learning_rate  # noqa: E402
from jr.session import Session  # noqa: E402

RES, BATCHES, WARM, READ_EVERY = 299, 40, 4, 50
OUT = sys.argv[1] if len(sys.argv) > 1 else None
DATA = os.path.join(tempfile.gettempdir(), "jr_train_loop_bench_records")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


def batches(ds, n):
    got = 0
    while got < n:
        it = iter(ds)
        try:
            for images, labels in it:
                if len(images) != train.TRAIN_BATCH_SIZE:
                    continue
                yield images, labels
                got += 1
                if got == n:
                    return
        finally:
            lib.dataset.close_iterator(it)


def run(dtype, ahead):
    ds = lib.dataset.initialize_dataset(
        DATA, train.TRAIN_BATCH_SIZE, num_workers=train.NUM_WORKERS, prefetch_buffer_size=2 * train.TRAIN_BATCH_SIZE,
        shuffle_buffer_size=train.SHUFFLE_BUFFER_SIZE, image_data_format="channels_last",
        num_channels=train.NUM_CHANNELS, image_dim=[RES, RES], seed=1, decode_dtype="uint8", shard=None)
    eng = Engine(64, RES, RES, device=0, dtype=dtype, conv_math="x6h" if dtype == "f32" else "bf16", tiles="pinned",
                 weight_decay=4e-5, clip_norm=2.0, device_lr=True, seed=0)
    sess = Session(eng, device_metrics=ahead)
    if ahead:
        eng.step_log_enable(READ_EVERY + WARM + 2)
    sink = io.StringIO()
    norms = []
    t0 = None
    for b, (images, labels) in enumerate(batches(ds, WARM + BATCHES)):
        if b == WARM:
            eng.synchronize()
            t0 = time.perf_counter()
        eng.set_lr(float(learning_rate(sess.global_step, train.LEARNING_RATE, None, 2)))
        step, xent, probs = sess.train_batch(images, labels)
        if ahead:
            if b % READ_EVERY == READ_EVERY - 1:
                rec = eng.step_log_read()
                norms += rec["grad_norm"].tolist()
                print(train.status_line(0, 1, b, float(rec["loss"][-1]), step), end="\r", file=sink)
        else:
            norms.append(eng.opt_step()[0])
            sess.update(labels, probs, "brier")
            print(train.status_line(0, 1, b, xent, step), end="\r", file=sink)
    if ahead:
        norms += eng.step_log_read()["grad_norm"].tolist()
        sess.pull_metrics("brier")
    eng.synchronize()
    dt = time.perf_counter() - t0
    brier = sess.value("brier")
    eng.close()
    del eng, sess
    torch.cuda.empty_cache()
    assert len(norms) == WARM + BATCHES and np.all(np.isfinite(norms))
    return BATCHES * 64 / dt, 1e3 * dt / BATCHES, brier


def main():
    t = time.perf_counter()
    if not os.path.isdir(DATA):
        synth_records.write_split(DATA, 10 * 64, size=RES, num_shards=2, name="train")
    say(f"# train-loop run-ahead A/B: {RES}^2, B = 64, {BATCHES} timed batches after {WARM} warm-up, loader included")
    say(f"# (640 synthetic records walked repeatedly; records written in {time.perf_counter() - t:.1f} s)")
    say("# A = every batch waits (loss_value, predictions, opt_step, host Brier: --status_every 1)")
    say(f"# B = Session(device_metrics=True), staged feed, step log read every {READ_EVERY} batches")
    say("# dtype order imgs_per_s ms_per_batch brier")
    for dtype in ("f32", "bf16"):
        res = {"A": [], "B": []}
        for k, which in enumerate("ABAB"):
            ips, ms, brier = run(dtype, which == "B")
            res[which].append(ips)
            say(f"{dtype} {which}{k // 2 + 1} {ips:9.1f} {ms:8.2f} {brier:.6f}")
        a, b = res["A"], res["B"]
        say(f"{dtype} summary: A mean {np.mean(a):.1f} img/s (spread of the two A runs {abs(a[0] - a[1]):.1f}), "
            f"B mean {np.mean(b):.1f} img/s (spread {abs(b[0] - b[1]):.1f}), B - A = {np.mean(b) - np.mean(a):+.1f} img/s")


if __name__ == "__main__":
    main()
