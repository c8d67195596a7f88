"""train.py --status_every end to end on the GPU (synthetic TFRecords, 107^2, one
epoch of five batches -- four of 64 and one of 8 -- 48 validation images, the
device recipe flags): N = 3 runs ahead of the host (the staged feed, the step
log, the metrics on the device) and must leave what N = 1 leaves -- the same
checkpoint and weight average byte for byte, the same report lines and
operating-point CSV -- with fewer status lines."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

RES, BATCHES = 107, 5
FLAGS = ["--optimizer", "rmsprop", "--weight_decay", "4e-5", "--clip_norm", "2", "--lr_decay", "0.94,1",
         "--lr_warmup", "2", "--weight_ema", "0.5"]
SAME_LINES = ("Learning rate:", "Brier score", "New peak auc")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    from jr import synth_records
    d = tmp_path_factory.mktemp("status_records")
    synth_records.write_split(str(d / "train"), 4 * 64 + 8, size=RES, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 48, size=RES, start=1000, num_shards=1, name="validation")
    return d


def _run(d, out, cwd, every):
    argv = ["-t", str(d / "train"), "-v", str(d / "val"), "-sm", str(out / "model"), "-ss", str(out / "logs"),
            "-so", str(out / "op.csv"), "--image_size", str(RES), "--num_epochs", "1", "--shuffle_seed", "1",
            "--max_steps_per_epoch", str(BATCHES), "--status_every", str(every)] + FLAGS
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py")] + argv, cwd=str(cwd),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(str(out / "model") + ".meta"), "no checkpoint was written:\n" + r.stdout[-3000:]
    return r.stdout


def _lines(stdout):
    return [ln for chunk in stdout.split("\n") for ln in chunk.split("\r")]


def _picked(stdout):
    lines = _lines(stdout)
    got = {k: [ln for ln in lines if ln.startswith(k)] for k in SAME_LINES}
    i = lines.index("Confusion matrix:")
    got["Confusion matrix"] = lines[i:i + 3]
    return got


def test_status_every_3_leaves_what_status_every_1_leaves(records, tmp_path):
    from jr import checkpoint
    out = {n: tmp_path / f"every{n}" for n in (1, 3)}
    stdout = {n: _run(records, out[n], tmp_path, n) for n in (1, 3)}
    model = {n: str(out[n] / "model") for n in (1, 3)}
    for suffix in (checkpoint.DATA_SUFFIX, checkpoint.EMA_SUFFIX):
        assert open(model[1] + suffix, "rb").read() == open(model[3] + suffix, "rb").read(), suffix
    assert open(out[1] / "op.csv", "rb").read() == open(out[3] / "op.csv", "rb").read()
    a, b = _picked(stdout[1]), _picked(stdout[3])
    for k in a:
        assert a[k] and a[k] == b[k], (k, a[k], b[k])
    assert len(a["Learning rate:"]) == 1 and "median gradient norm" in a["Learning rate:"][0]
    # End of epoch: the same line but for the Brier value, which the device sums in fp64 and the host in
    # fp32 -- it agrees to the printed digits but one
    end = {n: re.findall(r"^End of epoch (\d+)! \(Brier: ([^)]*)\)$", stdout[n], re.M) for n in (1, 3)}
    assert len(end[1]) == len(end[3]) == 1 and end[1][0][0] == end[3][0][0] == "0"
    b1, b3 = float(end[1][0][1]), float(end[3][0][1])
    assert 0 < b1 < 1 and abs(b1 - b3) <= 1e-5 * b1, (b1, b3)
    # the status lines: one per batch, or one per three batches, each with its batch's own step
    status = {n: [(int(x), int(s)) for x, s in re.findall(r"Batch:\s+(\d+), Xent:\s*[-+0-9.e]+, Step:\s+(\d+)",
                                                          stdout[n])] for n in (1, 3)}
    assert status[1] == [(i, i) for i in range(BATCHES)]
    assert status[3] == [(2, 2)]
    meta = {n: json.load(open(model[n] + ".meta")) for n in (1, 3)}
    assert meta[3]["status_every"] == 3 and "status_every" not in meta[1]
    assert meta[1]["weight_ema"]["updates"] == meta[3]["weight_ema"]["updates"] == BATCHES
