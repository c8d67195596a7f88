"""train.py with the optimizer recipe end to end on the GPU (synthetic
TFRecords, 107^2, two steps of one epoch): it exits 0, records the recipe in
the checkpoint .meta and prints the epoch's recipe line."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu


def test_recipe_flags_train_and_are_recorded(tmp_path):
    from jr import synth_records
    d = tmp_path / "data"
    synth_records.write_split(str(d / "train"), 24, size=107, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 12, size=107, start=100, num_shards=1, name="validation")
    out = tmp_path / "recipe"
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "-t", str(d / "train"), "-v", str(d / "val"),
                        "-sm", str(out / "model"), "-ss", str(out / "logs"), "-so", str(out / "op.csv"),
                        "--image_size", "107", "--num_epochs", "1", "--max_steps_per_epoch", "2", "--shuffle_seed", "1",
                        "--replica_dump_dir", str(out / "dump"),
                        "--weight_decay", "4e-5", "--clip_norm", "2", "--lr_decay", "0.94,1", "--lr_warmup", "2"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert np.all(np.isfinite(np.load(out / "dump" / "params_e0_r0.npy")))
    assert os.path.exists(str(out / "model") + ".meta"), "no checkpoint was written"
    meta = json.load(open(str(out / "model") + ".meta"))
    assert meta["optimizer"] == {"learning_rate": 3e-3, "lr_decay": [0.94, 1], "lr_warmup": 2, "weight_decay": 4e-5,
                                 "clip_norm": 2.0}
    assert "tile_table" in meta
    m = re.search(r"^Learning rate: (\S+), median gradient norm: (\S+), clipped steps: (\d+), skipped steps: (\d+)$",
                  r.stdout, re.M)
    assert m, r.stdout[-3000:]
    # the rate of the epoch's last step (its first or second, as the records fill one or two batches), to 6 digits
    from jr.schedule import learning_rate
    want = [float(learning_rate(s, 3e-3, (0.94, s + 1), 2)) for s in (0, 1)]      # (one epoch = s + 1 steps)
    assert any(abs(float(m.group(1)) - v) <= 1e-5 * v for v in want), (m.group(1), want)
    assert np.isfinite(float(m.group(2))) and float(m.group(2)) > 0
    assert 0 <= int(m.group(3)) <= 2 and int(m.group(4)) == 0
