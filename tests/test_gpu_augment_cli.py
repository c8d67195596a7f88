"""train.py --augment end to end on the GPU (synthetic TFRecords, 107^2, two
steps of one epoch): a seeded augmented run is reproducible, differs from the
unaugmented run, and only it records the augmentation in the checkpoint."""
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
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "-t", str(data / "train"), "-v", str(data / "val"),
                        "-sm", str(out / "model"), "-ss", str(out / "logs"), "-so", str(out / "op.csv"),
                        "--image_size", "107", "--num_epochs", "1", "--max_steps_per_epoch", "2", "--shuffle_seed", "1",
                        "--replica_dump_dir", str(out / "dump")] + extra,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    params = np.load(out / "dump" / "params_e0_r0.npy")
    meta = json.load(open(str(out / "model") + ".meta")) if os.path.exists(str(out / "model") + ".meta") else None
    return params, meta


def test_augment_flag_is_seeded_and_recorded(tmp_path):
    from jr import synth_records
    d = tmp_path / "data"
    synth_records.write_split(str(d / "train"), 24, size=107, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 12, size=107, start=100, num_shards=1, name="validation")
    a, meta_a = _train(tmp_path, d, "aug_a", ["--augment", "--augment_seed", "3"])
    b, meta_b = _train(tmp_path, d, "aug_b", ["--augment", "--augment_seed", "3"])
    c, meta_c = _train(tmp_path, d, "plain", [])
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != c.tobytes()
    assert np.all(np.isfinite(a))
    assert meta_a is not None and meta_c is not None, "no checkpoint was written"
    assert meta_a["augment"] == meta_b["augment"] == {
        "spec": {"flip": True, "hue": 0.2, "saturation": [0.5, 1.5], "contrast": [0.5, 1.5], "brightness": 0.125},
        "seed": 3}
    assert "augment" not in meta_c and "tile_table" in meta_c
