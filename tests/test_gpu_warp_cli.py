"""train.py --augment_rotate / --augment_zoom and evaluate.py --tta end to end
on the GPU (synthetic TFRecords, 107^2, two steps of one epoch): a seeded
geometric run is reproducible, differs from the colour-only run of the same
seed, and only it records `augment_warp`; test-time augmentation is bitwise
the mean of plain forwards over host-permuted copies of the same batches,
grouped and per member; without --tta evaluate.py prints and writes what it
does with --tta none."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

AUGMENT_META = {"spec": {"flip": True, "hue": 0.2, "saturation": [0.5, 1.5], "contrast": [0.5, 1.5],
                         "brightness": 0.125}, "seed": 3}


def _train(tmp_path, data, name, extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "-t", str(data / "train"), "-v", str(data / "val"),
                        "-sm", str(out / "model"), "-ss", str(out / "logs"), "-so", str(out / "op.csv"),
                        "--image_size", "107", "--num_epochs", "1", "--max_steps_per_epoch", "2", "--shuffle_seed", "1",
                        "--replica_dump_dir", str(out / "dump")] + extra,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(str(out / "model") + ".meta"), "no checkpoint was written"
    return np.load(out / "dump" / "params_e0_r0.npy"), json.load(open(str(out / "model") + ".meta")), str(out / "model")


def _evaluate(tmp_path, data, model, csv, extra):
    return subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "-o", "--data_dir", str(data / "val"),
                           "-lm", model, "-b", "8", "-so", str(tmp_path / csv)] + extra,
                          cwd=str(tmp_path), capture_output=True, text=True, timeout=600)


def _host_view(x, mode, k):
    """View k of a [n, h, w, 3] uint8 batch, permuted on the host."""
    if mode == "flips":
        x = x[:, :, ::-1] if k & 1 else x
        x = x[:, ::-1] if k & 2 else x
    else:
        x = np.rot90(x, k % 4, axes=(1, 2))
        x = x[:, :, ::-1] if k >= 4 else x
    return np.ascontiguousarray(x)


def _batches(data_dir, batch_size, size):
    """The uint8 batches evaluate.predict_all decodes, in its order."""
    import evaluate
    import lib.dataset
    dataset = lib.dataset.initialize_dataset(
        data_dir, batch_size, num_workers=evaluate.NUM_WORKERS, prefetch_buffer_size=2 * batch_size,
        image_data_format="channels_last", num_channels=3, image_dim=[size, size], decode_dtype="uint8", shard=(0, 1))
    it = iter(dataset)
    try:
        return [(np.array(x), np.array(y)) for x, y in it]
    finally:
        lib.dataset.close_iterator(it)


def test_geometric_augmentation_and_tta_end_to_end(tmp_path):
    import evaluate
    from jr import checkpoint, synth_records
    d = tmp_path / "data"
    synth_records.write_split(str(d / "train"), 24, size=107, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 12, size=107, start=100, num_shards=1, name="validation")
    geometry = ["--augment", "--augment_seed", "3", "--augment_rotate", "30", "--augment_zoom", "0.9,1.1"]
    a, meta_a, model_a = _train(tmp_path, d, "geo_a", geometry)
    b, meta_b, _ = _train(tmp_path, d, "geo_b", geometry)
    c, meta_c, model_c = _train(tmp_path, d, "colour", ["--augment", "--augment_seed", "3"])
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != c.tobytes()
    assert np.all(np.isfinite(a))
    assert meta_a["augment_warp"] == meta_b["augment_warp"] == {
        "spec": {"rotate": 30.0, "zoom": [0.9, 1.1], "shift": 0.0}, "seed": 3}
    assert "augment_warp" not in meta_c
    assert meta_a["augment"] == meta_b["augment"] == meta_c["augment"] == AUGMENT_META

    # ---- test-time augmentation against plain forwards of host-permuted batches
    paths = [model_a, model_c]
    meta = checkpoint.read_meta(model_a)
    batches = _batches(str(d / "val"), 8, 107)
    assert [len(x) for x, _ in batches] == [8, 4]           # a full and a partial batch
    for grouped in (True, False):
        engines = evaluate.make_engines(paths, meta, 8, grouped=grouped)
        every = [engines] if grouped else engines

        def forward(x, y):
            n = 0
            for e in every:
                n = e.set_batch(x, y)
                e.forward(n)
            return list(engines.predictions(n)) if grouped else [e.predictions(n) for e in every]

        for mode, nviews in (("flips", 4), ("d4", 8)):
            seen = [[forward(_host_view(x, mode, k), y) for k in range(nviews)] for x, y in batches]
            want = [np.vstack([np.mean(np.array([v[m] for v in views]), axis=0) for views in seen])
                    for m in range(len(paths))]
            got, labels, ids = evaluate.predict_all(engines, str(d / "val"), 8, tta=mode)
            assert ids == [0, 1] and labels.shape == (12, 1)
            for m in range(len(paths)):
                assert got[m].shape == (12, 1) and got[m].tobytes() == want[m].tobytes(), (grouped, mode, m)
            views0 = seen[0]
            assert any(not np.array_equal(views0[0][0], views0[k][0]) for k in range(1, nviews)), (grouped, mode)
        plain, _, _ = evaluate.predict_all(engines, str(d / "val"), 8)
        none, _, _ = evaluate.predict_all(engines, str(d / "val"), 8, tta="none")
        assert all(p.tobytes() == q.tobytes() for p, q in zip(plain, none))
        assert plain[0].tobytes() == np.vstack([forward(x, y)[0] for x, y in batches]).tobytes()
        del engines, every

    # ---- the command line
    r = _evaluate(tmp_path, d, model_a, "d4.csv", ["--tta", "d4"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("Test-time augmentation: d4 (8 views)") == 1
    assert "Brier score:" in r.stdout and "AUC:" in r.stdout
    p = _evaluate(tmp_path, d, model_a, "plain.csv", [])
    q = _evaluate(tmp_path, d, model_a, "none.csv", ["--tta", "none"])
    assert p.returncode == 0 and q.returncode == 0, p.stderr[-3000:] + q.stderr[-3000:]
    assert "Test-time augmentation" not in p.stdout
    assert p.stdout.replace("plain.csv", "none.csv") == q.stdout
    assert open(tmp_path / "plain.csv").read() == open(tmp_path / "none.csv").read()
