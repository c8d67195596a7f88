"""evaluate.py --attribution end to end on the GPU (synthetic TFRecords, two
checkpoints trained two steps with --bn_moving at 107^2): stdout and the
operating-points CSV byte-equal to the run without the flag, maps_<k>.npy of
the right shapes and bitwise the fp32 member mean of jr.attribution.attribute
on the same batches, index.csv matching labels and predictions, and the flag
refusals."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

RES, BATCH = 107, 8


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


def test_attribution_flags_end_to_end(tmp_path):
    import torch
    from jr import checkpoint, synth_records
    from jr.attribution import attribute
    sys.path.insert(0, PKG)
    import evaluate
    import lib.dataset
    d = tmp_path / "data"
    synth_records.write_split(str(d / "train"), 24, size=RES, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 12, size=RES, start=100, num_shards=1, name="validation")
    models = [_train(tmp_path, d, "a", 1), _train(tmp_path, d, "b", 2)]

    # the refusals, before any engine is built
    for extra, word in ((["--attribution", "gradient", "--attribution_dir", str(tmp_path / "x")], "--bn moving"),
                        (["--bn", "moving", "--tta", "flips", "--attribution", "gradient", "--attribution_dir",
                          str(tmp_path / "x")], "--tta")):
        r = _evaluate(tmp_path, d, models, "refused.csv", extra)
        assert r.returncode == 2 and word in r.stderr and not os.path.exists(tmp_path / "x")

    plain = _evaluate(tmp_path, d, models, "op.csv", ["--bn", "moving"])
    assert plain.returncode == 0, plain.stdout[-3000:] + plain.stderr[-3000:]
    op_plain = open(tmp_path / "op.csv", "rb").read()      # (the same -so path: stdout prints it)
    maps_dir = tmp_path / "maps"
    attr = _evaluate(tmp_path, d, models, "op.csv", ["--bn", "moving", "--attribution", "gradient",
                                                     "--attribution_dir", str(maps_dir)])
    assert attr.returncode == 0, attr.stdout[-3000:] + attr.stderr[-3000:]
    assert attr.stdout == plain.stdout and "Brier score:" in attr.stdout
    assert open(tmp_path / "op.csv", "rb").read() == op_plain and len(op_plain) > 0
    assert attr.stderr.count("one engine per member") == 1 and "one engine per member" not in plain.stderr

    # the same batches through per-member engines here
    meta = checkpoint.read_meta(models[0])
    engines = evaluate.make_engines(models, meta, BATCH, conv_math="x8", input_grad=True)
    stats, _ = evaluate.load_bn_stats(models, engines[0].g)
    evaluate.freeze_engines(engines, stats)
    dataset = lib.dataset.initialize_dataset(
        str(d / "val"), BATCH, num_workers=2, prefetch_buffer_size=2 * BATCH, image_data_format="channels_last",
        num_channels=3, image_dim=[RES, RES], decode_dtype="uint8", shard=(0, 1))
    rows = list(csv.reader(open(maps_dir / "index.csv")))
    assert rows[0] == ["batch", "row", "label", "prediction"] and len(rows) == 13
    it, seen = iter(dataset), 0
    try:
        for k, (x, y) in enumerate(it):
            maps, preds = [], []
            for e in engines:
                n = e.set_batch(torch.as_tensor(x), y)
                e.forward(n, bn="frozen")
                preds.append(e.predictions(n).copy())
                maps.append(attribute(e, "gradient", B=n).cpu().numpy())
            mean = (maps[0] + maps[1]) / np.float32(2)
            got = np.load(maps_dir / f"maps_{k:06d}.npy")
            assert got.dtype == np.float32 and got.shape == (n, RES, RES) == mean.shape
            assert np.array_equal(got.view(np.uint32), mean.view(np.uint32)) and np.any(got > 0)
            avg = np.mean(np.array(preds), axis=0)
            for r in range(n):
                row = rows[1 + seen + r]
                assert row[:3] == [str(k), str(r), str(int(y[r, 0]))]
                assert np.float32(row[3]) == np.float32(avg[r, 0])
            seen += n
    finally:
        lib.dataset.close_iterator(it)
    assert seen == 12 and sorted(os.listdir(maps_dir)) == ["index.csv", "maps_000000.npy", "maps_000001.npy"]
