"""What train.py and evaluate.py share (jr.cli), Session as the owner of a metrics pass and as
evaluate.py's scorer, and evaluate.py's reassembly of the ranks' batches -- on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG


# ---- jr.cli
def test_importing_cli_does_not_import_torch():
    code = "import sys; import jr.cli; sys.exit(int('torch' in sys.modules))"
    assert subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=PKG)).returncode == 0


@pytest.mark.parametrize("env,local,backend,coll_dev", [
    ({}, 3, "nccl", "cuda"), ({"JR_ONE_DEVICE": "1"}, 0, "nccl", "cuda"), ({"JR_BENCH_ONE_DEVICE": "1"}, 0, "nccl", "cuda"),
    ({"JR_ONE_DEVICE": "0", "JR_DIST_BACKEND": "gloo"}, 3, "gloo", "cpu")])
def test_ranks_of_one_process(monkeypatch, env, local, backend, coll_dev):
    from jr import cli
    for name in ("RANK", "JR_ONE_DEVICE", "JR_BENCH_ONE_DEVICE", "JR_DIST_BACKEND", "MASTER_ADDR"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("LOCAL_RANK", "3")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = cli.ranks()
    assert r == (0, 1, local, backend, None, coll_dev) and r.dist is None and r.local == local
    assert "MASTER_ADDR" not in os.environ       # no process group: nothing of its setup happened
    import torch.distributed as dist
    assert not dist.is_initialized()


def test_operating_point_csv_bytes(tmp_path):
    from jr import cli
    path = tmp_path / "made" / "here" / "op.csv"       # the parent directory is created
    cli.write_operating_points(str(path), [1e-7, 0.25, 0.99995, 0.5], np.float32([0, 0.5, 1, 9]),
                               np.float32([1, 0.33331, 0.00004, 9]), 3)
    assert path.read_bytes() == (b"threshold specificity sensitivity\r\n0.0000 0.0000 1.0000\r\n"
                                 b"0.2500 0.5000 0.3333\r\n1.0000 1.0000 0.0000\r\n")


# ---- Session owns the host / device difference of a pass
class _Eng:
    units = 1

    def __init__(self):
        self.calls = []

    def set_batch(self, images, labels, staged=False):
        self.calls.append("set_batch:staged" if staged else "set_batch")
        return len(images)

    def forward(self, B):
        self.calls.append("forward")

    def predictions(self, B):
        self.calls.append("predictions")
        return np.full((B, 1), 0.75, np.float32)

    def metrics_init(self, thresholds):
        self.T = len(thresholds)

    def metrics_reset(self):
        self.calls.append("metrics_reset")

    def metrics_update(self, B, counts, brier):
        self.calls.append(f"metrics_update:counts={counts},brier={brier}")

    def metrics_read(self):
        self.calls.append("metrics_read")
        counts = np.zeros((4, self.T), np.uint32)
        counts[0] = 6       # tp (lib.metrics ROW 0)
        return counts, 6 * 0.0625, 6


X, Y = np.zeros((3, 8, 8, 3), np.uint8), np.ones((3, 1), np.float32)
COUNTS = ("tp", "fp", "fn", "tn")


def test_pass_on_the_host(monkeypatch):
    from jr.session import Session
    eng = _Eng()
    sess = Session(eng, thresholds=[0.5])
    reduced = []
    sess.reduce = lambda vec: reduced.append(len(vec)) or vec
    monkeypatch.setattr(Session, "pull_metrics", lambda *a: pytest.fail("pull_metrics on a host session"))
    sess.update(Y, np.zeros_like(Y), *COUNTS)          # stale counts: begin_pass clears them
    sess.begin_pass(*COUNTS)
    for _ in range(2):
        probs = sess.score_batch(X, Y, *COUNTS)
        assert probs.shape == (3, 1) and probs[0, 0] == 0.75
    sess.end_pass(*COUNTS)
    assert eng.calls == ["set_batch", "forward", "predictions"] * 2
    assert reduced == [4]                               # one collective for the four names
    assert [float(sess.value(k)[0]) for k in COUNTS] == [6, 0, 0, 0]
    assert sess.value("brier") == 0.0                   # a name the pass did not ask for is untouched


def test_pass_on_the_device():
    from jr.session import Session
    eng = _Eng()
    sess = Session(eng, thresholds=[0.5], device_metrics=True)
    reduced = []
    sess.reduce = lambda vec: reduced.append(len(vec)) or vec
    sess.begin_pass(*COUNTS)
    for _ in range(2):
        assert sess.score_batch(X, Y, *COUNTS) is None  # nothing comes back: nothing was waited for
    sess.end_pass(*COUNTS)
    assert eng.calls == ["metrics_reset"] + ["set_batch:staged", "forward", "metrics_update:counts=True,brier=True"] * 2 \
        + ["metrics_read"]
    assert reduced == [4]
    assert [float(sess.value(k)[0]) for k in COUNTS] == [6, 0, 0, 0]


def test_perform_test_goes_through_the_pass(capsys):
    import lib.evaluation
    from jr.session import Session
    got = {}
    for device in (False, True):
        eng = _Eng()
        sess = Session(eng, thresholds=[0.5], device_metrics=device)
        lib.evaluation.perform_test(sess, [(X, Y), (X, Y)])
        got[device] = (eng.calls, capsys.readouterr().out.split("\n")[1:])
        assert got[device][1][0] == "Confusion matrix:"
    assert got[False][0] == ["set_batch", "forward", "predictions"] * 2
    assert got[True][0][0] == "metrics_reset" and got[True][0][-1] == "metrics_read" and "predictions" not in got[True][0]
    # custom_tensors: always the host path
    eng = _Eng()
    out = lib.evaluation.perform_test(Session(eng, thresholds=[0.5], device_metrics=True), [(X, Y), (X, Y)],
                                      custom_tensors=["predictions", "labels"])
    assert eng.calls == ["set_batch", "forward", "predictions"] * 2 and [o.shape for o in out] == [(6, 1), (6, 1)]


def test_session_without_an_engine_refuses_device_metrics():
    from jr.session import Session
    with pytest.raises(ValueError, match="engine"):
        Session(None, [0.5], device_metrics=True)


# ---- Session(None, ...) as evaluate.py's scorer, against the states evaluate.py built by hand
def test_scorer_equals_the_hand_built_states():
    import lib.metrics
    from jr.session import Session
    T, eps = 200, 1e-7
    thresholds = lib.metrics.generate_thresholds(T, eps) + [0.5]
    rng = np.random.default_rng(50)
    y = (rng.random((50, 1)) < 0.4).astype(np.float32)
    p = rng.random((50, 1)).astype(np.float32)
    p[7, 0], p[8, 0] = np.float32(thresholds[60]), 0.5           # exactly on a threshold, and on the operating one
    y[7, 0], y[8, 0] = 1.0, 0.0
    # evaluate.py before Session scored for it
    names = {"tp": lib.metrics.true_positives_at_thresholds, "fp": lib.metrics.false_positives_at_thresholds,
             "fn": lib.metrics.false_negatives_at_thresholds, "tn": lib.metrics.true_negatives_at_thresholds}
    state = {k: lib.metrics.create_reset_metric(f, scope=k, thresholds=thresholds) for k, f in names.items()}
    state["brier"] = lib.metrics.create_reset_metric(lib.metrics.mean_squared_error, scope="brier")
    state["auc"] = lib.metrics.create_reset_metric(lib.metrics.auc, scope="auc")
    for value, update, reset in state.values():
        reset()
        update(y, p)
    tp, fp, fn, tn = (state[k][0]() for k in ("tp", "fp", "fn", "tn"))
    conf = lib.metrics.confusion_matrix(tp[-1], fp[-1], fn[-1], tn[-1])
    spec, sens = tn / (tn + fp + np.float32(eps)), tp / (tp + fn + np.float32(eps))

    sess = Session(None, thresholds, T, eps)
    assert sess.engine is None and sess.device_metrics is False
    sess.reset()
    sess.update(y, p)

    def same(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    for k, want in zip(("tp", "fp", "fn", "tn"), (tp, fp, fn, tn)):
        assert same(sess.value(k), want), k
    assert same(sess.value("brier"), state["brier"][0]()) and same(sess.value("auc"), state["auc"][0]())
    assert same(sess.confusion_matrix(), conf)
    assert same(sess.specificities(), spec) and same(sess.sensitivities(), sens)
    assert len(spec) == T + 1 and 0 < tp[60] < tp[0]


# ---- evaluate.merge_ranks
def _shards(world, sizes, members, batch_size, seed=3):
    """The single-rank arrays, and what predict_all returns on each of `world` ranks (batch b on rank b % world)."""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    preds = [rng.random((n, 1)).astype(np.float32) for _ in range(members)]
    labels = (rng.random((n, 1)) < 0.5).astype(np.float32)
    start = np.cumsum([0] + sizes)
    empty = np.zeros((0, 1), np.float32)
    gathered = []
    for r in range(world):
        ids = list(range(r, len(sizes), world))
        rows = [np.arange(start[b], start[b + 1]) for b in ids]
        rows = np.concatenate(rows) if rows else np.zeros(0, int)
        gathered.append((ids, [m[rows] if ids else empty for m in preds], labels[rows] if ids else empty))
    return preds, labels, gathered


def test_merge_ranks_restores_dataset_order():
    import evaluate
    preds, labels, gathered = _shards(3, [4] * 6 + [2], 2, 4)
    assert gathered[0][0] == [0, 3, 6] and gathered[0][2].shape == (10, 1)      # rank 0 holds the partial batch
    got_p, got_y = evaluate.merge_ranks(gathered, 4, 2)
    assert len(got_p) == 2 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got_p, preds))
    assert np.array_equal(got_y, labels)


@pytest.mark.parametrize("sizes", [[4, 4, 4], [4, 4, 1], [3]])
def test_merge_ranks_with_a_rank_that_received_no_batch(sizes):
    import evaluate
    preds, labels, gathered = _shards(4, sizes, 2, 4)
    assert gathered[3][0] == [] and gathered[3][2].shape == (0, 1)
    got_p, got_y = evaluate.merge_ranks(gathered, 4, 2)
    assert all(np.array_equal(a, b) for a, b in zip(got_p, preds)) and np.array_equal(got_y, labels)
