"""Session: what the reference's tf.Session + graph bundle held.

train.py:99-184 builds, in one graph: the model replica (x:0 -> predictions:0),
the loss, the optimizer step, and streaming metrics named tp/fp/fn/tn/brier/
auc over `thresholds` (looked up by name in lib/evaluation.py:20-37).  Here
the replica is a jr.Engine on one GPU and the metrics are lib.metrics
states; `run_*` methods are the sess.run calls of the reference.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from lib import metrics as M


class Session:
    """engine: a jr.Engine -- or None for a pure scorer (evaluate.py: update, value,
    confusion_matrix, specificities, sensitivities over predictions computed elsewhere;
    device_metrics stays False and nothing under `model` below may be called)."""

    def __init__(self, engine, thresholds=None, num_thresholds: int = 200, kepsilon: float = 1e-7,
                 device_metrics: bool = False):
        self.engine = engine
        if thresholds is None:
            thresholds = M.generate_thresholds(num_thresholds, kepsilon) + [0.5]
        self.thresholds = list(thresholds)
        self.num_thresholds = num_thresholds
        self.kepsilon = kepsilon
        self.metrics = {
            "tp": M.create_reset_metric(M.true_positives_at_thresholds, scope="tp", thresholds=self.thresholds),
            "fp": M.create_reset_metric(M.false_positives_at_thresholds, scope="fp", thresholds=self.thresholds),
            "fn": M.create_reset_metric(M.false_negatives_at_thresholds, scope="fn", thresholds=self.thresholds),
            "tn": M.create_reset_metric(M.true_negatives_at_thresholds, scope="tn", thresholds=self.thresholds),
            "brier": M.create_reset_metric(M.mean_squared_error, scope="brier"),
            "auc": M.create_reset_metric(M.auc, scope="auc"),
        }
        self.global_step = 0
        # device_metrics: the streaming states live on the GPU while a pass runs (Engine.metrics_*:
        # this session's thresholds followed by the auc state's own), batches arrive through the
        # engine's staged feed, and train_batch / predict_enqueue return without waiting;
        # pull_metrics() brings the sums into the host states above once per pass
        self.device_metrics = bool(device_metrics)
        if self.device_metrics and engine is None:
            raise ValueError("device_metrics needs an engine: a Session without one only scores")
        if self.device_metrics:
            engine.metrics_init(self.thresholds + list(self.metrics["auc"][0].__self__.thresholds))
        # data-parallel ranks: reduce(vec float64) -> elementwise sum over ranks;
        # rank: only rank 0 prints the reference's per-pass lines
        self.reduce = None
        self.rank = 0

    def sync_metrics(self, *names) -> None:
        """Sum the streaming states of `names` over the ranks (collective: every
        rank calls it at the same point).  The states are counts and sums
        (tp/fp/fn/tn at thresholds, the AUC's own confusion counts, Brier
        total and count), so the reduced state is the state of one pass over
        every rank's batches, and every rank then reads the same value."""
        if self.reduce is None:
            return
        objs = [self.metrics[n][0].__self__ for n in names]
        parts = []
        for o in objs:
            parts += [np.ravel(o.acc)] if hasattr(o, "acc") else [np.array([o.total, o.count])]
        vec = self.reduce(np.concatenate(parts).astype(np.float64))
        k = 0
        for o in objs:
            if hasattr(o, "acc"):
                n = o.acc.size
                o.acc = vec[k:k + n].reshape(o.acc.shape).astype(np.float32)
            else:
                n = 2
                o.total, o.count = np.float32(vec[k]), np.float32(vec[k + 1])
            k += n

    # ------------------------------------------------------------ metrics
    def reset(self, *names):
        for n in names or self.metrics:
            self.metrics[n][2]()

    def update(self, labels, probs, *names):
        for n in names or self.metrics:
            self.metrics[n][1](labels, probs)

    def value(self, name):
        return self.metrics[name][0]()

    def confusion_matrix(self):
        tp, fp, fn, tn = (self.value(k) for k in ("tp", "fp", "fn", "tn"))
        return M.confusion_matrix(tp[-1], fp[-1], fn[-1], tn[-1])

    def specificities(self):
        tn, fp = self.value("tn"), self.value("fp")
        return tn / (tn + fp + np.float32(self.kepsilon))

    def sensitivities(self):
        tp, fn = self.value("tp"), self.value("fn")
        return tp / (tp + fn + np.float32(self.kepsilon))

    # ------------------------------------------------------ a metrics pass
    # begin_pass / score_batch per batch / end_pass: the one place that knows whether the
    # streaming states of a pass live on the host or on the device
    def begin_pass(self, *names) -> None:
        """Zero the states of `names` ahead of a pass (and the device sums, where they are kept there)."""
        self.reset(*names)
        if self.device_metrics:
            self.metrics_reset()

    def score_batch(self, images, labels, *names) -> Optional[np.ndarray]:
        """One batch of a pass: its forward and the update of `names`.  Returns the
        probabilities -- or None with device_metrics, where nothing is waited for
        (the device keeps every state; end_pass reads the ones it is asked for)."""
        if self.device_metrics:
            self.predict_enqueue(images, labels)
            return None
        probs = self.predict(images, labels)
        self.update(labels, probs, *names)
        return probs

    def end_pass(self, *names) -> None:
        """Close a pass: the device sums come into the host states (one synchronise),
        then the states are summed over the ranks (collective, as sync_metrics)."""
        if self.device_metrics:
            self.pull_metrics(*names)
        self.sync_metrics(*names)

    # ------------------------------------------------------------- model
    def predict(self, images, labels=None) -> np.ndarray:
        """Forward of one batch with batch-statistics BN (App. C Q1):
        `predictions:0` of evaluate.py:181-184."""
        B = self.engine.set_batch(images, labels if labels is not None else np.zeros((len(images), self.engine.units), np.float32))
        self.engine.forward(B)
        return self.engine.predictions(B)

    def train_batch(self, images, labels, augment=None, warp=None) -> tuple:
        """train.py:231-232: one step; returns (global_step, xent, probs).
        augment, warp: jr.augment tables for this (uint8) batch, or None.
        device_metrics: the batch goes through the staged feed, the step and the
        Brier sums of its probabilities are enqueued and nothing is waited for --
        the loss is in the engine's step log (Engine.step_log_enable), the
        probabilities stay on the device: (global_step, None, None)."""
        eng, ahead = self.engine, self.device_metrics
        B = eng.set_batch(images, labels, augment=augment, warp=warp, **({"staged": True} if ahead else {}))
        step = self.global_step
        eng.train_step(B, allreduce=getattr(self, "allreduce", None))
        if ahead:
            eng.metrics_update(B, counts=False, brier=True)
        # global_step counts optimizer updates: with Engine(accum_steps=K > 1) a batch that
        # leaves its group open is no step (the loss and predictions are this batch's own)
        if not getattr(eng, "accum_pending", int)():
            self.global_step += 1
        return (step, None, None) if ahead else (step, eng.loss_value(), eng.predictions(B))

    def accum_flush(self) -> bool:
        """Close a partial group of accumulated micro-batches (Engine.accum_flush;
        the end of an epoch): one more step when anything was pending."""
        flush = getattr(self.engine, "accum_flush", None)
        done = bool(flush(allreduce=getattr(self, "allreduce", None))) if flush is not None else False
        self.global_step += int(done)
        return done

    # ---------------------------------------------- device metrics (opt-in)
    def predict_enqueue(self, images, labels) -> None:
        """predict() without the wait: the forward, then the counts and the Brier
        sums of its probabilities against `labels` on the device."""
        self._need_device_metrics()
        B = self.engine.set_batch(images, labels, staged=True)
        self.engine.forward(B)
        self.engine.metrics_update(B, counts=True, brier=True)

    def metrics_reset(self) -> None:
        """Zero the device counts and Brier sums (in stream order)."""
        self._need_device_metrics()
        self.engine.metrics_reset()

    def pull_metrics(self, *names) -> None:
        """Read the device state (one synchronise) into the lib.metrics states of
        `names` (all six when none is given): `acc` of tp / fp / fn / tn and of
        auc from the counts, `total` and `count` of brier from the sums -- each
        rounded to float32 once, where the host path adds float32 batch by batch.
        value(), sync_metrics(), confusion_matrix(), specificities() then work
        as after a host pass."""
        self._need_device_metrics()
        counts, total, n = self.engine.metrics_read()
        T = len(self.thresholds)
        for name in names or self.metrics:
            state = self.metrics[name][0].__self__
            if name == "brier":
                state.total, state.count = np.float32(total), np.float32(n)
            elif name == "auc":
                state.acc = counts[:, T:].astype(np.float32)
            else:
                state.acc = counts[state.ROW, :T].astype(np.float32)

    def _need_device_metrics(self) -> None:
        if not self.device_metrics:
            raise ValueError("this session keeps its metrics on the host: Session(..., device_metrics=True)")
