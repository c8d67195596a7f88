"""train.py's loop on the CPU, against a stub engine that records its calls and returns canned
losses, probabilities, opt_step() tuples and step-log records: the batch loop of an epoch in both
modes (--status_every 1: every batch waits; N > 1: the host runs ahead), the tally of the updates,
early stopping, and what the flags hand to Engine(...) and to the checkpoint .meta."""
import io

import numpy as np
import pytest

F = lambda v: float(np.float32(v))      # noqa: E731  (the step log holds fp32: canned values that survive it)
CLIP = 0.1
LOSSES = [0.5, 0.25, 0.75, 0.125, 0.375]
# (norm, skipped) of the updates in order: one above the clip, one EQUAL to it in fp32 (above it as a
# double: only the fp32 comparison leaves it unclipped), one skipped with an infinite norm, ...
UPDATES = [(F(0.3), 0), (F(CLIP), 0), (float("inf"), 1), (F(0.05), 0), (F(0.25), 0)]
BATCHES = [(np.zeros((4, 8, 8, 3), np.uint8), np.zeros((4, 1), np.float32)) for _ in LOSSES]


class StubEngine:
    units = 1

    def __init__(self, k):
        from jr.runahead import STEP_REC
        self.rec, self.k, self.calls = STEP_REC, k, []
        self.batches = self.pending = self.updates = self.flushes = 0
        self.log, self.last = [], None

    def _update(self):
        self.pending, self.last, self.updates = 0, UPDATES[self.updates], self.updates + 1

    def _append(self, updated):
        norm, skip = self.last if updated else (0.0, 0)
        self.log.append((LOSSES[self.batches - 1], norm, 1.0, int(updated) | skip << 1))

    def set_batch(self, images, labels, augment=None, warp=None, staged=False):
        self.calls.append("set_batch:staged" if staged else "set_batch")
        return len(images)

    def set_lr(self, lr):
        self.calls.append("set_lr")

    def train_step(self, B, allreduce=None):
        self.calls.append("train_step")
        self.batches, self.pending = self.batches + 1, self.pending + 1
        updated = self.pending == self.k
        if updated:
            self._update()
        self._append(updated)

    def accum_pending(self):
        return self.pending

    def accum_flush(self, allreduce=None):
        self.calls.append("accum_flush")
        if not self.pending:
            return False
        self._update()
        self._append(True)
        self.flushes += 1
        return True

    def loss_value(self):
        self.calls.append("loss_value")
        return LOSSES[self.batches - 1]

    def predictions(self, B):
        self.calls.append("predictions")
        return np.full((B, 1), 0.25, np.float32)

    def opt_step(self):
        self.calls.append("opt_step")
        return self.last[0], 1.0, self.last[1], 0

    def step_log_read(self):
        self.calls.append("step_log_read")
        recs, self.log = np.array(self.log, self.rec), []
        return recs

    def forward(self, B):
        self.calls.append("forward")

    def metrics_init(self, thresholds):
        self.T = len(thresholds)

    def metrics_reset(self):
        self.calls.append("metrics_reset")

    def metrics_update(self, B, counts, brier):
        self.calls.append(f"metrics_update:counts={counts},brier={brier}")

    def metrics_read(self):
        self.calls.append("metrics_read")
        return np.zeros((4, self.T), np.uint32), 0.0625 * 4 * self.batches, 4 * self.batches


def _epoch(every, k, **more):
    import train
    from jr.schedule import accum_groups
    from jr.session import Session
    argv = ["--clip_norm", str(CLIP), "--status_every", str(every), "--num_epochs", "1"]
    args = train.build_parser().parse_args(argv + (["--accum_steps", str(k)] if k > 1 else []))
    eng = StubEngine(k)
    sess = Session(eng, thresholds=[0.5], device_metrics=every > 1)
    sched = train.Schedule(train.opt_recipe(args), accum_groups(len(BATCHES), k)[1])
    tally, out = train.UpdateTally(args.clip_norm), io.StringIO()
    train.train_epoch(sess, eng, BATCHES, args, 0, sched, train.Augmenter(args, 0), tally, 0, out=out, **more)
    return eng, sess, tally, out.getvalue()


STATUS = {      # (status_every, accum_steps) -> the printed lines: which batches, which Step values
    (1, 1): ["Epoch: 0/1, Batch:    0, Xent:    0.5, Step:          0",
             "Epoch: 0/1, Batch:    1, Xent:   0.25, Step:          1",
             "Epoch: 0/1, Batch:    2, Xent:   0.75, Step:          2",
             "Epoch: 0/1, Batch:    3, Xent:  0.125, Step:          3",
             "Epoch: 0/1, Batch:    4, Xent:  0.375, Step:          4"],
    (1, 2): ["Epoch: 0/1, Batch:    0, Xent:    0.5, Step:          0",       # Step counts updates
             "Epoch: 0/1, Batch:    1, Xent:   0.25, Step:          0",
             "Epoch: 0/1, Batch:    2, Xent:   0.75, Step:          1",
             "Epoch: 0/1, Batch:    3, Xent:  0.125, Step:          1",
             "Epoch: 0/1, Batch:    4, Xent:  0.375, Step:          2"],
    (3, 1): ["Epoch: 0/1, Batch:    2, Xent:   0.75, Step:          2"],
    (3, 2): ["Epoch: 0/1, Batch:    2, Xent:   0.75, Step:          1"],
}


@pytest.mark.parametrize("every,k", sorted(STATUS))
def test_status_lines_and_tally(every, k):
    eng, sess, tally, printed = _epoch(every, k)
    assert printed == "".join(line + "\r" for line in STATUS[every, k])
    assert eng.batches == 5 and sess.global_step == eng.updates == (5 if k == 1 else 3)
    # a partial group is flushed exactly once (and a flush with nothing pending is no update)
    assert eng.calls.count("accum_flush") == 1 and eng.flushes == (0 if k == 1 else 1)
    assert tally.norms == [u[0] for u in UPDATES[:eng.updates]]
    # only a norm strictly above clip_norm (both in fp32) is clipped; the skipped step is not
    assert (tally.clipped, tally.skipped) == ((2, 1) if k == 1 else (1, 1))
    assert tally.median() == ((F(CLIP) + F(0.25)) / 2 if k == 1 else (F(0.3) + F(CLIP)) / 2)
    assert tally.step_lr == F(3e-3)
    assert tally.line() == ("Learning rate: 0.003, median gradient norm: {}, clipped steps: {}, skipped steps: 1"
                            .format(*(("0.175", 2) if k == 1 else ("0.2", 1))))
    assert tally.summary() == {"grad_norm": tally.median(), "learning_rate": F(3e-3)}
    assert sess.value("brier") == np.float32(0.0625)       # (0.25 - 0)^2 on either path


def test_call_order_every_batch_waits():
    eng = _epoch(1, 1)[0]
    batch = ["set_lr", "set_batch", "train_step", "loss_value", "predictions", "opt_step"]
    assert eng.calls == batch * 5 + ["accum_flush"]
    eng = _epoch(1, 2)[0]       # opt_step only after a batch that closed an update, and after the flush
    open_, close = batch[:-1], batch
    assert eng.calls == open_ + close + open_ + close + open_ + ["accum_flush", "opt_step"]


def test_call_order_running_ahead():
    batch = ["set_lr", "set_batch:staged", "train_step", "metrics_update:counts=False,brier=True"]
    end = ["accum_flush", "step_log_read", "metrics_read"]
    for k in (1, 2):        # nothing is read per batch: the log every third batch and at the end, the sums once
        eng = _epoch(3, k)[0]
        assert eng.calls == ["metrics_reset"] + batch * 3 + ["step_log_read"] + batch * 2 + end


@pytest.mark.parametrize("k", [1, 2])
def test_both_modes_keep_the_same_tally(k):
    a, b = _epoch(1, k)[2], _epoch(3, k)[2]
    assert (a.norms, a.clipped, a.skipped, a.step_lr) == (b.norms, b.clipped, b.skipped, b.step_lr)
    assert a.line() == b.line() and a.summary() == b.summary()


def test_batch_limits():
    assert _epoch(1, 1, limit=3)[0].batches == 3        # data parallel: every rank runs the same number
    import train
    from jr.session import Session
    args = train.build_parser().parse_args(["--max_steps_per_epoch", "2"])
    eng = StubEngine(1)
    tally = train.UpdateTally()
    train.train_epoch(Session(eng, thresholds=[0.5]), eng, BATCHES, args, 0, None, train.Augmenter(args, 0), tally, 1,
                      out=None)       # (rank 1 prints nothing; no schedule: no rate is set, no update is read)
    assert eng.calls == ["set_batch", "train_step", "loss_value", "predictions"] * 2 + ["accum_flush"]
    assert tally.norms == [] and tally.step_lr is None


# ---- early stopping: the present code's decisions, transcribed
def _decisions(aucs):
    import train
    stop, got = train.EarlyStop(), []
    for auc in aucs:
        got.append((stop.step(auc), stop.peak, stop.waited))
        if got[-1][0] == "stop":
            break
    return got


def test_early_stop_after_wait_epochs_plus_one():
    import train
    assert (train.EarlyStop.wait, train.EarlyStop.min_delta) == (train.WAIT_EPOCHS, train.MIN_DELTA_AUC) == (10, 0.01)
    # a peak, then epochs that do not beat it by 0.01: ten of them wait, the eleventh stops
    got = _decisions([0.7] + [0.705] * 30)
    assert got == [("peak", 0.7, 0)] + [("wait", 0.7, w) for w in range(1, 11)] + [("stop", 0.7, 10)]
    # no epoch ever reaches 0.01: the peak stays 0.0 and nothing is saved
    got = _decisions([0.005] * 30)
    assert got == [("wait", 0.0, w) for w in range(1, 11)] + [("stop", 0.0, 10)]


def test_early_stop_wait_is_reset_by_a_new_peak():
    got = _decisions([0.6, 0.605, 0.6, 0.609, 0.62] + [0.62] * 10 + [0.629, 0.64])
    assert got == ([("peak", 0.6, 0), ("wait", 0.6, 1), ("wait", 0.6, 2), ("wait", 0.6, 3), ("peak", 0.62, 0)]
                   + [("wait", 0.62, w) for w in range(1, 11)] + [("stop", 0.62, 10)])
    # an AUC of exactly peak + MIN_DELTA_AUC is a new peak (the test is `<`)
    assert _decisions([0.5, 0.5 + 0.01])[-1] == ("peak", 0.5 + 0.01, 0)


# ---- what the flags hand to Engine(...) and to the checkpoint .meta
def test_no_flags_are_the_reference_settings():
    import train
    args = train.build_parser().parse_args([])
    assert train.engine_kwargs(args, 0, 0) == {"device": 0, "optimizer": "nesterov", "lr": 3e-3, "momentum": 0.9,
                                               "seed": 0, "dtype": "f32", "conv_math": "x6h", "tiles": "pinned"}
    assert train.engine_kwargs(args, 5, 2)["device"] == 2
    assert train.run_meta(args, None, None) == {}


def test_every_feature_flag_at_once_is_the_union_of_the_helpers():
    import train
    args = train.build_parser().parse_args(
        ["--augment", "--augment_rotate", "10", "--bn_moving", "--learning_rate", "0.01", "--lr_decay", "0.94,2",
         "--lr_warmup", "3", "--weight_decay", "4e-5", "--clip_norm", "2", "--optimizer", "rmsprop", "--rmsprop",
         "0.95,0.8,0.1", "--weight_ema", "--label_smoothing", "0.1", "--pos_weight", "2", "--focal_gamma", "1",
         "--dropout", "0.2", "--dropout_seed", "7", "--accum_steps", "2", "--status_every", "3", "--dtype", "bf16",
         "--tiles", "autotune", "--seed", "4", "--augment_seed", "9"])
    assert train.engine_kwargs(args, 3, 1) == {
        "device": 1, "optimizer": "rmsprop", "lr": 0.01, "momentum": 0.9, "seed": 4, "dtype": "bf16",
        "conv_math": "bf16", "tiles": "heuristic", "bn_moving": 0.99, **train.opt_engine_kwargs(args),
        **train.ema_engine_kwargs(args), **train.loss_engine_kwargs(args, 3), **train.accum_meta(args)}
    assert {"device_lr", "rmsprop_rho", "weight_ema", "dropout_stream", "accum_steps"} <= set(train.engine_kwargs(args, 3, 1))
    aug, geo = train.augment_spec(args), train.warp_spec(args)
    assert train.run_meta(args, aug, geo) == {
        "augment": {"spec": aug.to_meta(), "seed": 9}, "augment_warp": {"spec": geo.to_meta(), "seed": 9},
        "optimizer": {**train.opt_recipe(args), **train.optimizer_meta(args)}, "loss": train.loss_meta(args),
        "accum_steps": 2, "status_every": 3}
    assert train.run_meta(args, aug, None).keys() == train.run_meta(args, aug, geo).keys() - {"augment_warp"}
