"""Gradient accumulation's host side (no GPU): the group planner, the learning
rate evaluated at update counts, Session's step counter, train.py's
--accum_steps, and jr_grad_accumulate's argument validation before any HIP
call."""
import numpy as np
import pytest

import accum_ref
from accum_ref import f32


# ---- the planner
@pytest.mark.parametrize("batches,k,sizes", [
    (10, 4, [4, 4, 2]), (7, 3, [3, 3, 1]), (8, 4, [4, 4]), (10, 1, [1] * 10), (3, 8, [3]), (1, 1, [1]), (0, 4, []),
    (5, 5, [5]), (6, 5, [5, 1])])
def test_planner(batches, k, sizes):
    from jr.schedule import accum_groups
    assert accum_groups(batches, k) == (sizes, len(sizes)) == accum_ref.groups(batches, k)
    assert sum(sizes) == batches and len(sizes) == -(-batches // k)
    assert all(s == k for s in sizes[:-1]) and all(1 <= s <= k for s in sizes)


def test_planner_matches_its_restatement_and_refuses_nonsense():
    from jr.schedule import accum_groups
    for batches in range(0, 40):
        for k in range(1, 12):
            assert accum_groups(batches, k) == accum_ref.groups(batches, k)
    assert accum_groups(10, 1)[1] == 10                  # K = 1: today's count, one update per batch
    for bad in ((-1, 2), (4, 0), (4, -3)):
        with pytest.raises(ValueError):
            accum_groups(*bad)


# ---- Session counts updates; the rate is a function of that count
class _FakeEngine:
    """train_step / accum_flush / accum_pending of jr.Engine, counting only."""
    units = 1

    def __init__(self, k):
        self.k, self.pending, self.updates_run, self.flushes = k, 0, 0, 0

    def set_batch(self, images, labels, augment=None, warp=None):
        return len(images)

    def train_step(self, B, allreduce=None):
        self.pending += 1
        if self.pending == self.k:
            self.pending, self.updates_run = 0, self.updates_run + 1

    def accum_pending(self):
        return self.pending

    def accum_flush(self, allreduce=None):
        if not self.pending:
            return False
        self.pending, self.updates_run, self.flushes = 0, self.updates_run + 1, self.flushes + 1
        return True

    def loss_value(self):
        return 0.5

    def predictions(self, B):
        return np.zeros((B, 1), np.float32)


@pytest.mark.parametrize("batches,k", [(10, 4), (7, 3), (6, 3), (5, 1), (2, 5)])
def test_session_counts_updates_and_the_rate_follows_them(batches, k):
    """Two epochs of `batches` batches: global_step is the number of updates,
    the value train_batch returns is the one before the batch, the rate set
    ahead of every batch is learning_rate(updates so far) -- constant inside a
    group -- with the staircase counted in updates per epoch and the warm-up
    in updates."""
    from jr.schedule import accum_groups, learning_rate
    from jr.session import Session
    eng = _FakeEngine(k)
    sess = Session(eng, thresholds=[0.5])
    sizes, per_epoch = accum_groups(batches, k)
    base, decay, warmup = 0.045, (0.94, 1 * per_epoch), 3
    x, y = np.zeros((2, 4, 4, 3), np.uint8), np.zeros((2, 1), np.float32)
    seen = []
    for epoch in range(2):
        for size in sizes:
            first = sess.global_step
            for j in range(size):
                lr = learning_rate(sess.global_step, base, decay, warmup)
                step, _, _ = sess.train_batch(x, y)
                assert step == first                          # the status line's Step: updates before this batch
                seen.append((sess.global_step, lr))
                assert sess.global_step == first + int(j + 1 == k)
            flushed = sess.accum_flush() if size < k else False
            assert flushed == (size < k) and sess.global_step == first + 1
        assert sess.accum_flush() is False                    # nothing pending: a no-op
        assert sess.global_step == (epoch + 1) * per_epoch == eng.updates_run
    assert eng.flushes == 2 * int(batches % k != 0)
    # the rate of update u, in float32 and in the stated order
    for u in range(2 * per_epoch):
        p = f32(1)
        for _ in range(u // per_epoch):
            p = f32(p * f32(0.94))
        want = f32(f32(base) * p)
        if u + 1 < warmup:
            want = f32(want * f32(f32(u + 1) / f32(warmup)))
        assert learning_rate(u, base, decay, warmup) == want
    # the first epoch's batches all ran at epoch-0 rates, the second's one staircase step down
    assert {lr for _, lr in seen[batches:]} <= {learning_rate(u, base, decay, warmup)
                                                 for u in range(per_epoch, 2 * per_epoch)}


def test_session_with_an_engine_that_does_not_accumulate():
    """An engine without accum_pending / accum_flush (jr.EnsembleEngine, stand-ins): one step per batch, as ever."""
    from jr.session import Session

    class Plain:
        units = 1
        set_batch = _FakeEngine.set_batch
        loss_value = _FakeEngine.loss_value
        predictions = _FakeEngine.predictions

        def train_step(self, B, allreduce=None):
            pass

    sess = Session(Plain(), thresholds=[0.5])
    x, y = np.zeros((2, 4, 4, 3), np.uint8), np.zeros((2, 1), np.float32)
    assert [sess.train_batch(x, y)[0] for _ in range(3)] == [0, 1, 2] and sess.global_step == 3
    assert sess.accum_flush() is False and sess.global_step == 3


# ---- train.py's flag
def test_flag_off_by_default():
    import train
    args = train.build_parser().parse_args([])
    assert args.accum_steps is None
    assert train.accum_meta(args) == {} and train.accum_line(args, 1, 10) is None


@pytest.mark.parametrize("text,k", [("1", 1), ("3", 3), ("25", 25)])
def test_flag_values(text, k):
    import train
    args = train.build_parser().parse_args(["--accum_steps", text])
    assert args.accum_steps == k
    assert train.accum_meta(args) == {"accum_steps": k}       # the .meta entry and the Engine keyword
    line = train.accum_line(args, 8, 10)
    assert line == ("Gradient accumulation: {} batches of 64 per update, {} images per update, {} updates per epoch"
                    .format(k, 64 * k * 8, -(-10 // k)))


@pytest.mark.parametrize("text", ["0", "-2", "2.5", "x", "", "1e1", "nan"])
def test_flag_rejects(text, capsys):
    import train
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--accum_steps", text])
    assert "--accum_steps" in capsys.readouterr().err


def test_engine_keyword_is_validated_before_anything_else():
    """Engine(accum_steps=...) refuses what is no count >= 1 (raised ahead of any device work)."""
    from jr.engine import Engine
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="accum_steps"):
            Engine(4, 107, 107, accum_steps=bad)


# ---- the restatement itself
def test_restatement_order_and_overwrite():
    a, b, c = (accum_ref.special_values(64, s, nans=0) for s in (1, 2, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        want = ((a + b) + c).astype(f32)
    got = accum_ref.closed_gradient([a, b, c])
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]) and np.all(np.isnan(got[~ok]))
    nan = np.full(64, np.nan, f32)
    assert np.array_equal(accum_ref.accumulate(nan, a, True).view(np.uint32), a.view(np.uint32))   # first: a copy
    x = accum_ref.special_values(1025, 7, nans=2)
    assert int(np.isnan(x).sum()) == 2 and np.isinf(x).sum() == 2
    assert np.any((x != 0) & (np.abs(x) < np.finfo(f32).tiny)) and np.any(np.signbit(x) & (x == 0))


# ---- argument validation before any HIP call (no GPU present)
def test_grad_accumulate_validates_without_gpu():
    from jr import _ffi
    L = _ffi.load()
    P, Q = 4096, 1 << 20       # non-null, 16-byte aligned, 1 MiB apart: validation fails before either is used
    for args, what in (((None, Q, 8, 0, None), "bad arguments"), ((P, None, 8, 1, None), "bad arguments"),
                       ((P, Q, 0, 0, None), "bad arguments"), ((P, Q, -4, 1, None), "bad arguments"),
                       ((P, P, 8, 0, None), "overlap"), ((P, P + 16, 8, 0, None), "overlap"),
                       ((P + 28, P, 8, 1, None), "overlap"), ((P, P + 4 * 7, 8, 0, None), "overlap"),
                       ((P + 2, Q, 8, 0, None), "misaligned"), ((P, Q + 1, 8, 0, None), "misaligned")):
        assert L.jr_grad_accumulate(*args) == -1 == _ffi.JR_ERR_INVALID, args
        msg = _ffi.last_error()
        assert msg.startswith("grad_accumulate:") and what in msg, (args, msg)
