"""The loop that runs ahead of the host against the synchronous
one, 107^2, batch 8: one seed, the same four batches (one with a colour table,
one with a colour and a warp table), once through Session(device_metrics=True)
-- the staged feed, the step log, the metrics on the device -- and once the way
every batch waits.  Parameters, losses, norms, scales, skip flags and the
threshold counts are the same bits; each Brier value is held against an fp64
sum with the bound its own arithmetic gives."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RES, B, NB = 107, 8, 4
KW = dict(optimizer="rmsprop", weight_decay=4e-5, clip_norm=2.0, device_lr=True, weight_ema=0.5)
f32 = np.float32


def _batches():
    from jr import augment, synth
    rng = np.random.Generator(np.random.PCG64(11))
    out = []
    for i in range(NB):
        x, y = synth.fundus_batch(700 + 10 * i, B, RES), synth.labels(700 + 10 * i, B, p=0.5)
        aug = augment.draw(augment.AugmentSpec(), rng, B) if i in (1, 2) else None
        warp = (augment.draw_warp(augment.WarpSpec(rotate=20.0, zoom=(0.9, 1.1), shift=0.05), rng, B, RES, RES)
                if i == 2 else None)
        out.append((x, y, aug, warp))
    return out


def _engine(**kw):
    from jr.engine import Engine
    return Engine(B, RES, RES, seed=3, tiles="heuristic", **KW, **kw)


def _state(sess):
    return {k: sess.value(k) for k in ("tp", "fp", "fn", "tn", "auc", "brier")}


@pytest.fixture(scope="module")
def runs():
    import lib.evaluation
    from jr.session import Session
    batches = _batches()
    val = [(x, y) for x, y, _, _ in batches]
    # the synchronous way: every batch waits for its loss, its probabilities and its jr_opt_step
    eng = _engine()
    sess = Session(eng)
    a = {"loss": [], "opt": [], "probs": []}
    sess.reset()
    for x, y, aug, warp in batches:
        _, loss, probs = sess.train_batch(x, y, aug, warp)
        a["loss"].append(f32(loss))
        a["opt"].append(eng.opt_step())
        a["probs"].append(probs)
        sess.update(y, probs, "brier")
    a["train_brier"] = sess.value("brier")
    a["params"], a["ema"] = eng.params_numpy(), eng.ema_numpy()
    a["auc_ret"] = lib.evaluation.perform_test(sess, val)
    a["val"] = _state(sess)
    a["val_probs"] = [sess.predict(x, y) for x, y in val]
    eng.close()
    # ahead of the host: nothing is read until the four steps are enqueued
    eng = _engine()
    eng.step_log_enable(NB)
    sess = Session(eng, device_metrics=True)
    b = {}
    sess.metrics_reset()
    b["ret"] = [sess.train_batch(x, y, aug, warp) for x, y, aug, warp in batches]
    b["log"] = eng.step_log_read()
    sess.pull_metrics("brier")
    b["train_brier"] = sess.value("brier")
    b["train_state"] = (sess.metrics["brier"][0].__self__.total, sess.metrics["brier"][0].__self__.count)
    b["params"], b["ema"] = eng.params_numpy(), eng.ema_numpy()
    b["auc_ret"] = lib.evaluation.perform_test(sess, val)
    b["val"] = _state(sess)
    b["val_probs"] = [sess.predict(x, y) for x, y in val]
    b["again"] = len(eng.step_log_read())
    eng.close()
    return batches, a, b


def test_parameters_are_the_same_bits(runs):
    _, a, b = runs
    assert b["ret"] == [(i, None, None) for i in range(NB)]
    assert a["params"].tobytes() == b["params"].tobytes()
    assert a["ema"].tobytes() == b["ema"].tobytes()
    for pa, pb in zip(a["val_probs"], b["val_probs"]):
        assert pa.tobytes() == pb.tobytes()


def test_step_log_is_the_four_steps(runs):
    _, a, b = runs
    log = b["log"]
    assert len(log) == NB and b["again"] == 0               # a read hands every record out once
    assert log["loss"].tobytes() == np.asarray(a["loss"], f32).tobytes()
    norm, scale, skipped, _ = zip(*a["opt"])
    assert log["grad_norm"].tobytes() == np.asarray(norm, f32).tobytes()
    assert log["scale"].tobytes() == np.asarray(scale, f32).tobytes()
    assert (log["flags"] & 1).tolist() == [1] * NB
    assert (log["flags"] >> 1).tolist() == list(skipped) == [0] * NB


def test_counts_and_auc_are_equal(runs):
    _, a, b = runs
    for k in ("tp", "fp", "fn", "tn"):
        assert a["val"][k].dtype == b["val"][k].dtype == np.float32
        assert a["val"][k].tobytes() == b["val"][k].tobytes(), k
    assert a["val"]["tp"].shape == (201,) and a["val"]["tp"][0] + a["val"]["fn"][0] > 0
    assert a["val"]["auc"] == b["val"]["auc"] and a["auc_ret"] == b["auc_ret"] == a["val"]["auc"]


def _ulps(value, ref64):
    return abs(float(value) - ref64) / float(np.spacing(f32(ref64)))


def test_brier_against_an_fp64_sum(runs):
    """Device: f32(S) / f32(n) with S an fp64 sum whose own error is 2^-29 of an fp32 ulp: two conversions
    and one fp32 division, each half an ulp, the first two carried through the division: within 4 ulp.
    Host: every term is an fp32 subtract and a multiply of the rounded difference by itself (3 u), the
    B * NB = 32 terms are added in fp32 (31 u on a sum of non-negative terms), count and division (2 u):
    36 u <= 36 ulp.  Each against the fp64 sum of the same probabilities, not against the other."""
    batches, a, b = runs
    for key, probs in (("train_brier", a["probs"]), ("val", a["val_probs"])):
        d = np.concatenate([p.astype(np.float64).ravel() - y.astype(np.float64).ravel()
                            for p, (_, y, _, _) in zip(probs, batches)])
        ref = float(np.sum(d * d) / d.size)
        dev, host = (b[key], a[key]) if key == "train_brier" else (b[key]["brier"], a[key]["brier"])
        print(f"{key}: fp64 {ref!r} device {dev!r} ({_ulps(dev, ref):.2f} ulp) host {host!r} ({_ulps(host, ref):.2f} ulp)")
        assert _ulps(dev, ref) <= 4.0
        assert _ulps(host, ref) <= 36.0
    total, count = b["train_state"]
    assert total.dtype == np.float32 and count == f32(B * NB)


def test_accumulation_logs_every_micro_batch_and_the_flush():
    """accum_steps = 3 over four batches and the flush: five records, updates on the third and the fifth,
    the flush's loss the last micro-batch's; then a ring that is not read in time refuses the append."""
    from jr.session import Session
    eng = _engine(accum_steps=3)
    eng.step_log_enable(5)
    sess = Session(eng, device_metrics=True)
    steps = [sess.train_batch(x, y, aug, warp)[0] for x, y, aug, warp in _batches()]
    assert steps == [0, 0, 0, 1] and eng.accum_pending() == 1
    assert sess.accum_flush() is True and sess.global_step == 2
    log = eng.step_log_read()
    assert len(log) == 5
    assert (log["flags"] & 1).tolist() == [0, 0, 1, 0, 1]
    assert log["grad_norm"][[0, 1, 3]].tolist() == [0.0] * 3 and log["scale"][[0, 1, 3]].tolist() == [0.0] * 3
    assert np.all(log["grad_norm"][[2, 4]] > 0) and np.all(np.isfinite(log["loss"]))
    assert log["loss"][4].tobytes() == log["loss"][3].tobytes()
    norm, scale, skipped, _ = eng.opt_step()
    assert (f32(norm), f32(scale), skipped) == (log["grad_norm"][4], log["scale"][4], log["flags"][4] >> 1)
    assert sess.accum_flush() is False and len(eng.step_log_read()) == 0      # nothing pending: no record
    eng.step_log_enable(1)
    x, y, _, _ = _batches()[0]
    sess.train_batch(x, y)
    with pytest.raises(RuntimeError, match="step log full"):
        sess.train_batch(x, y)
    eng.close()


@pytest.mark.parametrize("tables", ["none", "augment", "warp", "both"])
def test_staged_and_unstaged_uploads_write_the_same_bytes(tables):
    """Three consecutive uint8 batches of 3 in an engine planned for 4 (both slots, and one refilled), with
    no table, a colour table, a warp table and both: set_batch(..., staged=True) leaves the input buffer and
    the labels bit for bit as set_batch(...) does.  Both start from the same poisoned buffers, and the
    staged three are enqueued back to back and read after one synchronise."""
    from jr import augment, synth
    from jr.engine import Engine
    n = 3
    eng = Engine(4, RES, RES, seed=3, tiles="heuristic", train=False)
    rng = np.random.Generator(np.random.PCG64(5))
    batches = []
    for i in range(3):
        aug = augment.draw(augment.AugmentSpec(), rng, n) if tables in ("augment", "both") else None
        warp = (augment.draw_warp(augment.WarpSpec(rotate=20.0, zoom=(0.9, 1.1), shift=0.05), rng, n, RES, RES)
                if tables in ("warp", "both") else None)
        batches.append((synth.fundus_batch(300 + 10 * i, n, RES), synth.labels(300 + 10 * i, n, p=0.5), aug, warp))
    xbuf = eng.acts[eng.g.input_buf]

    def uploads(staged):
        out = []
        for x, y, aug, warp in batches:
            with torch.cuda.stream(eng.stream):
                xbuf.fill_(-3.0)
                eng.labels.fill_(-3.0)
            assert eng.set_batch(x, y, augment=aug, warp=warp, staged=staged) == n
            with torch.cuda.stream(eng.stream):
                out.append((xbuf.clone(), eng.labels.clone()))
        eng.synchronize()
        return [(a.view(torch.uint8).cpu().numpy(), b.view(torch.uint8).cpu().numpy()) for a, b in out]

    plain, staged = uploads(False), uploads(True)
    for (xa, ya), (xb, yb) in zip(plain, staged):
        assert xa.tobytes() == xb.tobytes()
        assert ya.tobytes() == yb.tobytes()
    assert plain[0][0].tobytes() != plain[1][0].tobytes()       # the batches differ: a stale slot would show
    eng.close()


def test_staged_feed_takes_only_uint8_host_batches():
    """float32 batches and staged=False go the old way and leave the feed unbuilt."""
    from jr.engine import Engine
    eng = Engine(2, RES, RES, seed=3, tiles="heuristic", train=False)
    from jr import synth
    x = synth.fundus_batch(0, 2, RES)
    y = np.array([[1.0], [0.0]], f32)
    eng.set_batch(x.astype(f32) / f32(255), y, staged=True)
    eng.set_batch(x, y)
    assert eng._feed is None
    eng.forward(2)
    want = eng.predictions(2)
    for _ in range(3):          # both slots, and a refill
        eng.set_batch(x, y, staged=True)
        eng.forward(2)
        assert eng.predictions(2).tobytes() == want.tobytes()
    assert eng._feed is not None and all(p.is_pinned() for p in eng._feed.pin)
    eng.close()
