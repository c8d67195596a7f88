"""tests/metrics_ref.py (the numpy restatement of jr_metrics_accumulate and
jr_step_log_append) against the host states it has to agree with:
lib.metrics._counts and the `auc` state, bit for bit as float32 integers; and
its Brier sum against a plain fp64 sum."""
import numpy as np
import pytest

import metrics_ref as R
from lib import metrics as M

f32 = np.float32


def session_thresholds():
    """The 401 thresholds of a Session(device_metrics=True): its own 201, then the auc state's 200."""
    own = M.generate_thresholds(200, 1e-7) + [0.5]
    return own, M.auc().thresholds


def edge_set(thr):
    """Probabilities on and around the fp32 thresholds, 0, 1 and NaN; labels 0, 1, 0.5 and -0.0."""
    t32 = np.asarray(thr, f32)
    pick = t32[[0, 1, 57, 100, len(t32) - 2, len(t32) - 1]]
    p = np.concatenate([pick, np.nextafter(pick, f32(2)), np.nextafter(pick, f32(-2)),
                        np.array([0.0, 1.0, np.nan, f32(-1e-7), f32(1 - 1e-7), f32(1 + 1e-7)], f32)]).astype(f32)
    y = np.resize(np.array([0.0, 1.0, 0.5, -0.0], f32), p.size)
    return p, y


@pytest.mark.parametrize("units", [1, 3])
def test_counts_match_the_host_states_on_random_probabilities(units):
    rng = np.random.default_rng(5 + units)
    own, auc_thr = session_thresholds()
    p = rng.random((37, units), dtype=f32)
    y = (rng.random((37, units)) < 0.4).astype(f32)
    got = R.counts_ref(p, y, own + auc_thr)
    assert got.dtype == np.uint32 and got.shape == (4, 401)
    assert got[:, :201].astype(f32).tobytes() == M._counts(y, p, own).tobytes()
    state = M.auc()
    state.update(y, p)
    assert got[:, 201:].astype(f32).tobytes() == state.acc.tobytes()
    assert np.all(got.sum(axis=0) == p.size)


def test_counts_match_the_host_states_on_the_edge_set():
    own, auc_thr = session_thresholds()
    thr = own + auc_thr
    p, y = edge_set(thr)
    got = R.counts_ref(p, y, thr)
    with np.errstate(invalid="ignore"):
        want = M._counts(y, p, thr)
    assert got.astype(f32).tobytes() == want.tobytes()
    # a probability equal to a threshold's float32 value is not positive there; NaN never is
    t = 57
    one = R.counts_ref(np.asarray(thr, f32)[t:t + 1], [1.0], thr)
    assert one[0, t] == 0 and one[2, t] == 1 and one[0, t - 1] == 1
    nan = R.counts_ref([np.nan], [1.0], thr)
    assert nan[0].sum() == 0 and np.all(nan[2] == 1)
    # labels: 0.5 is true, -0.0 is false
    lab = R.counts_ref([0.9, 0.9], [0.5, -0.0], [0.5])
    assert lab[:, 0].tolist() == [1, 1, 0, 0]


def test_accumulate_which_and_reset():
    rng = np.random.default_rng(0)
    thr = [0.25, 0.5]
    c, b = R.metrics_reset_ref(2)
    p, y = rng.random(300, dtype=f32), (rng.random(300) < 0.5).astype(f32)
    c1, b1 = R.metrics_accumulate_ref(c, b, p, y, thr, which=1)
    assert c1.sum() == 600 and b1.tolist() == [0.0, 0.0]
    c2, b2 = R.metrics_accumulate_ref(c, b, p, y, thr, which=2)
    assert c2.sum() == 0 and b2[1] == 300.0
    c3, b3 = R.metrics_accumulate_ref(c1, b2, p, y, thr, which=3)
    assert np.array_equal(c3, 2 * c1) and b3[1] == 600.0
    # the fixed-order fp64 sum is a correct sum: within n ulp(fp64) of the exactly rounded one
    d = p.astype(np.float64) - y.astype(np.float64)
    exact = float(np.sum(np.asarray(d * d, np.longdouble)))
    assert abs(b2[0] - exact) <= 300 * 2.0 ** -53 * exact


def test_step_log_ring_wraps():
    ring = np.zeros(2, R.STEP_REC)
    cur = 0
    cur = R.step_log_append_ref(ring, cur, 0.7, (0.5, 4.0, 0))
    cur = R.step_log_append_ref(ring, cur, 0.6, None)
    cur = R.step_log_append_ref(ring, cur, 0.5, (0.0, np.inf, 1))
    assert cur == 3
    assert ring[0].tolist() == (f32(0.5), np.inf, 0.0, 3) and ring[1].tolist() == (f32(0.6), 0.0, 0.0, 0)
