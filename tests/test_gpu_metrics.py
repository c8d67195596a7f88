"""jr_metrics_accumulate, jr_metrics_reset and jr_step_log_append on the GPU
against tests/metrics_ref.py, exactly: the counts as integers, the Brier sums
bit for bit (and bit for bit jr_brier_accumulate's), the ring records bit for
bit.  Sizes: one sample, around one wavefront, more than one pass of a block,
one above the LDS chunk; one threshold, the session's 201 and 401, around one
block of thresholds, the most a call takes."""
import ctypes

import numpy as np
import pytest

import metrics_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 0xDEADBEEF
T_ALL = (1, 201, 256, 257, 401, 1024)


@pytest.fixture(scope="module")
def L():
    from jr import _ffi
    _ffi.init(0)
    return _ffi.load()


def check(rc):
    from jr import _ffi
    _ffi.check("call", rc)


def thresholds(T):
    """The edge thresholds first, then 0.5 and the session's grid, then more of the same kind."""
    from lib import metrics as M
    pool = [f32(-1e-7), f32(1 - 1e-7), f32(1 + 1e-7), f32(0.5)] + M.generate_thresholds(200, 1e-7)[1:-1] + \
        M.auc().thresholds + list(np.linspace(0.001, 0.999, 640))
    return np.asarray(pool[:T], f32)


def batch(seed, B, units, thr):
    """Random probabilities with the edge values laid over them; labels 0, 1, 0.5 and -0.0."""
    rng = np.random.default_rng(seed)
    n = B * units
    p = rng.random(n, dtype=f32)
    edges = np.concatenate([thr[rng.permutation(thr.size)[:8]], [0.0, 1.0, np.nan], thr[:3]]).astype(f32)
    where = rng.permutation(n)[:edges.size]
    p[where] = edges[:where.size]
    y = rng.choice(np.array([0.0, 1.0, 0.5, -0.0], f32), n)
    return p.reshape(B, units), y.reshape(B, units)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class State:
    """counts with a sentinel tail, brier with a third double nobody may touch."""

    def __init__(self, T):
        self.T = T
        c = np.full(4 * T + 8, SENTINEL, np.uint32)
        c[:4 * T] = 0
        self.counts = dev(c.view(np.int32))
        self.brier = dev(np.array([0.0, 0.0, -7.0]))
        self.ref_c, self.ref_b = R.metrics_reset_ref(T)

    def read(self):
        torch.cuda.synchronize()
        c = self.counts.cpu().numpy().view(np.uint32)
        b = self.brier.cpu().numpy()
        assert np.all(c[4 * self.T:] == SENTINEL) and b[2] == -7.0
        return c[:4 * self.T].reshape(4, self.T), b[:2]

    def same_as_ref(self):
        c, b = self.read()
        assert np.array_equal(c, self.ref_c)
        assert b.tobytes() == self.ref_b.tobytes(), (b, self.ref_b)


@pytest.mark.parametrize("units", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, R.CHUNK + 1])
def test_accumulate_matches_the_restatement(L, B, units):
    from jr import _ffi
    assert R.CHUNK == _ffi.METRICS_CHUNK
    for T in T_ALL:
        thr = thresholds(T)
        THR = dev(thr)
        st = State(T)
        acc = dev(np.zeros(2))                                   # jr_brier_accumulate on the same data
        for call, which in enumerate((3, 1, 2, 3)):              # counts over three calls, brier over three
            p, y = batch(1000 * call + B + units, B, units, thr)
            P, Y = dev(p), dev(y)
            check(L.jr_metrics_accumulate(P.data_ptr(), Y.data_ptr(), p.size, THR.data_ptr(), T,
                                          st.counts.data_ptr(), st.brier.data_ptr(), which, None))
            before = (st.ref_c.copy(), st.ref_b.copy())
            st.ref_c, st.ref_b = R.metrics_accumulate_ref(st.ref_c, st.ref_b, p, y, thr, which)
            # each `which` touches only its own state
            assert (which & 1) or np.array_equal(st.ref_c, before[0])
            assert (which & 2) or st.ref_b.tobytes() == before[1].tobytes()
            st.same_as_ref()
            if which & 2:
                check(L.jr_brier_accumulate(P.data_ptr(), Y.data_ptr(), p.size, acc.data_ptr(), None))
                torch.cuda.synchronize()
                assert acc.cpu().numpy().tobytes() == st.read()[1].tobytes()
        assert int(st.ref_c.sum()) == 3 * T * B * units
        # the host states read the same integers (lib.metrics._counts flattens the same way)
        from lib import metrics as M
        with np.errstate(invalid="ignore"):
            assert R.counts_ref(p, y, thr).astype(f32).tobytes() == M._counts(y, p, thr).tobytes()


def test_which_without_the_other_state(L):
    """which = 1 takes a NULL brier, which = 2 NULL thresholds and counts."""
    thr = thresholds(5)
    p, y = batch(3, 40, 1, thr)
    P, Y, THR = dev(p), dev(y), dev(thr)
    st = State(5)
    check(L.jr_metrics_accumulate(P.data_ptr(), Y.data_ptr(), 40, THR.data_ptr(), 5, st.counts.data_ptr(), None, 1, None))
    check(L.jr_metrics_accumulate(P.data_ptr(), Y.data_ptr(), 40, None, 5, None, st.brier.data_ptr(), 2, None))
    st.ref_c, st.ref_b = R.metrics_accumulate_ref(st.ref_c, st.ref_b, p, y, thr, 3)
    st.same_as_ref()


def test_reset(L):
    T = 257
    thr = thresholds(T)
    p, y = batch(9, 65, 3, thr)
    P, Y, THR = dev(p), dev(y), dev(thr)
    st = State(T)

    def fill():
        st.ref_c, st.ref_b = R.metrics_reset_ref(T)
        check(L.jr_metrics_reset(st.counts.data_ptr(), T, st.brier.data_ptr(), None))
        check(L.jr_metrics_accumulate(P.data_ptr(), Y.data_ptr(), p.size, THR.data_ptr(), T, st.counts.data_ptr(),
                                      st.brier.data_ptr(), 3, None))
        st.ref_c, st.ref_b = R.metrics_accumulate_ref(st.ref_c, st.ref_b, p, y, thr, 3)
        st.same_as_ref()
        assert st.ref_c.any() and st.ref_b.all()
    fill()
    check(L.jr_metrics_reset(st.counts.data_ptr(), T, None, None))          # counts alone
    st.ref_c[:] = 0
    st.same_as_ref()
    fill()
    check(L.jr_metrics_reset(None, 0, st.brier.data_ptr(), None))           # brier alone
    st.ref_b[:] = 0
    st.same_as_ref()
    fill()
    check(L.jr_metrics_reset(st.counts.data_ptr(), T, st.brier.data_ptr(), None))
    st.ref_c, st.ref_b = R.metrics_reset_ref(T)
    st.same_as_ref()


def _step(scale, norm, skipped, total=0):
    return dev(np.array([(scale, norm, skipped, total)],
                        np.dtype([("scale", "<f4"), ("grad_norm", "<f4"), ("skipped", "<u4"), ("total", "<u4")])
                        ).view(np.uint8))


def _ring(cap):
    """cap records and one more that must stay as it is."""
    r = np.zeros(cap + 1, R.STEP_REC)
    r[cap] = (-1.0, -2.0, -3.0, SENTINEL)
    return dev(r.view(np.uint8))


def test_step_log_wraps_and_flags(L):
    cap = 2
    RING, CUR = _ring(cap), dev(np.zeros(2, np.int32))
    LOSS = dev(np.zeros(4, f32))
    ran, skipped = _step(0.25, 8.0, 0), _step(0.0, np.inf, 1, 4)
    ref, cur = np.zeros(cap, R.STEP_REC), 0
    for loss, S, s in ((0.75, ran, (0.25, 8.0, 0)), (0.5, None, None), (f32(0.3), skipped, (0.0, np.inf, 1))):
        LOSS[0] = float(loss)
        torch.cuda.synchronize()
        check(L.jr_step_log_append(RING.data_ptr(), cap, CUR.data_ptr(), LOSS.data_ptr(),
                                   None if S is None else S.data_ptr(), None))
        cur = R.step_log_append_ref(ref, cur, loss, s)
        torch.cuda.synchronize()
        got = RING.cpu().numpy().view(R.STEP_REC)
        assert got[:cap].tobytes() == ref.tobytes(), (got, ref)
        assert got[cap].tolist() == (-1.0, -2.0, -3.0, SENTINEL)
        assert CUR.cpu().numpy().tolist() == [cur, 0]
    assert cur == 3 and ref["flags"].tolist() == [3, 0] and ref["loss"].tolist() == [f32(0.3), f32(0.5)]


def test_step_log_append_in_a_graph(L):
    """One captured append, launched three times: the cursor (device memory, not a bound scalar) moves by three."""
    cap = 2
    RING, CUR, LOSS = _ring(cap), dev(np.zeros(1, np.int32)), dev(np.array([0.125], f32))
    S = _step(0.5, 3.0, 0)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    check(L.jr_graph_begin(sp))
    check(L.jr_step_log_append(RING.data_ptr(), cap, CUR.data_ptr(), LOSS.data_ptr(), S.data_ptr(), sp))
    ex = ctypes.c_void_p()
    check(L.jr_graph_end(sp, ctypes.byref(ex)))
    try:
        stream.synchronize()
        assert CUR.cpu().numpy().tolist() == [0]            # capturing ran nothing
        ref, cur = np.zeros(cap, R.STEP_REC), 0
        for k in range(3):
            LOSS.fill_(0.125 * (k + 1))
            torch.cuda.synchronize()
            check(L.jr_graph_launch(ex, sp))
            stream.synchronize()
            cur = R.step_log_append_ref(ref, cur, 0.125 * (k + 1), (0.5, 3.0, 0))
        assert CUR.cpu().numpy().tolist() == [3] and cur == 3
        got = RING.cpu().numpy().view(R.STEP_REC)
        assert got[:cap].tobytes() == ref.tobytes() and got[cap]["flags"] == SENTINEL
    finally:
        check(L.jr_graph_destroy(ex))
