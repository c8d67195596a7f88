"""The guarded BN + ReLU entry points, jr_bn_relu_bwd_frozen_absmax and
jr_absmax_reset at op level, fp32 and bf16 storage.

Guarded forward (jr_bn_relu_apply_guard, _multi_guard, _grouped_guard,
jr_bn_relu_maxpool3x3s2_fwd_guard, _grouped_guard): every stored output (and
argmax) is bitwise the unguarded call's; with limit exactly the largest stored
value jr_device_check is clean, with nextafter(that, 0) it reports
JR_ERR_DEVICE once (one block counted) and is clean afterwards -- with the one
offending element in the first row and channel, in the last row and channel,
in a row owned by a block other than block 0 and, grouped, in the last member
only.  A huge negative pre-activation (ReLU stores 0) sits in every case and
never trips the guard.  The fused pool guards the pooled values it stores: a
raw value in the uncovered last row / column of an even-sized map never trips
it, the same value in a covered position does.

jr_bn_relu_bwd_frozen_absmax: dx bitwise jr_bn_relu_bwd_frozen's, max(words) ==
max |dx| exactly, words started above it stay, floats beside the 64 untouched.
jr_absmax_reset zeroes exactly its range.

Shapes: (m, c) = (5, 16) one partial block; (1031, 48) c / vector = 12 (fp32)
leaves idle threads in every block, several blocks, a partial last one;
(4099, 16) 17 (fp32) / 9 (bf16) blocks; the multi form takes the same row
counts over its 16 + 48 + 64 channels.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_KEEP = []
SHAPES = [(5, 16), (1031, 48), (4099, 16)]
HUGE_NEG = -1e30


def _lib():
    from jr import _ffi
    _ffi.init(0)
    return _ffi, _ffi.load()


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _et(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


def dev(a, dtype=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype=dtype)
    _KEEP.append(t)
    return t


def bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy()
    if t.dtype == torch.uint8:
        return t.numpy()
    return t.numpy().view(np.uint32)


def _clean(ffi):
    torch.cuda.synchronize()
    ffi.device_check()


def _trips_once(ffi):
    """jr_device_check: JR_ERR_DEVICE with one block counted, then clean."""
    torch.cuda.synchronize()
    with pytest.raises(ffi.JRError) as err:
        ffi.device_check()
    assert err.value.status == ffi.JR_ERR_DEVICE
    assert "device check: 1 failure(s)" in str(err.value) and "stream-K" in str(err.value), str(err.value)
    ffi.device_check()


def _below(v):
    return float(np.nextafter(np.float32(v), np.float32(0)))


def _rows_per_block(ffi, dt, m, c):
    """(rows a block of the elementwise pass owns, blocks) from jr_bn_plan."""
    p = ffi.bn_plan(ffi.JR_BF16 if dt == "bf16" else ffi.JR_F32, m, c)
    rows = 256 // (c // p.vec_width) * 4
    assert p.apply_grid == -(-m // rows)
    return rows, p.apply_grid


def _positions(ffi, dt, m, c):
    rows, blocks = _rows_per_block(ffi, dt, m, c)
    pos = [("first", 0, 0), ("last", m - 1, c - 1)]
    if blocks > 1:
        pos.append(("block>0", rows + 1, c // 2))
    return pos, blocks


def _inputs(rng, m, c, hot, neg):
    """x [m, c], mean, invstd, beta with y ~ |N(0, 1)| + beta, one element `hot`
    = (row, channel) near 100 (the unique largest), one `neg` hugely negative."""
    x = (rng.standard_normal((m, c)) * 2).astype(np.float32)
    mean = rng.standard_normal(c).astype(np.float32)
    invstd = (1 / np.sqrt(rng.uniform(0.5, 3, c))).astype(np.float32)
    beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
    x[hot] = mean[hot[1]] + np.float32(100.0) / invstd[hot[1]]
    x[neg] = HUGE_NEG
    return x, mean, invstd, beta


def _neg_pos(m, c, hot):
    neg = (m // 2, 1)
    return neg if neg != hot else (m // 2, 2)


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("m,c", SHAPES)
def test_apply_guard(m, c, dt):
    ffi, L = _lib()
    code, et = (ffi.JR_BF16 if dt == "bf16" else ffi.JR_F32), _et(dt)
    pos, blocks = _positions(ffi, dt, m, c)
    assert (blocks > 1) == (m > 5)
    _clean(ffi)
    for name, r, ch in pos:
        rng = np.random.default_rng(m + c + r)
        neg = _neg_pos(m, c, (r, ch))
        x, mean, invstd, beta = _inputs(rng, m, c, (r, ch), neg)
        xo, xs, yo, ys = 8, c + 16, 16, c + 24                 # slices of wider buffers
        xb = np.full((m, xs), 3.0, np.float32)
        xb[:, xo:xo + c] = x
        X, MEAN, INV, BETA = dev(xb, et), dev(mean), dev(invstd), dev(beta)

        def run(limit):
            Y = dev(np.full((m, ys), -7.0, np.float32), et)
            args = (code, X.data_ptr(), xo, xs, m, c, MEAN.data_ptr(), INV.data_ptr(), BETA.data_ptr(), Y.data_ptr(),
                    yo, ys)
            if limit is None:
                ffi.check("apply", L.jr_bn_relu_apply(*args, None))
            else:
                ffi.check("apply_guard", L.jr_bn_relu_apply_guard(*args, limit, None))
            return Y

        y0 = run(None)
        _clean(ffi)
        top = float(y0.float().max())
        assert float(y0[r, yo + ch]) == top and 90 < top < 110 and float(y0[neg[0], yo + neg[1]]) == 0
        assert int((y0.float() == top).sum()) == 1
        y1 = run(top)
        _clean(ffi)                                            # limit == the largest stored value: clean
        assert np.array_equal(bits(y1), bits(y0)), (name, dt)
        y2 = run(_below(top))
        _trips_once(ffi)
        assert np.array_equal(bits(y2), bits(y0)), (name, dt)
        y3 = run(float(np.float32(top) * 4))
        _clean(ffi)
        assert np.array_equal(bits(y3), bits(y0))


def test_apply_guard_inf_trips_and_error_word_counts_blocks():
    """+inf trips the guard; two offending blocks count two failures."""
    ffi, L = _lib()
    m, c = 1031, 48
    rows, blocks = _rows_per_block(ffi, "f32", m, c)
    rng = np.random.default_rng(3)
    x, mean, invstd, beta = _inputs(rng, m, c, (0, 0), (7, 1))
    x[rows * 2 + 3, 5] = np.inf
    X, MEAN, INV, BETA = dev(x), dev(mean), dev(invstd), dev(beta)
    Y = dev(np.zeros((m, c), np.float32))
    _clean(ffi)
    ffi.check("apply_guard", L.jr_bn_relu_apply_guard(ffi.JR_F32, X.data_ptr(), 0, c, m, c, MEAN.data_ptr(),
                                                      INV.data_ptr(), BETA.data_ptr(), Y.data_ptr(), 0, c, 50.0, None))
    torch.cuda.synchronize()
    with pytest.raises(ffi.JRError) as err:
        ffi.device_check()
    assert err.value.status == ffi.JR_ERR_DEVICE and "device check: 2 failure(s)" in str(err.value)
    assert float(Y[rows * 2 + 3, 5]) == np.inf
    ffi.device_check()


# ------------------------------------------------------------------ multi
MULTI = [16, 48, 64]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("m", [5, 1031, 4099])
def test_apply_multi_guard(m, dt):
    ffi, L = _lib()
    code, et = (ffi.JR_BF16 if dt == "bf16" else ffi.JR_F32), _et(dt)
    c = sum(MULTI)
    pos, blocks = _positions(ffi, dt, m, c)
    _clean(ffi)
    for name, r, ch in pos:
        rng = np.random.default_rng(m + 11 * r)
        neg = _neg_pos(m, c, (r, ch))
        x, mean, invstd, beta = _inputs(rng, m, c, (r, ch), neg)
        X, MEAN, INV = dev(x, et), dev(mean), dev(invstd)

        def run(limit):
            outs, segs, c0 = [], [], 0
            for i, ci in enumerate(MULTI):      # distinct destination strides and offsets
                off, stride = 8 * (i + 1), ci + 8 * (2 * i + 3)
                Y = dev(np.full((m, stride), -7.0, np.float32), et)
                outs.append((Y, off, ci))
                segs.append(ffi.BnApplySeg(Y.data_ptr(), off, stride, ci, dev(beta[c0:c0 + ci]).data_ptr()))
                c0 += ci
            arr = (ffi.BnApplySeg * 3)(*segs)
            args = (code, 3, ctypes.byref(arr), X.data_ptr(), 0, c, m, c, MEAN.data_ptr(), INV.data_ptr())
            if limit is None:
                ffi.check("multi", L.jr_bn_relu_apply_multi(*args, None))
            else:
                ffi.check("multi_guard", L.jr_bn_relu_apply_multi_guard(*args, limit, None))
            torch.cuda.synchronize()
            return outs

        y0 = run(None)
        _clean(ffi)
        top = max(float(Y[:, off:off + ci].float().max()) for Y, off, ci in y0)
        assert 90 < top < 110
        for limit, trips in ((top, False), (_below(top), True)):
            y1 = run(limit)
            _trips_once(ffi) if trips else _clean(ffi)
            for (Y, _, _), (Y0, _, _) in zip(y1, y0):
                assert np.array_equal(bits(Y), bits(Y0)), (name, dt, limit)     # canary channels included


# ------------------------------------------------------------------ grouped
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("m,c", SHAPES)
def test_apply_grouped_guard(m, c, dt):
    ffi, L = _lib()
    code, et = (ffi.JR_BF16 if dt == "bf16" else ffi.JR_F32), _et(dt)
    M = 3
    pos, blocks = _positions(ffi, dt, m, c)
    cases = [(0,) + p for p in pos] + [(M - 1, "last member", m // 3, c - 4)]
    x_ms, y_ms, st_ms, be_ms = m * c + 16, m * c + 32, 2 * c + 4, c + 8      # padded member strides (elements)
    _clean(ffi)
    for member, name, r, ch in cases:
        rng = np.random.default_rng(m + c + r + member)
        xs = np.full(M * x_ms, 3.0, np.float32)
        stats = np.full(M * st_ms, 1.0, np.float32)
        betas = np.zeros(M * be_ms, np.float32)
        for k in range(M):
            hot = (r, ch) if k == member else (0, 0)
            x, mean, invstd, beta = _inputs(rng, m, c, hot, _neg_pos(m, c, hot))
            if k != member:
                x[hot] = mean[0]                    # only `member` holds the offender
            xs[k * x_ms:k * x_ms + m * c] = x.reshape(-1)
            stats[k * st_ms:k * st_ms + c], stats[k * st_ms + c:k * st_ms + 2 * c] = mean, invstd
            betas[k * be_ms:k * be_ms + c] = beta
        X, ST, BE = dev(xs, et), dev(stats), dev(betas)

        def run(limit):
            Y = dev(np.full(M * y_ms, -7.0, np.float32), et)
            args = (code, M, X.data_ptr(), 0, c, x_ms, m, c, ST.data_ptr(), ST.data_ptr() + 4 * c, st_ms, BE.data_ptr(),
                    be_ms, Y.data_ptr(), 0, c, y_ms)
            if limit is None:
                ffi.check("grouped", L.jr_bn_relu_apply_grouped(*args, None))
            else:
                ffi.check("grouped_guard", L.jr_bn_relu_apply_grouped_guard(*args, limit, None))
            return Y

        y0 = run(None)
        _clean(ffi)
        yv = y0.float().cpu().numpy()
        top = float(yv.max())
        assert 90 < top < 110 and yv[member * y_ms + r * c + ch] == top and int((yv == top).sum()) == 1
        y1 = run(top)
        _clean(ffi)
        assert np.array_equal(bits(y1), bits(y0)), (name, dt)
        y2 = run(_below(top))
        _trips_once(ffi)                                       # one error word for all members
        assert np.array_equal(bits(y2), bits(y0)), (name, dt)


# ------------------------------------------------------------------ fused stem pool
def _pool_case(rng, n, h, w, c):
    raw = (rng.standard_normal((n, h, w, c)) * 2).astype(np.float32)
    mean = rng.standard_normal(c).astype(np.float32)
    invstd = (1 / np.sqrt(rng.uniform(0.5, 3, c))).astype(np.float32)
    beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
    return raw, mean, invstd, beta


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fused_pool_guard(dt, grouped):
    ffi, L = _lib()
    code, et = (ffi.JR_BF16 if dt == "bf16" else ffi.JR_F32), _et(dt)
    c, per, M = 8, 2, 2 if grouped else 1
    n = per * M
    _clean(ffi)

    def run(h, raw, stats, betas, limit):
        ho = (h - 3) // 2 + 1
        d = ffi.PoolDesc(n, h, h, c, ho, ho, 0, c, 8, c + 16)
        RAW, ST, BE = dev(raw, et), dev(stats), dev(betas)
        Y = dev(np.full((n, ho, ho, c + 16), -7.0, np.float32), et)
        AM = torch.full((n * ho * ho * c + 8,), 77, dtype=torch.uint8, device="cuda")
        _KEEP.append(AM)
        lim = () if limit is None else (limit,)
        if grouped:
            fn = L.jr_bn_relu_maxpool3x3s2_fwd_grouped if limit is None else L.jr_bn_relu_maxpool3x3s2_fwd_grouped_guard
            rc = fn(ctypes.byref(d), code, per, RAW.data_ptr(), ST.data_ptr(), ST.data_ptr() + 4 * c, 2 * c + 4,
                    BE.data_ptr(), c + 8, Y.data_ptr(), AM.data_ptr(), *lim, None)
        else:
            fn = L.jr_bn_relu_maxpool3x3s2_fwd if limit is None else L.jr_bn_relu_maxpool3x3s2_fwd_guard
            rc = fn(ctypes.byref(d), code, RAW.data_ptr(), ST.data_ptr(), ST.data_ptr() + 4 * c, BE.data_ptr(),
                    Y.data_ptr(), AM.data_ptr(), *lim, None)
        ffi.check("pool", rc)
        torch.cuda.synchronize()
        return Y, AM

    def same(a, b):
        return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))

    for h in (9, 10):
        rng = np.random.default_rng(h + 2 * grouped)
        raw = np.zeros((n, h, h, c), np.float32)
        stats = np.ones(M * (2 * c + 4), np.float32)
        betas = np.zeros(M * (c + 8), np.float32)
        for k in range(M):
            r_, mean, invstd, beta = _pool_case(rng, per, h, h, c)
            raw[k * per:(k + 1) * per] = r_
            stats[k * (2 * c + 4):k * (2 * c + 4) + c] = mean
            stats[k * (2 * c + 4) + c:k * (2 * c + 4) + 2 * c] = invstd
            betas[k * (c + 8):k * (c + 8) + c] = beta
        last = M - 1                                    # the offender's member (grouped: the last only)
        mean_l, inv_l = stats[last * (2 * c + 4) + 3], stats[last * (2 * c + 4) + c + 3]
        big = mean_l + np.float32(100.0) / inv_l        # maps to ~100 + beta
        raw[n - 1, 2, 2, 3] = big                       # a covered tap: the largest pooled value
        raw[0, 4, 4, 1] = HUGE_NEG                      # a huge negative pre-activation: stores 0
        y0 = run(h, raw, stats, betas, None)
        _clean(ffi)
        top = float(y0[0].float().max())
        assert 90 < top < 110
        y1 = run(h, raw, stats, betas, top)
        _clean(ffi)
        assert same(y1, y0), (h, dt)
        y2 = run(h, raw, stats, betas, _below(top))
        _trips_once(ffi)
        assert same(y2, y0), (h, dt)
        if h == 10:
            # rows / columns 9 lie in no window: a raw value there that would map
            # to ~1e6 is never stored, so never trips the guard ...
            far = mean_l + np.float32(1e6) / inv_l
            for at in ((n - 1, 9, 9, 3), (n - 1, 9, 2, 3), (0, 4, 9, 3)):
                raw2 = raw.copy()
                raw2[at] = far if at[0] == n - 1 else stats[3] + np.float32(1e6) / stats[c + 3]
                y3 = run(h, raw2, stats, betas, top)
                _clean(ffi)
                assert same(y3, y0), at
            # ... and the same value in a covered position does
            raw2 = raw.copy()
            raw2[n - 1, 6, 6, 3] = far
            y4 = run(h, raw2, stats, betas, top)
            _trips_once(ffi)
            y5 = run(h, raw2, stats, betas, None)
            _clean(ffi)
            assert same(y4, y5) and float(y5[0].float().max()) > 1e5


# ------------------------------------------------------------------ frozen backward magnitude
def test_bwd_frozen_absmax():
    ffi, L = _lib()
    m, c, split = 1031, 48, [16, 32]
    rng = np.random.default_rng(17)
    x = (rng.standard_normal((m, c)) * 2).astype(np.float32)
    dy = rng.standard_normal((m, c)).astype(np.float32)
    mean = rng.standard_normal(c).astype(np.float32)
    invstd = (1 / np.sqrt(rng.uniform(0.3, 3, c))).astype(np.float32)
    beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
    dy[m - 1, c - 1] = 40.0                              # the largest |dx| in the last row of the last block ...
    x[m - 1, c - 1], beta[c - 1] = mean[c - 1] + 1, 0.25  # ... with its gate open
    X, MEAN, INV = dev(x), dev(mean), dev(invstd)
    segs, c0 = [], 0
    for i, ci in enumerate(split):
        off, stride = 8 * (i + 1), ci + 8 * (i + 3)
        buf = np.full((m, stride), np.nan, np.float32)
        buf[:, off:off + ci] = dy[:, c0:c0 + ci]
        segs.append(ffi.BnSeg(dev(buf).data_ptr(), off, stride, ci, dev(beta[c0:c0 + ci]).data_ptr(), None))
        c0 += ci
    arr = (ffi.BnSeg * len(segs))(*segs)

    def run(words):
        DX = dev(np.full((m, c), -7.0, np.float32))
        args = (ffi.JR_F32, len(segs), ctypes.byref(arr), X.data_ptr(), 0, c, m, c, MEAN.data_ptr(), INV.data_ptr(),
                DX.data_ptr())
        if words is None:
            ffi.check("bwd_frozen", L.jr_bn_relu_bwd_frozen(*args, None))
        else:
            ffi.check("bwd_frozen_absmax", L.jr_bn_relu_bwd_frozen_absmax(*args, words.data_ptr() + 4 * 8, None))
        torch.cuda.synchronize()
        return DX

    dx0 = run(None)
    top = float(dx0.abs().max())
    assert top == abs(float(dx0[m - 1, c - 1])) > 10
    W = dev(np.full(8 + 64 + 8, -7.0, np.float32))
    ffi.check("reset", L.jr_absmax_reset(W.data_ptr() + 4 * 8, 64, None))
    dx1 = run(W)
    w = W.cpu().numpy()
    assert np.array_equal(bits(dx1), bits(dx0))
    assert float(w[8:72].max()) == top and np.all(w[8:72] >= 0)
    assert np.all(w[:8] == -7) and np.all(w[72:] == -7)          # floats beside the 64 words untouched
    run(W)                                                       # a second launch feeding them: still the maximum
    assert np.array_equal(bits(W), bits(torch.from_numpy(w)))
    W2 = dev(np.concatenate([np.full(8, -7.0), np.full(64, 1e9), np.full(8, -7.0)]).astype(np.float32))
    dx2 = run(W2)
    assert np.array_equal(bits(dx2), bits(dx0))
    assert np.all(W2.cpu().numpy()[8:72] == np.float32(1e9))     # words started above max |dx| keep their value
    _clean(ffi)


def test_absmax_reset_zeroes_exactly_its_range():
    ffi, L = _lib()
    T = dev(np.full(300, 3.5, np.float32))
    ffi.check("reset", L.jr_absmax_reset(T.data_ptr() + 4 * 17, 129, None))
    ffi.check("reset", L.jr_absmax_reset(T.data_ptr(), 0, None))
    torch.cuda.synchronize()
    t = T.cpu().numpy()
    assert np.all(t[:17] == 3.5) and np.all(t[17:146] == 0) and np.all(t[146:] == 3.5)
