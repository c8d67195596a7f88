"""The fused stem pool at op level: jr_bn_relu_maxpool3x3s2_fwd (+ _grouped),
jr_bn_relu_bwd_maxpool and jr_bn_relu_bwd_maxpool_absmax through the C-ABI,
fp32 and bf16, against the unfused kernels (bitwise where jr.h claims it) and
the fp64 oracle (oracle/tf_ops.py).

Forward: y and argmax bitwise jr_bn_relu_apply + jr_maxpool3x3s2_fwd; y equals
the oracle's max-pool of the kernel's own apply output exactly, argmax wherever
y > 0; the grouped form (2 members x 1 image, each with its own mean / invstd
/ beta) bitwise the per-member calls.

Backward: the dy it writes is bitwise jr_maxpool3x3s2_bwd(accumulate = 0) and,
in fp32, within 1e-6 of the oracle (the bar of test_maxpool); dx and dbeta
against the unfused jr_bn_relu_bwd fed that dy at the regrouping bars of
test_bn_relu_bwd_multi_segments (1e-6 fp32; bf16 dx one bf16 ulp plus 1e-5 of
the term scale) and, in fp32, against the oracle at the bars of
test_bn_relu_fwd_bwd (dx 1e-4, dbeta 1e-5); bytes outside the slices keep
their fill; the _absmax form is bitwise the plain one and its 64 words hold
max |dx| exactly (bf16: the fp32 value before the store's rounding, so its
bf16 rounding is max |dx| as stored), and words started above it stay.

Shapes: each names its edge (SHAPES).  On an even h (w) the last row (column)
lies in no pooling window: dy == 0 there while dx is not, compared there on
its own.  One channel has a pre-activation <= 0 everywhere: every window of it
is an all-tie (argmax 0), dbeta exactly 0, nothing NaN.
"""
import ctypes

import numpy as np
import pytest

from oracle import tf_ops as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_KEEP = []
EPS = 1e-3

SHAPES = [
    (1, 3, 3, 8),         # ho = wo = 1
    (2, 10, 9, 8),        # even h: the last row uncovered
    (1, 9, 12, 16),       # even w: the last column uncovered
    (1, 12, 14, 48),      # c4 = 12 (block 252), both even
    (2, 7, 7, 192),       # c4 = 48
    (1, 5, 5, 1024),      # c4 = 256, the maximum
]
BIG = (2, 204, 204, 192)  # 998,784 cells > 4096 blocks x 240 threads: the grid cap and the stride loop
BIG12 = (2, 420, 420, 48)  # c4 = 12 through the stride loop: 1,058,400 cells > 4096 blocks x 256 threads


def _lib():
    from jr import _ffi
    _ffi.init(0)
    return _ffi


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def dev(a, dtype=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype=dtype)
    _KEEP.append(t)
    return t


def full(n, v, dtype=torch.float32):
    t = torch.full((n,), v, dtype=dtype, device="cuda")
    _KEEP.append(t)
    return t


def host(t):
    torch.cuda.synchronize()
    return t.double().cpu().numpy() if t.dtype != torch.uint8 else t.cpu().numpy()


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30))


class Stem:
    """Inputs of one case and the UNFUSED forward (jr_bn_stats, jr_bn_relu_apply,
    jr_maxpool3x3s2_fwd).  sliced: x / y at channel offsets 8 / 16 of wider
    buffers, the backward's raw x / dx rows 8 channels wider than c."""

    def __init__(self, shape, dtype, sliced, seed=None):
        ffi = self.ffi = _lib()
        L = self.L = ffi.load()
        n, h, w, c = self.shape = shape
        self.dt = 1 if dtype == "bf16" else 0
        self.td = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.esz = 2 if dtype == "bf16" else 4
        rnd = self.rnd = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(self.td).double().numpy()
        self.xo, self.xs, self.yo, self.ys, self.xr = (8, c + 24, 16, c + 40, c + 8) if sliced else (0, c, 0, c, c)
        ho, wo = self.ho, self.wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        self.m = n * h * w
        rng = np.random.default_rng(sum(shape) + 13 if seed is None else seed)
        self.x = rnd(rng.standard_normal(shape) * 2 + rng.standard_normal(c))       # post-conv-like
        beta = (rng.standard_normal(c) * 0.5).astype(np.float32)                    # ~ half the taps masked
        self.dead = c // 2
        beta[self.dead] = -100.0                                                     # pre-activation <= 0 everywhere
        self.beta = beta
        self.pdy = rnd(rng.standard_normal((n, ho, wo, c)))
        self.BETA = dev(beta)
        self.MEAN, self.INV = full(c, 0.0), full(c, 0.0)
        wsb = L.jr_bn_workspace_size(self.m, c)
        self.bn_ws, self.bn_wsb = full(wsb // 4 + 4, 0.0), wsb
        ffi.check("stats", L.jr_bn_stats(self.dt, dev(self.x, self.td).data_ptr(), self.m, c, EPS,
                                         self.MEAN.data_ptr(), self.INV.data_ptr(), self.bn_ws.data_ptr(), wsb, None))
        # forward raw x in the descriptor's x slice (fill 3 around it)
        buf = np.full((n, h, w, self.xs), 3.0)
        buf[..., self.xo:self.xo + c] = self.x
        self.RAW = dev(buf, self.td)
        self.d = ffi.PoolDesc(n, h, w, c, ho, wo, self.xo, self.xs, self.yo, self.ys)
        self.ACT = full(self.m * self.xs, 3.0, self.td)
        ffi.check("apply", L.jr_bn_relu_apply(self.dt, self.RAW.data_ptr(), self.xo, self.xs, self.m, c,
                                              self.MEAN.data_ptr(), self.INV.data_ptr(), self.BETA.data_ptr(),
                                              self.ACT.data_ptr(), self.xo, self.xs, None))
        self.Y = full(n * ho * wo * self.ys, 5.0, self.td)
        self.AM = full(n * ho * wo * c, 77, torch.uint8)
        ffi.check("mp fwd", L.jr_maxpool3x3s2_fwd(ctypes.byref(self.d), self.dt, self.ACT.data_ptr(), self.Y.data_ptr(),
                                                  self.AM.data_ptr(), None))
        torch.cuda.synchronize()
        self.act = host(self.ACT).reshape(n, h, w, self.xs)[..., self.xo:self.xo + c]


def _forward(shape, dtype, sliced):
    s = Stem(shape, dtype, sliced)
    ffi, L = s.ffi, s.L
    n, h, w, c = shape
    ho, wo = s.ho, s.wo
    Y = full(n * ho * wo * s.ys, 5.0, s.td)
    AM = full(n * ho * wo * c, 77, torch.uint8)
    ffi.check("fused fwd", L.jr_bn_relu_maxpool3x3s2_fwd(ctypes.byref(s.d), s.dt, s.RAW.data_ptr(), s.MEAN.data_ptr(),
                                                         s.INV.data_ptr(), s.BETA.data_ptr(), Y.data_ptr(),
                                                         AM.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(Y, s.Y) and torch.equal(AM, s.AM)                  # the header's claim: bitwise the two calls
    yg = host(Y).reshape(n, ho, wo, s.ys)
    y = yg[..., s.yo:s.yo + c]
    am = host(AM).reshape(n, ho, wo, c)
    assert np.all(yg[..., :s.yo] == 5) and np.all(yg[..., s.yo + c:] == 5)
    y_ref, am_ref = R.maxpool3x3s2(s.act)
    assert np.isfinite(y).all() and np.array_equal(y, y_ref)
    assert np.array_equal(am[y > 0], am_ref[y > 0]) and am.max() <= 8
    assert np.all(y[..., s.dead] == 0) and np.all(am[..., s.dead] == 0)    # the all-tie windows: first tap
    assert 0.15 < np.mean(s.act > 0) < 0.85                                # roughly half the taps masked
    if n != 2:
        return
    # grouped: 2 members x 1 image, member k with its own mean / invstd / beta
    rng = np.random.default_rng(3)
    ST = dev(np.stack([np.concatenate([rng.standard_normal(c) * 0.5, rng.uniform(0.5, 1.5, c)]) for _ in range(2)]))
    BE = dev(rng.standard_normal((2, c)) * 0.5)
    Yg = full(n * ho * wo * s.ys, 5.0, s.td)
    AMg = full(n * ho * wo * c, 77, torch.uint8)
    ffi.check("grouped", L.jr_bn_relu_maxpool3x3s2_fwd_grouped(
        ctypes.byref(s.d), s.dt, 1, s.RAW.data_ptr(), ST.data_ptr(), ST.data_ptr() + 4 * c, 2 * c, BE.data_ptr(), c,
        Yg.data_ptr(), AMg.data_ptr(), None))
    d1 = ffi.PoolDesc(1, h, w, c, ho, wo, s.xo, s.xs, s.yo, s.ys)
    Y1 = full(n * ho * wo * s.ys, 5.0, s.td)
    AM1 = full(n * ho * wo * c, 77, torch.uint8)
    for k in range(2):
        ffi.check("member", L.jr_bn_relu_maxpool3x3s2_fwd(
            ctypes.byref(d1), s.dt, s.RAW.data_ptr() + s.esz * k * h * w * s.xs, ST.data_ptr() + 4 * k * 2 * c,
            ST.data_ptr() + 4 * (k * 2 * c + c), BE.data_ptr() + 4 * k * c, Y1.data_ptr() + s.esz * k * ho * wo * s.ys,
            AM1.data_ptr() + k * ho * wo * c, None))
    torch.cuda.synchronize()
    assert torch.equal(Yg, Y1) and torch.equal(AMg, AM1)


def _backward(shape, dtype, sliced):
    s = Stem(shape, dtype, sliced)
    ffi, L = s.ffi, s.L
    n, h, w, c = shape
    ho, wo, m, f32 = s.ho, s.wo, s.m, dtype == "f32"
    pbuf = np.full((n, ho, wo, s.ys), 9.0)
    pbuf[..., s.yo:s.yo + c] = s.pdy
    PDY = dev(pbuf, s.td)
    xbuf = np.full((n, h, w, s.xr), 3.0)
    xbuf[..., :c] = s.x
    XR = dev(xbuf, s.td)
    wsb = L.jr_bn_relu_bwd_maxpool_workspace_size(ctypes.byref(s.d))
    ws = full(wsb // 4 + 4, 0.0)
    out = {}
    for form in ("plain", "absmax", "absmax_high"):
        DY, DX, DB = full(m * s.xs, 7.0, s.td), full(m * s.xr, 7.0, s.td), full(c, 7.0)
        args = (s.dt, ctypes.byref(s.d), s.AM.data_ptr(), PDY.data_ptr(), DY.data_ptr(), XR.data_ptr(), s.xr,
                s.MEAN.data_ptr(), s.INV.data_ptr(), s.BETA.data_ptr(), DX.data_ptr(), DB.data_ptr(), ws.data_ptr(), wsb)
        if form == "plain":
            WORDS = None
            ffi.check("fused bwd", L.jr_bn_relu_bwd_maxpool(*args, None))
        else:
            WORDS = full(64, 0.0 if form == "absmax" else 2.0 * float(out["plain"][1].float().abs().max()) + 1.0)
            w0 = WORDS.clone()
            ffi.check("fused bwd absmax", L.jr_bn_relu_bwd_maxpool_absmax(*args, WORDS.data_ptr(), None))
        torch.cuda.synchronize()
        out[form] = (DY, DX, DB, WORDS)
        if form != "plain":
            assert all(torch.equal(a, b) for a, b in zip(out[form][:3], out["plain"][:3]))
        if form == "absmax":
            top = WORDS.max()
            if not f32:        # the words hold the fp32 value before the bf16 store (docstring)
                top = top.to(torch.bfloat16).float()
            assert float(top) == float(DX.view(m, s.xr)[:, :c].float().abs().max()) > 0
        if form == "absmax_high":
            assert torch.equal(WORDS, w0)
    DY, DX, DB, _ = out["plain"]
    # the unfused pair fed the same pooled gradient
    DY2, DX2, DB2 = full(m * s.xs, 7.0, s.td), full(m * s.xr, 7.0, s.td), full(c, 7.0)
    ffi.check("mp bwd", L.jr_maxpool3x3s2_bwd(ctypes.byref(s.d), s.dt, s.AM.data_ptr(), PDY.data_ptr(), DY2.data_ptr(),
                                              0, None))
    ffi.check("bn bwd", L.jr_bn_relu_bwd(s.dt, DY2.data_ptr(), s.xo, s.xs, XR.data_ptr(), 0, s.xr, m, c,
                                         s.MEAN.data_ptr(), s.INV.data_ptr(), s.BETA.data_ptr(), DX2.data_ptr(),
                                         DB2.data_ptr(), s.bn_ws.data_ptr(), s.bn_wsb, None))
    torch.cuda.synchronize()
    assert torch.equal(DY, DY2)                                            # dy: bitwise the max-pool backward
    dyg = host(DY).reshape(n, h, w, s.xs)
    dy = dyg[..., s.xo:s.xo + c]
    assert np.all(dyg[..., :s.xo] == 7) and np.all(dyg[..., s.xo + c:] == 7)      # outside the x_c_off slice
    dxg = host(DX).reshape(n, h, w, s.xr)
    dx, dx2 = dxg[..., :c], host(DX2).reshape(n, h, w, s.xr)[..., :c]
    assert np.all(dxg[..., c:] == 7)                                              # outside the c channels
    db, db2 = host(DB), host(DB2)
    assert np.isfinite(dx).all() and np.isfinite(db).all() and np.isfinite(dy).all()
    assert db[s.dead] == 0.0                                                      # the all-masked channel
    am = host(s.AM).reshape(n, ho, wo, c)
    dy_ref = R.maxpool3x3s2_bwd(s.pdy, am, shape)
    # uncovered last row / column: no gradient arrives, but dx = invstd (-k1 - xhat k2) is not 0
    edges = ([np.s_[:, h - 1]] if h % 2 == 0 else []) + ([np.s_[:, :, w - 1]] if w % 2 == 0 else [])
    for e in edges:
        assert np.all(dy[e] == 0)
    mean, inv = host(s.MEAN), host(s.INV)
    mask = s.act > 0
    dx_ref, db_ref = R.bn_relu_bwd(dy_ref, s.x, s.beta.astype(np.float64), mask=mask)
    print(f"STEMPOOL {shape} {dtype}: fused vs unfused dx {relerr(dx, dx2):.1e} dbeta {relerr(db, db2):.1e}; vs oracle "
          f"dx {relerr(dx, dx_ref):.1e} dbeta {relerr(db, db_ref):.1e} uncovered dx "
          f"{max([relerr(dx[e], dx_ref[e]) for e in edges], default=0.0):.1e}")
    assert relerr(db, db2) <= 1e-6
    if f32:
        assert np.allclose(dy, dy_ref, rtol=1e-6, atol=1e-6)
        assert relerr(dx, dx2) <= 1e-6
        assert relerr(db, db_ref) < 1e-5, relerr(db, db_ref)
        assert relerr(dx, dx_ref) < 1e-4, relerr(dx, dx_ref)
        # (scratch perturbation, the uncovered row's dx left unwritten: 1.0 of the row's max |dx|, 6.4e-2 of the
        # tensor's, at (2, 10, 9, 8); unperturbed 1.2e-7)
        for e in edges:
            assert np.abs(dx_ref[e]).max() > 0
            assert relerr(dx[e], dx_ref[e]) < 1e-4, relerr(dx[e], dx_ref[e])
    else:
        assert np.all(np.abs(dy - dy_ref) <= 2.0 ** -8 * np.abs(dy_ref))      # fp32 sums of <= 4 terms, rounded once
        xh = (s.x - mean) * inv
        g = np.where(mask, dy, 0.0)
        scale = inv * (np.abs(g) + np.abs(g).mean((0, 1, 2)) + np.abs(xh) * np.abs(g * xh).mean((0, 1, 2)))
        assert np.all(np.abs(dx - dx2) <= np.abs(dx2) * 2.0 ** -7 + 1e-5 * scale)
        for e in edges:
            assert np.abs(dx[e]).max() > 0


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_forward(shape, dtype, sliced):
    _forward(shape, dtype, sliced)


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_backward(shape, dtype, sliced):
    _backward(shape, dtype, sliced)


@pytest.mark.parametrize("shape", [BIG, BIG12], ids=["c4_48", "c4_12"])
def test_fused_backward_grid_cap_and_stride_loop(shape):
    """More cells than the capped grid of 4096 blocks holds threads: the
    grid-stride loop runs (the bench workload's regime), fp32, once per c4.
    A thread keeps its channel quad q across strides only because the block
    (240 / 252 threads), and so the stride, is a multiple of c4: the small
    c4 = 12 shape above (504 cells, 2 blocks) never strides and cannot see a
    stale q, so c4 = 12 runs here too, with more cells than 4096 x 256.
    (Scratch perturbation, blocks of 256 threads whatever c4: the c4 = 12 case
    fails at the bitwise dy -- cells of the second stride written for the wrong
    channel quad; the c4 = 48 shape, fixed at 998,784 cells, then fits 4096 x
    256 threads without a stride and cannot see it.)"""
    _backward(shape, "f32", False)


def test_refusals_before_any_launch():
    ffi = _lib()
    L = ffi.load()

    def call(dt, n, h, w, c, ho=None, wo=None, short=0, alloc_hw=None):
        ah, aw = alloc_hw or (h, w)
        td = torch.bfloat16 if dt else torch.float32
        aho, awo = (ah - 3) // 2 + 1, (aw - 3) // 2 + 1
        d = ffi.PoolDesc(n, h, w, c, aho if ho is None else ho, awo if wo is None else wo, 0, c, 0, c)
        m = n * ah * aw
        bufs = [full(m * c, 7.0, td) for _ in range(3)]          # dy, x, dx
        PDY, AM = full(n * aho * awo * c, 1.0, td), full(n * aho * awo * c, 0, torch.uint8)
        st = [full(c, 1.0) for _ in range(4)]                    # mean, invstd, beta, dbeta
        wsb = L.jr_bn_relu_bwd_maxpool_workspace_size(ctypes.byref(d))
        ws = full(wsb // 4 + 4, 0.0)
        rc = L.jr_bn_relu_bwd_maxpool(dt, ctypes.byref(d), AM.data_ptr(), PDY.data_ptr(), bufs[0].data_ptr(),
                                      bufs[1].data_ptr(), c, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                      bufs[2].data_ptr(), st[3].data_ptr(), ws.data_ptr(), wsb - short, None)
        torch.cuda.synchronize()
        assert all(bool((b == 7).all()) for b in bufs) and bool((st[3] == 1).all())     # nothing ran
        return rc

    assert call(0, 1, 5, 5, 1028) == ffi.JR_ERR_UNSUPPORTED
    assert call(1, 1, 5, 5, 12) == ffi.JR_ERR_INVALID
    assert call(0, 1, 2, 5, 8, alloc_hw=(3, 5)) == ffi.JR_ERR_INVALID
    assert call(0, 1, 7, 7, 8, ho=2) == ffi.JR_ERR_INVALID
    assert call(0, 1, 7, 7, 8, short=1) == ffi.JR_ERR_WORKSPACE
