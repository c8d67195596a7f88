"""jr_bn_stats, jr_bn_relu_apply and jr_bn_relu_bwd in JR_BF16 against the
fp64 oracle (oracle/tf_ops.py) evaluated on the bf16-rounded inputs: the
bf16 launch forms are otherwise only compared with one another
(test_gpu_apply_multi.py, test_gpu_bn_batch.py, test_bn_relu_bwd_multi_segments),
where an error of the device code they share cancels.  x is read, and y / dx
written, through channel slices of wider buffers, as test_bn_relu_fwd_bwd does
in fp32.

Bars:
  mean, invstd  1e-6 of the largest reference value (the fp32 bar: the sums
                are fp64 over exactly representable inputs);
  y             |got - bf16(ref)| <= 2^-8 |ref| + 2e-5 max(1, max |ref|): one
                bf16 ulp on top of the fp32 bar;
  dx            <= 2^-8 |ref| + 1e-4 max |ref|;
  dbeta         per channel <= 1e-6 sum |dy'| + 1e-5 |ref| (dy' the masked dy:
                the reduce sums batches of 8 rows in fp32, 8 2^-24 < 1e-6);
  bytes outside the slices untouched; the ReLU mask is the kernel's own y > 0.

Measured on an MI355X: mean and invstd within 5.4e-8; y beyond the 2^-8 |ref|
term by at most 8.4e-5 (bar 1e-4 at max |ref| ~ 5: where the kernel's fp32
value and the fp64 one straddle a bf16 tie the two roundings differ by one ulp,
2^-8 .. 2^-7 of |ref|; on these seeded inputs that happens below |ref| = 0.03
only); dbeta within 4.6e-9 of sum |dy'|; dx beyond its ulp term by 2.5e-10.
"""
import numpy as np
import pytest

from oracle import tf_ops as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BF16, F32 = 1, 0
_KEEP = []


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
    return t.double().cpu().numpy()


def bf16(a):
    return torch.as_tensor(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30))


@pytest.mark.parametrize("m,c", [(5, 48), (1, 8),                 # (1, 8): a population of one, variance 0
                                 (2 * 35 * 35, 64), (3 * 17 * 17, 192),
                                 (37, 2048),                      # 256 vectors per row, the maximum
                                 (100003, 80)])                   # the most chunks
def test_bn_relu_fwd_bwd_bf16(m, c):
    ffi = _lib()
    L = ffi.load()
    rng = np.random.default_rng(m + c)
    x = bf16(rng.standard_normal((m, c)) * 3 + rng.standard_normal(c) * 2)
    beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
    dy = bf16(rng.standard_normal((m, c)))
    y_ref, mean_ref, inv_ref = R.bn_relu_fwd(x, beta.astype(np.float64))
    X, BETA = dev(x, torch.bfloat16), dev(beta)
    MEAN, INV = full(c, 0.0), full(c, 0.0)
    wsb = L.jr_bn_workspace_size(m, c)
    ws = full(wsb // 4 + 4, 0.0)
    ffi.check("stats", L.jr_bn_stats(BF16, X.data_ptr(), m, c, 1e-3, MEAN.data_ptr(), INV.data_ptr(), ws.data_ptr(),
                                     wsb, None))
    e_mean, e_inv = relerr(host(MEAN), mean_ref), relerr(host(INV), inv_ref)
    assert e_mean < 1e-6 and e_inv < 1e-6, (e_mean, e_inv)
    if m == 1:
        assert np.all(host(MEAN) == x[0]) and np.all(host(INV) == np.float32(1.0 / np.sqrt(1e-3)))
    # x: channel slice [8, 8 + c) of a wider raw buffer; y: slice [16, 16 + c) of a wider output
    xs, ys = c + 24, c + 32
    XW = np.full((m, xs), 3.0)
    XW[:, 8:8 + c] = x
    XS = dev(XW, torch.bfloat16)
    Y = full(m * ys, 5.0, torch.bfloat16)
    ffi.check("apply", L.jr_bn_relu_apply(BF16, XS.data_ptr(), 8, xs, m, c, MEAN.data_ptr(), INV.data_ptr(),
                                          BETA.data_ptr(), Y.data_ptr(), 16, ys, None))
    yg = host(Y).reshape(m, ys)
    y = yg[:, 16:16 + c]
    assert np.all(yg[:, :16] == 5) and np.all(yg[:, 16 + c:] == 5)
    assert np.isfinite(y).all()
    e_y = np.abs(y - bf16(y_ref)) - 2.0 ** -8 * np.abs(y_ref)
    assert e_y.max() <= 2e-5 * max(1.0, np.abs(y_ref).max()), e_y.max()
    mask = y > 0
    dx_ref, db_ref = R.bn_relu_bwd(dy, x, beta.astype(np.float64), mask=mask)
    dys = c + 8
    DYb = np.full((m, dys), 9.0)
    DYb[:, 8:] = dy
    DX, DB = full(m * xs, 7.0, torch.bfloat16), full(c, 7.0)
    ffi.check("bwd", L.jr_bn_relu_bwd(BF16, dev(DYb, torch.bfloat16).data_ptr(), 8, dys, XS.data_ptr(), 8, xs, m, c,
                                      MEAN.data_ptr(), INV.data_ptr(), BETA.data_ptr(), DX.data_ptr(), DB.data_ptr(),
                                      ws.data_ptr(), wsb, None))
    dxg = host(DX).reshape(m, xs)
    dx, db = dxg[:, 8:8 + c], host(DB)
    assert np.all(dxg[:, :8] == 7) and np.all(dxg[:, 8 + c:] == 7)          # only the slice is written
    assert np.isfinite(dx).all() and np.isfinite(db).all()
    g = np.where(mask, dy, 0.0)
    e_db = np.abs(db - db_ref) - 1e-5 * np.abs(db_ref)
    lim_db = 1e-6 * np.abs(g).sum(0)
    e_dx = np.abs(dx - dx_ref) - 2.0 ** -8 * np.abs(dx_ref)
    print(f"BNBF16 m={m} c={c}: mean {e_mean:.1e} invstd {e_inv:.1e} y excess {max(e_y.max(), 0):.1e} "
          f"dbeta err / sum|dy'| {(np.abs(db - db_ref) / np.maximum(np.abs(g).sum(0), 1e-30)).max():.1e} "
          f"dx excess / max|ref| {max(e_dx.max(), 0) / max(np.abs(dx_ref).max(), 1e-30):.1e}")
    # (scratch perturbation, one row dropped from a batch sum of chunk 0: 1.2e-4 (m = 100003) .. 5.6e-1 (m = 37) of
    # sum |dy'|, against the 1e-6 here; unperturbed at most 4.6e-9)
    assert np.all(e_db <= lim_db), (e_db - lim_db).max()
    assert e_dx.max() <= 1e-4 * np.abs(dx_ref).max(), e_dx.max()


def test_bn_too_many_vectors_per_row_is_unsupported():
    """More than 256 16-byte vectors per row: JR_ERR_UNSUPPORTED from every BN
    entry point, bf16 (c = 2056) and fp32 (c = 1028), before any launch."""
    ffi = _lib()
    L = ffi.load()
    for dt, c, td in ((BF16, 2056, torch.bfloat16), (F32, 1028, torch.float32)):
        m = 2
        X, Y, DY, DX = (full(m * c, 7.0, td) for _ in range(4))
        MEAN, INV, BETA, DB = (full(c, 1.0) for _ in range(4))
        ws = full(1 << 16, 0.0)
        wsb = 4 << 16
        assert L.jr_bn_stats(dt, X.data_ptr(), m, c, 1e-3, MEAN.data_ptr(), INV.data_ptr(), ws.data_ptr(), wsb,
                             None) == ffi.JR_ERR_UNSUPPORTED
        assert L.jr_bn_relu_apply(dt, X.data_ptr(), 0, c, m, c, MEAN.data_ptr(), INV.data_ptr(), BETA.data_ptr(),
                                  Y.data_ptr(), 0, c, None) == ffi.JR_ERR_UNSUPPORTED
        assert L.jr_bn_relu_bwd(dt, DY.data_ptr(), 0, c, X.data_ptr(), 0, c, m, c, MEAN.data_ptr(), INV.data_ptr(),
                                BETA.data_ptr(), DX.data_ptr(), DB.data_ptr(), ws.data_ptr(), wsb,
                                None) == ffi.JR_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((Y == 7).all()) and bool((DX == 7).all()) and bool((MEAN == 1).all()) and bool((DB == 1).all())
