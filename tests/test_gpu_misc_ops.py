"""The small kernels no GPU test called: jr_cast_f32_to_bf16 /
jr_cast_bf16_to_f32 (the data-parallel gradient path, jr/dist.py),
jr_brier_accumulate, jr_gap_fwd / jr_gap_bwd in JR_BF16 and
jr_conv_weights_x8p_multi, through the C-ABI against exact references."""

import numpy as np
import pytest

from oracle import tf_ops as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

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


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
    t = t.to("cuda") if dtype is None else t.to("cuda", dtype=dtype)
    _KEEP.append(t)
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu()


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30))


# fp32 bit patterns: +-0, fp32 subnormals, values that are subnormal in bf16 too, half-way ties (to even: down and
# up), just off the ties, the largest finite fp32 (rounds to inf) and bf16, +-inf, NaNs (one whose payload sits in
# the 16 dropped bits only: truncation or a carry would make it inf)
SPECIAL_BITS = [0x3f818000, 0x7f800001, 0x80000000, 0x00000000, 0x00018000, 0x3f808000, 0x7f7fffff, 0x00000001,
                0x80000001, 0x00012345, 0x007fffff, 0x00008000, 0xbf808000, 0xbf818000, 0x3f808001, 0x3f807fff,
                0x3f817fff, 0x3f818001, 0xff7fffff, 0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, 0x7f800000, 0xff800000,
                0x7fc00000, 0xffc01234, 0x7fffffff]


@pytest.mark.parametrize("n", [1, 7, 1003, 2 ** 20 + 3])
def test_cast_f32_to_bf16_is_round_to_nearest_even(n):
    ffi = _lib()
    L = ffi.load()
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)      # every exponent, NaNs and infs included
    k = min(n, len(SPECIAL_BITS))
    bits[n - k:] = np.array(SPECIAL_BITS[:k], np.uint32)                        # (also at the tail of the last block)
    if n >= 2 * len(SPECIAL_BITS):
        bits[:len(SPECIAL_BITS)] = np.array(SPECIAL_BITS, np.uint32)
    src = torch.as_tensor(bits.view(np.int32)).view(torch.float32)
    want = src.to(torch.bfloat16)
    S = dev(src)
    D = torch.full((n + 1,), -7.0, dtype=torch.bfloat16, device="cuda")
    _KEEP.append(D)
    ffi.check("cast", L.jr_cast_f32_to_bf16(S.data_ptr(), D.data_ptr(), n, None))
    got = host(D)
    assert float(got[n]) == -7.0                                                # the element after n
    nan = torch.isnan(src)
    assert torch.isnan(got[:n][nan]).all() and bool(nan.any()) == (n > 1)       # a NaN stays NaN (n = 1: the tie)
    assert torch.equal(got[:n][~nan].view(torch.int16), want[~nan].view(torch.int16))


@pytest.mark.parametrize("n", [1, 7, 1003, 2 ** 20 + 3])
def test_cast_bf16_to_f32_is_exact(n):
    ffi = _lib()
    L = ffi.load()
    bits = (np.arange(n, dtype=np.int64) * (40503 if n < 65536 else 1)) % 65536   # every bf16 pattern at n > 65536
    special = [0x7f81, 0x8000, 0x0001, 0x807f, 0x7f7f, 0xff80, 0xffc1, 0x7f80, 0xff7f, 0x0000]   # NaNs, infs, subnormals
    bits[n - min(n, len(special)):] = special[:min(n, len(special))]
    src = torch.as_tensor(bits.astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    S = dev(src)
    D = torch.full((n + 1,), -7.0, device="cuda")
    _KEEP.append(D)
    ffi.check("cast", L.jr_cast_bf16_to_f32(S.data_ptr(), D.data_ptr(), n, None))
    got = host(D)
    assert float(got[n]) == -7.0
    want = (torch.as_tensor(bits.astype(np.int64)) << 16).to(torch.int64)
    assert torch.equal(got[:n].view(torch.int32).to(torch.int64) & 0xffffffff, want)     # the exact widening, NaNs too
    assert torch.isnan(got[:n][torch.isnan(src)]).all() and bool(torch.isnan(src).any())


@pytest.mark.parametrize("n", [1, 5, 1000])
def test_brier_accumulate(n):
    ffi = _lib()
    L = ffi.load()
    rng = np.random.default_rng(n)
    p = rng.uniform(0, 1, n).astype(np.float32)
    y = (rng.uniform(0, 1, n) < 0.3).astype(np.float32)
    P, Y = dev(p), dev(y)
    ACC = torch.zeros(3, dtype=torch.float64, device="cuda")
    ACC[2] = -7.0
    _KEEP.append(ACC)
    want = float(((p.astype(np.float64) - y.astype(np.float64)) ** 2).sum())
    for rep in (1, 2):                                   # twice on the same accumulator
        ffi.check("brier", L.jr_brier_accumulate(P.data_ptr(), Y.data_ptr(), n, ACC.data_ptr(), None))
        acc = host(ACC).numpy()
        assert abs(acc[0] - rep * want) <= 1e-12 * rep * want, (acc[0], rep * want)
        assert acc[1] == rep * n and acc[2] == -7.0


@pytest.mark.parametrize("n,hw,c", [(3, 64, 2048), (2, 9, 8)])
def test_gap_bf16(n, hw, c):
    ffi = _lib()
    L = ffi.load()
    rng = np.random.default_rng(n + hw + c)
    X = dev(np.maximum(rng.standard_normal((n, hw, c)), 0).astype(np.float32), torch.bfloat16)
    x = X.double().cpu().numpy()                          # the rounded input
    F = torch.full((n * c + 1,), -7.0, device="cuda")
    _KEEP.append(F)
    ffi.check("gap fwd", L.jr_gap_fwd(ffi.JR_BF16, X.data_ptr(), n, hw, c, F.data_ptr(), None))
    f = host(F).numpy()
    assert f[n * c] == -7.0
    assert relerr(f[:n * c].reshape(n, c), R.global_avg_pool(x.reshape(n, hw, 1, c))) < 1e-6   # the fp32 bar
    dy = rng.standard_normal((n, c)).astype(np.float32)
    DX = torch.full((n * hw * c + 8,), -7.0, dtype=torch.bfloat16, device="cuda")
    _KEEP.append(DX)
    ffi.check("gap bwd", L.jr_gap_bwd(ffi.JR_BF16, dev(dy).data_ptr(), n, hw, c, DX.data_ptr(), None))
    dx = host(DX).double().numpy()
    assert np.all(dx[n * hw * c:] == -7.0)
    ref = np.repeat(dy.astype(np.float64)[:, None, :] / hw, hw, axis=1)
    assert np.all(np.abs(dx[:n * hw * c].reshape(n, hw, c) - ref) <= 2.0 ** -8 * np.abs(ref))


def test_conv_weights_x8p_multi_equals_per_layer():
    """Three layers of different (kh, kw, c_in, c_out), c_in = 3 among them (W^T
    padded to 8 channels), a c_out that is no multiple of 32: both layouts
    bitwise jr_conv_weights_x8p per layer, and h + m + l == the fp32 source."""
    ffi = _lib()
    L = ffi.load()
    layers = [(3, 3, 3, 32), (1, 7, 40, 48), (1, 1, 64, 80)]
    rng = np.random.default_rng(9)
    srcs = [(rng.standard_normal(l) * 10.0 ** rng.integers(-3, 3, l)).astype(np.float32) for l in layers]
    SRC = dev(np.concatenate([s.ravel() for s in srcs]))
    table = (ffi.WPrep * len(layers))()
    so = ho = to = tiles = 0
    offs = []
    for i, (kh, kw, ci, co) in enumerate(layers):
        c8 = (ci + 7) // 8 * 8
        nt = L.jr_conv_weights_bf16_tiles(kh, kw, ci, co)
        assert nt == kh * kw * ((c8 + 31) // 32) * ((co + 31) // 32)
        table[i] = ffi.WPrep(so, ho, to, kh, kw, ci, co, tiles, 0)
        offs.append((so, ho, to))
        so, ho, to, tiles = so + kh * kw * ci * co, ho + 3 * kh * kw * ci * co, to + 3 * co * kh * kw * c8, tiles + nt
    T = dev(np.frombuffer(bytes(table), np.uint8).copy())
    HW = torch.full((ho + 1,), 0x5555, dtype=torch.int16, device="cuda")
    WT = torch.full((to + 1,), 0x5555, dtype=torch.int16, device="cuda")
    _KEEP.extend([HW, WT])
    ffi.check("multi", L.jr_conv_weights_x8p_multi(T.data_ptr(), len(layers), tiles, SRC.data_ptr(), HW.data_ptr(),
                                                   WT.data_ptr(), None))
    hw, wt = host(HW), host(WT)
    assert int(hw[ho]) == 0x5555 and int(wt[to]) == 0x5555
    f64 = lambda t: t.view(torch.bfloat16).double().numpy()  # noqa: E731
    for (kh, kw, ci, co), src, (so, ho_, to_) in zip(layers, srcs, offs):
        c8 = (ci + 7) // 8 * 8
        ne, nw = kh * kw * ci * co, co * kh * kw * c8
        H1 = torch.full((3 * ne,), 0x5555, dtype=torch.int16, device="cuda")
        W1 = torch.full((3 * nw,), 0x5555, dtype=torch.int16, device="cuda")
        _KEEP.extend([H1, W1])
        ffi.check("single", L.jr_conv_weights_x8p(SRC.data_ptr() + 4 * so, kh, kw, ci, co, H1.data_ptr(), W1.data_ptr(),
                                                  None))
        assert torch.equal(hw[ho_:ho_ + 3 * ne], host(H1)) and torch.equal(wt[to_:to_ + 3 * nw], host(W1))
        planes = f64(hw[ho_:ho_ + 3 * ne]).reshape(3, kh, kw, ci, co)
        assert np.array_equal(planes.sum(0), src.astype(np.float64))                     # x = h + m + l exactly
        tp = f64(wt[to_:to_ + 3 * nw]).reshape(3, co, kh, kw, c8).sum(0)
        assert np.array_equal(tp[..., :ci], src.astype(np.float64).transpose(3, 0, 1, 2))
        assert np.all(tp[..., ci:] == 0)
