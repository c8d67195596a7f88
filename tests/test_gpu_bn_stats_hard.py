"""BN statistics on hard channels, through every path that computes them.

The inputs come from bn_hard_gen.py (checked on the CPU by
test_bn_stats_hard_gen.py): every aligned group of 4 output channels holds a
channel with mean 0 / spread 1, one with |mean| = 256 x spread, one exactly
constant (what a dead ReLU input gives in training) and one exactly zero.

Bars, as test_gpu_fused.py: the statistics are compared with the fp64
statistics of y AS THE KERNEL STORED IT; invstd within 1e-5 relative (biased
variance, eps 1e-3), mean within 1e-5 of THAT CHANNEL's max |y|; an all-zero
channel gives mean == 0 and invstd == float32(1 / sqrt(eps)) exactly; nothing
is NaN or inf.  The ratio 256 keeps those bars derivable: a partial mean over
R <= 128 rows summed in fp32 is off by at most R 2^-24 |mean| = 2e-3 of the
spread, squared into M2 that is 4e-6 of the variance, the fp32 sum of R
squares adds R 2^-24 ~ 8e-6, so invstd stays within 1e-5.  y itself is held
to the conv bars of test_gpu_fused.py (1e-5, bf16 8e-3, of max |ref|).

Paths (selected with jr_conv2d_set_config, dropped again with -1, confirmed
through jr_conv2d_get_config / jr_conv2d_bn_partials_layout): the GEMM
epilogue's two-pass (mean, M2); the split-K reduce at forced factors 3 and 5;
one stream-K grid per dtype that has them (JR_F32 has no stream-K ids); a
ragged M whose last partial holds fewer than R rows; the conv1 geometry
(c_in 3, 3x3 stride 2 'valid', c_out 32; the opt-in direct kernel is run in a
child process with JR_CONV1_DIRECT=1); the grouped launch of 2 members
(bitwise the single calls); the finalize folded into the BN apply (bitwise
jr_conv2d_fwd_bn_stats); jr_bn_stats on the stored y; and the three finalize
tiers (P <= 512 k_stats_finalize8, P <= 4096 one k_stats_finalize block,
above that two stages), with P, R and single_stage asserted so that a planner
change cannot silently move a case into another tier.

JR_F32_X8P is left out: test_x8p_bitwise_equals_x8 ties it to JR_F32_X8.

Measured on an MI355X (largest invstd error in units of 1e-6, f32 / x8 / x6h /
bf16; the bar is 10; always on a |mean| = 256 x spread channel where > 0.3):
  epilogue        P 8    R 64   1.7  / 1.6  / 1.7  / 0.05
  split 3, 5      P 52   R 10   1.7  / 2.7  / 2.2  / 1.6
  stream-K        P 8    R 64   -    / 2.4  / 2.2  / 0.05
  ragged          P 4    R 64   2.4  / 2.7  / 1.8  / 0.26
  ragged split 3  P 20   R 10   2.7  / 2.3  / 3.0  / 2.0
  conv1 (GEMM)    P 22   R 32   0.78 / 0.90 / 0.72 / 0.04   (bf16: P 24)
  grouped         P 16   R 32   1.2  / 1.7  / 1.8  / 0.04
  fold            P 16, 52      1.5  / 2.1  / 1.8  / 1.5
  jr_bn_stats                   0.03 on every dtype
  tier 1          P 512  R 32   0.23 / 0.26 / 0.18 / 0.03   k_stats_finalize8
  tier 2          P 516  R 32   0.16 / 0.16 / 0.18 / 0.03   one k_stats_finalize block
  tier 3          P 4608 R 32   0.11 / 0.12 / 0.04 / 0.05   two stages
and the largest mean error 1.3e-7 of the channel's max |y| (bar 1e-5).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tf_ops as R

import bn_hard_gen as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32, BF16, X8, X6H = 0, 1, 2, 4
DT = {"f32": F32, "f32x8": X8, "f32x6h": X6H, "bf16": BF16}
SK = {"f32x8": 28 + 3, "f32x6h": 28 + 3, "bf16": 33 + 3}     # test_gpu_streamk.py: SK0 / BF_SK0, tile 3 (128 x 64)
EPS = 1e-3
DIRECT = os.environ.get("JR_CONV1_DIRECT") == "1"
_KEEP = []

BASE = (2, 18, 18, 32, 96, 3, 3, 1, "valid")       # M = 512: whole partials for every tile
RAGGED = (1, 15, 17, 32, 96, 3, 3, 1, "valid")    # M = 195 = 3 * 64 + 3 = 19 * 10 + 5
CONV1 = (2, 37, 37, 3, 32, 3, 3, 2, "valid")       # M = 648


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


def zeros(n, dtype=torch.float32):
    t = torch.zeros(n, dtype=dtype, device="cuda")
    _KEEP.append(t)
    return t


class Operands:
    """One conv of the hard generator bound for `dtype`: the descriptor, the
    device operands, the fp64 oracle output on the operands as the kernel sees
    them, and a workspace with room for forced split factors up to 5."""

    def __init__(self, ffi, L, case, dtype, seed):
        n, h, w, cin, cout, kh, kw, s, pad = case
        self.case, self.dtype, self.dt = case, dtype, DT[dtype]
        self.f32 = dtype != "bf16"
        self.tdt = torch.float32 if self.f32 else torch.bfloat16
        q = 4 if self.f32 else 8
        x, wt, self.cls = G.hard_case(*case, seed=seed)
        cq = (cin + q - 1) // q * q
        xp = np.zeros((n, h, w, cq), np.float32)
        xp[..., :cin] = x
        self.X = dev(xp, self.tdt)
        xr = self.X.double().cpu().numpy()[..., :cin]
        W32 = dev(wt)
        if self.f32:
            self.W, wr = W32, wt.astype(np.float64)
        else:
            self.W = zeros(cout * kh * kw * cq, torch.bfloat16)
            ffi.check("wprep", L.jr_conv_weights_bf16(W32.data_ptr(), kh, kw, cin, cout, None, self.W.data_ptr(), None))
            wr = torch.as_tensor(wt).to(torch.bfloat16).double().numpy()
        ph, pw = ((kh - 1) // 2, (kw - 1) // 2) if pad == "same" else (0, 0)
        ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
        self.d = ffi.ConvDesc(n, h, w, cin, cout, kh, kw, s, s, ph, pw, ho, wo, 0, cq, 0, cout)
        if dtype == "f32x6h":      # as test_gpu_x6h.py: a host bound for x, device magnitude words for w
            self.wm = zeros(64)
            self.wm[5] = float(np.abs(wt).max())
            self.wm[12] = float(np.abs(wt).max()) / 3
            self.d.x_bound = float(x.max()) * 1.5
            self.d.w_absmax = self.wm.data_ptr()
        self.M, self.cout, self.cq = n * ho * wo, cout, cq
        self.ref = R.conv2d(xr, wr, s, pad).reshape(self.M, cout)
        self.wsb = L.jr_conv2d_workspace_size(ctypes.byref(self.d), 0, self.dt) + 5 * self.M * cout * 4 + (1 << 20)
        self.ws = zeros(self.wsb // 4 + 4)

    def layout(self, ffi, L):
        lay = ffi.BnPartials()
        ffi.check("layout", L.jr_conv2d_bn_partials_layout(ctypes.byref(self.d), self.dt, ctypes.byref(lay)))
        assert lay.M == self.M and lay.N == self.cout and lay.P * lay.R >= self.M
        return lay

    def fwd_bn_stats(self, ffi, L):
        Y, MEAN, INV = zeros(self.M * self.cout, self.tdt), zeros(self.cout), zeros(self.cout)
        ffi.check("fwd_bn_stats", L.jr_conv2d_fwd_bn_stats(
            ctypes.byref(self.d), self.dt, self.X.data_ptr(), self.W.data_ptr(), Y.data_ptr(), EPS, MEAN.data_ptr(),
            INV.data_ptr(), self.ws.data_ptr(), self.wsb, None))
        torch.cuda.synchronize()
        return Y, MEAN, INV


def check_stats(tag, y, got_mu, got_inv, cls):
    """The file's bars on (mean, invstd) against the fp64 statistics of the
    stored y [M][c]; returns (max invstd rel. error, max mean error / channel max |y|)."""
    got_mu, got_inv = got_mu.astype(np.float64), got_inv.astype(np.float64)
    assert np.isfinite(got_mu).all() and np.isfinite(got_inv).all(), tag
    mu = y.mean(0)
    var = ((y - mu) ** 2).mean(0)
    inv = 1.0 / np.sqrt(var + EPS)
    ymax = np.abs(y).max(0)
    e_inv = np.abs(got_inv / inv - 1)
    e_mu = np.abs(got_mu - mu) / np.maximum(ymax, 1e-30)
    print(f"BNHARD {tag}: invstd err {e_inv.max():.2e} (class {cls[e_inv.argmax()]}), "
          f"mean err / max|y| {e_mu[ymax > 0].max():.2e}")
    zero = ymax == 0
    assert zero[cls == G.D].all()
    assert np.all(got_mu[zero] == 0.0), (tag, got_mu[zero])
    # (eps reaches the kernels as a float)
    assert np.all(got_inv[zero] == np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))), (tag, got_inv[zero])
    assert np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS)))) == np.float32(1.0 / np.sqrt(EPS))
    # (scratch perturbations of the combine: one partial's M2 zeroed -> invstd off by 1.5e-3 (P = 512) .. 2.9e-1
    # (P = 4); the last partial counted as R rows -> invstd 2.4e-2 .. 9.8e-1 and mean 7e-3 .. 1.2e-1 of max |y| on
    # every path whose last partial is short; unperturbed at most 3.1e-6 and 1.4e-7)
    assert np.all(np.abs(got_mu - mu) <= 1e-5 * ymax), (tag, e_mu.max(), cls[e_mu.argmax()])
    assert e_inv.max() <= 1e-5, (tag, e_inv.max(), cls[e_inv.argmax()])
    return e_inv.max(), e_mu.max()


def check_y(tag, op, Y):
    y = Y.double().cpu().numpy().reshape(op.M, op.cout)
    assert np.isfinite(y).all(), tag
    scale = np.abs(op.ref).max()
    tol = 1e-5 if op.f32 else 8e-3
    assert np.abs(y - op.ref).max() <= tol * scale, (tag, np.abs(y - op.ref).max() / scale)
    const = (op.cls == G.C) | (op.cls == G.D)
    assert np.array_equal(y[:, const], op.ref[:, const]), tag      # exact whatever the operand split
    return y


def run_path(ffi, L, op, cfg, tag):
    """One jr_conv2d_fwd_bn_stats under config `cfg` (None: the planner's),
    checked; returns the layout the plan reported."""
    ref = ctypes.byref(op.d)
    if cfg is not None:
        ffi.check("set", L.jr_conv2d_set_config(ref, 0, op.dt, 0, cfg))
    try:
        if cfg is not None:
            assert L.jr_conv2d_get_config(ref, 0, op.dt, 0) == cfg
        lay = op.layout(ffi, L)
        Y, MEAN, INV = op.fwd_bn_stats(ffi, L)
        ffi.device_check()
    finally:
        if cfg is not None:
            ffi.check("reset", L.jr_conv2d_set_config(ref, 0, op.dt, 0, -1))
    y = check_y(tag, op, Y)
    check_stats(f"{tag} {op.dtype} P={lay.P} R={lay.R}", y, MEAN.cpu().numpy(), INV.cpu().numpy(), op.cls)
    return lay, Y, MEAN, INV


def _splitk_geom(M, N):
    """stats_geom of a split-K plan (jr_conv_plan.cpp): the reduce's rows per partial."""
    rpp = 256 // (min(N, 1024) // 4)
    r = max(rpp, -(-M // 512))
    r = -(-r // rpp) * rpp
    return -(-M // r), r


PATHS = ["epilogue", "split3", "split5", "streamk", "ragged", "ragged_split3", "conv1"]


# (JR_F32 has no stream-K ids: jr_conv2d_num_configs(JR_F32) == 14, asserted below)
@pytest.mark.parametrize("path,dtype", [(p, dt) for p in PATHS for dt in DT if p != "streamk" or dt in SK],
                         ids=lambda v: v)
def test_hard_channels_every_path(path, dtype):
    ffi = _lib()
    L = ffi.load()
    case = {"ragged": RAGGED, "ragged_split3": RAGGED, "conv1": CONV1}.get(path, BASE)
    cfg = {"epilogue": 0 | (1 << 8), "split3": 0 | (3 << 8), "split5": 0 | (5 << 8), "streamk": SK.get(dtype),
           "ragged": 0 | (1 << 8), "ragged_split3": 0 | (3 << 8), "conv1": None}[path]
    op = Operands(ffi, L, case, dtype, seed=11)
    lay, Y, MEAN, INV = run_path(ffi, L, op, cfg, path)
    if path in ("epilogue", "ragged"):
        tile_r = 64                                            # tile 0 of either table: BM 128 / 2 waves along M
        assert (lay.P, lay.R) == (-(-op.M // 128) * 2, tile_r)
    if path in ("split3", "split5", "ragged_split3"):
        assert (lay.P, lay.R) == _splitk_geom(op.M, op.cout)
    if path.startswith("ragged"):
        assert op.M % lay.R != 0 and (lay.P - 1) * lay.R < op.M     # the last partial is short, not empty
    if path == "streamk":
        assert L.jr_conv2d_num_configs(F32) == 14 and L.jr_conv2d_num_configs(op.dt) > SK[dtype]
    if path == "epilogue":
        # jr_bn_stats (fp64 sum and sum of squares) on the same stored y, fp32 and bf16
        adt = F32 if op.f32 else BF16
        wsb = L.jr_bn_workspace_size(op.M, op.cout)
        ws, M2, I2 = zeros(wsb // 4 + 4), zeros(op.cout), zeros(op.cout)
        ffi.check("bn_stats", L.jr_bn_stats(adt, Y.data_ptr(), op.M, op.cout, EPS, M2.data_ptr(), I2.data_ptr(),
                                            ws.data_ptr(), wsb, None))
        torch.cuda.synchronize()
        y = Y.double().cpu().numpy().reshape(op.M, op.cout)
        check_stats(f"jr_bn_stats {dtype}", y, M2.cpu().numpy(), I2.cpu().numpy(), op.cls)


@pytest.mark.skipif(DIRECT, reason="the child run itself")
def test_conv1_direct_kernel_on_hard_channels():
    """The opt-in direct conv1 kernel (fp32 Chan combine of 1,024-row
    partials) on the same inputs: the knob is read once per process, so the
    conv1 cases of this module run again in a child with JR_CONV1_DIRECT=1."""
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", here, "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        "-k", "conv1-f32"], cwd=os.path.dirname(os.path.dirname(here)), capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, JR_CONV1_DIRECT="1"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "3 passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]     # f32, f32x8, f32x6h


@pytest.mark.parametrize("dtype", list(DT))
def test_hard_channels_grouped_members_bitwise(dtype):
    ffi = _lib()
    L = ffi.load()
    ops = [Operands(ffi, L, BASE, dtype, seed=21 + k) for k in range(2)]
    o = ops[0]
    esz = 4 if o.f32 else 2
    X = torch.cat([p.X.reshape(-1) for p in ops])
    W = torch.cat([p.W.reshape(-1) for p in ops])
    xm, wm, ym = ops[0].X.numel(), ops[0].W.numel(), o.M * o.cout
    _KEEP.extend([X, W])
    d = o.d
    if dtype == "f32x6h":               # member i's magnitude words at w_absmax + 64 i floats
        words = torch.cat([p.wm for p in ops])
        _KEEP.append(words)
        d.w_absmax = words.data_ptr()
        d.x_bound = max(p.d.x_bound for p in ops)
        for p in ops:
            p.d.x_bound = d.x_bound
    wsb = L.jr_conv2d_workspace_size_grouped(ctypes.byref(d), o.dt, 2)
    ws = zeros(wsb // 4 + 64)
    Yg, Sg = zeros(2 * ym, o.tdt), zeros(2 * 2 * o.cout)
    ffi.check("grouped", L.jr_conv2d_fwd_bn_stats_grouped(
        ctypes.byref(d), o.dt, 2, X.data_ptr(), xm, W.data_ptr(), wm, Yg.data_ptr(), ym, EPS, Sg.data_ptr(),
        Sg.data_ptr() + 4 * o.cout, 2 * o.cout, ws.data_ptr(), wsb, None))
    torch.cuda.synchronize()
    assert esz * xm % 16 == 0 and esz * wm % 16 == 0
    for k, p in enumerate(ops):
        Y, MEAN, INV = p.fwd_bn_stats(ffi, L)
        assert torch.equal(Yg[k * ym:(k + 1) * ym], Y), k
        sg = Sg[k * 2 * o.cout:(k + 1) * 2 * o.cout]
        assert torch.equal(sg[:o.cout], MEAN) and torch.equal(sg[o.cout:], INV), k
        y = check_y(f"grouped member {k}", p, Y)
        check_stats(f"grouped {dtype} member {k}", y, sg[:o.cout].cpu().numpy(), sg[o.cout:].cpu().numpy(), p.cls)


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("cfg", [None, 0 | (3 << 8)], ids=["planner", "split3"])
def test_hard_channels_fold_is_bitwise(cfg, dtype):
    """jr_conv2d_fwd_bn_partials + jr_bn_relu_apply_stats: mean and invstd
    bitwise those of jr_conv2d_fwd_bn_stats on the same tensors."""
    ffi = _lib()
    L = ffi.load()
    op = Operands(ffi, L, BASE, dtype, seed=31)
    ref = ctypes.byref(op.d)
    adt = F32 if op.f32 else BF16
    if cfg is not None:
        ffi.check("set", L.jr_conv2d_set_config(ref, 0, op.dt, 0, cfg))
    try:
        lay = op.layout(ffi, L)
        assert lay.single_stage == 1
        Y0, MEAN0, INV0 = op.fwd_bn_stats(ffi, L)
        Y1, MEAN1, INV1 = zeros(op.M * op.cout, op.tdt), zeros(op.cout), zeros(op.cout)
        beta = dev(np.linspace(-0.5, 0.5, op.cout).astype(np.float32))
        ACT = zeros(op.M * op.cout, op.tdt)
        ffi.check("partials", L.jr_conv2d_fwd_bn_partials(ref, op.dt, op.X.data_ptr(), op.W.data_ptr(), Y1.data_ptr(),
                                                          op.ws.data_ptr(), op.wsb, None))
        ffi.check("apply_stats", L.jr_bn_relu_apply_stats(
            adt, Y1.data_ptr(), 0, op.cout, op.M, op.cout, op.ws.data_ptr() + lay.ws_offset, lay.P, lay.R, op.cout, 0,
            EPS, MEAN1.data_ptr(), INV1.data_ptr(), beta.data_ptr(), ACT.data_ptr(), 0, op.cout, None))
        torch.cuda.synchronize()
    finally:
        if cfg is not None:
            ffi.check("reset", L.jr_conv2d_set_config(ref, 0, op.dt, 0, -1))
    assert torch.equal(Y0, Y1) and torch.equal(MEAN0, MEAN1) and torch.equal(INV0, INV1)
    y = check_y("fold", op, Y1)
    check_stats(f"fold {dtype} P={lay.P} R={lay.R}", y, MEAN1.cpu().numpy(), INV1.cpu().numpy(), op.cls)
    # the activation it applied: BN + ReLU of the stored y with those statistics
    act = ACT.double().cpu().numpy().reshape(op.M, op.cout)
    want = np.maximum((y - MEAN1.double().cpu().numpy()) * INV1.double().cpu().numpy() + beta.double().cpu().numpy(), 0)
    assert np.isfinite(act).all()
    assert np.all(np.abs(act - want) <= (2.0 ** -8 if not op.f32 else 0) * np.abs(want) + 2e-5 * max(1.0, want.max()))


# The three finalize tiers: a 1x1 conv, c_out 16, tile 7 of either table (BM 64,
# 2 waves along M: R = 32, P = 2 ceil(M / 64)), no split.  (n, h, w) -> (P, tier)
TIERS = [((1, 128, 128), 512, 1), ((1, 128, 129), 516, 2), ((4, 192, 192), 4608, 3)]


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("nhw,P,tier", TIERS, ids=["tier1", "tier2", "tier3"])
def test_hard_channels_finalize_tiers(nhw, P, tier, dtype):
    ffi = _lib()
    L = ffi.load()
    n, h, w = nhw
    op = Operands(ffi, L, (n, h, w, 4 if dtype != "bf16" else 8, 16, 1, 1, 1, "same"), dtype, seed=41)
    lay, Y, MEAN, INV = run_path(ffi, L, op, 7 | (1 << 8), f"tier{tier}")
    assert (lay.P, lay.R, lay.single_stage) == (P, 32, 1 if tier == 1 else 0)
    assert (lay.P <= 512, 512 < lay.P <= 4096, lay.P > 4096) == (tier == 1, tier == 2, tier == 3)
    ref = ctypes.byref(op.d)
    ffi.check("set", L.jr_conv2d_set_config(ref, 0, op.dt, 0, 7 | (1 << 8)))
    try:
        rc = L.jr_conv2d_fwd_bn_partials(ref, op.dt, op.X.data_ptr(), op.W.data_ptr(), Y.data_ptr(), op.ws.data_ptr(),
                                         op.wsb, None)
        torch.cuda.synchronize()
    finally:
        ffi.check("reset", L.jr_conv2d_set_config(ref, 0, op.dt, 0, -1))
    assert rc == (ffi.JR_OK if tier == 1 else ffi.JR_ERR_UNSUPPORTED)
