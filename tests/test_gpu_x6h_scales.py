"""JR_F32_X6H operand scales and fp16 subnormals, held to a bit-exact model.

What makes JR_F32_X6H differ from JR_F32_X8 is one mechanism: each operand is
multiplied by a power of two taken from a stated magnitude (pow2_scale over
the descriptor's *_absmax words or *_bound) and truncated into three fp16
terms whose low ones live in fp16's subnormal range (SplitFrag16).  That split
is deterministic, so x6h_model.py restates it bit for bit in numpy, and the
kernel is held to the model per output element:

    |got - model| <= (6 K + 8) 2^-23 S,   S = sum |a| |b| over the reduction

(products of two fp16 terms are exact in fp32; any order of fp32 additions of
the 6 K products errs by at most one unit per addition, the unit taken as 2^-23
to allow a truncating accumulator; + 8 for the pieces of a split or stream-K
reduction, a forced split-K factor added on top; the scale-back is exact).
Where the model gives 0 the kernel must give exactly 0, and nothing may be NaN
or inf.  test_x6h_model.py shows on the CPU, for the same generated inputs,
that a kernel that lost its fp16 subnormals (every ladder, mixed and grouped
case), or used a scale off by a factor of two (every ladder), would be at
least 4 bars away on at least a tenth of the outputs.

Cases:
  * ladders: 1x1 GEMMs with K = 16 whose rows and columns step down from twice
    the stated magnitude to 2^-40 of it, all three ops, each operand's
    magnitude given as device words (max in lane 0 / 31 / 63 among smaller
    junk, the host bound then set to nonsense), as a host bound, or as bound 0;
    magnitudes 4096, 2048 (the engine's), 1 (the image), powers of two and the
    fp32 below one, 2^-100 against 2^100; planner, forced split-K and stream-K
    configs;
  * 21 magnitudes inside one dot product (3x3 'same' and stride-2 'valid',
    fwd / dgrad / wgrad, every config), the A operand under a bound of 4096;
  * the engine's bounds (x_bound 4096, 2048; 1.0 on k / 255 images) on four
    geometries of test_gpu_x6h.py, at its fp32 bars and the model bar;
  * an all-zero operand (zero words, or zeros under a bound): exactly 0;
  * jr_conv2d_fwd_bn_stats_grouped over three members 2^10 / 2^-7 apart with
    both operands' words at + 64 i: bitwise the single calls, and in the bar.

The scale-back acc / s_a / s_b is two multiplies by powers of two.  It stays
exact even where acc / s_a is an fp32 subnormal (s_a = 2^100, the clamp, for a
2^-100 operand against one of 2^100): acc is a multiple of 2^-48, the grid of
products of two fp16 terms, so acc 2^-100 is a multiple of 2^-148 -- the clamp
at 2^100 is what keeps it on fp32's subnormal grid.  Ladders 7 to 9 run there.

Measured on an MI355X, the largest |got - model| / bar over each family
(fwd / dgrad / wgrad; the bar is 1):
  ladders, planner's config        0.163 / 0.153 / 0.153
  ladders, tile 3 forced split-K 3 0.032 / 0.036 / 0.030
  ladders, stream-K id 28 + 3      0.033 / 0.037 / 0.031
  mixed, planner                   0.0006 / 0.0048 / 0.0145
  mixed, tile 3 forced split-K 3   0.0003 / 0.0042 / 0.0141
  mixed, stream-K id 28 + 3        0.0003 / 0.0062 / 0.0145
  engine's bounds, plain data      0.0084 / -      / 0.0029
  grouped members                  0.0007
so per op 0.163 / 0.153 / 0.153 of the bar at the worst; on the plain data the
error against fp64 is 2.3e-7 to 2.6e-7 (fwd, bar 5e-6) and 2.4e-7 to 5.9e-7
(wgrad, bar 1e-5) of max |ref| under every x_bound.  Every zero of the model
was an exact zero.
"""
import ctypes
import functools

import numpy as np
import pytest

import x6h_model as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

X6H, SK0 = 4, 28                                    # test_gpu_streamk.py: stream-K grid of x8 tile id - 28
CFGS = {"planner": None, "tile3-splitk3": 3 | (3 << 8), "sk3": SK0 + 3}
OPNUM = {"fwd": 0, "dgrad": 1, "wgrad": 2}
AB = {"fwd": ("x", "w"), "dgrad": ("dy", "w"), "wgrad": ("x", "dy")}
_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _lib():
    from jr import _ffi
    _ffi.init(0)
    return _ffi


def dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a)).to("cuda")
    _KEEP.append(t)
    return t


def _words(v, lane, seed=0):
    """64 magnitude words whose max v sits in `lane`, smaller junk elsewhere."""
    rng = np.random.default_rng(seed)
    w = (np.float64(v) * rng.uniform(0.01, 0.45, 64)).astype(np.float32)
    w[lane] = np.float32(v)
    assert w.argmax() == lane or v == 0
    return w


def _desc(ffi, geom):
    n, h, w, cin, cout, kh, kw, s, pad = geom
    ph, pw, ho, wo = X.geometry(geom)
    cs = (cin + 3) // 4 * 4
    return ffi.ConvDesc(n, h, w, cin, cout, kh, kw, s, s, ph, pw, ho, wo, 0, cs, 0, cout), cs


def _state(d, key, kind, v, seed=0):
    """States operand `key`'s (x / w / dy) magnitude v in the descriptor:
    "w<lane>" = device words (and a nonsense host bound, which must be
    ignored), "bnd" = the host bound, "zero" = bound 0."""
    if kind.startswith("w"):
        setattr(d, key + "_absmax", dev(_words(v, int(kind[1:]), seed)).data_ptr())
        setattr(d, key + "_bound", 3e30)
    elif kind == "bnd":
        setattr(d, key + "_bound", v)
    else:
        assert kind == "zero" and v == 0.0


def _set(ffi, L, d, op, stride, cfg):
    for ph in range(stride * stride if op == "dgrad" else 1):
        ffi.check("set", L.jr_conv2d_set_config(ctypes.byref(d), OPNUM[op], X6H, ph, cfg))


def _run(ffi, L, d, cs, op, geom, tensors, cfg=None):
    """The op on the GPU under config `cfg` (None: the planner's), as a numpy
    array in the oracle's shape; the output buffer starts as 7.0."""
    n, h, w, cin, cout, kh, kw, s, pad = geom
    _, _, ho, wo = X.geometry(geom)
    x, wt, dy = tensors
    if x is not None and cs != cin:
        xp = np.zeros((n, h, w, cs), np.float32)
        xp[..., :cin] = x
        x = xp
    shape = {"fwd": (n, ho, wo, cout), "dgrad": (n, h, w, cs), "wgrad": (kh, kw, cin, cout)}[op]
    out = torch.full((int(np.prod(shape)),), 7.0, device="cuda")
    wsb = L.jr_conv2d_workspace_size(ctypes.byref(d), OPNUM[op], X6H) + 3 * 4 * out.numel()
    ws = torch.zeros(wsb // 4 + 4, device="cuda")
    if cfg is not None:
        _set(ffi, L, d, op, s, cfg)
    try:
        if op == "fwd":
            ffi.check("fwd", L.jr_conv2d_fwd(ctypes.byref(d), X6H, dev(x).data_ptr(), dev(wt).data_ptr(),
                                             out.data_ptr(), ws.data_ptr(), wsb, None))
        elif op == "dgrad":
            ffi.check("dgrad", L.jr_conv2d_bwd_data(ctypes.byref(d), X6H, dev(dy).data_ptr(), dev(wt).data_ptr(),
                                                    out.data_ptr(), 0, ws.data_ptr(), wsb, None))
        else:
            ffi.check("wgrad", L.jr_conv2d_bwd_filter(ctypes.byref(d), X6H, dev(x).data_ptr(), dev(dy).data_ptr(),
                                                      out.data_ptr(), ws.data_ptr(), wsb, None))
        torch.cuda.synchronize()
    finally:
        if cfg is not None:
            _set(ffi, L, d, op, s, -1)
    return out.cpu().numpy().astype(np.float64).reshape(shape)[..., :cin if op == "dgrad" else None]


def _splits(cfg):
    return (cfg >> 8) if cfg is not None and (cfg & 0xFF) < SK0 else 1


def _hold(tag, op, got, model, S, K, splits=1):
    """got against the model at the bar; prints the largest error in bars."""
    assert np.all(np.isfinite(got)), tag
    bar = X.bar(K, S, splits) * np.ones_like(S)
    err = np.abs(got - model)
    pos = bar > 0
    worst = float(np.max(err[pos] / bar[pos])) if pos.any() else 0.0
    print(f"X6H-MARGIN {op} {worst:.4f} {tag}")
    assert np.all(got[model == 0] == 0), tag          # (covers S == 0)
    assert np.all(err <= bar), (tag, worst)


@functools.lru_cache(maxsize=None)
def _model(case_id):
    case = {c.id: c for c in X.ladder_cases() + X.mixed_cases() + X.grouped_cases() + X.ordinary_cases()}[case_id]
    tensors, stated = case.make()
    sa, sb = X.scales(case.op, stated)
    return case, tensors, stated, X.conv(case.op, case.geom, *tensors, sa, sb)


# ------------------------------------------------------------------ ladders
LADDERS = [(op, i, "planner") for op in X.OPS for i in range(len(X.LADDER_MAGS))] + \
          [(op, i, c) for op in X.OPS for i in (0, 1, 7) for c in ("tile3-splitk3", "sk3")]


@pytest.mark.parametrize("op,i,cfg", LADDERS, ids=lambda v: str(v))
def test_ladder(op, i, cfg):
    ffi = _lib()
    L = ffi.load()
    case, tensors, stated, (model, exact, S, K) = _model(f"ladder-{op}-{i}")
    ka, va, kb, vb = X.LADDER_MAGS[i]
    d, cs = _desc(ffi, case.geom)
    _state(d, AB[op][0], ka, va, 2 * i)
    _state(d, AB[op][1], kb, vb, 2 * i + 1)
    got = _run(ffi, L, d, cs, op, case.geom, tensors, CFGS[cfg])
    assert np.allclose(S, exact, rtol=1e-12, atol=0)    # all operands positive: S is the reference
    assert (model != 0).mean() > 0.5 and (model == 0).any()
    _hold(f"ladder-{i}-{cfg}", op, got, model, S, K, _splits(CFGS[cfg]))
    ffi.device_check()


# ------------------------------------------- 21 magnitudes in one dot product
@pytest.mark.parametrize("cfg", list(CFGS))
@pytest.mark.parametrize("op", X.OPS)
@pytest.mark.parametrize("geom", X.MIXED_GEOM, ids=lambda g: f"s{g[7]}{g[8]}")
def test_mixed_magnitudes_in_one_dot_product(geom, op, cfg):
    ffi = _lib()
    L = ffi.load()
    case, tensors, stated, (model, exact, S, K) = _model(f"mixed-{op}-{geom[7]}{geom[8]}")
    d, cs = _desc(ffi, geom)
    a, b = AB[op]
    _state(d, a, "bnd", stated[a])                      # x_bound / dy_bound = 4096
    _state(d, b, "bnd" if op == "dgrad" else "w5", stated[b], 3)     # w_bound once, words otherwise
    got = _run(ffi, L, d, cs, op, geom, tensors, CFGS[cfg])
    _hold(f"mixed-s{geom[7]}-{cfg}", op, got, model, S, K, _splits(CFGS[cfg]))
    ffi.device_check()


# -------------------------------------------- the engine's bounds, plain data
def _relerr(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30))


@pytest.mark.parametrize("case,xb", [(c, b) for c, bs in X.ORDINARY for b in bs],
                         ids=lambda v: f"{v[1]}x{v[3]}k{v[5]}x{v[6]}" if isinstance(v, tuple) else f"xb{v:g}")
def test_engine_bounds_on_ordinary_data(case, xb):
    ffi = _lib()
    L = ffi.load()
    for op, lim in (("fwd", 5e-6), ("wgrad", 1e-5)):    # test_gpu_x6h.py's fp32 bars
        _, tensors, stated, (model, exact, S, K) = _model(
            f"ordinary-{op}-{case[1]}x{case[3]}k{case[5]}x{case[6]}-xb{xb:g}")
        d, cs = _desc(ffi, case)
        _state(d, "x", "bnd", xb)
        assert float(np.abs(tensors[0]).max()) <= 2 * xb
        _state(d, "w", "w5", stated["w"], 1)
        _state(d, "dy", "w5", stated["dy"], 2)
        got = _run(ffi, L, d, cs, op, case, tensors)
        rel = _relerr(got, exact)
        print(f"X6H-FP32BAR {op} {rel:.3e} of {lim:g} {case} xb {xb:g}")
        assert rel < lim
        _hold(f"ordinary-{case[1]}x{case[3]}-xb{xb:g}", op, got, model, S, K)
    ffi.device_check()


# ----------------------------------------------------------- all-zero operand
@pytest.mark.parametrize("how", ["zero-words", "zeros-under-a-bound"])
@pytest.mark.parametrize("side", [0, 1], ids=["A", "B"])
@pytest.mark.parametrize("op", X.OPS)
def test_all_zero_operand_gives_exact_zero(op, side, how):
    ffi = _lib()
    L = ffi.load()
    geom = X.MIXED_GEOM[1] if op == "dgrad" else X.MIXED_GEOM[0]
    tensors, stated = X.mixed_case(op, geom, 7)
    zkey, okey = AB[op][side], AB[op][1 - side]
    tensors = tuple(None if t is None else (np.zeros_like(t) if k == zkey else t)
                    for k, t in zip(("x", "w", "dy"), tensors))
    d, cs = _desc(ffi, geom)
    _state(d, okey, "w9", float(np.abs(tensors[("x", "w", "dy").index(okey)]).max()), 4)
    if how == "zero-words":
        setattr(d, zkey + "_absmax", dev(np.zeros(64, np.float32)).data_ptr())
        setattr(d, zkey + "_bound", 3e30)
    else:
        _state(d, zkey, "bnd", 4096.0)
    got = _run(ffi, L, d, cs, op, geom, tensors)
    assert got.shape[-1] > 0 and np.all(got == 0)       # (the buffer started as 7.0)
    ffi.device_check()


# ------------------------------------------------------------ grouped launch
def test_grouped_members_use_their_own_words():
    """Three members, x 2^10 and w 2^-7 apart in the order middle, large,
    small, both operands' words at + 64 i: each member's y, mean and invstd
    are bitwise the single call's with its own words, y within the bar."""
    ffi = _lib()
    L = ffi.load()
    geom = X.GROUPED_GEOM
    n, h, w, cin, cout, kh, kw, s, pad = geom
    members = X.grouped_case()
    M = len(members)
    xm, wm, ym = n * h * w * cin, kh * kw * cin * cout, n * h * w * cout
    Xs = dev(np.concatenate([m[0].ravel() for m in members]))
    Ws = dev(np.concatenate([m[1].ravel() for m in members]))
    lanes = (63, 0, 31)
    xw = dev(np.concatenate([_words(m[2]["x"], lanes[i], 10 + i) for i, m in enumerate(members)]))
    ww = dev(np.concatenate([_words(m[2]["w"], lanes[-1 - i], 20 + i) for i, m in enumerate(members)]))
    d, cs = _desc(ffi, geom)
    d.x_absmax, d.w_absmax, d.x_bound, d.w_bound = xw.data_ptr(), ww.data_ptr(), 3e30, 3e30
    wsb = L.jr_conv2d_workspace_size_grouped(ctypes.byref(d), X6H, M)
    ws = torch.zeros(wsb // 4 + 4, device="cuda")
    Yg, Sg = torch.full((M * ym,), 7.0, device="cuda"), torch.zeros(M * 2 * cout, device="cuda")
    ffi.check("grouped", L.jr_conv2d_fwd_bn_stats_grouped(
        ctypes.byref(d), X6H, M, Xs.data_ptr(), xm, Ws.data_ptr(), wm, Yg.data_ptr(), ym, 1e-3, Sg.data_ptr(),
        Sg.data_ptr() + 4 * cout, 2 * cout, ws.data_ptr(), wsb, None))
    torch.cuda.synchronize()
    ws1 = L.jr_conv2d_workspace_size(ctypes.byref(d), 0, X6H)
    w1 = torch.zeros(ws1 // 4 + 4, device="cuda")
    for i in range(M):
        d1, _ = _desc(ffi, geom)
        d1.x_absmax, d1.w_absmax = xw.data_ptr() + 4 * 64 * i, ww.data_ptr() + 4 * 64 * i
        Y, St = torch.full((ym,), 7.0, device="cuda"), torch.zeros(2 * cout, device="cuda")
        ffi.check("single", L.jr_conv2d_fwd_bn_stats(
            ctypes.byref(d1), X6H, Xs.data_ptr() + 4 * i * xm, Ws.data_ptr() + 4 * i * wm, Y.data_ptr(), 1e-3,
            St.data_ptr(), St.data_ptr() + 4 * cout, w1.data_ptr(), ws1, None))
        torch.cuda.synchronize()
        assert torch.equal(Yg[i * ym:(i + 1) * ym], Y), i
        assert torch.equal(Sg[i * 2 * cout:(i + 1) * 2 * cout], St), i
        case, _, _, (model, exact, S, K) = _model(f"grouped-member{i}")
        got = Yg[i * ym:(i + 1) * ym].cpu().numpy().astype(np.float64).reshape(model.shape)
        _hold(f"grouped-member{i}", "fwd", got, model, S, K)
        assert np.all(np.isfinite(St.cpu().numpy()))
    ffi.device_check()
