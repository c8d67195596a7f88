"""Per-image input gradients under frozen BN on the GPU: the new kernels
bitwise against the float32 restatements of tests/attribution_ref.py, the
whole chain (107^2, B = 4) against the masked-linear fp64 model within the
project's 3x envelope of an independent fp32 (bf16-emulating) evaluation of
the same model, and what Engine.input_gradient / jr.attribution.attribute
promise: fused == unfused pools and one == two lanes bitwise, per-image
independence, nothing else moved, the integrated-gradients driver bitwise its
host-driven restatement, the refusals.

Whole chain, measured on an MI355X (relative L2 error per image against the
fp64 masked-linear model; the envelope is the fp32 / bf16-emulating model's;
DESIGN.md section 9):
  x8    gpu 1.14e-6 .. 1.62e-6   fp32 masked-linear 9.03e-7 .. 9.90e-7
  f32   gpu 9.41e-7 .. 1.07e-6   fp32 masked-linear 9.19e-7 .. 9.79e-7
  bf16  gpu 1.52e-2 .. 1.66e-2   bf16-storage masked-linear 1.58e-2 .. 1.77e-2
"""
import ctypes
import functools

import numpy as np
import pytest

import attribution_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RES, B = 107, 4
CONFIGS = {"x8": dict(dtype="f32", conv_math="x8"), "f32": dict(dtype="f32", conv_math="f32"),
           "bf16": dict(dtype="bf16"), "x6h": dict(dtype="f32", conv_math="x6h")}
_KEEP = []


def _lib():
    from jr import _ffi
    _ffi.init(0)
    return _ffi, _ffi.load()


def dev(a, dtype=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()
    _KEEP.append(t)
    return t


def bits(t):
    """The bit patterns of a device / host tensor or array (fp32 -> uint32, bf16 -> uint16)."""
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t, np.float32).view(np.uint32)
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy().view(np.uint32)


def ref_bits(a, bf16):
    return R.bf16_bits(a) if bf16 else np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. frozen BN backward
def _split(c, bf16, multi):
    if not multi:
        return [c]
    return {16: [8, 8] if bf16 else [4, 4, 8], 48: [16, 8, 24], 448: [64, 192, 192]}[c]


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [16, 48, 448])
@pytest.mark.parametrize("m", [1, 255, 257, 4099])
def test_frozen_bn_backward_is_bitwise_the_restatement(m, c, dt, multi):
    ffi, L = _lib()
    bf = dt == "bf16"
    code, et = (ffi.JR_BF16, torch.bfloat16) if bf else (ffi.JR_F32, torch.float32)
    rng = np.random.default_rng(m * 1000 + c + 7 * multi)
    q = lambda a: R.to_bf16(a) if bf else np.asarray(a, np.float32)   # noqa: E731  (values as stored)
    x = q(rng.standard_normal((m, c)) * 2)
    dy = q(rng.standard_normal((m, c)))
    mean = q(rng.standard_normal(c))                   # (storable: x == mean is reachable)
    invstd = (1 / np.sqrt(rng.uniform(0.3, 3, c))).astype(np.float32)
    beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
    # row 0: pre == 0 under a NaN dy (gate closed); pre the smallest positive
    # subnormal (gate open); an inf dy under a closed gate
    beta[:3] = 0
    x[0, 0], dy[0, 0] = mean[0], np.nan
    mean[1], invstd[1], x[0, 1], dy[0, 1] = 0, 2.0 ** -126, 2.0 ** -23, 1.5
    x[0, 2], dy[0, 2] = mean[2] - 1, np.inf
    pre = R.bn_pre_ref(x, mean, invstd, beta)
    assert pre[0, 0] == 0 and pre[0, 1] == np.float32(2.0 ** -149) and pre[0, 2] < 0
    want = R.bn_relu_bwd_frozen_ref(x, dy, mean, invstd, beta, bf16=bf)
    assert want[0, 0] == 0 and want[0, 2] == 0 and want[0, 1] == np.float32(1.5 * 2.0 ** -126)

    pad, xs = 8, c + 16
    xbuf = np.full((m, xs), 3.25, np.float32)
    xbuf[:, pad:pad + c] = x
    X, DX = dev(xbuf, et), dev(np.full((m, xs), -7.0, np.float32), et)
    Y = dev(np.full((m, xs), -7.0, np.float32), et)
    MEAN, INV = dev(mean), dev(invstd)
    segs, c0 = [], 0
    for i, ci in enumerate(_split(c, bf, multi)):      # distinct dy slices and strides, canaries around each
        off, stride = 8 * (i + 1), ci + 8 * (i + 3)
        buf = np.full((m, stride), np.nan, np.float32)
        buf[:, off:off + ci] = dy[:, c0:c0 + ci]
        segs.append(ffi.BnSeg(dev(buf, et).data_ptr(), off, stride, ci, dev(beta[c0:c0 + ci]).data_ptr(), None))
        c0 += ci
    arr = (ffi.BnSeg * len(segs))(*segs)
    ffi.check("bn_relu_bwd_frozen", L.jr_bn_relu_bwd_frozen(
        code, len(segs), ctypes.byref(arr), X.data_ptr(), pad, xs, m, c, MEAN.data_ptr(), INV.data_ptr(),
        DX.data_ptr(), None))
    ffi.check("bn_relu_apply", L.jr_bn_relu_apply(code, X.data_ptr(), pad, xs, m, c, MEAN.data_ptr(), INV.data_ptr(),
                                                 dev(beta).data_ptr(), Y.data_ptr(), pad, xs, None))
    torch.cuda.synchronize()
    got = DX.cpu()
    assert np.array_equal(bits(got[:, pad:pad + c]), ref_bits(want, bf))
    assert torch.all(got[:, :pad] == -7) and torch.all(got[:, pad + c:] == -7)          # canary channels untouched
    y = Y.float().cpu().numpy()[:, pad:pad + c]
    # (where dy * invstd != 0 AS STORED, and the stored activation shows the
    # gate: a positive pre below the smallest bf16, like the subnormal above,
    # is stored as 0 by the bf16 apply although its gate is open)
    with np.errstate(all="ignore"):
        store = R.to_bf16 if bf else np.float32
        live = np.isfinite(dy) & (store(dy * invstd) != 0) & ~((pre > 0) & (store(np.maximum(pre, 0)) == 0))
    assert np.array_equal((got.float().numpy()[:, pad:pad + c] != 0)[live], (y > 0)[live])


# ------------------------------------------------------------------ 2. the image gradient
IMG_CASES = [  # (n, h, w, c_in, c_out, k, stride, pad, dx_c_stride)
    (1, 11, 9, 3, 32, 3, 2, 0, 4), (3, 11, 9, 4, 32, 3, 2, 0, 8), (3, 12, 10, 1, 32, 3, 2, 0, 3),
    (1, 12, 10, 3, 16, 3, 2, 0, 4), (1, 75, 75, 3, 32, 3, 2, 0, 4), (3, 75, 75, 3, 48, 3, 2, 0, 3),
    (1, 107, 107, 3, 32, 3, 2, 0, 4), (3, 107, 107, 1, 32, 3, 2, 0, 8),
    (1, 13, 10, 3, 32, 3, 1, 1, 4),      # 'same' (the 8x8-pixel tile: the 16x16 one's dy patch exceeds the LDS budget)
    (3, 13, 10, 3, 16, 3, 1, 1, 3),      # 'same' on the 16x16 tile
    (1, 13, 10, 3, 32, 7, 2, 3, 4), (3, 13, 10, 1, 16, 7, 2, 3, 8)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", IMG_CASES)
def test_image_gradient_is_bitwise_the_restatement(case, dt):
    ffi, L = _lib()
    n, h, w, cin, cout, k, s, pad, dxs = case
    bf = dt == "bf16"
    rng = np.random.default_rng(sum(case) + bf)
    ho, wo = R.out_size(h, k, s, pad), R.out_size(w, k, s, pad)
    dy = rng.standard_normal((n, ho, wo, cout)).astype(np.float32)
    dy = R.to_bf16(dy) if bf else dy
    wt = (rng.standard_normal((k, k, cin, cout)) * 0.3).astype(np.float32)
    want = R.conv_bwd_image_ref(dy, wt, h, w, s, pad)
    yoff, ys = 16, 64                                   # a strided y slice; NaN around it
    buf = np.full((n, ho, wo, ys), np.nan, np.float32)
    buf[..., yoff:yoff + cout] = dy
    DY = dev(buf, torch.bfloat16 if bf else torch.float32)
    W = dev(wt)
    size = n * h * w * dxs
    DX = dev(np.concatenate([np.full(size, np.nan, np.float32), np.full(64, -7.0, np.float32)]))
    d = ffi.ConvDesc(n, h, w, cin, cout, k, k, s, s, pad, pad, ho, wo, 0, 4, yoff, ys)
    ffi.check("conv2d_bwd_image", L.jr_conv2d_bwd_image(ctypes.byref(d), ffi.JR_BF16 if bf else ffi.JR_F32,
                                                       DY.data_ptr(), W.data_ptr(), DX.data_ptr(), dxs, None))
    torch.cuda.synchronize()
    got = DX.cpu().numpy()
    assert np.all(got[size:] == -7)                                              # nothing behind the buffer
    got = got[:size].reshape(n, h, w, dxs)
    assert np.array_equal(bits(got[..., :cin]), bits(want))                     # every pixel written, bit for bit
    assert np.array_equal(bits(got[..., cin:]), np.zeros((n, h, w, dxs - cin), np.uint32))
    if s == 2 and pad == 0 and h % 2 == 0:
        assert not got[:, -1].any() and not got[:, :, -1].any()                 # the uncovered last row and column


# ------------------------------------------------------------------ 3. head and elementwise kernels
@pytest.mark.parametrize("units", [1, 5])
def test_head_logit_bwd_is_bitwise(units):
    ffi, L = _lib()
    n, c = 7, 301
    rng = np.random.default_rng(units)
    w = rng.standard_normal((c, units)).astype(np.float32)
    target = np.array([0, units - 1, units, -1, 0, 2 ** 30, units - 1], np.int32)   # in range and out of range
    W, T = dev(w), dev(target, torch.int32)
    for tgt, T_ in ((target, T), (None, None)):
        D = dev(np.full(n * c + 16, -7.0, np.float32))
        ffi.check("head_logit_bwd", L.jr_head_logit_bwd(W.data_ptr(), None if T_ is None else T_.data_ptr(), n, c, units,
                                                       D.data_ptr(), None))
        torch.cuda.synchronize()
        got = D.cpu().numpy()
        assert np.array_equal(bits(got[:n * c].reshape(n, c)), bits(R.head_logit_bwd_ref(w, tgt, n)))
        assert np.all(got[n * c:] == -7)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_elementwise_kernels_are_bitwise(dt):
    ffi, L = _lib()
    bf = dt == "bf16"
    code, et = (ffi.JR_BF16, torch.bfloat16) if bf else (ffi.JR_F32, torch.float32)
    rng = np.random.default_rng(5 + bf)
    n = 3 * 257 + 11                                    # odd, not a multiple of 256
    src = rng.standard_normal(n).astype(np.float32) * 3
    src[:4] = [0.0, -0.0, 2.0 ** -140, 1e30]
    src = R.to_bf16(src) if bf else src
    alpha = np.float32((1 + 0.5) / 3)
    S, D = dev(src, et), dev(np.full(n + 8, -7.0, np.float32), et)
    ffi.check("scale", L.jr_attr_scale_input(code, S.data_ptr(), D.data_ptr(), n, float(alpha), None))
    torch.cuda.synchronize()
    assert np.array_equal(bits(D[:n]), ref_bits(R.scale_input_ref(src, alpha, bf), bf)) and torch.all(D[n:] == -7)
    if bf:
        return
    dx = rng.standard_normal(n).astype(np.float32)
    acc0 = np.full(n + 8, np.nan, np.float32)           # first = 1 ignores what acc held
    ACC, DXd = dev(acc0), dev(dx)
    wgt = np.float32(1.0 / 3)
    ffi.check("acc", L.jr_attr_accumulate(DXd.data_ptr(), ACC.data_ptr(), n, float(wgt), 1, None))
    a1 = R.accumulate_ref(dx, None, wgt, True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(ACC[:n]), bits(a1))
    ffi.check("acc", L.jr_attr_accumulate(S.data_ptr(), ACC.data_ptr(), n, float(wgt), 0, None))
    torch.cuda.synchronize()
    assert np.array_equal(bits(ACC[:n]), bits(R.accumulate_ref(src, a1, wgt, False)))
    assert torch.all(torch.isnan(ACC[n:]))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_attr_map_is_bitwise(dt):
    ffi, L = _lib()
    bf = dt == "bf16"
    code, et = (ffi.JR_BF16, torch.bfloat16) if bf else (ffi.JR_F32, torch.float32)
    rng = np.random.default_rng(8 + bf)
    px, xs = 5 * 256 + 77, 8 if bf else 4
    acc = rng.standard_normal((px, 4)).astype(np.float32)
    acc[:, 3] = np.nan                                  # never read
    x = rng.uniform(0, 1, (px, xs)).astype(np.float32)
    x = R.to_bf16(x) if bf else x
    xd = x.copy()
    xd[:, 3:] = np.nan
    A, X = dev(acc), dev(xd, et)
    for mode in (0, 1):
        M = dev(np.full(px + 8, -7.0, np.float32))
        ffi.check("map", L.jr_attr_map(mode, A.data_ptr(), 4, X.data_ptr() if mode else None, code, xs, px, 3,
                                       M.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(bits(M[:px]), bits(R.map_ref(mode, acc, x))) and torch.all(M[px:] == -7)


# ------------------------------------------------------------------ engines
def _imgs(start=360, n=B):
    from jr import synth
    return synth.fundus_batch(start, n, RES)


def _engine(cfg="x8", fuse_pool=True, lanes=2, input_grad=True, units=1, head="sigmoid"):
    """seed-3 parameters, statistics calibrated on fundus_batch(350), frozen (one engine per configuration)."""
    return _build_engine(cfg, fuse_pool, lanes, input_grad, units, head)


@functools.lru_cache(maxsize=None)
def _build_engine(cfg, fuse_pool, lanes, input_grad, units, head):
    from jr.engine import Engine
    e = Engine(B, RES, RES, units=units, head=head, seed=3, train=False, tiles="heuristic", fuse_pool=fuse_pool,
               lanes=lanes, input_grad=input_grad, **CONFIGS[cfg])
    if cfg != "x6h":
        assert e.calibrate_bn([_imgs(350)]) == 1
        e.freeze_bn("moving")
    return e


def _grad(e, imgs, target=None, n=None):
    n = e.set_batch(imgs) if n is None else n
    e.forward(n, bn="frozen")
    e.input_gradient(n, target)
    return e.input_gradient_numpy(n)


def _rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.array([np.linalg.norm(a[i] - ref[i]) / np.linalg.norm(ref[i]) for i in range(len(ref))])


# ------------------------------------------------------------------ 4. the whole chain
@pytest.mark.parametrize("cfg", ["x8", "f32", "bf16"])
def test_whole_chain_against_the_masked_linear_fp64_model(cfg):
    """ReLU gates and pool argmaxes that flip at rounding level move the input
    gradient by percent, so the reference takes the ENGINE's gates: the
    network with ReLU replaced by the engine's masks (acts > 0) and max-pool
    by a gather at its argmaxes is linear in x, autograd gives its exact
    backward, and an independent fp32 evaluation of the same model (bf16:
    stored tensors and their gradients rounded to bf16) is the envelope."""
    from jr.init import unflatten
    e = _engine(cfg, fuse_pool=False)
    imgs = _imgs()
    got = _grad(e, imgs)
    e.synchronize()
    masks = {}
    for n in e.g.nodes:
        if n.kind == "conv":
            bf = e.g.bufs[n.y.buf]
            a = e.acts[n.y.buf][:B * bf.h * bf.w * bf.c].view(B, bf.h, bf.w, bf.c)[..., n.y.c_off:n.y.c_off + n.cout]
            masks[n.idx + 1] = (a > 0).permute(0, 3, 1, 2).cpu().numpy()
    argmax = []
    for i in sorted(e.argmax):
        n = e.g.nodes[i]
        argmax.append(e.argmax[i][:B * n.ho * n.wo * n.c].view(B, n.ho, n.wo, n.c).permute(0, 3, 1, 2).cpu().numpy())
    P, stats = unflatten(e.g, e.params_numpy()), e.bn_moving_numpy()
    x = imgs.astype(np.float32) * np.float32(1 / 255)
    ref = R.MaskedLinearRef(P, stats, masks, argmax, torch.float64).input_gradient(x)
    assert np.all(np.linalg.norm(ref.reshape(B, -1), axis=1) > 0)
    e32 = _rel_l2(R.MaskedLinearRef(P, stats, masks, argmax, torch.float32).input_gradient(x), ref)
    if cfg == "bf16":
        env = _rel_l2(R.MaskedLinearRef(P, stats, masks, argmax, torch.float64, emulate_bf16=True).input_gradient(x), ref)
    else:
        env = e32
    err = _rel_l2(got, ref)
    print(f"\ninput gradient {cfg} 107^2 B={B}: relL2 vs fp64 masked-linear per image gpu {err}, envelope {env}, "
          f"fp32 masked-linear {e32}")
    assert np.all(e32 < 1e-5), e32            # (a degenerate envelope cannot hide a failure)
    assert np.all(err <= 3 * env), (err, env)


# ------------------------------------------------------------------ 5. fused pools, lanes
def test_fused_pool_and_one_lane_are_bitwise():
    imgs = _imgs()
    a = _grad(_engine("x8", True, 2), imgs)
    assert np.any(a != 0)
    assert np.array_equal(bits(a), bits(_grad(_engine("x8", False, 2), imgs)))
    assert np.array_equal(bits(a), bits(_grad(_engine("x8", True, 1), imgs)))
    e = _engine("x8", True, 2)
    from jr.lanes import check_schedule
    calls = e._build_input_grad(B)
    check_schedule(calls)
    check_schedule(calls, precise=True)
    names = {c.name for c in calls}
    assert "conv_bwd_image" in names and "bn_relu_bwd_frozen" in names and "head_logit_bwd" in names
    assert not names & {"conv_wgrad", "wgrad_reduce", "param_ready", "bn_relu_bwd", "head_bwd"}
    assert (B, 2, "input_grad") in e._calls


# ------------------------------------------------------------------ 6. per-image independence
def test_gradient_of_an_image_depends_on_that_image_alone():
    e = _engine("x8")
    imgs = _imgs()
    other = imgs.copy()
    other[1:] = _imgs(900, B - 1)
    a, b = _grad(e, imgs), _grad(e, other)
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert all(np.any(a[i] != b[i]) for i in range(1, B))


def test_target_selects_the_logit():
    e = _engine("x8", units=5, head="softmax")
    imgs = _imgs()
    a = _grad(e, imgs)
    assert np.array_equal(bits(a), bits(_grad(e, imgs, target=[0, 0, 0, 0])))
    t = _grad(e, imgs, target=[0, 1, 2, 4])
    assert np.array_equal(bits(a[0]), bits(t[0])) and all(np.any(a[i] != t[i]) for i in range(1, B))
    assert not _grad(e, imgs, target=[0, 5, -1, 0])[1:3].any()       # out of range: a zero gradient
    with pytest.raises(ValueError, match="one class index per image"):
        e.input_gradient(B, target=[0, 1])


# ------------------------------------------------------------------ 7. nothing else moves
def test_nothing_else_moves():
    from jr.attribution import attribute
    e = _engine("x8")
    imgs = _imgs()
    n = e.set_batch(imgs)
    e.forward(n, bn="frozen")
    pred = e.predictions(n).copy()
    logits, params = e.logits.clone(), e.params.clone()
    e.input_gradient(n)
    assert np.array_equal(bits(e.predictions(n)), bits(pred)) and torch.equal(e.logits, logits)
    m = attribute(e, "integrated", steps=2)
    g = attribute(e, "gradient")
    e.synchronize()
    assert tuple(m.shape) == tuple(g.shape) == (B, RES, RES) and m.dtype == torch.float32
    assert np.array_equal(bits(e.predictions(n)), bits(pred)) and torch.equal(e.logits, logits)
    assert torch.equal(e.params, params)
    assert torch.all(g >= 0) and torch.any(g > 0)
    assert np.array_equal(bits(g), bits(R.map_ref(0, e.input_gradient_numpy(n))))
    plain = _engine("x8", input_grad=False)
    assert not hasattr(plain, "dinput") and not hasattr(plain, "dacts")
    plain.set_batch(imgs)
    plain.forward(B, bn="frozen")
    with pytest.raises(ValueError, match="input_grad=True"):
        plain.input_gradient()
    with pytest.raises(ValueError, match="input_grad=True"):
        attribute(plain, "gradient")
    assert not hasattr(e, "grads") and not hasattr(e, "accum")


# ------------------------------------------------------------------ 8. integrated gradients
def test_integrated_gradients_driver_is_bitwise():
    from jr.attribution import attribute
    e = _engine("x8")
    n, steps = 2, 3
    imgs = _imgs(360, n)
    e.set_batch(imgs)
    x0 = e.acts[e.g.input_buf][:n * RES * RES * 4].view(n, RES, RES, 4)[..., :3].cpu().numpy().copy()
    got = attribute(e, "integrated", steps=steps, B=n).cpu().numpy()
    logit = e.logits[:n].cpu().numpy().copy()
    back = e.acts[e.g.input_buf][:n * RES * RES * 4].view(n, RES, RES, 4)[..., :3].cpu().numpy()
    assert np.array_equal(bits(back), bits(x0))                     # the input buffer holds the batch again
    acc = None
    for k in range(steps):
        alpha = np.float32((k + 0.5) / steps)
        acc = R.accumulate_ref(_grad(e, R.scale_input_ref(x0, alpha)), acc, np.float32(1.0 / steps), k == 0)
    assert np.array_equal(bits(got), bits(R.map_ref(1, acc, x0)))
    e.set_batch(np.zeros_like(x0))
    e.forward(n, bn="frozen")
    e.synchronize()
    gap = np.abs(got.reshape(n, -1).astype(np.float64).sum(axis=1) - (logit - e.logits[:n].cpu().numpy()))
    print(f"\nintegrated gradients, {steps} steps: completeness gap |sum map - (logit(x) - logit(0))| = {gap} "
          f"(logit(x) - logit(0) = {logit - e.logits[:n].cpu().numpy()}); no bar at random initialisation")


# ------------------------------------------------------------------ 9. refusals
def test_refusals():
    from jr.attribution import attribute
    from jr.engine import Engine
    e = _engine("x8")
    e.set_batch(_imgs())
    with pytest.raises(ValueError, match="bn='frozen'"):
        e.input_gradient()                                          # no frozen forward since set_batch
    e.forward(B)                                                    # a batch-statistics forward is none either
    with pytest.raises(ValueError, match="bn='frozen'"):
        e.input_gradient()
    with pytest.raises(ValueError, match="steps"):
        attribute(e, "integrated", steps=0)
    with pytest.raises(ValueError, match="unknown method"):
        attribute(e, "smoothgrad")
    with pytest.raises(ValueError, match="x8p"):
        Engine(B, RES, RES, train=False, tiles="heuristic", conv_math="x8p", input_grad=True)
    x6h = _engine("x6h")
    x6h.set_batch(_imgs())
    with pytest.raises(ValueError, match="conv_math='x6h'"):
        x6h.input_gradient()
    with pytest.raises(ValueError, match="conv_math='x6h'"):
        attribute(x6h, "gradient")
