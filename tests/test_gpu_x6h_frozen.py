"""Frozen-BN inference and the input gradient on conv_math="x6h" behind the
device guard (Engine / EnsembleEngine x6h_frozen=True).  107^2, batch 4.

a. refusals and defaults: x6h_frozen with another conv_math is a ValueError;
   without it x6h still refuses forward(bn="frozen").
b. freeze_bn("batch") + forward(bn="frozen") is bitwise forward(bn="batch"),
   Engine and a 2-member EnsembleEngine, whose members are bitwise the
   per-member engines.
c. image 0's frozen prediction is bitwise unchanged when images 1..3 change
   (and changes under bn="batch": the control).
d. the frozen logits against the fp64 functional model with fixed statistics,
   within 3x the error of the same model in fp32.
e. the guard end to end: a moving mean of -1e6 in one channel of the first BN
   layer raises JRError(JR_ERR_DEVICE) at synchronize(); with the sane
   statistics back, the frozen forward is bitwise what it was.
f. the input gradient: against the masked-linear fp64 model built from the
   engine's own gates and argmaxes within 3x the fp32 masked-linear envelope;
   two calls after one forward, and one lane and two lanes, bitwise equal;
   image 0's gradient moves by at most 3x the x8-vs-f32 difference on the same
   batch when images 1..3 change (its dy scales are measured per batch);
   predictions and parameters untouched.

f, measured on an MI355X (relative L2 per image against the fp64 masked-linear
model):
  x6h   gpu 2.46e-6 .. 2.71e-6   fp32 masked-linear 8.94e-7 .. 9.52e-7
image 0's gradient when images 1..3 change: relative L2 change 0 (the
power-of-two dy scales did not move); x8 vs f32 on the batch 3.7e-3.
d: max |logit - fp64| gpu 3.69e-4, fp32 model 3.07e-4 (max |logit| 5.5).
"""
import functools

import numpy as np
import pytest

import attribution_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RES, B = 107, 4
X6H = dict(dtype="f32", conv_math="x6h", x6h_frozen=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _batch(k):
    from jr import synth
    return synth.fundus_batch(300 + 10 * k, B, RES)


def _f(x):
    return x.astype(np.float32) * np.float32(1 / 255)


@functools.lru_cache(maxsize=None)
def _params(seed=3):
    from jr.inception import build_inception_v3
    from jr.init import init_params, unflatten
    g = build_inception_v3(RES, RES)
    flat = init_params(g, seed)
    return g, flat, unflatten(g, flat)


@functools.lru_cache(maxsize=None)
def _engine(math="x6h", lanes=2, input_grad=False, fuse_pool=True):
    """seed-3 parameters; statistics calibrated on _batch(3) by the x6h engine
    and shared (bit for bit) with every other one; frozen."""
    from jr.engine import Engine
    cfg = X6H if math == "x6h" else dict(dtype="f32", conv_math=math)
    e = Engine(B, RES, RES, seed=3, train=False, tiles="heuristic", lanes=lanes, input_grad=input_grad,
               fuse_pool=fuse_pool, **cfg)
    if (math, lanes, input_grad, fuse_pool) == ("x6h", 2, False, True):
        assert e.calibrate_bn([_batch(3)]) == 1
    else:
        e.load_bn_moving(_engine().bn_moving_numpy())
    e.freeze_bn("moving")
    return e


# ---------------------------------------------------------------- a. refusals
def test_refusals_and_defaults():
    from jr.engine import Engine
    from jr.ensemble import EnsembleEngine
    with pytest.raises(ValueError, match="x6h_frozen"):
        Engine(B, RES, RES, train=False, tiles="heuristic", conv_math="x8", x6h_frozen=True)
    with pytest.raises(ValueError, match="x6h_frozen"):
        Engine(B, RES, RES, train=False, tiles="heuristic", dtype="bf16", x6h_frozen=True)
    _, flat, _ = _params()
    with pytest.raises(ValueError, match="x6h_frozen"):
        EnsembleEngine([flat], B, RES, RES, tiles="heuristic", conv_math="f32", x6h_frozen=True)
    e = Engine(B, RES, RES, train=False, tiles="heuristic", conv_math="x6h")        # the default stays a refusal
    assert e.x6h_frozen is False
    e.freeze_bn("moving")
    with pytest.raises(ValueError, match="x6h"):
        e.forward(bn="frozen")
    g = Engine(B, RES, RES, train=False, tiles="heuristic", **X6H)
    with pytest.raises(ValueError, match="freeze_bn"):          # the other refusals stand
        g.forward(bn="frozen")
    # the frozen lists alone carry the guarded entry points
    g.freeze_bn("moving")
    frozen = {c.fn.__name__ for c in g._build_calls(B, frozen=True)[0]}
    batch = {c.fn.__name__ for c in g._build_calls(B)[0]}
    assert {"jr_bn_relu_apply_guard", "jr_bn_relu_apply_multi_guard", "jr_bn_relu_maxpool3x3s2_fwd_guard"} <= frozen
    assert not frozen & {"jr_bn_relu_apply", "jr_bn_relu_apply_multi", "jr_bn_relu_maxpool3x3s2_fwd"}
    assert not any(n.endswith("_guard") for n in batch)


# ---------------------------------------------------------------- b. identity
def test_frozen_batch_statistics_are_the_identity():
    from jr.engine import Engine
    from jr.ensemble import EnsembleEngine
    from jr.init import init_params
    g, _, _ = _params()
    params = [init_params(g, 50 + m) for m in range(2)]
    x = _batch(2)
    per_member = []
    for m in range(2):
        e = Engine(B, RES, RES, train=False, tiles="heuristic", **X6H)
        e.load_params(params[m])
        e.set_batch(x)
        e.forward()
        p0 = e.predictions()
        z0 = e.logits.cpu().numpy()
        e.freeze_bn("batch")
        e.synchronize()
        e.stats.zero_()                     # the frozen forward must not read the batch statistics it rewrites
        torch.cuda.synchronize()
        e.forward(bn="frozen")
        assert _same(e.predictions(), p0) and _same(e.logits.cpu().numpy(), z0), m
        per_member.append(p0)
    ens = EnsembleEngine(params, B, RES, RES, tiles="heuristic", **X6H)
    ens.set_batch(x)
    ens.forward()
    p0 = ens.predictions()
    z0 = ens.logits.cpu().numpy()
    ens.freeze_bn("batch")
    ens.forward(bn="frozen")
    got = ens.predictions()
    assert _same(got, p0) and _same(ens.logits.cpu().numpy(), z0)
    for m in range(2):
        assert _same(got[m], per_member[m]), m
    assert got[0].tobytes() != got[1].tobytes()
    names = {c.fn.__name__ for c in ens._build_calls(B, frozen=True)[0]}
    assert {"jr_bn_relu_apply_grouped_guard", "jr_bn_relu_maxpool3x3s2_fwd_grouped_guard"} <= names
    assert not names & {"jr_bn_relu_apply_grouped", "jr_bn_relu_maxpool3x3s2_fwd_grouped"}


# --------------------------------------------------- c. batch independence
def test_frozen_prediction_depends_on_its_image_alone():
    from jr import synth
    x = _batch(4)
    other = x.copy()
    other[1:] = synth.fundus_batch(900, B - 1, RES)
    e = _engine()
    pred = {}
    for bn in ("frozen", "batch"):
        for name, imgs in (("x", x), ("other", other)):
            e.set_batch(imgs)
            e.forward(bn=bn)
            pred[bn, name] = e.predictions()
    assert _same(pred["frozen", "x"][0], pred["frozen", "other"][0])
    assert not _same(pred["frozen", "x"][1:], pred["frozen", "other"][1:])
    assert not _same(pred["batch", "x"][0], pred["batch", "other"][0])           # the control


# ------------------------------------------------ d. frozen forward vs fp64
def test_frozen_forward_against_the_fp64_model():
    from bn_moving_ref import BNStatsRef
    _, _, P = _params()
    xa, xb = _batch(3), _batch(6)
    e = _engine()
    e.set_batch(xb)
    e.forward(bn="frozen")
    e.synchronize()
    z = e.logits[:B].cpu().numpy().reshape(B, 1).astype(np.float64)
    logits = {}
    for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        cal = BNStatsRef(P, dt)
        with torch.no_grad():
            cal.forward(_f(xa))
            logits[name] = BNStatsRef(P, dt, fixed=cal.unbiased()).forward(_f(xb))[0].numpy().astype(np.float64)
    e_gpu = float(np.max(np.abs(z - logits["fp64"])))
    e_32 = float(np.max(np.abs(logits["fp32"] - logits["fp64"])))
    print(f"\nfrozen x6h forward: max |logit - fp64| gpu {e_gpu:.3g}, fp32 model {e_32:.3g}, "
          f"max |logit| {np.max(np.abs(logits['fp64'])):.3g}")
    assert e_gpu <= 3 * e_32, (e_gpu, e_32)


# ------------------------------------------------------------- e. the guard
def test_guard_reports_an_activation_above_the_bound():
    from jr import _ffi
    e = _engine()
    x = _batch(5)
    e.set_batch(x)
    e.forward(bn="frozen")
    before = e.predictions().copy()
    z0 = e.logits.cpu().numpy()
    sane = e.bn_moving_numpy()
    bad = {k: v.copy() for k, v in sane.items()}
    bad["batch_normalization_1/moving_mean"][5] = -1e6
    e.load_bn_moving(bad)
    e.freeze_bn("moving")
    e.forward(bn="frozen")
    with pytest.raises(_ffi.JRError) as err:
        e.synchronize()
    assert err.value.status == _ffi.JR_ERR_DEVICE
    assert "guard" in str(err.value) and "stream-K" in str(err.value)
    e.synchronize()                             # reported once
    e.load_bn_moving(sane)
    e.freeze_bn("moving")
    e.forward(bn="frozen")
    assert _same(e.predictions(), before) and _same(e.logits.cpu().numpy(), z0)


# ------------------------------------------------------- f. input gradient
def _grad(e, imgs):
    n = e.set_batch(imgs)
    e.forward(n, bn="frozen")
    e.input_gradient(n)
    return e.input_gradient_numpy(n)


def _rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.array([np.linalg.norm(a[i] - ref[i]) / np.linalg.norm(ref[i]) for i in range(len(ref))])


def test_input_gradient_against_the_masked_linear_fp64_model():
    """The method of tests/test_gpu_attribution.py: the reference takes the
    ENGINE's ReLU gates and pool argmaxes (unfused pools, so every gate is
    stored), which makes the network linear in x."""
    from jr.init import unflatten
    e = _engine(input_grad=True, fuse_pool=False)
    imgs = _batch(7)
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
    x = _f(imgs)
    ref = R.MaskedLinearRef(P, stats, masks, argmax, torch.float64).input_gradient(x)
    assert np.all(np.linalg.norm(ref.reshape(B, -1), axis=1) > 0)
    env = _rel_l2(R.MaskedLinearRef(P, stats, masks, argmax, torch.float32).input_gradient(x), ref)
    err = _rel_l2(got, ref)
    print(f"\ninput gradient x6h 107^2 B={B}: relL2 vs fp64 masked-linear per image gpu {err}, "
          f"fp32 masked-linear {env}")
    assert np.all(env < 1e-5), env            # (a degenerate envelope cannot hide a failure)
    assert np.all(err <= 3 * env), (err, env)


def test_input_gradient_repeats_lanes_and_nothing_else_moves():
    from jr.lanes import check_schedule
    e = _engine(input_grad=True)
    imgs = _batch(7)
    n = e.set_batch(imgs)
    e.forward(n, bn="frozen")
    pred = e.predictions(n).copy()
    logits, params = e.logits.clone(), e.params.clone()
    e.input_gradient(n)
    a = e.input_gradient_numpy(n)
    e.input_gradient(n)                          # the data-gradient rows start from zero again: the same bits
    b = e.input_gradient_numpy(n)
    assert np.any(a != 0) and _same(a, b)
    assert _same(e.predictions(n), pred) and torch.equal(e.logits, logits) and torch.equal(e.params, params)
    calls = e._build_input_grad(B)
    check_schedule(calls)
    check_schedule(calls, precise=True)
    names = [c.name for c in calls]
    assert names[0] == "absmax_reset" and calls[0].lane == 0 and names.count("absmax_reset") == 1
    assert {c.fn.__name__ for c in calls if c.name == "bn_relu_bwd_frozen"} == {"jr_bn_relu_bwd_frozen_absmax"}
    one = _grad(_engine(lanes=1, input_grad=True), imgs)
    assert _same(a, one)
    unfused = _grad(_engine(input_grad=True, fuse_pool=False), imgs)
    assert _same(a, unfused)


def test_gradient_of_an_image_moves_within_the_x6h_error_class():
    """The x6h data gradients take their dy scale from the batch: image 0's
    gradient is not bitwise independent of images 1..3, but moves by no more
    than 3x what x8 and f32 differ by on the same batch."""
    from jr import synth
    imgs = _batch(7)
    other = imgs.copy()
    other[1:] = synth.fundus_batch(900, B - 1, RES)
    e = _engine(input_grad=True)
    a, b = _grad(e, imgs), _grad(e, other)
    moved = float(_rel_l2(b[:1], a[:1])[0])
    assert all(np.any(a[i] != b[i]) for i in range(1, B))
    g8, g32 = _grad(_engine("x8", input_grad=True), imgs), _grad(_engine("f32", input_grad=True), imgs)
    envelope = float(_rel_l2(g8[:1], g32[:1])[0])
    print(f"\nx6h input gradient of image 0, images 1..3 changed: relL2 change {moved:.3g}; "
          f"x8 vs f32 on the batch: {envelope:.3g}")
    assert envelope > 0
    assert moved <= 3 * envelope, (moved, envelope)


def test_attribute_runs_unchanged():
    from jr.attribution import attribute
    e = _engine(input_grad=True)
    n = e.set_batch(_batch(7))
    e.forward(n, bn="frozen")
    pred = e.predictions(n).copy()
    g = attribute(e, "gradient")
    m = attribute(e, "integrated", steps=2)
    e.synchronize()                             # (the guard stayed clean through the scaled passes)
    assert tuple(m.shape) == tuple(g.shape) == (B, RES, RES) and torch.all(g >= 0) and torch.any(g > 0)
    assert _same(e.predictions(n), pred)
