"""Moving BN statistics and frozen (batch-independent) inference on the GPU.

a. jr_bn_moving_update / jr_bn_moving_freeze alone: bitwise the numpy
   restatement of the formulas in jr.h (tests/bn_moving_ref.py), canaries
   between segments and members untouched.
b. the side-car of the training step (Engine(bn_moving=...)): bitwise the
   restatement applied to the engine's own statistics; parameters and loss
   bitwise those of the step without it; one lane, two lanes and a replayed
   graph agree bit for bit.
c. the moving statistics of two steps against the fp64 functional model,
   within 3x the deviation of the same model in fp32.
d. freeze_bn("batch") + forward(bn="frozen") is bitwise forward(bn="batch").
e. frozen predictions do not depend on the other images of the batch.
f. the frozen forward against the fp64 functional model with fixed statistics.
g. refusals.
All at 107^2, batch 4.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RES, B = 107, 4
CONFIGS = {"x6h": dict(dtype="f32", conv_math="x6h"), "x8": dict(dtype="f32", conv_math="x8"),
           "f32": dict(dtype="f32", conv_math="f32"), "bf16": dict(dtype="bf16")}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _diff(what, cfg, k, a, b, units=None):
    """The message of a failed bitwise comparison: which array, which step,
    how many words differ, the first differing word and -- for arrays in the
    statistics layout ([mean(c) | invstd(c)] per conv launch, `units` =
    [(c, rows)]) -- the first differing BN launch and which half of it."""
    a, b = _bits(a).reshape(-1), _bits(b).reshape(-1)
    if a.shape != b.shape:
        return f"{cfg} step {k}: {what}: shapes {a.shape} vs {b.shape}"
    bad = np.flatnonzero(a != b)
    msg = f"{cfg} step {k}: {what}: {bad.size} of {a.size} words differ"
    if bad.size:
        i = int(bad[0])
        msg += f", first at word {i} (0x{int(a[i]):08x} vs 0x{int(b[i]):08x})"
        o = 0
        for j, (c, _) in enumerate(units or ()):
            if i < o + 2 * c:
                half = "mean" if i < o + c else "invstd / variance"
                msg += f": BN launch {j} (c = {c}), {half}, channel {(i - o) % c}"
                break
            o += 2 * c
    return msg


# ---------------------------------------------------------------- a. kernels
SEGS = [(16, 2), (48, 16), (192, 1420864), (448, 2), (192, 16), (448, 1420864), (16, 1420864)]   # (c, rows)
CANARY = np.float32(-7777.25)
EPS = 1e-3


def _layout(gap):
    """Offsets of the segments in a buffer with `gap` canary floats before each and after the last."""
    offs, o = [], gap
    for c, _ in SEGS:
        offs.append(o)
        o += 2 * c + gap
    return offs, o


def _invstd(rng, c):
    from bn_moving_ref import EPS64
    v = np.exp(rng.normal(0, 3, c))
    s = (1.0 / np.sqrt(v + EPS64)).astype(np.float32)
    s[0] = np.float32(1.0 / np.sqrt(EPS64))     # variance 0: step 1 lands at or below 0, the clamp
    s[1] = np.float32(1e-3)                     # variance 1e6
    s[2] = np.nextafter(s[0], np.float32(np.inf))     # just past 1/sqrt(eps): negative before the clamp
    return s


@pytest.mark.parametrize("members", [1, 3])
def test_kernels_are_bitwise_the_restatement(members):
    from jr import _ffi
    from bn_moving_ref import freeze_ref, update_ref
    _ffi.init(0)
    L = _ffi.load()
    rng = np.random.default_rng(11 + members)
    s_off, s_len = _layout(5)
    m_off, m_len = _layout(9)
    s_ms, m_ms, f_ms = s_len + 7, m_len + 3, s_len + 11       # padded member strides
    table = (_ffi.BnMovingSeg * len(SEGS))(*[_ffi.BnMovingSeg(so, mo, rows, c, 0)
                                             for (c, rows), so, mo in zip(SEGS, s_off, m_off)])
    dtab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    max_c = max(c for c, _ in SEGS)
    assert max_c > 256                                        # two blocks in x
    moving = np.full(members * m_ms, CANARY, np.float32)
    for m in range(members):
        for (c, _), mo in zip(SEGS, m_off):
            moving[m * m_ms + mo:m * m_ms + mo + c] = 0.0
            moving[m * m_ms + mo + c:m * m_ms + mo + 2 * c] = 1.0
    want = moving.copy()
    dmov = torch.from_numpy(moving).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for momentum in (0.99, 0.5, 0.0):
        stats = np.full(members * s_ms, CANARY, np.float32)
        for m in range(members):
            for (c, rows), so, mo in zip(SEGS, s_off, m_off):
                mean_b, inv = rng.normal(0, 2, c).astype(np.float32), _invstd(rng, c)
                stats[m * s_ms + so:m * s_ms + so + c] = mean_b
                stats[m * s_ms + so + c:m * s_ms + so + 2 * c] = inv
                a = m * m_ms + mo
                want[a:a + c], want[a + c:a + 2 * c] = update_ref(want[a:a + c], want[a + c:a + 2 * c], mean_b, inv,
                                                                  rows, momentum)
        dst = torch.from_numpy(stats).cuda()
        _ffi.check("update", L.jr_bn_moving_update(dtab.data_ptr(), len(SEGS), max_c, members, dst.data_ptr(), s_ms,
                                                   dmov.data_ptr(), m_ms, momentum, EPS, s))
        torch.cuda.synchronize()
        got = dmov.cpu().numpy()
        assert _same(got, want), (momentum, int(np.sum(_bits(got) != _bits(want))))      # canaries included
        assert _same(dst.cpu().numpy(), stats)
    assert np.sum(want == CANARY) == members * m_ms - members * sum(2 * c for c, _ in SEGS)
    # freeze: the statistics layout, bitwise; fp64 / and sqrt are correctly rounded on the device
    frozen = np.full(members * f_ms, CANARY, np.float32)
    dfr = torch.from_numpy(frozen).cuda()
    _ffi.check("freeze", L.jr_bn_moving_freeze(dtab.data_ptr(), len(SEGS), max_c, members, dmov.data_ptr(), m_ms,
                                               dfr.data_ptr(), f_ms, EPS, s))
    torch.cuda.synchronize()
    for m in range(members):
        for (c, _), so, mo in zip(SEGS, s_off, m_off):
            a = m * m_ms + mo
            frozen[m * f_ms + so:m * f_ms + so + c], frozen[m * f_ms + so + c:m * f_ms + so + 2 * c] = freeze_ref(
                want[a:a + c], want[a + c:a + 2 * c])
    got = dfr.cpu().numpy()
    assert _same(got, frozen), int(np.sum(_bits(got) != _bits(frozen)))
    assert _same(dmov.cpu().numpy(), want)


# --------------------------------------------------------------- b. side-car
def _batch(k):
    from jr import synth
    return synth.fundus_batch(300 + 10 * k, B, RES), synth.labels(300 + 10 * k, B, p=0.5)


def _run_steps(cfg, steps=3, bn_moving=0.99, lanes=2, graph=False):
    """moving / stats / loss after each step, the final parameters."""
    from jr.engine import Engine
    e = Engine(B, RES, RES, seed=3, lanes=lanes, tiles="heuristic", bn_moving=bn_moving, **CONFIGS[cfg])
    out = {"moving": [], "stats": [], "loss": []}
    for k in range(steps):
        e.set_batch(*_batch(k))
        if graph:
            if k == 0:
                e.capture()
            e.replay()
        else:
            e.train_step()
        out["loss"].append(e.loss_value())
        out["stats"].append(e.stats.cpu().numpy())
        out["moving"].append(e.moving.cpu().numpy())
    out["params"] = e.params_numpy()
    out["updates"] = e.updates
    out["units"] = [(u.cout, B * u.ho * u.wo) for u in e.cunits]
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def _sidecar(cfg):
    return _run_steps(cfg)


@pytest.mark.parametrize("cfg", ["x6h", "bf16"])
def test_sidecar_is_the_restatement_and_leaves_the_step_alone(cfg):
    from bn_moving_ref import update_ref
    on, off = _sidecar(cfg), _run_steps(cfg, bn_moving=None)
    n = sum(2 * c for c, _ in on["units"])
    want = np.zeros(n, np.float32)
    o = 0
    for c, _ in on["units"]:
        want[o + c:o + 2 * c] = 1.0
        o += 2 * c
    # never touched without the feature
    assert _same(off["moving"][-1], want), _diff("moving without the side-car vs mean 0 / variance 1", cfg, 2,
                                                 off["moving"][-1], want, on["units"])
    assert off["updates"] == 0
    for k in range(3):
        st, o = on["stats"][k], 0
        for c, rows in on["units"]:
            want[o:o + c], want[o + c:o + 2 * c] = update_ref(want[o:o + c], want[o + c:o + 2 * c], st[o:o + c],
                                                              st[o + c:o + 2 * c], rows, 0.99)
            o += 2 * c
        assert _same(on["moving"][k], want), _diff("moving, side-car vs restatement", cfg, k, on["moving"][k], want,
                                                   on["units"])
    assert on["updates"] == 3
    assert _same(on["params"], off["params"]), _diff("params, side-car on vs off", cfg, 2, on["params"], off["params"])
    assert on["loss"] == off["loss"], (cfg, "loss per step, side-car on vs off", on["loss"], off["loss"])
    for k, (a, b) in enumerate(zip(on["stats"], off["stats"])):
        assert _same(a, b), _diff("stats, side-car on vs off", cfg, k, a, b, on["units"])


@pytest.mark.parametrize("cfg", ["x6h", "bf16"])
def test_sidecar_one_lane_and_replayed_graph_are_bitwise(cfg):
    on = _sidecar(cfg)
    for name, other in (("one lane", _run_steps(cfg, lanes=1)), ("replayed graph", _run_steps(cfg, graph=True))):
        assert other["loss"] == on["loss"], (cfg, f"loss per step, {name} vs two lanes", other["loss"], on["loss"])
        assert _same(other["params"], on["params"]), _diff(f"params, {name} vs two lanes", cfg, 2, other["params"],
                                                           on["params"])
        assert other["updates"] == 3
        for k in range(3):
            assert _same(other["moving"][k], on["moving"][k]), _diff(f"moving, {name} vs two lanes", cfg, k,
                                                                     other["moving"][k], on["moving"][k], on["units"])


# ------------------------------------------------------- c. trajectory vs fp64
def _params(seed=3):
    from jr.inception import build_inception_v3
    from jr.init import init_params, unflatten
    g = build_inception_v3(RES, RES)
    flat = init_params(g, seed)
    return g, flat, unflatten(g, flat)


def _f(x):
    return x.astype(np.float32) * np.float32(1 / 255)


def test_moving_trajectory_within_the_fp32_envelope():
    """Two steps, momentum 0.5.  Per layer and statistic: max |gpu - fp64| /
    max |fp64| <= 3 x the same figure of the fp32 functional model."""
    from jr.engine import Engine
    from bn_moving_ref import moving_trajectory
    g, flat, P = _params()
    batches = [_batch(0), _batch(1)]
    e = Engine(B, RES, RES, seed=3, tiles="heuristic", bn_moving=0.5)
    for x, y in batches:
        e.set_batch(x, y)
        e.train_step()
    got = e.bn_moving_numpy()
    ref = [(_f(x), y) for x, y in batches]
    m64 = moving_trajectory(P, torch.float64, ref, 0.5)
    m32 = moving_trajectory(P, torch.float32, ref, 0.5)
    worst = {}
    for k in sorted(m64):
        for j, name in enumerate(("moving_mean", "moving_variance")):
            r64 = m64[k][j]
            scale = np.max(np.abs(r64))
            e_gpu = np.max(np.abs(got[f"batch_normalization_{k}/{name}"].astype(np.float64) - r64)) / scale
            e_32 = np.max(np.abs(m32[k][j].astype(np.float64) - r64)) / scale
            worst[(k, name)] = (e_gpu, e_32)
    ratios = {key: a / b for key, (a, b) in worst.items()}
    top = sorted(ratios, key=ratios.get)[-3:]
    print("trajectory: max gpu err %.3g, max fp32 err %.3g, largest gpu/fp32 ratios %s" % (
        max(a for a, _ in worst.values()), max(b for _, b in worst.values()),
        [(key, round(ratios[key], 3)) for key in top]))
    bad = {key: v for key, v in worst.items() if not v[0] <= 3 * v[1]}
    assert not bad, bad


# --------------------------------------------------------------- d. identity
@pytest.mark.parametrize("cfg", ["x8", "f32", "bf16"])
def test_frozen_batch_statistics_are_the_identity(cfg):
    from jr.engine import Engine
    from jr.ensemble import EnsembleEngine
    from jr.init import init_params
    g, _, _ = _params()
    params = [init_params(g, 50 + m) for m in range(2)]
    x, y = _batch(2)
    per_member = []
    for m in range(2):
        e = Engine(B, RES, RES, train=False, tiles="heuristic", **CONFIGS[cfg])
        e.load_params(params[m])
        e.set_batch(x, y)
        e.forward()
        p0 = e.predictions()                # (synchronises the engine's streams)
        z0 = e.logits.cpu().numpy()
        e.freeze_bn("batch")
        e.synchronize()
        e.stats.zero_()                     # the frozen forward must not read the batch statistics it rewrites
        torch.cuda.synchronize()
        e.forward(bn="frozen")
        assert _same(e.predictions(), p0) and _same(e.logits.cpu().numpy(), z0), (cfg, m)
        assert float(np.abs(e.stats.cpu().numpy()).max()) > 0       # the convs still write them
        per_member.append(p0)
    ens = EnsembleEngine(params, B, RES, RES, tiles="heuristic", **CONFIGS[cfg])
    ens.set_batch(x, y)
    ens.forward()
    p0 = ens.predictions()
    ens.freeze_bn("batch")
    ens.forward(bn="frozen")
    got = ens.predictions()
    assert _same(got, p0)
    for m in range(2):
        assert _same(got[m], per_member[m]), (cfg, m)
    assert got[0].tobytes() != got[1].tobytes()


# --------------------------------------------------- e. batch independence
def _frozen_engine(cfg, calib, stats=None):
    from jr.engine import Engine
    _, flat, _ = _params()
    e = Engine(B, RES, RES, train=False, tiles="heuristic", **CONFIGS[cfg])
    e.load_params(flat)
    if stats is None:
        assert e.calibrate_bn([calib]) == 1
    else:
        e.load_bn_moving(stats)
    e.freeze_bn("moving")
    return e


def test_frozen_prediction_depends_on_its_image_alone():
    from jr import synth
    xa, _ = _batch(3)
    x, _ = _batch(4)
    other = x.copy()
    other[1:] = synth.fundus_batch(900, B - 1, RES)
    e = _frozen_engine("x8", xa)
    pred = {}
    for bn in ("frozen", "batch"):
        for name, imgs in (("x", x), ("other", other)):
            e.set_batch(imgs)
            e.forward(bn=bn)
            pred[bn, name] = e.predictions()
    assert _same(pred["frozen", "x"][0], pred["frozen", "other"][0])
    assert not _same(pred["frozen", "x"][1:], pred["frozen", "other"][1:])
    assert not _same(pred["batch", "x"][0], pred["batch", "other"][0])           # the control
    # one image on its own: another tile plan, so an fp32 reordering of the same
    # arithmetic -- bounded by 3x what the x8 / f32 reordering moves this batch
    e.set_batch(x[:1])
    e.forward(1, bn="frozen")
    alone = e.predictions(1)
    f = _frozen_engine("f32", xa, e.bn_moving_numpy())
    f.set_batch(x)
    f.forward(bn="frozen")
    envelope = float(np.max(np.abs(f.predictions().astype(np.float64) - pred["frozen", "x"])))
    moved = float(np.max(np.abs(alone.astype(np.float64) - pred["frozen", "x"][:1])))
    print(f"frozen n=1 vs n={B}: |dp| {moved:.3g}; x8 vs f32 on the batch: {envelope:.3g}")
    assert moved <= 3 * envelope, (moved, envelope)


# ------------------------------------------------ f. frozen forward vs fp64
def test_frozen_forward_against_the_fp64_model():
    from bn_moving_ref import BNStatsRef
    _, _, P = _params()
    xa, _ = _batch(5)
    xb, _ = _batch(6)
    e = _frozen_engine("x8", xa)
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
    print(f"frozen forward: max |logit - fp64| gpu {e_gpu:.3g}, fp32 model {e_32:.3g}, "
          f"max |logit| {np.max(np.abs(logits['fp64'])):.3g}")
    assert e_gpu <= 1e-3
    assert e_gpu <= 3 * e_32, (e_gpu, e_32)


# --------------------------------------------------------------- g. refusals
def test_refusals():
    from jr.engine import Engine
    e = Engine(B, RES, RES, train=False, tiles="heuristic", conv_math="x6h")
    e.freeze_bn("moving")
    with pytest.raises(ValueError, match="x6h"):
        e.forward(bn="frozen")
    e = Engine(B, RES, RES, train=False, tiles="heuristic", conv_math="x8", fold_stats=True)
    e.freeze_bn("moving")
    with pytest.raises(ValueError, match="fold_stats"):
        e.forward(bn="frozen")
    e = Engine(B, RES, RES, train=False, tiles="heuristic", conv_math="x8")
    with pytest.raises(ValueError, match="freeze_bn"):
        e.forward(bn="frozen")
    with pytest.raises(ValueError):
        e.forward(bn="moving")
    with pytest.raises(ValueError):
        e.freeze_bn("running")
    st = e.bn_moving_numpy()
    assert len(st) == 2 * 94 and float(st["batch_normalization_94/moving_variance"].min()) == 1.0
    bad = dict(st)
    bad["batch_normalization_7/moving_variance"] = st["batch_normalization_7/moving_variance"] - 2.0
    with pytest.raises(ValueError, match="negative variance"):
        e.load_bn_moving(bad)
    bad["batch_normalization_7/moving_variance"] = st["batch_normalization_7/moving_variance"] * np.float32("nan")
    with pytest.raises(ValueError, match="non-finite"):
        e.load_bn_moving(bad)
    del bad["batch_normalization_7/moving_variance"]
    with pytest.raises(ValueError, match="lack"):
        e.load_bn_moving(bad)
    assert all(_same(v, st[k]) for k, v in e.bn_moving_numpy().items())     # refused loads change nothing
    with pytest.raises(ValueError, match="momentum"):
        Engine(B, RES, RES, tiles="heuristic", bn_moving=1.5)
    # a launch with one row has no unbiased variance: 75^2 ends in 1x1 maps
    t = Engine(2, 75, 75, tiles="heuristic", bn_moving=0.9)
    with pytest.raises(ValueError, match="at least 2 rows"):
        t.train_step(1)
