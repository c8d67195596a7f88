"""The device optimizer recipe on the GPU, through the C-ABI and the Engine:

* jr_grad_sqnorm + jr_opt_prepare: the sum of squares within the a-priori
  bound n * 2^-53 * S of an exact float64 sum, the norm within 1 fp32 ulp,
  bitwise equal from run to run, non-finite gradients skipped and counted;
* every jr_*_update_ex bitwise the numpy restatement (tests/opt_ref.py) over
  four steps, with decay ranges that split a quad, hold one element, leave an
  undecayed tail and cross tile boundaries; nothing written on a skipped step;
  with no decay, no clipping and grad_scale 1 bitwise the by-value kernels;
* every by-value jr_*_update bitwise the same restatement with scale =
  grad_scale, at sizes around a quad and a tile, and on buffers that are not
  16-byte aligned where the call accepts them;
* the Engine's device path: bitwise the default path when the recipe changes
  nothing, the restatement under clipping, weight decay, a grad_scale, a NaN
  gradient, bf16 storage, and replays of a captured step under a changing
  learning rate.
"""
import math

import numpy as np
import pytest

import opt_ref
from opt_ref import f32

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OPTS = ("nesterov", "momentum", "sgd", "adam")


def _lib():
    from jr import _ffi
    _ffi.init(0)
    return _ffi, _ffi.load()


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class Recipe:
    """The device structs of one parameter buffer of n elements."""

    def __init__(self, n, ranges=()):
        self.ffi, self.L = _lib()
        self.n = n
        self.ws = self.L.jr_grad_sqnorm_workspace_size(n)
        self.part = torch.zeros(self.ws // 8, dtype=torch.float64, device="cuda")
        self.hyper = torch.zeros(4, device="cuda")
        self.step = torch.zeros(4, device="cuda")
        self.nr = len(ranges)
        self.ranges = dev(np.asarray(ranges, np.int64).reshape(-1, 2), np.int64) if ranges else None

    def set_hyper(self, lr, wd, clip, gs):
        self.ffi.check("set_hyper", self.L.jr_opt_set_hyper(self.hyper.data_ptr(), lr, wd, clip, gs, None))

    def prepare(self, G):
        self.ffi.check("sqnorm", self.L.jr_grad_sqnorm(G.data_ptr(), self.n, self.part.data_ptr(), self.ws, None))
        self.ffi.check("prepare", self.L.jr_opt_prepare(self.part.data_ptr(), self.n, self.hyper.data_ptr(),
                                                        self.step.data_ptr(), None))

    def read_step(self):
        """(scale, grad_norm, skipped, skipped_total)"""
        raw = host(self.step)
        u = raw.view(np.uint32)
        return f32(raw[0]), f32(raw[1]), int(u[2]), int(u[3])

    def s_dev(self):
        """jr_opt_prepare's fixed tree over the partials, restated in fp64."""
        p = host(self.part)
        red = np.zeros(256, np.float64)
        for t in range(min(256, p.size)):
            s = np.float64(0)
            for v in p[t::256]:
                s = s + v
            red[t] = s
        o = 128
        while o > 0:
            red[:o] = red[:o] + red[o:2 * o]
            o >>= 1
        return float(red[0])

    def update(self, opt, W, G, state, momentum=0.9):
        L, R = self.L, (self.ranges.data_ptr() if self.nr else None)
        hy, st, n = self.hyper.data_ptr(), self.step.data_ptr(), self.n
        if opt in ("nesterov", "momentum"):
            fn = L.jr_nesterov_update_ex if opt == "nesterov" else L.jr_momentum_update_ex
            rc = fn(W.data_ptr(), G.data_ptr(), state[0].data_ptr(), n, momentum, R, self.nr, hy, st, None)
        elif opt == "sgd":
            rc = L.jr_sgd_update_ex(W.data_ptr(), G.data_ptr(), n, R, self.nr, hy, st, None)
        else:
            rc = L.jr_adam_update_ex(W.data_ptr(), G.data_ptr(), state[0].data_ptr(), state[1].data_ptr(), n, 0.9,
                                     0.999, 1e-8, R, self.nr, hy, st, None)
        self.ffi.check(opt + "_ex", rc)


def mixed_gradient(n, seed):
    """Normal values of mixed magnitudes, 1e-20 ... 1e10."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 10, n)).astype(np.float32)


# ---- the norm
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 4 * 256 * 1024 + 3])
def test_sqnorm_and_prepare(n):
    g = mixed_gradient(n, n)
    r = Recipe(n)
    G = dev(g)
    r.set_hyper(0.1, 0.0, 0.0, 1.0)
    r.prepare(G)
    first = (host(r.part).tobytes(), host(r.step).tobytes())
    S = opt_ref.exact_sqsum(g)
    S_dev = r.s_dev()
    print(f"n={n} S={S!r} S_dev={S_dev!r} |diff|/S={abs(S_dev - S) / S:.3e} bound={n * 2.0 ** -53:.3e}")
    assert abs(S_dev - S) <= opt_ref.sqsum_bound(n, S)
    scale, gn, skipped, total = r.read_step()
    exact = math.sqrt(S)
    print(f"grad_norm={gn!r} exact={exact!r}")
    assert abs(float(gn) - exact) <= float(np.spacing(f32(exact)))          # within 1 ulp of fp32
    assert (scale, skipped, total) == (f32(1), 0, 0)
    r.part.zero_()
    r.prepare(G)                                                              # run to run: bitwise
    assert (host(r.part).tobytes(), host(r.step).tobytes()) == first


def test_prepare_clips_and_scales():
    n = 1025
    g = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    r = Recipe(n)
    G = dev(g)
    for clip, gs in ((0.0, 1.0), (1e9, 1.0), (2.0, 1.0), (2.0, 0.5), (1e9, 0.5)):
        r.set_hyper(0.1, 0.0, clip, gs)
        r.prepare(G)
        scale, gn, skipped, _ = r.read_step()
        want = opt_ref.prepare_ref(r.s_dev(), clip, gs)
        assert (scale, gn, skipped) == want, (clip, gs)
        if clip == 2.0:
            assert scale < f32(gs)


def test_non_finite_gradients_are_skipped_and_counted():
    n = 1025
    g = np.random.default_rng(6).standard_normal(n).astype(np.float32)
    r = Recipe(n)
    r.set_hyper(0.1, 0.0, 2.0, 1.0)
    bad = g.copy()
    bad[700] = np.inf
    r.prepare(dev(bad))
    scale, gn, skipped, total = r.read_step()
    assert (scale, skipped, total) == (f32(0), 1, 1) and not np.isfinite(gn)
    bad[700] = np.nan
    r.prepare(dev(bad))
    scale, gn, skipped, total = r.read_step()
    assert (scale, skipped, total) == (f32(0), 1, 2) and np.isnan(gn)
    r.prepare(dev(g))
    scale, gn, skipped, total = r.read_step()
    assert skipped == 0 and total == 2 and scale > 0 and np.isfinite(gn)      # a clean call does not reset the count
    big = np.full(n, 3e38, np.float32)                                        # finite, the norm overflows fp32
    r.prepare(dev(big))
    assert r.read_step()[2:] == (1, 3)


# ---- the updates
RANGE_CASES = {
    "split": (1030, [(0, 5), (6, 7), (9, 1027)]),       # a boundary inside a quad, one element, an undecayed tail
    "none": (1030, []),
    "all": (1030, [(0, 1030)]),
    # several blocks and grid-stride tiles (1024 elements each): ranges that straddle and end near tile edges, a decayed tail
    "tiles": (3 * 4096 + 5, [(0, 5), (6, 7), (9, 4100), (8190, 8200), (12286, 12293)]),
}


def _state0(opt, n):
    return {"nesterov": 1, "momentum": 1, "sgd": 0, "adam": 2}[opt] * (np.zeros(n, np.float32),)


@pytest.mark.parametrize("case", list(RANGE_CASES))
@pytest.mark.parametrize("opt", OPTS)
def test_update_ex_bitwise_restatement(opt, case):
    n, ranges = RANGE_CASES[case]
    rng = np.random.default_rng(11)
    w = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    mask = opt_ref.decay_mask(n, ranges)
    r = Recipe(n, ranges)
    W = dev(w)
    state = _state0(opt, n)
    S = [dev(s) for s in state]
    wd, clip = 0.01, 8.0
    for t, g in enumerate(grads, 1):
        lr = float(opt_ref.adam_alpha(1e-3, t)) if opt == "adam" else 3e-3 * t      # a changing rate, by set_hyper
        G = dev(g)
        r.set_hyper(lr, wd, clip, 1.0)
        r.prepare(G)
        r.update(opt, W, G, S)
        scale, gn, skipped, _ = r.read_step()
        assert skipped == 0 and scale < 1                                          # the norm (about 32) is clipped
        w, state = opt_ref.update_ref(opt, w, g, state, scale, lr, wd, mask)
        assert np.array_equal(host(W), w), (opt, case, t)
        for k, s in enumerate(state):
            assert np.array_equal(host(S[k]), s), (opt, case, t, k)
    # a skipped step writes nothing
    bad = grads[0].copy()
    bad[n // 2] = np.nan
    G = dev(bad)
    r.prepare(G)
    assert r.read_step()[2] == 1
    r.update(opt, W, G, S)
    assert np.array_equal(host(W), w)
    for k, s in enumerate(state):
        assert np.array_equal(host(S[k]), s)


@pytest.mark.parametrize("opt", OPTS)
def test_update_ex_equals_by_value_kernels(opt):
    """weight_decay 0, clip_norm 0, grad_scale 1: four steps bitwise the jr_*_update of the same inputs."""
    ffi, L = _lib()
    n = 10007
    rng = np.random.default_rng(12)
    w0 = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    r = Recipe(n, [(0, 5000)])          # ranges present, but no decay
    W, Wl = dev(w0), dev(w0)
    S, Sl = [dev(s) for s in _state0(opt, n)], [dev(s) for s in _state0(opt, n)]
    for t, g in enumerate(grads, 1):
        lr = float(opt_ref.adam_alpha(1e-3, t)) if opt == "adam" else 3e-3
        G = dev(g)
        r.set_hyper(lr, 0.0, 0.0, 1.0)
        r.prepare(G)
        r.update(opt, W, G, S)
        if opt in ("nesterov", "momentum"):
            fn = L.jr_nesterov_update if opt == "nesterov" else L.jr_momentum_update
            rc = fn(Wl.data_ptr(), G.data_ptr(), Sl[0].data_ptr(), n, lr, 0.9, 1.0, None)
        elif opt == "sgd":
            rc = L.jr_sgd_update(Wl.data_ptr(), G.data_ptr(), n, lr, 1.0, None)
        else:
            rc = L.jr_adam_update(Wl.data_ptr(), G.data_ptr(), Sl[0].data_ptr(), Sl[1].data_ptr(), n, lr, 0.9, 0.999,
                                  1e-8, 1.0, None)
        ffi.check(opt, rc)
        assert np.array_equal(host(W), host(Wl)), (opt, t)
        for a, b in zip(S, Sl):
            assert np.array_equal(host(a), host(b)), (opt, t)


# ---- the by-value calls: the same body with lr and grad_scale as arguments, no decay, never skipped
def _by_value(L, opt, W, G, S, n, lr, grad_scale):
    if opt in ("nesterov", "momentum"):
        fn = L.jr_nesterov_update if opt == "nesterov" else L.jr_momentum_update
        return fn(W.data_ptr(), G.data_ptr(), S[0].data_ptr(), n, lr, 0.9, grad_scale, None)
    if opt == "sgd":
        return L.jr_sgd_update(W.data_ptr(), G.data_ptr(), n, lr, grad_scale, None)
    return L.jr_adam_update(W.data_ptr(), G.data_ptr(), S[0].data_ptr(), S[1].data_ptr(), n, lr, 0.9, 0.999, 1e-8,
                            grad_scale, None)


def _two_steps_by_value(opt, n, grad_scale, place):
    """Two steps from non-zero state against opt_ref.update_ref (scale = grad_scale, weight decay 0);
    place(array) -> the device tensor the call gets."""
    ffi, L = _lib()
    rng = np.random.default_rng(13)
    w = rng.standard_normal(n).astype(np.float32)
    state = tuple(rng.standard_normal(n).astype(np.float32) ** (2 if k else 1)       # Adam's v is a mean of squares
                  for k in range(len(_state0(opt, n))))
    W, S = place(w), [place(s) for s in state]
    for t in (1, 2):
        g = rng.standard_normal(n).astype(np.float32)
        lr = float(opt_ref.adam_alpha(1e-3, t)) if opt == "adam" else 3e-3
        G = place(g)
        ffi.check(opt, _by_value(L, opt, W, G, S, n, lr, grad_scale))
        w, state = opt_ref.update_ref(opt, w, g, state, grad_scale, lr, 0.0, None)
        assert np.array_equal(host(W), w), (opt, n, t)
        for k, s in enumerate(state):
            assert np.array_equal(host(S[k]), s), (opt, n, t, k)
        assert np.array_equal(host(G), g)


# no quad, tail only, one quad, quad + tail, one tile of 256 quads - and + one element, several blocks with a tail
@pytest.mark.parametrize("grad_scale", [1.0, 0.3])       # 0.3: the first multiply rounds
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 3 * 4096 + 5])
@pytest.mark.parametrize("opt", OPTS)
def test_by_value_bitwise_restatement(opt, n, grad_scale):
    _two_steps_by_value(opt, n, grad_scale, dev)


@pytest.mark.parametrize("n", [5, 1025])
@pytest.mark.parametrize("opt", ["momentum", "sgd", "adam"])
def test_by_value_accepts_buffers_off_16_bytes(opt, n):
    """Every buffer a [1:] view (4-byte, not 16-byte aligned): the same values, the element before each view untouched."""
    bases = []

    def place(a):
        base = dev(np.concatenate([np.float32([-7.5]), a]))
        bases.append(base)
        assert base.data_ptr() % 16 == 0 and base[1:].data_ptr() % 16 == 4
        return base[1:]
    _two_steps_by_value(opt, n, 0.3, place)
    assert bases and all(host(b)[0] == np.float32(-7.5) for b in bases)


# ---- the Engine: 107^2, B = 2, conv_math="x8", nesterov
LR, MOM = 3e-3, 0.9


@pytest.fixture(scope="module")
def batch():
    from jr import synth
    return synth.fundus_batch(0, 2, 107), np.array([[1.0], [0.0]], np.float32)


def _engine(batch, **kw):
    from jr.engine import Engine
    eng = Engine(2, 107, 107, seed=4, conv_math=kw.pop("conv_math", "x8"), lr=LR, momentum=MOM, **kw)
    eng.set_batch(*batch)
    return eng


def _state(eng):
    eng.synchronize()
    return eng.params.cpu().numpy().copy(), eng.accum.cpu().numpy().copy()


def _grads(eng):
    eng.forward()
    eng.backward()
    eng.synchronize()
    return eng.grads.cpu().numpy().copy()


@pytest.fixture(scope="module")
def default_run(batch):
    """Three steps of the default engine: (params, momentum) after each, and the first step's gradient."""
    eng = _engine(batch)
    out, g0 = [], None
    for t in range(3):
        g = _grads(eng)
        g0 = g if g0 is None else g0
        eng.apply_update()
        out.append(_state(eng))
    with pytest.raises(ValueError):
        eng.set_lr(1e-3)                # the default path binds the rate
    with pytest.raises(ValueError):
        eng.opt_step()
    eng.close()
    return out, g0


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_engine_device_path_is_bitwise_the_default(batch, default_run):
    """(a), (i), then on the same engine (f) and (e)."""
    ref, g0 = default_run
    eng = _engine(batch, device_lr=True)
    opt = eng._build_calls(2)[2]
    assert [c.name for c in opt] == ["grad_sqnorm", "opt_prepare", "nesterov_update_ex"]            # (i)
    assert [c.fn.__name__ for c in opt] == ["jr_grad_sqnorm", "jr_opt_prepare", "jr_nesterov_update_ex"]
    assert all(c.lane == 0 for c in opt) and ("gnorm",) in opt[0].writes and ("gnorm",) in opt[2].reads
    for t in range(3):                                                                                # (a)
        g = _grads(eng)
        eng.apply_update()
        assert _same(_state(eng), ref[t]), t
        norm, scale, skipped, total = eng.opt_step()
        assert (scale, skipped, total) == (1.0, 0, 0)
        if t == 0:
            S = opt_ref.exact_sqsum(g)
            assert np.array_equal(g, g0)
            assert abs(norm - math.sqrt(S)) <= float(np.spacing(f32(math.sqrt(S))))
    mask = opt_ref.decay_mask(eng.nparam, eng.opt_ranges)
    # (f) the data-parallel 1/world, without further processes
    w, a = _state(eng)
    g = _grads(eng)
    eng.apply_update(grad_scale=0.5)
    norm, scale, skipped, _ = eng.opt_step()
    assert scale == 0.5 and skipped == 0
    assert abs(norm - 0.5 * math.sqrt(opt_ref.exact_sqsum(g))) <= float(np.spacing(f32(norm)))   # (the halving is exact)
    w, (a,) = opt_ref.update_ref("nesterov", w, g, (a,), scale, LR, 0.0, mask, momentum=MOM)
    assert _same(_state(eng), (w, a))
    # (e) one NaN in the gradient: the step is skipped, the next one is normal
    eng.forward()
    eng.backward()
    with torch.cuda.stream(eng.stream):
        eng.grads[5] = float("nan")
    eng.apply_update()
    assert _same(_state(eng), (w, a))
    norm, scale, skipped, total = eng.opt_step()
    assert math.isnan(norm) and (scale, skipped, total) == (0.0, 1, 1)
    g = _grads(eng)
    eng.apply_update()
    norm, scale, skipped, total = eng.opt_step()
    assert (scale, skipped, total) == (1.0, 0, 1) and np.isfinite(g).all()
    w, (a,) = opt_ref.update_ref("nesterov", w, g, (a,), scale, LR, 0.0, mask, momentum=MOM)
    assert _same(_state(eng), (w, a))
    eng.close()


def test_engine_clip_norm(batch, default_run):
    """(b) a clip far above the norm changes nothing; (c) half the first norm: the restatement."""
    ref, g0 = default_run
    eng = _engine(batch, clip_norm=1e30)
    first = None
    for t in range(3):
        eng.train_step()
        assert _same(_state(eng), ref[t]), t
        first = eng.opt_step()[0] if first is None else first     # the first step's measured norm
    eng.close()
    eng = _engine(batch, clip_norm=0.5 * first)
    mask = opt_ref.decay_mask(eng.nparam, eng.opt_ranges)
    w, a = _state(eng)
    for t in range(3):
        g = _grads(eng)
        eng.apply_update()
        norm, scale, skipped, _ = eng.opt_step()
        S = opt_ref.exact_sqsum(g)
        print(f"step {t}: grad_norm={norm!r} exact={math.sqrt(S)!r} scale={scale!r}")
        assert abs(norm - math.sqrt(S)) <= float(np.spacing(f32(math.sqrt(S))))
        assert skipped == 0
        if t == 0:
            assert np.array_equal(g, g0) and abs(scale - 0.5) <= 2.0 ** -22
        assert f32(scale) == (f32(f32(0.5 * first) / f32(norm)) if norm > f32(0.5 * first) else f32(1))
        w, (a,) = opt_ref.update_ref("nesterov", w, g, (a,), scale, LR, 0.0, mask, momentum=MOM)
        assert _same(_state(eng), (w, a)), t
    assert not _same((w, a), ref[2])
    eng.close()


def test_engine_weight_decay(batch):
    """(d) filters follow the restatement, betas and the bias the undecayed update."""
    wd = 4e-5
    eng = _engine(batch, weight_decay=wd)
    mask = opt_ref.decay_mask(eng.nparam, eng.opt_ranges)
    w, a = _state(eng)
    for t in range(3):
        g = _grads(eng)
        eng.apply_update()
        norm, scale, skipped, _ = eng.opt_step()
        assert (scale, skipped) == (1.0, 0)
        plain_w, (plain_a,) = opt_ref.update_ref("nesterov", w, g, (a,), scale, LR, 0.0, mask, momentum=MOM)
        w, (a,) = opt_ref.update_ref("nesterov", w, g, (a,), scale, LR, wd, mask, momentum=MOM)
        got_w, got_a = _state(eng)
        assert np.array_equal(got_w[~mask], plain_w[~mask]) and np.array_equal(got_a[~mask], plain_a[~mask]), t
        assert np.array_equal(got_w[mask], w[mask]) and np.array_equal(got_a[mask], a[mask]), t
        assert not np.array_equal(w[mask], plain_w[mask])
    eng.close()


def test_engine_capture_replays_under_a_changing_rate(batch):
    """(g) capture, then three replays with another rate before each == three eager steps with those rates."""
    rates = (1e-3, 5e-3, 2e-3)
    eager = _engine(batch, device_lr=True)
    graph = _engine(batch, device_lr=True)
    graph.capture()
    for lr in rates:
        eager.set_lr(lr)
        eager.train_step()
        graph.set_lr(lr)
        graph.replay()
        assert _same(_state(eager), _state(graph)), lr
    fixed = _engine(batch, device_lr=True)
    for _ in rates:
        fixed.train_step()
    assert not _same(_state(fixed), _state(eager))          # the rates did change the steps
    assert eager.opt_step() == graph.opt_step()
    for e in (eager, graph, fixed):
        e.close()


def test_engine_bf16_recipe(batch):
    """(h) bf16 storage, weight decay and clipping on: the restatement on the engine's own fp32 gradient."""
    wd = 4e-5
    probe = _engine(batch, conv_math=None, dtype="bf16", device_lr=True)
    first = math.sqrt(opt_ref.exact_sqsum(_grads(probe)))
    probe.close()
    eng = _engine(batch, conv_math=None, dtype="bf16", weight_decay=wd, clip_norm=0.5 * first)
    mask = opt_ref.decay_mask(eng.nparam, eng.opt_ranges)
    w, a = _state(eng)
    g = _grads(eng)
    assert g.dtype == np.float32
    eng.apply_update()
    norm, scale, skipped, _ = eng.opt_step()
    assert skipped == 0 and abs(scale - 0.5) <= 2.0 ** -22
    assert abs(norm - math.sqrt(opt_ref.exact_sqsum(g))) <= float(np.spacing(f32(norm)))
    w, (a,) = opt_ref.update_ref("nesterov", w, g, (a,), scale, LR, wd, mask, momentum=MOM)
    assert _same(_state(eng), (w, a))
    eng.close()
