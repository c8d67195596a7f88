"""RMSProp and the moving average of the weights on the GPU, through the
C-ABI and the Engine.  Every comparison is bitwise against the numpy
restatements (tests/ema_ref.py): jr_opt.hip is built with contraction off and
uses correctly rounded sqrt and division.

* jr_ema_set / jr_ema_prepare / jr_ema_update: four steps at sizes around a
  quad, a tile and the 8192-block grid's wrap; the device counter and warm-up
  decay; a skipped step leaves every byte alone; a misaligned shadow is refused;
* jr_rmsprop_update_ex over the recipe test's decay-range cases, against the
  by-value kernel when the recipe changes nothing; jr_rmsprop_update at sizes
  around a quad and a tile and on buffers off 16 bytes;
* the Engine: unchanged call lists without the new keywords; the average after
  eager, skipped and replayed steps; averaged_weights(); RMSProp eager and
  replayed under a changing rate; bf16 storage; the audit of one EMA step.
"""
import contextlib

import numpy as np
import pytest

import ema_ref
import opt_ref
from opt_ref import f32
from test_gpu_opt_recipe import RANGE_CASES, Recipe, _lib, dev, host, mixed_gradient

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

JR_ERR_INVALID = -1


# ---- the average, C-ABI
class Ema:
    """A jr_ema_state on the device."""

    def __init__(self, decay, warm, updates=0):
        self.ffi, self.L = _lib()
        self.state = torch.zeros(4, device="cuda")
        self.ffi.check("ema_set", self.L.jr_ema_set(self.state.data_ptr(), decay, int(warm), updates, None))

    def read(self):
        raw = host(self.state)
        u = raw.view(np.uint32)
        return {"decay": f32(raw[0]), "one_minus_decay": f32(raw[1]), "updates": int(u[2]), "warm": int(u[3])}

    def step(self, S, W, n, step=None):
        sp = None if step is None else step.data_ptr()
        self.ffi.check("ema_prepare", self.L.jr_ema_prepare(self.state.data_ptr(), sp, None))
        self.ffi.check("ema_update", self.L.jr_ema_update(S.data_ptr(), W.data_ptr(), n, self.state.data_ptr(), sp, None))


def _same_state(a, b):
    return all(a[k] == b[k] for k in ("decay", "one_minus_decay", "updates", "warm"))


# no quad, tail only, one quad, quad + tail, one tile of 256 quads - and + one element, many blocks with a tail, and the
# smallest size at which the 8192-block grid takes a second tile (block 0 alone) and a tail is left
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 1024 * 1024 + 3, 4 * 256 * 8192 + 4 * 256 + 3])
def test_ema_update_bitwise_restatement(n):
    shadow = mixed_gradient(n, n + 1)
    e = Ema(0.9999, True)
    ref = ema_ref.ema_set_ref(0.9999, True)
    assert _same_state(e.read(), ref)
    S = dev(shadow)
    for t in range(4):
        w = mixed_gradient(n, 100 * n + t)
        W = dev(w)
        e.step(S, W, n)
        shadow, ref = ema_ref.ema_step_ref(shadow, w, ref)
        assert _same_state(e.read(), ref), t
        assert np.array_equal(host(S), shadow), (n, t)
        assert np.array_equal(host(W), w)


@pytest.mark.parametrize("warm", [True, False])
def test_ema_counter_and_decay(warm):
    e = Ema(0.75, warm, updates=0)
    ref = ema_ref.ema_set_ref(0.75, warm)
    seen = []
    for t in range(30):          # (1 + t) / (10 + t) passes 0.75 at t = 26
        e.ffi.check("ema_prepare", e.L.jr_ema_prepare(e.state.data_ptr(), None, None))
        ref = ema_ref.ema_prepare_ref(ref)
        got = e.read()
        assert _same_state(got, ref), t
        seen.append(float(got["one_minus_decay"]))
    if warm:
        assert seen[0] == float(f32(1) - f32(0.1)) and seen[25] > 0.25 and seen[26] == 0.25 and seen[29] == 0.25
    else:
        assert set(seen) == {0.25}
    # a counter set from a checkpoint: 2^24 + 1 updates (the fp32 of it rounds), and the largest
    for updates in (2 ** 24 + 1, 2 ** 32 - 2):
        e = Ema(0.9999, True, updates=updates)
        ref = ema_ref.ema_prepare_ref(ema_ref.ema_set_ref(0.9999, True, updates))
        e.ffi.check("ema_prepare", e.L.jr_ema_prepare(e.state.data_ptr(), None, None))
        assert _same_state(e.read(), ref) and ref["updates"] == updates + 1


def test_ema_skipped_step_writes_nothing():
    n = 1025
    rng = np.random.default_rng(7)
    g, w, shadow = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    r = Recipe(n)
    r.set_hyper(0.1, 0.0, 2.0, 1.0)
    e = Ema(0.5, True)
    S, W = dev(shadow), dev(w)
    r.prepare(dev(g))
    e.step(S, W, n, r.step)                  # a clean step first: counted, averaged
    shadow, ref = ema_ref.ema_step_ref(shadow, w, ema_ref.ema_set_ref(0.5, True))
    assert np.array_equal(host(S), shadow) and e.read()["updates"] == 1 and r.read_step()[2:] == (0, 0)
    bad = g.copy()
    bad[700] = np.nan
    r.prepare(dev(bad))
    before = host(S).tobytes()
    e.step(S, W, n, r.step)
    assert r.read_step()[2:] == (1, 1)       # skipped, skipped_total advanced
    got = e.read()
    assert host(S).tobytes() == before and got["updates"] == 1 and got["one_minus_decay"] == 0
    assert _same_state(got, ema_ref.ema_prepare_ref(ref, skipped=1))
    r.prepare(dev(g))                        # the next clean step continues from the count
    e.step(S, W, n, r.step)
    shadow, ref = ema_ref.ema_step_ref(shadow, w, ref)
    assert np.array_equal(host(S), shadow) and _same_state(e.read(), ref) and ref["updates"] == 2


def test_ema_update_refuses_misaligned_buffers():
    ffi, L = _lib()
    n = 1025
    e = Ema(0.5, False)
    base, W = dev(np.arange(n + 1, dtype=np.float32)), dev(np.zeros(n + 1, np.float32))
    assert base.data_ptr() % 16 == 0
    st = e.state.data_ptr()
    assert L.jr_ema_update(base[1:].data_ptr(), W.data_ptr(), n, st, None, None) == JR_ERR_INVALID
    assert "16-byte" in ffi.last_error()
    assert L.jr_ema_update(base.data_ptr(), W[1:].data_ptr(), n, st, None, None) == JR_ERR_INVALID
    assert L.jr_ema_update(None, W.data_ptr(), n, st, None, None) == JR_ERR_INVALID
    assert L.jr_ema_update(base.data_ptr(), W.data_ptr(), n, None, None, None) == JR_ERR_INVALID
    assert L.jr_ema_set(st, 1.0, 1, 0, None) == JR_ERR_INVALID          # decay in [0, 1)
    assert L.jr_ema_prepare(None, None, None) == JR_ERR_INVALID
    assert np.array_equal(host(base), np.arange(n + 1, dtype=np.float32))   # no launch


# ---- RMSProp, C-ABI
RHO, RMOM, REPS = 0.9, 0.9, 1.0


def _rms_ex(r, W, G, MOM, MS):
    R = r.ranges.data_ptr() if r.nr else None
    r.ffi.check("rmsprop_ex", r.L.jr_rmsprop_update_ex(W.data_ptr(), G.data_ptr(), MOM.data_ptr(), MS.data_ptr(), r.n, RHO,
                                                       RMOM, REPS, R, r.nr, r.hyper.data_ptr(), r.step.data_ptr(), None))


@pytest.mark.parametrize("case", list(RANGE_CASES))
def test_rmsprop_ex_bitwise_restatement(case):
    n, ranges = RANGE_CASES[case]
    rng = np.random.default_rng(11)
    w = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    mask = opt_ref.decay_mask(n, ranges)
    r = Recipe(n, ranges)
    mom, ms = np.zeros(n, np.float32), np.ones(n, np.float32)      # TF's initial slots
    W, MOM, MS = dev(w), dev(mom), dev(ms)
    wd, clip = 0.01, 8.0
    for t, g in enumerate(grads, 1):
        lr = 0.045 * t                                             # a changing rate, by set_hyper
        G = dev(g)
        r.set_hyper(lr, wd, clip, 1.0)
        r.prepare(G)
        _rms_ex(r, W, G, MOM, MS)
        scale, gn, skipped, _ = r.read_step()
        assert skipped == 0 and scale < 1                          # the norm (about 32) is clipped
        w, mom, ms = ema_ref.rmsprop_ref(w, g, mom, ms, scale, lr, wd, mask, rho=RHO, momentum=RMOM, eps=REPS)
        for name, a, b in (("w", W, w), ("mom", MOM, mom), ("ms", MS, ms)):
            assert np.array_equal(host(a), b), (case, t, name)
    bad = grads[0].copy()                                          # a skipped step writes nothing
    bad[n // 2] = np.nan
    G = dev(bad)
    r.prepare(G)
    assert r.read_step()[2] == 1
    _rms_ex(r, W, G, MOM, MS)
    assert np.array_equal(host(W), w) and np.array_equal(host(MOM), mom) and np.array_equal(host(MS), ms)


def test_rmsprop_ex_equals_by_value_kernel():
    """weight_decay 0, clip_norm 0, grad_scale 1: four steps bitwise jr_rmsprop_update of the same inputs."""
    ffi, L = _lib()
    n = 10007
    rng = np.random.default_rng(12)
    w0 = rng.standard_normal(n).astype(np.float32)
    r = Recipe(n, [(0, 5000)])          # ranges present, but no decay
    one = np.ones(n, np.float32)
    W, MOM, MS = dev(w0), dev(0 * one), dev(one)
    Wl, MOMl, MSl = dev(w0), dev(0 * one), dev(one)
    for t in range(4):
        G = dev(rng.standard_normal(n).astype(np.float32))
        r.set_hyper(0.045, 0.0, 0.0, 1.0)
        r.prepare(G)
        _rms_ex(r, W, G, MOM, MS)
        ffi.check("rmsprop", L.jr_rmsprop_update(Wl.data_ptr(), G.data_ptr(), MOMl.data_ptr(), MSl.data_ptr(), n, 0.045,
                                                 RHO, RMOM, REPS, 1.0, None))
        for a, b in ((W, Wl), (MOM, MOMl), (MS, MSl)):
            assert np.array_equal(host(a), host(b)), t
    assert not np.array_equal(host(W), w0)


def _two_rmsprop_steps(n, grad_scale, place, eps=REPS):
    """Two by-value steps from non-zero state against the restatement; place(array) -> the device tensor."""
    ffi, L = _lib()
    rng = np.random.default_rng(13)
    w = rng.standard_normal(n).astype(np.float32)
    mom = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    ms = rng.standard_normal(n).astype(np.float32) ** 2            # a mean of squares
    W, MOM, MS = place(w), place(mom), place(ms)
    for t in (1, 2):
        g = rng.standard_normal(n).astype(np.float32)
        G = place(g)
        ffi.check("rmsprop", L.jr_rmsprop_update(W.data_ptr(), G.data_ptr(), MOM.data_ptr(), MS.data_ptr(), n, 0.045,
                                                 RHO, RMOM, eps, grad_scale, None))
        w, mom, ms = ema_ref.rmsprop_ref(w, g, mom, ms, grad_scale, 0.045, rho=RHO, momentum=RMOM, eps=eps)
        for name, a, b in (("w", W, w), ("mom", MOM, mom), ("ms", MS, ms)):
            assert np.array_equal(host(a), b), (n, t, name)
        assert np.array_equal(host(G), g)


@pytest.mark.parametrize("grad_scale", [1.0, 0.3])       # 0.3: the first multiply rounds
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 3 * 4096 + 5])
def test_rmsprop_by_value_bitwise_restatement(n, grad_scale):
    _two_rmsprop_steps(n, grad_scale, dev)


def test_rmsprop_small_epsilon_exercises_sqrt_and_division():
    """eps = 1e-7: the root and the quotient span their whole range instead of sitting near 1."""
    _two_rmsprop_steps(3 * 4096 + 5, 0.3, dev, eps=1e-7)


@pytest.mark.parametrize("n", [5, 1025])
def test_rmsprop_by_value_accepts_buffers_off_16_bytes(n):
    bases = []

    def place(a):
        base = dev(np.concatenate([np.float32([-7.5]), a]))
        bases.append(base)
        assert base.data_ptr() % 16 == 0 and base[1:].data_ptr() % 16 == 4
        return base[1:]
    _two_rmsprop_steps(n, 0.3, place)
    assert bases and all(host(b)[0] == np.float32(-7.5) for b in bases)


def test_rmsprop_ex_refuses_misaligned_buffers():
    ffi, L = _lib()
    r = Recipe(16)
    a = [dev(np.zeros(17, np.float32)) for _ in range(4)]
    p = [t.data_ptr() for t in a]
    hy, st = r.hyper.data_ptr(), r.step.data_ptr()
    assert L.jr_rmsprop_update_ex(p[0] + 4, p[1], p[2], p[3], 16, RHO, RMOM, REPS, None, 0, hy, st, None) == JR_ERR_INVALID
    assert L.jr_rmsprop_update_ex(p[0], p[1], p[2], None, 16, RHO, RMOM, REPS, None, 0, hy, st, None) == JR_ERR_INVALID


# ---- the Engine: 107^2, B = 2, conv_math="x8"
LR = 3e-3


@pytest.fixture(scope="module")
def batch():
    from jr import synth
    return synth.fundus_batch(0, 2, 107), np.array([[1.0], [0.0]], np.float32)


def _engine(batch, **kw):
    from jr.engine import Engine
    eng = Engine(2, 107, 107, seed=4, conv_math=kw.pop("conv_math", "x8"), lr=kw.pop("lr", LR), **kw)
    eng.set_batch(*batch)
    return eng


def _bwd(eng, nan=False):
    eng.forward()
    eng.backward()
    if nan:
        with torch.cuda.stream(eng.stream):
            eng.grads[5] = float("nan")


def _internal(eng, *names):
    eng.synchronize()
    return tuple(getattr(eng, n).cpu().numpy().copy() for n in names)


def test_call_lists_without_the_keywords_are_unchanged(batch):
    from jr.engine import Engine
    from jr.lanes import signature
    for kw in ({}, {"device_lr": True}, {"optimizer": "adam"}):
        a = Engine(2, 107, 107, seed=4, conv_math="x8", **kw)
        b = Engine(2, 107, 107, seed=4, conv_math="x8", weight_ema=None, weight_ema_warm=True, rmsprop_rho=0.5, **kw)
        for la, lb in zip(a._build_calls(2)[:3], b._build_calls(2)[:3]):
            assert signature(la) == signature(lb), kw
        assert b.ema is None and b.ema_state is None
        with pytest.raises(ValueError):
            b.ema_numpy()
        a.close()
        b.close()
    e = Engine(2, 107, 107, seed=4, conv_math="x8", weight_ema=0.9, bn_moving=0.99, clip_norm=2.0)
    opt = e._build_calls(2)[2]
    assert [c.name for c in opt] == ["grad_sqnorm", "opt_prepare", "nesterov_update_ex", "ema_prepare", "ema_update",
                                     "bn_moving"]
    assert [c.fn.__name__ for c in opt[3:5]] == ["jr_ema_prepare", "jr_ema_update"]
    assert all(c.lane == 0 for c in opt)
    assert ("gnorm",) in opt[3].reads and ("ema",) in opt[3].writes
    assert {("p",), ("ema",), ("gnorm",)} <= set(opt[4].reads) and list(opt[4].writes) == [("ema",)]
    assert opt[4].nbytes == 12 * e.nparam
    e.close()
    e = Engine(2, 107, 107, seed=4, conv_math="x8", weight_ema=0.9)
    opt = e._build_calls(2)[2]
    assert [c.name for c in opt] == ["nesterov", "ema_prepare", "ema_update"]
    assert opt[1].args[1] is None and opt[2].args[4] is None and ("gnorm",) not in opt[2].reads   # no step struct
    e.close()
    with pytest.raises(ValueError):
        Engine(2, 107, 107, conv_math="x8", weight_ema=1.0)


@pytest.mark.parametrize("path", ["by_value", "device"])
def test_engine_average_follows_the_restatement(batch, path):
    """Three eager steps; device path: every step clipped, the second one skipped by a NaN gradient."""
    device = path == "device"
    eng = _engine(batch, weight_ema=0.9, **({"clip_norm": 1e-3} if device else {}))
    st = ema_ref.ema_set_ref(0.9, True)
    shadow = eng.ema_numpy()
    assert np.array_equal(shadow, eng.params_numpy()) and eng.ema_updates() == 0
    for t in range(3):
        _bwd(eng, nan=device and t == 1)
        eng.apply_update()
        skipped = 0
        if device:
            _, scale, skipped, _ = eng.opt_step()
            assert skipped == int(t == 1) and (skipped or 0 < scale < 1)
        shadow, st = ema_ref.ema_step_ref(shadow, eng.params_numpy(), st, skipped)
        assert np.array_equal(eng.ema_numpy(), shadow), t
        assert eng.ema_updates() == st["updates"]
    assert eng.ema_updates() == (2 if device else 3)
    assert not np.array_equal(shadow, eng.params_numpy())
    # a saved average goes back in with its count; new parameters restart it
    saved = shadow * np.float32(0.5)         # (exact; the layout's padding stays zero)
    eng.load_ema(saved, 41)
    assert np.array_equal(eng.ema_numpy(), saved) and eng.ema_updates() == 41
    eng.load_params(shadow)
    assert np.array_equal(eng.ema_numpy(), shadow) and eng.ema_updates() == 0
    eng.close()


@pytest.mark.parametrize("path", ["by_value", "device"])
def test_engine_average_replayed_equals_eager(batch, path):
    kw = {"clip_norm": 1e-3} if path == "device" else {}
    eager = _engine(batch, weight_ema=0.9, **kw)
    graph = _engine(batch, weight_ema=0.9, **kw)
    graph.capture()
    for t in range(3):
        eager.train_step()
        graph.replay()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_internal(eager, "params", "accum", "ema", "ema_state"),
                                                              _internal(graph, "params", "accum", "ema", "ema_state"))), t
    assert graph.ema_updates() == 3
    eager.close()
    graph.close()


def test_averaged_weights(batch):
    eng = _engine(batch, weight_ema=0.9)
    for _ in range(2):
        eng.train_step()
    params, ema = _internal(eng, "params", "ema")
    avg = eng.ema_numpy()
    eng.forward()
    trained = eng.predictions().copy()
    with eng.averaged_weights() as inside:
        assert inside is eng
        eng.forward()
        got = eng.predictions().copy()
        assert np.array_equal(eng.params_numpy(), avg)
        for call in (eng.train_step, eng.apply_update, eng.replay, eng.capture):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(RuntimeError):
            with eng.averaged_weights():
                pass
    after = _internal(eng, "params", "ema")
    assert after[0].tobytes() == params.tobytes() and after[1].tobytes() == ema.tobytes()
    fresh = _engine(batch)
    fresh.load_params(avg)
    fresh.forward()
    assert np.array_equal(got, fresh.predictions())
    assert not np.array_equal(got, trained)
    eng.forward()                               # and the trained weights predict what they did
    assert np.array_equal(eng.predictions(), trained)
    with contextlib.suppress(KeyError):         # an exception inside still swaps back
        with eng.averaged_weights():
            raise KeyError
    assert _internal(eng, "params")[0].tobytes() == params.tobytes()
    eng.train_step()                            # and training goes on
    eng.close()
    fresh.close()


def test_engine_rmsprop_by_value_follows_the_restatement(batch):
    """Keras layout throughout: the update is element-wise, the layouts differ by a permutation."""
    eng = _engine(batch, optimizer="rmsprop", lr=0.045)
    keras = lambda t: eng.plan.to_keras(eng.g, t.cpu().numpy())     # noqa: E731
    w = eng.params_numpy()
    eng.synchronize()
    mom, ms = keras(eng.accum), keras(eng.adam_v)
    assert not eng.accum.any().item() and bool((eng.adam_v == 1).all().item())   # TF's initial slots
    assert not mom.any() and np.all((ms == 1) | (w == 0))                         # (the Keras layout's padding is zero)
    assert [c.name for c in eng._build_calls(2)[2]] == ["rmsprop"]
    for t in range(3):
        _bwd(eng)
        g = eng.grads_numpy()
        eng.apply_update(grad_scale=0.5 if t == 2 else 1.0)
        w, mom, ms = ema_ref.rmsprop_ref(w, g, mom, ms, 0.5 if t == 2 else 1.0, 0.045)
        assert np.array_equal(eng.params_numpy(), w), t
        assert np.array_equal(keras(eng.accum), mom) and np.array_equal(keras(eng.adam_v), ms), t
    eng.load_params(w)
    eng.synchronize()
    assert not eng.accum.any().item() and bool((eng.adam_v == 1).all().item())       # the slots restart
    eng.close()


def test_engine_rmsprop_recipe_follows_the_restatement(batch):
    """Weight decay and clipping: the internal layout, where the decay ranges live."""
    wd = 4e-5
    eng = _engine(batch, optimizer="rmsprop", lr=0.045, weight_decay=wd, clip_norm=1e-3, rmsprop_rho=0.95,
                  rmsprop_momentum=0.8, rmsprop_eps=0.1)
    mask = opt_ref.decay_mask(eng.nparam, eng.opt_ranges)
    assert [c.name for c in eng._build_calls(2)[2]] == ["grad_sqnorm", "opt_prepare", "rmsprop_update_ex"]
    w, mom, ms = _internal(eng, "params", "accum", "adam_v")
    for t in range(3):
        _bwd(eng, nan=t == 1)
        (g,) = _internal(eng, "grads")
        eng.apply_update()
        _, scale, skipped, _ = eng.opt_step()
        assert skipped == int(t == 1)
        w, mom, ms = ema_ref.rmsprop_ref(w, g, mom, ms, scale, 0.045, wd, mask, skipped, rho=0.95, momentum=0.8, eps=0.1)
        assert all(np.array_equal(a, b) for a, b in zip(_internal(eng, "params", "accum", "adam_v"), (w, mom, ms))), t
    eng.close()


def test_engine_rmsprop_replays_under_a_changing_rate(batch):
    rates = (0.045, 0.01, 0.03)
    eager = _engine(batch, optimizer="rmsprop", device_lr=True)
    graph = _engine(batch, optimizer="rmsprop", device_lr=True)
    graph.capture()
    for lr in rates:
        eager.set_lr(lr)
        eager.train_step()
        graph.set_lr(lr)
        graph.replay()
        assert all(np.array_equal(a, b) for a, b in zip(_internal(eager, "params", "accum", "adam_v"),
                                                        _internal(graph, "params", "accum", "adam_v"))), lr
    fixed = _engine(batch, optimizer="rmsprop", device_lr=True)
    for _ in rates:
        fixed.train_step()
    assert not np.array_equal(_internal(fixed, "params")[0], _internal(eager, "params")[0])
    # the by-value path captures too: RMSProp has no per-step host scalar
    byval, again = _engine(batch, optimizer="rmsprop"), _engine(batch, optimizer="rmsprop")
    again.capture()
    for _ in range(2):
        byval.train_step()
        again.replay()
    assert all(np.array_equal(a, b) for a, b in zip(_internal(byval, "params", "accum", "adam_v"),
                                                    _internal(again, "params", "accum", "adam_v")))
    for e in (eager, graph, fixed, byval, again):
        e.close()


def test_engine_bf16_rmsprop_and_average(batch):
    """bf16 storage: both restatements on the engine's own fp32 gradient and parameters."""
    wd = 4e-5
    eng = _engine(batch, conv_math=None, dtype="bf16", optimizer="rmsprop", lr=0.045, weight_decay=wd, clip_norm=1e-3,
                  weight_ema=0.9)
    mask = opt_ref.decay_mask(eng.nparam, eng.opt_ranges)
    w, mom, ms, shadow = _internal(eng, "params", "accum", "adam_v", "ema")
    st = ema_ref.ema_set_ref(0.9, True)
    for t in range(2):
        _bwd(eng)
        (g,) = _internal(eng, "grads")
        assert g.dtype == np.float32
        eng.apply_update()
        _, scale, skipped, _ = eng.opt_step()
        assert skipped == 0 and 0 < scale < 1
        w, mom, ms = ema_ref.rmsprop_ref(w, g, mom, ms, scale, 0.045, wd, mask)
        shadow, st = ema_ref.ema_step_ref(shadow, w, st)
        assert all(np.array_equal(a, b) for a, b in zip(_internal(eng, "params", "accum", "adam_v", "ema"),
                                                        (w, mom, ms, shadow))), t
    eng.close()


def test_audit_of_one_ema_step(batch):
    """The update phase of a step with the average on, serial, shadowed and poisoned:
    every call writes inside its declared writes and reads nothing it does not declare."""
    import step_audit
    eng = _engine(batch, weight_ema=0.9, clip_norm=2.0, bn_moving=0.99, optimizer="rmsprop")
    eng.train_step()
    _bwd(eng)
    eng.synchronize()
    torch.cuda.synchronize()
    lists = eng._build_calls(2)
    audit = step_audit.SerialAudit(eng.universe(lists), lambda k: eng.regions(k, lists), torch.cuda.synchronize)
    wfind, rfind = audit.run(list(lists[2]))
    assert ("ema",) in audit.keys
    assert not wfind, "\n".join(wfind)
    assert not rfind, "\n".join(rfind)
    eng.synchronize()
    assert eng.ema_updates() == 2
    eng.close()
