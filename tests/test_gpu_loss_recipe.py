"""The loss recipe (label smoothing, class weights, the focal term) and
dropout on the GPU, through the C-ABI and the Engine, against tests/loss_ref.py.

* jr_head_fwd_ex / jr_head_bwd_ex against the fp64 models: logits, dfeat, dW,
  db within 1e-5 of max|ref|; with gamma = 0 probs and loss within 1e-6 (the
  bars of test_gpu_extras.py).  With gamma > 0 the loss is held to 4x the error
  of the numpy float32 restatement of the same formula on the device's own
  logits (floor 1e-6): the factor allows for a different powf;
* logits of +-40 and +-100 in one batch: everything finite, the same bars;
* a neutral spec and NULL: bitwise jr_head_fwd / jr_head_bwd, both modes;
* jr_dropout_*: y and the in-place dx bitwise the numpy restatement at sizes
  around a quad and a block, rates 0, 0.2 and 0.5, steps 0, 1 and 2^32 - 1;
* the Engine (107^2, B = 4, tiles="heuristic"): unchanged call lists without
  the keywords, one eager step, capture and replay against eager steps, the
  audit of one step, and train.py with all five flags.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import loss_ref
from conftest import PKG
from oracle import tf_ops as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

JR_ERR_INVALID = -1
SIGMOID, SOFTMAX = 0, 1


def _lib():
    from jr import _ffi
    _ffi.init(0)
    return _ffi, _ffi.load()


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30))


def _spec(units, eps=0.0, cw=None, gamma=0.0):
    from jr import _ffi
    s = _ffi.LossSpec(eps, gamma)
    for u in range(16):
        s.class_weight[u] = float(cw[u]) if cw is not None and u < units else 1.0
    return s


class Head:
    """One head problem on the device: feat [n][c], W [c][units], b, labels."""

    def __init__(self, f, W, b, y):
        self.ffi, self.L = _lib()
        self.n, self.c = f.shape
        self.units = W.shape[1]
        self.f, self.W, self.b, self.y = f, W, b, y
        self.F, self.Wd, self.Bd, self.Y = dev(f), dev(W), dev(b), dev(y)
        nu = self.n * self.units
        self.Z, self.P, self.LOSS = (torch.zeros(k, device="cuda") for k in (nu, nu, 1))
        self.DF, self.DW, self.DB = (torch.zeros(k, device="cuda") for k in (self.n * self.c, self.c * self.units,
                                                                            self.units))
        self.z64 = R.dense(f, W, b)

    def _dims(self):
        return self.n, self.c, self.units

    def outputs(self):
        return tuple(host(t).copy() for t in (self.Z, self.P, self.LOSS, self.DF, self.DW, self.DB))

    def poison(self):
        for t in (self.Z, self.P, self.LOSS, self.DF, self.DW, self.DB):
            t.fill_(float("nan"))

    def run_ex(self, mode, spec):
        sp = None if spec is None else ctypes.byref(spec)
        p = lambda t: t.data_ptr()      # noqa: E731
        self.ffi.check("head_fwd_ex", self.L.jr_head_fwd_ex(mode, sp, p(self.F), p(self.Wd), p(self.Bd), p(self.Y),
                                                            *self._dims(), p(self.Z), p(self.P), p(self.LOSS), None))
        self.ffi.check("head_bwd_ex", self.L.jr_head_bwd_ex(mode, sp, p(self.Z), p(self.F), p(self.Wd), p(self.P),
                                                            p(self.Y), *self._dims(), p(self.DF), p(self.DW), p(self.DB),
                                                            None))
        return self.outputs()

    def run_plain(self, mode):
        p = lambda t: t.data_ptr()      # noqa: E731
        self.ffi.check("head_fwd", self.L.jr_head_fwd(mode, p(self.F), p(self.Wd), p(self.Bd), p(self.Y), *self._dims(),
                                                      p(self.Z), p(self.P), p(self.LOSS), None))
        self.ffi.check("head_bwd", self.L.jr_head_bwd(mode, p(self.F), p(self.Wd), p(self.P), p(self.Y), *self._dims(),
                                                      p(self.DF), p(self.DW), p(self.DB), None))
        return self.outputs()

    def check(self, got, model, gamma, tag):
        """The bars of the module docstring; model: (loss, probs, dz) in fp64 from the fp64 logits."""
        z, p, loss, df, dw, db = got
        n, c, units = self._dims()
        rloss, rp, rdz = model
        assert all(np.all(np.isfinite(a)) for a in got), tag
        assert relerr(z.reshape(n, units), self.z64) < 1e-5, tag
        assert relerr(dw.reshape(c, units), self.f.T.astype(np.float64) @ rdz) < 1e-5, tag
        assert relerr(db, rdz.sum(0)) < 1e-5, tag
        assert relerr(df.reshape(n, c), rdz @ self.W.T.astype(np.float64)) < 1e-5, tag
        err = abs(float(loss[0]) - rloss)
        floor = 1e-6 * max(1.0, abs(rloss))
        if gamma == 0:
            assert np.max(np.abs(p.reshape(n, units) - rp)) < 1e-6, tag
            assert err < floor, (tag, err)
            return None
        return err, floor


def _problem(n, c, units, seed, onehot=False):
    rng = np.random.default_rng(seed)
    f = np.maximum(rng.standard_normal((n, c)), 0).astype(np.float32)
    W = (rng.standard_normal((c, units)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(units) * 0.1).astype(np.float32)
    if onehot:
        y = np.eye(units, dtype=np.float32)[rng.integers(0, units, n)]
    else:
        y = (rng.random((n, units)) < 0.4).astype(np.float32)
    cw = (0.5 + 3 * rng.random(units)).astype(np.float32)
    return f, W, b, y, cw


# (eps, class weight of every unit, gamma)
SIGMOID_SPECS = [(0.1, 1.0, 0.0), (0.0, 3.5, 0.0), (0.0, 1.0, 2.0), (0.1, 3.5, 2.0)]


def _focal_bar(h, got, spec_args, tag):
    """gamma > 0: the loss against 4x the error of the float32 restatement on the device's own logits."""
    eps, cw, gamma = spec_args
    err, floor = h.check(got, loss_ref.sigmoid_recipe(h.z64, h.y, eps, cw, gamma), gamma, tag)
    z32 = got[0].reshape(h.n, h.units)
    e32 = abs(loss_ref.sigmoid_recipe_loss_f32(z32, h.y, eps, cw, gamma) - loss_ref.sigmoid_recipe(h.z64, h.y, eps, cw, gamma)[0])
    print(f"focal loss error {tag}: gpu {err:.3e} float32 restatement {e32:.3e}")
    assert err <= max(4 * e32, floor), (tag, err, e32)


@pytest.mark.parametrize("units", [1, 5, 16])
@pytest.mark.parametrize("c", [1, 255, 257, 2048])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_head_recipe_against_the_fp64_models(n, c, units):
    f, W, b, y, cw_rand = _problem(n, c, units, 1000 * n + 10 * c + units)
    h = Head(f, W, b, y)
    for eps, c0, gamma in SIGMOID_SPECS:
        cw = [c0] * units
        tag = (n, c, units, eps, c0, gamma)
        h.poison()
        got = h.run_ex(SIGMOID, _spec(units, eps, cw, gamma))
        if gamma == 0:
            h.check(got, loss_ref.sigmoid_recipe(h.z64, y, eps, cw, gamma), gamma, tag)
        else:
            _focal_bar(h, got, (eps, cw, gamma), tag)
    # non-uniform weights: sigmoid (one weight per unit) and softmax with eps = 0.1
    h.poison()
    got = h.run_ex(SIGMOID, _spec(units, 0.1, cw_rand, 0.0))
    h.check(got, loss_ref.sigmoid_recipe(h.z64, y, 0.1, cw_rand, 0.0), 0, (n, c, units, "weights"))
    f, W, b, y, cw_rand = _problem(n, c, units, 2000 * n + 10 * c + units, onehot=True)
    h = Head(f, W, b, y)
    h.poison()
    got = h.run_ex(SOFTMAX, _spec(units, 0.1, cw_rand, 0.0))
    h.check(got, loss_ref.softmax_recipe(h.z64, y, 0.1, cw_rand), 0, (n, c, units, "softmax"))


@pytest.mark.parametrize("c,units", [(255, 1), (2048, 1), (2048, 5)])
def test_head_recipe_at_saturated_logits(c, units):
    """Features placed so that the logits of one batch reach +-40 and +-100 beside moderate ones.
    A form that takes log(1 - p) from a stored p gives inf or NaN here."""
    rng = np.random.default_rng(c + units)
    n = 8
    W = (rng.standard_normal((c, units)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(units) * 0.1).astype(np.float32)
    pinv = np.linalg.pinv(W.astype(np.float64))
    mix = np.array([100, -100, 40, -40, 0.3])[:units]           # (units > 1) every magnitude inside one sample
    T = rng.standard_normal((n, units)) * 2                       # row 7 stays moderate
    y = np.zeros((n, units), np.float32)
    # right answers at +-40 and +-100, the mixed row, then two confident mistakes
    for r, (t, lab) in enumerate([(40, 1), (-40, 0), (100, 1), (-100, 0), (mix, 1), (40, 0), (-100, 1)]):
        T[r], y[r] = t, lab
    if units > 1:
        y[4] = np.eye(units)[1]
    h = Head(((T - b) @ pinv).astype(np.float32), W, b, y)
    assert np.max(h.z64) > 99 and np.min(h.z64) < -99 and np.any(np.abs(np.abs(h.z64) - 40) < 0.1)
    for eps, c0, gamma in SIGMOID_SPECS:
        cw = [c0] * units
        tag = ("saturated", c, units, eps, c0, gamma)
        h.poison()
        got = h.run_ex(SIGMOID, _spec(units, eps, cw, gamma))
        if gamma == 0:
            h.check(got, loss_ref.sigmoid_recipe(h.z64, y, eps, cw, gamma), gamma, tag)
        else:
            _focal_bar(h, got, (eps, cw, gamma), tag)
    if units > 1:
        # softmax: every row a rotation of the mixed row (one logit 60 to 200 above the rest); rows 0-4 are
        # labelled at their maximum, rows 5-7 elsewhere (confident mistakes)
        T = np.stack([np.roll(mix, r) for r in range(n)])
        y1 = np.eye(units, dtype=np.float32)[[(r + (r >= 5)) % units for r in range(n)]]
        hs = Head(((T - b) @ pinv).astype(np.float32), W, b, y1)
        cw = np.linspace(0.5, 3.5, units)
        hs.poison()
        got = hs.run_ex(SOFTMAX, _spec(units, 0.1, cw, 0.0))
        hs.check(got, loss_ref.softmax_recipe(hs.z64, y1, 0.1, cw), 0, ("saturated softmax", c, units))


@pytest.mark.parametrize("mode", [SIGMOID, SOFTMAX])
@pytest.mark.parametrize("n,c,units", [(1, 1, 1), (3, 257, 5), (64, 2048, 16), (64, 2048, 1)])
def test_neutral_spec_is_bitwise_the_plain_calls(mode, n, c, units):
    f, W, b, y, _ = _problem(n, c, units, 77 + n + c + units, onehot=mode == SOFTMAX)
    h = Head(f, W, b, y)
    h.poison()
    plain = h.run_plain(mode)
    assert all(np.all(np.isfinite(a)) for a in plain)
    junk = _spec(units)
    for u in range(units, 16):      # weights past `units` are not part of the spec
        junk.class_weight[u] = -3.0
    for spec in (None, _spec(units), junk):
        h.poison()
        got = h.run_ex(mode, spec)
        assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(got, plain)), (mode, n, c, units)
    # and a spec that is not neutral does change the loss and the gradients (a one-unit softmax has neither)
    got = h.run_ex(mode, _spec(units, 0.1))
    if mode == SIGMOID or units > 1:
        assert got[2].tobytes() != plain[2].tobytes() and got[3].tobytes() != plain[3].tobytes()
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()


# ---- dropout, C-ABI
class Drop:
    def __init__(self, key, rate, step=0):
        self.ffi, self.L = _lib()
        self.state = torch.zeros(8, device="cuda")
        self.ffi.check("dropout_set", self.L.jr_dropout_set(self.state.data_ptr(), key[0], key[1], rate, step, None))

    def read(self):
        raw = host(self.state)
        u = raw.view(np.uint32)
        return {"key": (int(u[0]), int(u[1])), "step": int(u[2]), "threshold": int(u[3]), "scale": np.float32(raw[4])}, u[5:]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 64 * 2048])
def test_dropout_bitwise_restatement(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    for rate in (0.0, 0.2, 0.5):
        for step in (0, 1, 2 ** 32 - 1):
            d = Drop((7, 3), rate, step)
            ref = loss_ref.dropout_state(7, 3, rate, step)
            st, pad = d.read()
            assert st == ref and st["scale"].tobytes() == ref["scale"].tobytes() and not pad.any(), (rate, step)
            X, Y, G = dev(x), dev(np.full(n + 4, -7.5, np.float32)), dev(g)
            sp = d.state.data_ptr()
            d.ffi.check("dropout_fwd", d.L.jr_dropout_fwd(X.data_ptr(), Y.data_ptr(), n, sp, None))
            d.ffi.check("dropout_bwd", d.L.jr_dropout_bwd(G.data_ptr(), n, sp, None))
            y = host(Y)
            assert y[:n].tobytes() == loss_ref.dropout_apply(x, ref).tobytes(), (n, rate, step)
            assert np.all(y[n:] == np.float32(-7.5))                        # nothing past n
            assert host(G).tobytes() == loss_ref.dropout_apply(g, ref).tobytes(), (n, rate, step)
            assert host(X).tobytes() == x.tobytes()                         # x is untouched
            if rate == 0.0:
                assert y[:n].tobytes() == x.tobytes()
            d.ffi.check("dropout_advance", d.L.jr_dropout_advance(sp, None))
            st2, _ = d.read()
            assert st2 == loss_ref.dropout_advance(ref) and st2["step"] == (step + 1) % 2 ** 32
            if step == 2 ** 32 - 1:
                assert st2["step"] == 0
    if n >= 1023:       # the next step and another key draw other masks
        masks = []
        for key, step in (((7, 3), 0), ((7, 3), 1), ((7, 4), 0), ((8, 3), 0)):
            d = Drop(key, 0.5, step)
            X1, Y = dev(np.ones(n, np.float32)), dev(np.zeros(n, np.float32))
            d.ffi.check("dropout_fwd", d.L.jr_dropout_fwd(X1.data_ptr(), Y.data_ptr(), n, d.state.data_ptr(), None))
            masks.append(host(Y) != 0)
            assert np.array_equal(masks[-1], loss_ref.dropout_mask(n, loss_ref.dropout_state(*key, 0.5, step)))
        assert all(not np.array_equal(masks[0], m) for m in masks[1:])


def test_dropout_refuses_misaligned_buffers():
    ffi, L = _lib()
    n = 1025
    d = Drop((1, 2), 0.5)
    base, other = dev(np.arange(n + 1, dtype=np.float32)), dev(np.arange(n + 1, dtype=np.float32))
    assert base.data_ptr() % 16 == 0 and other.data_ptr() % 16 == 0
    st = d.state.data_ptr()
    assert L.jr_dropout_fwd(base[1:].data_ptr(), other.data_ptr(), n, st, None) == JR_ERR_INVALID
    assert "16-byte" in ffi.last_error()
    assert L.jr_dropout_fwd(base.data_ptr(), other[1:].data_ptr(), n, st, None) == JR_ERR_INVALID
    assert L.jr_dropout_bwd(base[1:].data_ptr(), n, st, None) == JR_ERR_INVALID
    assert L.jr_dropout_bwd(base.data_ptr(), 0, st, None) == JR_ERR_INVALID
    assert L.jr_dropout_set(st, 1, 2, 1.0, 0, None) == JR_ERR_INVALID
    for t in (base, other):                                                  # no launch, no write
        assert np.array_equal(host(t), np.arange(n + 1, dtype=np.float32))
    assert d.read()[0] == loss_ref.dropout_state(1, 2, 0.5)


# ---- the Engine: 107^2, B = 4, tiles="heuristic"
RES, B = 107, 4
ON = dict(dropout=0.5, label_smoothing=0.1)


def _batch(k=0):
    from jr import synth
    return synth.fundus_batch(40 + 10 * k, B, RES), np.array([[1.0], [0.0], [0.0], [1.0]], np.float32)


def _engine(**kw):
    from jr.engine import Engine
    return Engine(B, RES, RES, seed=5, tiles="heuristic", conv_math=kw.pop("conv_math", "x8"), **kw)


def _internal(eng, *names):
    eng.synchronize()
    return tuple(getattr(eng, n).cpu().numpy().copy() for n in names)


def _names(calls):
    out = {}
    for c in calls:
        out[c.name] = out.get(c.name, 0) + 1
    return out


def _diff(a, b):
    """Per-name count differences of two call lists: {name: count in a - count in b}."""
    na, nb = _names(a), _names(b)
    return {k: na.get(k, 0) - nb.get(k, 0) for k in set(na) | set(nb) if na.get(k, 0) != nb.get(k, 0)}


def test_call_lists():
    from jr.lanes import signature
    a = _engine()
    b = _engine(label_smoothing=0.0, class_weight=None, focal_gamma=0.0, dropout=None, dropout_seed=9, dropout_stream=2)
    assert b.loss_spec is None and b.drop_state is None and b.feat_drop is None
    for training in (False, True):
        la, lb = a._build_calls(B, training=training)[:3], b._build_calls(B, training=training)[:3]
        assert la is not None and b._build_calls(B, training=training) is b._build_calls(B)     # one build
        for pa, pb in zip(la, lb):
            assert _names(pa) == _names(pb) and signature(pa) == signature(pb)
    with pytest.raises(ValueError):
        b.dropout_steps()
    base = a._build_calls(B)[:3]
    # dropout: the training lists alone change, by exactly the three calls
    d = _engine(dropout=0.5, dropout_seed=9)
    plain, train = d._build_calls(B)[:3], d._build_calls(B, training=True)[:3]
    for pa, pb in zip(plain, base):
        assert signature(pa) == signature(pb)
    assert [_diff(t, p) for t, p in zip(train, plain)] == [{"dropout_fwd": 1}, {"dropout_bwd": 1}, {"dropout_advance": 1}]
    fwd, bwd, opt = train
    i = [c.name for c in fwd].index("dropout_fwd")
    assert [c.name for c in fwd[i - 1:i + 2]] == ["gap_fwd", "dropout_fwd", "head_fwd"]
    assert [c.fn.__name__ for c in fwd[i:i + 2]] == ["jr_dropout_fwd", "jr_head_fwd"]
    assert fwd[i].reads == (("feat",), ("drop",)) and fwd[i].writes == (("feat_drop",),)
    assert ("feat_drop",) in fwd[i + 1].reads and ("feat",) not in fwd[i + 1].reads
    assert [c.name for c in bwd[:3]] == ["head_bwd", "dropout_bwd", "gap_bwd"] and ("feat_drop",) in bwd[0].reads
    assert bwd[1].reads == (("drop",),) and bwd[1].writes == (("dfeat",),)
    assert opt[-1].name == "dropout_advance" and opt[-1].writes == (("drop",),)
    assert all(c.lane == 0 for c in (fwd[i], bwd[1], opt[-1]))
    assert all(c.name != "dropout_fwd" for c in d._build_calls(B, frozen=True)[0])
    # a loss keyword: every list's head calls are the _ex ones, nothing else changes
    for kw in (dict(label_smoothing=0.1), dict(class_weight=[3.5]), dict(focal_gamma=2.0)):
        e = _engine(**kw)
        for training in (False, True):
            lists = e._build_calls(B, training=training)[:3]
            assert [_diff(t, p) for t, p in zip(lists, base)] == [{"head_fwd_ex": 1, "head_fwd": -1},
                                                                    {"head_bwd_ex": 1, "head_bwd": -1}, {}], kw
        assert [c.fn.__name__ for c in lists[0] if c.name == "head_fwd_ex"] == ["jr_head_fwd_ex"]
        assert [c.fn.__name__ for c in lists[1] if c.name == "head_bwd_ex"] == ["jr_head_bwd_ex"]
        e.close()
    e = _engine(train=False, dropout=0.5, label_smoothing=0.1)       # inference: the objective, never dropout
    inf = _names(e._build_calls(B, training=True)[0])
    assert e.drop_state is None and inf.get("head_fwd_ex") == 1 and "head_fwd" not in inf and "dropout_fwd" not in inf
    for bad in (dict(dropout=1.0), dict(label_smoothing=1.0), dict(class_weight=[0.0]), dict(focal_gamma=-1.0),
                dict(class_weight=[1.0, 2.0])):
        with pytest.raises(ValueError):
            _engine(**bad)
    for x in (a, b, d, e):
        x.close()


def test_one_eager_step_with_dropout_and_smoothing():
    from jr.init import unflatten
    eng = _engine(dropout_seed=7, dropout_stream=3, **ON)
    eng.set_batch(*_batch())
    P0 = unflatten(eng.g, eng.params_numpy())
    assert eng.dropout_steps() == 0
    eng.train_step()
    feat, feat_drop, dfeat, labels = _internal(eng, "feat", "feat_drop", "dfeat", "labels")
    st0 = loss_ref.dropout_state(7, 3, 0.5, 0)
    keep = loss_ref.dropout_mask(feat.size, st0)
    assert feat_drop.tobytes() == loss_ref.dropout_apply(feat, st0).tobytes()
    assert 0.4 < keep.mean() < 0.6 and np.count_nonzero(feat[~keep]) > 0
    assert not dfeat[~keep].any() and np.count_nonzero(dfeat[keep]) > 0.9 * keep.sum()
    z = R.dense(feat_drop.reshape(B, -1), P0["dense/kernel"], P0["dense/bias"])
    want = loss_ref.sigmoid_recipe(z, labels.reshape(B, 1), 0.1)[0]
    assert abs(eng.loss_value() - want) < 1e-6 * max(1.0, want)
    assert eng.dropout_steps() == 1
    # a plain forward never drops: the predictions of an engine without dropout on the same weights
    eng.forward()
    got = eng.predictions().copy()
    twin = _engine()
    twin.load_params(eng.params_numpy())
    twin.set_batch(*_batch())
    twin.forward()
    assert got.tobytes() == twin.predictions().tobytes()
    assert eng.dropout_steps() == 1                             # and draws nothing
    # ... while its loss_value() is the training objective without dropout
    f2, lg = _internal(eng, "feat", "logits")
    want = loss_ref.sigmoid_recipe(lg.reshape(B, 1).astype(np.float64), labels.reshape(B, 1), 0.1)[0]
    assert abs(eng.loss_value() - want) < 1e-6 * max(1.0, want)
    eng.close()
    twin.close()


def test_replayed_steps_draw_the_masks_of_eager_steps():
    names = ("params", "accum", "drop_state", "feat_drop")
    eager, graph, other = _engine(dropout_seed=7, **ON), _engine(dropout_seed=7, **ON), _engine(dropout_seed=8, **ON)
    for e in (eager, graph, other):
        e.set_batch(*_batch())
    graph.capture()
    drops = []
    for t in range(3):
        for e in (eager, graph, other):
            e.set_batch(*_batch(t))
        eager.train_step()
        graph.replay()
        other.train_step()
        a, b_ = _internal(eager, *names), _internal(graph, *names)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b_)), t
        drops.append(a[3] != 0)
    assert graph.dropout_steps() == 3 and eager.dropout_steps() == 3
    assert not np.array_equal(drops[0], drops[1]) and not np.array_equal(drops[1], drops[2])    # a new mask per replay
    assert _internal(other, "params")[0].tobytes() != _internal(eager, "params")[0].tobytes()
    for e in (eager, graph, other):
        e.close()


def test_audit_of_one_step_with_everything_on():
    """The training lists of a step with every new keyword, serial, shadowed and poisoned: every call
    writes inside its declared writes and reads nothing it does not declare."""
    import step_audit
    # (x6h with the BN moving averages: the configuration test_gpu_step_audit.py audits without the keywords)
    eng = _engine(dropout=0.5, dropout_seed=7, label_smoothing=0.1, class_weight=[3.5], focal_gamma=2.0, lanes=2,
                  conv_math="x6h", bn_moving=0.99)
    eng.set_batch(*_batch())
    eng.train_step()
    eng.set_batch(*_batch(1))
    eng.synchronize()
    torch.cuda.synchronize()
    lists = eng._build_calls(B, training=True)
    audit = step_audit.SerialAudit(eng.universe(lists), lambda k: eng.regions(k, lists), torch.cuda.synchronize)
    t0 = time.perf_counter()
    calls = [c for p in lists[:3] for c in p]
    wfind, rfind = audit.run(calls)
    print(f"audit of {len(calls)} calls: {time.perf_counter() - t0:.2f} s")
    assert {("drop",), ("feat_drop",), ("feat",), ("dfeat",), ("head",)} <= set(audit.keys)
    assert {"dropout_fwd", "head_fwd_ex", "head_bwd_ex", "dropout_bwd", "dropout_advance"} <= {c.name for c in calls}
    assert not wfind, "\n".join(wfind)
    assert not rfind, "\n".join(rfind)
    eng.synchronize()
    assert eng.dropout_steps() == 2
    eng.close()


# ---- train.py
def test_cli_trains_with_all_five_flags(tmp_path):
    from jr import synth_records
    d = tmp_path / "data"
    synth_records.write_split(str(d / "train"), 24, size=107, num_shards=2, name="train")
    synth_records.write_split(str(d / "val"), 12, size=107, start=100, num_shards=1, name="validation")
    out = tmp_path / "loss"
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "-t", str(d / "train"), "-v", str(d / "val"),
                        "-sm", str(out / "model"), "-ss", str(out / "logs"), "-so", str(out / "op.csv"),
                        "--image_size", "107", "--num_epochs", "2", "--max_steps_per_epoch", "2", "--shuffle_seed", "1",
                        "--replica_dump_dir", str(out / "dump"),
                        "--label_smoothing", "0.1", "--pos_weight", "3.5", "--focal_gamma", "2", "--dropout", "0.2",
                        "--dropout_seed", "7"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert np.all(np.isfinite(np.load(out / "dump" / "params_e1_r0.npy")))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Objective:")]
    assert len(line) == 1 and all(s in line[0] for s in ("label smoothing 0.1", "positive weight 3.5", "focal gamma 2",
                                                         "dropout 0.2", "seed 7")), r.stdout[-3000:]
    meta = json.load(open(str(out / "model") + ".meta"))
    assert meta["loss"] == {"label_smoothing": 0.1, "pos_weight": 3.5, "focal_gamma": 2.0, "dropout": 0.2,
                            "dropout_seed": 7}
