"""The loss recipe and dropout without a GPU: the reference models of
tests/loss_ref.py (Philox known answers, analytic gradients against central
differences, the neutral spec against oracle/tf_ops, the kept share of the
mask), train.py's flags, and libjr's argument validation."""
import ctypes
import json

import numpy as np
import pytest

import loss_ref
from oracle import tf_ops as R

# the seeds (dropout_seed, dropout_stream) test_gpu_loss_recipe.py draws masks with
GPU_TEST_KEYS = [(0, 0), (1, 0), (7, 0), (7, 3), (0xDEADBEEF, 0xFFFFFFFF)]


# ---- Philox4x32-10
def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = tuple(int(w[0]) for w in loss_ref.philox4x32_10(ctr, key))
        assert got == want, (ctr, [hex(v) for v in got])
    # vectorised over counters: the same words as one at a time
    ctrs = np.array([k[0] for k in kat], np.uint64).T
    for key in ((0, 0), (0xA4093822, 0x299F31D0)):
        many = loss_ref.philox4x32_10(tuple(ctrs), key)
        for j, (ctr, _, _) in enumerate(kat):
            one = loss_ref.philox4x32_10(ctr, key)
            assert [int(w[j]) for w in many] == [int(w[0]) for w in one]


def test_dropout_state_and_mask_contract():
    st = loss_ref.dropout_state(3, 4, 0.2)
    assert st["threshold"] == int(np.floor(float(np.float32(0.2)) * 2 ** 32)) and st["step"] == 0
    assert st["scale"] == np.float32(1.0 / (1.0 - st["threshold"] / 2 ** 32)) and st["scale"].dtype == np.float32
    zero = loss_ref.dropout_state(3, 4, 0.0)
    assert zero["threshold"] == 0 and zero["scale"] == np.float32(1)
    x = np.random.default_rng(0).standard_normal(1025).astype(np.float32)
    assert loss_ref.dropout_apply(x, zero).tobytes() == x.tobytes()         # rate 0: y == x bitwise
    # element i takes word i & 3 of the block of quad i >> 2, whatever n is
    full = loss_ref.dropout_mask(1025, st)
    for n in (1, 3, 4, 5, 1023):
        assert np.array_equal(loss_ref.dropout_mask(n, st), full[:n])
    words = loss_ref.philox4x32_10((256, 0, 0, 0), st["key"])
    assert full[1024] == (int(words[0][0]) >= st["threshold"])
    y = loss_ref.dropout_apply(x, st)
    assert np.array_equal(y[full], x[full] * st["scale"]) and not y[~full].any()
    # the counter wraps; another step, another key: another mask
    last = loss_ref.dropout_state(3, 4, 0.2, 2 ** 32 - 1)
    assert loss_ref.dropout_advance(last)["step"] == 0
    assert not np.array_equal(loss_ref.dropout_mask(1025, loss_ref.dropout_advance(st)), full)
    assert not np.array_equal(loss_ref.dropout_mask(1025, loss_ref.dropout_state(3, 5, 0.2)), full)


@pytest.mark.parametrize("key", GPU_TEST_KEYS)
def test_kept_share_of_the_mask(key):
    """64 * 2048 elements at rate 0.2: the kept share within 5 sigma of 0.8 (sigma = sqrt(0.16 / 131072) = 0.0011)."""
    n = 64 * 2048
    for step in (0, 1, 2 ** 32 - 1):
        share = float(loss_ref.dropout_mask(n, loss_ref.dropout_state(*key, 0.2, step)).mean())
        assert abs(share - 0.8) <= 0.0055, (key, step, share)


# ---- the fp64 models
def _case(n, units, seed, onehot=False):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, units)) * 3
    if onehot:
        y = np.eye(units)[rng.integers(0, units, n)]
    else:
        y = (rng.random((n, units)) < 0.3).astype(np.float64)
    cw = 0.5 + 3 * rng.random(units)
    return z, y, cw


def _central(f, z, h=1e-6):
    g = np.zeros_like(z)
    for i in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        g[i] = (f(zp) - f(zm)) / (2 * h)
    return g


@pytest.mark.parametrize("eps,weighted,gamma", [(0.1, True, 2.0), (0.1, False, 0.0), (0.0, True, 0.0), (0.0, False, 2.0),
                                                (0.3, True, 0.5)])
def test_sigmoid_gradient_matches_central_differences(eps, weighted, gamma):
    z, y, cw = _case(5, 3, 11)
    cw = cw if weighted else None
    _, _, dz = loss_ref.sigmoid_recipe(z, y, eps, cw, gamma)
    num = _central(lambda v: loss_ref.sigmoid_recipe(v, y, eps, cw, gamma)[0], z)
    assert np.max(np.abs(dz - num)) < 1e-8 * max(1.0, np.max(np.abs(num)))


@pytest.mark.parametrize("eps,weighted", [(0.1, True), (0.1, False), (0.0, True)])
def test_softmax_gradient_matches_central_differences(eps, weighted):
    z, y, cw = _case(6, 5, 12, onehot=True)
    cw = cw if weighted else None
    _, _, dz = loss_ref.softmax_recipe(z, y, eps, cw)
    num = _central(lambda v: loss_ref.softmax_recipe(v, y, eps, cw)[0], z)
    assert np.max(np.abs(dz - num)) < 1e-8 * max(1.0, np.max(np.abs(num)))


def test_neutral_spec_is_the_plain_loss():
    z, y, _ = _case(7, 4, 13)
    loss, p, dz = loss_ref.sigmoid_recipe(z, y)
    assert abs(loss - R.sigmoid_xent_mean(z, y)) < 1e-14
    assert np.max(np.abs(dz - R.sigmoid_xent_grad(z, y))) < 1e-15
    assert np.max(np.abs(p - R.sigmoid(z))) < 1e-15
    z, y, _ = _case(7, 4, 14, onehot=True)
    loss, p, dz = loss_ref.softmax_recipe(z, y)
    rl, rp, rdz = R.softmax_xent_mean(z, y)
    assert abs(loss - rl) < 1e-14 and np.max(np.abs(p - rp)) < 1e-15 and np.max(np.abs(dz - rdz)) < 1e-15


def test_models_are_finite_at_saturated_logits():
    z = np.array([[40.0, -40.0, 100.0, -100.0, 0.5]]).T
    for y in (np.zeros_like(z), np.ones_like(z)):
        loss, _, dz = loss_ref.sigmoid_recipe(z, y, 0.1, [3.5], 2.0)
        assert np.isfinite(loss) and np.all(np.isfinite(dz))
        assert np.isfinite(loss_ref.sigmoid_recipe_loss_f32(z, y, 0.1, [3.5], 2.0))
    # gamma = 0, c = 1: the plain loss on the smoothed target
    y = np.array([[1.0, 0.0, 0.0, 1.0, 1.0]]).T
    assert abs(loss_ref.sigmoid_recipe(z, y, 0.2)[0] - R.sigmoid_xent_mean(z, y * 0.8 + 0.1)) < 1e-12


# ---- train.py's flags
def _args(*argv):
    import train
    return train, train.build_parser().parse_args(list(argv))


def test_flags_give_engine_keywords_and_meta():
    train, a = _args()
    assert train.loss_meta(a) is None and train.loss_engine_kwargs(a) == {} and train.objective_line(a) is None
    train, a = _args("--label_smoothing", "0.1", "--pos_weight", "3.5", "--focal_gamma", "2", "--dropout", "0.2",
                     "--dropout_seed", "7")
    assert train.loss_engine_kwargs(a, rank=3) == {"label_smoothing": 0.1, "class_weight": [3.5], "focal_gamma": 2.0,
                                                   "dropout": 0.2, "dropout_seed": 7, "dropout_stream": 3}
    meta = train.loss_meta(a)
    assert meta == {"label_smoothing": 0.1, "pos_weight": 3.5, "focal_gamma": 2.0, "dropout": 0.2, "dropout_seed": 7}
    assert json.loads(json.dumps(meta)) == meta
    line = train.objective_line(a)
    assert line.startswith("Objective:") and all(s in line for s in ("0.1", "3.5", "focal gamma 2", "dropout 0.2"))
    for flag, kw in (("--label_smoothing", "label_smoothing"), ("--focal_gamma", "focal_gamma"), ("--dropout", "dropout")):
        train, a = _args(flag, "0.25")
        assert list(train.loss_engine_kwargs(a))[0] == kw and train.loss_meta(a) is not None
    train, a = _args("--pos_weight", "4")
    assert train.loss_engine_kwargs(a) == {"class_weight": [4.0]}
    assert train.loss_meta(a)["dropout"] is None and train.loss_meta(a)["dropout_seed"] is None
    help_text = train.build_parser().format_help()
    assert "training objective" in help_text


@pytest.mark.parametrize("argv", [("--label_smoothing", "1"), ("--label_smoothing", "-0.1"), ("--label_smoothing", "nan"),
                                  ("--pos_weight", "0"), ("--pos_weight", "inf"), ("--focal_gamma", "-1"),
                                  ("--dropout", "1"), ("--dropout", "x"), ("--dropout_seed", "1.5"),
                                  ("--dropout_seed", "3")])
def test_bad_flag_values_are_refused(argv, capsys):
    import train
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(list(argv))
    capsys.readouterr()


def test_engine_keyword_validation():
    from jr.engine import Engine
    spec = Engine._loss_spec
    assert spec(1, "sigmoid", 0.0, None, 0.0) is None
    s = spec(2, "sigmoid", 0.1, [2.0, 3.0], 1.5)
    assert (round(s.label_smoothing, 6), s.focal_gamma, list(s.class_weight)[:3]) == (0.1, 1.5, [2.0, 3.0, 1.0])
    assert list(spec(3, "softmax", 0.1, None, 0.0).class_weight) == [1.0] * 16
    for bad in ((1, "sigmoid", 1.0, None, 0.0), (1, "sigmoid", 0.0, [0.0], 0.0), (1, "sigmoid", 0.0, [1.0, 2.0], 0.0),
                (1, "sigmoid", 0.0, None, -1.0), (2, "softmax", 0.0, None, 2.0), (1, "sigmoid", 0.0, [np.inf], 0.0)):
        with pytest.raises(ValueError):
            spec(*bad)


# ---- libjr's validation, before any HIP call
def test_validation_errors_without_gpu():
    from jr import _ffi
    L = _ffi.load()
    assert ctypes.sizeof(_ffi.LossSpec) == 72 and ctypes.sizeof(_ffi.DropoutState) == 32
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0

    def spec(eps=0.0, gamma=0.0, c0=1.0):
        s = _ffi.LossSpec(eps, gamma)
        for u in range(16):
            s.class_weight[u] = 1.0
        s.class_weight[0] = c0
        return ctypes.byref(s)
    fwd = lambda mode, sp, feat=p: L.jr_head_fwd_ex(mode, sp, feat, p, p, p, 1, 1, 1, p, p, p, None)   # noqa: E731
    bwd = lambda mode, sp, z=p: L.jr_head_bwd_ex(mode, sp, z, p, p, p, p, 1, 1, 1, p, p, p, None)       # noqa: E731
    assert fwd(0, spec(eps=1.0)) == -1 and "label_smoothing" in _ffi.last_error()
    assert fwd(0, spec(eps=-0.5)) == -1 and fwd(0, spec(eps=float("nan"))) == -1
    assert fwd(0, spec(gamma=-1.0)) == -1 and fwd(0, spec(gamma=float("inf"))) == -1
    assert fwd(1, spec(gamma=2.0)) == -1 and "sigmoid-only" in _ffi.last_error()
    assert fwd(0, spec(c0=0.0)) == -1 and fwd(0, spec(c0=float("inf"))) == -1 and "class_weight" in _ffi.last_error()
    assert fwd(0, spec(), None) == -1 and fwd(0, None, None) == -1 and fwd(2, None) == -1
    assert bwd(0, spec(eps=1.0)) == -1 and bwd(0, spec(), None) == -1 and bwd(0, None, None) == -1
    assert bwd(1, spec(gamma=1.0)) == -1
    assert L.jr_head_fwd_ex(0, None, p, p, p, p, 1, 1, 17, p, p, p, None) == -1        # units past 16
    # dropout
    assert L.jr_dropout_set(p, 1, 2, 1.0, 0, None) == -1 and "rate" in _ffi.last_error()
    assert L.jr_dropout_set(p, 1, 2, -0.1, 0, None) == -1 and L.jr_dropout_set(p, 1, 2, float("nan"), 0, None) == -1
    assert L.jr_dropout_set(None, 1, 2, 0.2, 0, None) == -1
    assert L.jr_dropout_fwd(None, p, 4, p, None) == -1 and L.jr_dropout_fwd(p, None, 4, p, None) == -1
    assert L.jr_dropout_fwd(p, p, 4, None, None) == -1 and L.jr_dropout_fwd(p, p, 0, p, None) == -1
    assert L.jr_dropout_fwd(p + 4, p, 4, p, None) == -1 and "16-byte" in _ffi.last_error()
    assert L.jr_dropout_fwd(p, p + 4, 4, p, None) == -1
    assert L.jr_dropout_bwd(None, 4, p, None) == -1 and L.jr_dropout_bwd(p + 4, 4, p, None) == -1
    assert L.jr_dropout_bwd(p, -1, p, None) == -1 and L.jr_dropout_bwd(p, 4, None, None) == -1
    assert L.jr_dropout_advance(None, None) == -1
    assert {"jr_head_fwd_ex", "jr_head_bwd_ex", "jr_dropout_set", "jr_dropout_fwd", "jr_dropout_bwd",
            "jr_dropout_advance"} <= set(_ffi.EXPORTED)
