"""RMSProp and the weight average without a GPU: the numpy restatements
(tests/ema_ref.py) against float64 models with error bounds derived from the
roundings they count, the warm-up decay sequence, the .ema checkpoint file,
the train.py flags and evaluate.py's refusals."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import ema_ref
from ema_ref import U
from opt_ref import f32


# ---- the restatements against float64
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.9999])
def test_ema_constant_weights_closed_form(decay):
    """Constant w, k steps at a fixed decay: shadow_k = w + (s0 - w) d^k, d = 1 - one_minus_decay.

    Bound.  One step is three fp32 roundings: e = fl(s - w), |error| <= U |s - w|
    <= 2 U M with M = max |s0|, |w| (s stays between s0 and w up to the
    overshoot covered below); p = fl(e * omd) adds at most U |p| <= 2 U M to the
    first error scaled by omd <= 1; s' = fl(s - p) adds U |s'| <= U M.  That is
    5 U M per step, 6 U M with the second-order terms and an overshoot of w by
    at most 2 U |e| when omd = 1.  The error a step inherits is multiplied by
    |1 - omd (1 + d1)(1 + d2)| <= 1 + 3 U, so k steps stay within 6 k U M
    (1 + 3 U)^k; the float64 closed form itself is within k 2^-52 M."""
    k = 50
    rng = np.random.default_rng(3)
    s0 = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-3, 3, 4096)).astype(np.float32)
    w = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-3, 3, 4096)).astype(np.float32)
    st = ema_ref.ema_set_ref(decay, warm=False)
    s = s0
    for _ in range(k):
        s, st = ema_ref.ema_step_ref(s, w, st)
    assert st["updates"] == k
    d = 1.0 - float(st["one_minus_decay"])
    want = w.astype(np.float64) + (s0.astype(np.float64) - w) * d ** k
    M = np.maximum(np.abs(s0), np.abs(w)).astype(np.float64)
    bound = 6 * k * U * M * (1 + 3 * U) ** k + k * 2.0 ** -52 * M
    err = np.abs(s.astype(np.float64) - want)
    print(f"decay {decay}: max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    if decay == 0.0:
        assert np.array_equal(s, w)         # decay 0: the shadow is the weights


def test_ema_skipped_step_is_the_identity():
    s = np.float32([1.5, -2.0, 3.0])
    st = ema_ref.ema_set_ref(0.9, warm=True, updates=7)
    s1, st1 = ema_ref.ema_step_ref(s, np.float32([0, 0, 0]), st, skipped=1)
    assert np.array_equal(s1, s) and st1["updates"] == 7 and st1["one_minus_decay"] == 0


@pytest.mark.parametrize("eps", [1.0, 1e-3])
def test_rmsprop_one_step_within_the_rounding_bound(eps):
    """One step on mixed magnitudes against float64; the bound is carried through every
    one of the step's twelve fp32 operations by ema_ref.Err (U per rounding, TINY on underflow)."""
    n = 4096
    rng = np.random.default_rng(4)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 10, n)).astype(np.float32)
    w = rng.standard_normal(n).astype(np.float32)
    mom = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    ms = (rng.standard_normal(n).astype(np.float32) ** 2 + f32(0.5)).astype(np.float32)
    got = ema_ref.rmsprop_ref(w, g, mom, ms, 0.3, 0.045, eps=eps)
    want = ema_ref.rmsprop_model(w, g, mom, ms, 0.3, 0.045, eps=eps)
    for name, a, b in zip(("w", "mom", "ms"), got, want):
        err = np.abs(a.astype(np.float64) - b.v)
        print(f"{name}: max err/bound {np.max(err / b.e):.3f}, max bound/|value| {np.max(b.e / np.abs(b.v)):.3e}")
        assert np.all(np.isfinite(b.e)) and np.all(err <= b.e), name


def test_rmsprop_first_step_from_tf_initial_state():
    """ms = 1, mom = 0, eps = 1, one element by hand in float64."""
    w, mom, ms = ema_ref.rmsprop_ref(np.float32([1.0]), np.float32([2.0]), np.float32([0.0]), np.float32([1.0]), 1.0, 0.5)
    ms64 = 1.0 + (4.0 - 1.0) * (1.0 - float(f32(0.9)))
    mom64 = 1.0 / np.sqrt(ms64 + 1.0)
    assert abs(float(ms[0]) - ms64) <= 4 * U * ms64 and abs(float(mom[0]) - mom64) <= 8 * U * mom64
    assert abs(float(w[0]) - (1.0 - mom64)) <= 8 * U


def test_rmsprop_decay_and_skip():
    w, g = np.float32([1.0, 1.0]), np.float32([0.5, 0.5])
    z, one = np.zeros(2, np.float32), np.ones(2, np.float32)
    w1, mom1, ms1 = ema_ref.rmsprop_ref(w, g, z, one, 1.0, 0.1, 0.25, np.array([True, False]))
    plain = ema_ref.rmsprop_ref(w, f32(0.5) + np.float32([0.25, 0]), z, one, 1.0, 0.1)
    assert np.array_equal(w1, plain[0]) and np.array_equal(ms1, plain[2])
    assert all(np.array_equal(a, b) for a, b in zip(ema_ref.rmsprop_ref(w, g, z, one, 1.0, 0.1, skipped=1), (w, z, one)))


# ---- the warm-up
def _f32_of(q: Fraction) -> Fraction:
    """A fraction in [1/2, 1) rounded to fp32 (ulp 2^-24, ties to even: Python's round)."""
    assert Fraction(1, 2) <= q < 1
    return Fraction(round(q * 2 ** 24), 2 ** 24)


def test_warm_up_sequence_and_crossing():
    decay = f32(0.9999)
    D = Fraction(float(decay))
    st = ema_ref.ema_set_ref(0.9999, warm=True)
    for t in range(21):
        q = Fraction(1 + t, 10 + t)
        want = min(D, _f32_of(q) if q >= Fraction(1, 2) else Fraction(float(f32(float(q)))))
        assert Fraction(float(ema_ref.warm_decay(decay, t))) == want, t
        st = ema_ref.ema_prepare_ref(st)
        assert Fraction(float(st["one_minus_decay"])) == Fraction(float(f32(1) - f32(float(want)))), t
        assert st["updates"] == t + 1
    assert float(ema_ref.warm_decay(decay, 0)) == float(f32(0.1)) and ema_ref.warm_decay(decay, 20) == f32(0.7)
    # where (1 + t) / (10 + t), rounded to fp32, reaches the decay: in exact arithmetic at
    # t >= (10 D - 1) / (1 - D), about 89,990; the rounded quotient gets there a few steps sooner
    exact = -((1 - 10 * D) // (1 - D))                     # ceil((10 D - 1) / (1 - D))
    first = next(t for t in range(exact - 200, exact + 1) if _f32_of(Fraction(1 + t, 10 + t)) >= D)
    ts = np.arange(exact - 200, exact + 200)
    got = ema_ref.warm_decay(decay, ts)
    assert np.all(got[ts < first] < decay) and np.all(got[ts >= first] == decay)
    assert 89000 < first <= exact < 91000
    assert ema_ref.warm_decay(decay, 5, warm=False) == decay


# ---- the checkpoint's .ema
@pytest.fixture(scope="module")
def graph():
    from jr.inception import build_inception_v3
    return build_inception_v3(107, 107, 1)


@pytest.fixture(scope="module")
def flats(graph):
    from jr.init import param_layout
    total = param_layout(graph.params)[1]
    flat = np.zeros(total, np.float32)
    flat[::1000] = 1.0
    ema = flat.copy()
    ema[::1000] = 0.5
    return flat, ema


def test_checkpoint_ema_round_trip_refusal_and_stale_file(tmp_path, graph, flats):
    from jr import checkpoint
    flat, ema = flats
    path = str(tmp_path / "model")
    checkpoint.save(path, graph, flat, {"epoch": 3}, weight_ema={"flat": ema, "decay": 0.9999, "warm": True,
                                                                 "updates": 17})
    assert os.path.getsize(path + ".ema") == os.path.getsize(path + checkpoint.DATA_SUFFIX)
    meta = json.load(open(path + ".meta"))
    assert meta["weight_ema"]["decay"] == 0.9999 and meta["weight_ema"]["warm"] is True
    assert meta["weight_ema"]["updates"] == 17 and len(meta["weight_ema"]["sha256"]) == 64
    got, info = checkpoint.load_ema(path, graph)
    assert got.dtype == np.float32 and np.array_equal(got, ema) and info["updates"] == 17
    assert np.array_equal(checkpoint.load(path, graph)[0], flat)            # the data file keeps the trained weights
    # the ensemble glob still recovers the path: the name has one extension
    import evaluate
    assert evaluate.expand_model_paths(str(tmp_path / "mod*")) == [path]
    # a flipped byte, then a short file
    raw = bytearray(open(path + ".ema", "rb").read())
    raw[5] ^= 1
    open(path + ".ema", "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="checksum"):
        checkpoint.load_ema(path, graph)
    open(path + ".ema", "wb").write(bytes(raw[:-4]))
    with pytest.raises(ValueError, match="size"):
        checkpoint.load_ema(path, graph)
    os.remove(path + ".ema")
    with pytest.raises(ValueError, match="missing"):
        checkpoint.load_ema(path, graph)
    with pytest.raises(ValueError):
        checkpoint.save(path, graph, flat, weight_ema={"flat": ema[:-1], "decay": 0.5, "warm": False, "updates": 0})
    # a save without the average removes the one it replaces
    checkpoint.save(path, graph, flat, weight_ema={"flat": ema, "decay": 0.5, "warm": False, "updates": 1})
    assert os.path.exists(path + ".ema")
    checkpoint.save(path, graph, flat)
    assert not os.path.exists(path + ".ema") and checkpoint.load_ema(path, graph) is None
    assert "weight_ema" not in json.load(open(path + ".meta"))


# ---- the flags
def test_parser_new_flags_off_by_default():
    import train
    args = train.build_parser().parse_args([])
    assert (args.optimizer, args.rmsprop, args.weight_ema, args.weight_ema_no_warm) == (None, None, None, False)
    assert train.optimizer_name(args) == "nesterov" and train.ema_engine_kwargs(args) == {}
    assert train.optimizer_meta(args) == {}
    assert train.optimizer_name(train.build_parser().parse_args(["-sgd"])) == "sgd"


def test_parser_recipe_of_the_published_flags():
    import train
    args = train.build_parser().parse_args(["--optimizer", "rmsprop", "--weight_ema"])
    assert train.optimizer_name(args) == "rmsprop" and args.weight_ema == 0.9999
    assert train.ema_engine_kwargs(args) == {"rmsprop_rho": 0.9, "rmsprop_momentum": 0.9, "rmsprop_eps": 1.0,
                                             "weight_ema": 0.9999, "weight_ema_warm": True}
    assert train.optimizer_meta(args) == {"name": "rmsprop", "rmsprop": {"rho": 0.9, "momentum": 0.9, "epsilon": 1.0},
                                          "weight_ema": {"decay": 0.9999, "warm": True}}
    args = train.build_parser().parse_args(["--optimizer", "rmsprop", "--rmsprop", "0.95,0.8,0.1", "--weight_ema", "0.5",
                                            "--weight_ema_no_warm"])
    assert args.rmsprop == (0.95, 0.8, 0.1) and args.weight_ema == 0.5
    assert train.ema_engine_kwargs(args)["weight_ema_warm"] is False
    assert train.optimizer_name(train.build_parser().parse_args(["--optimizer", "adam"])) == "adam"


@pytest.mark.parametrize("argv", [["--optimizer", "rmsprop", "-sgd"], ["--optimizer", "sgd", "-sgd"],
                                  ["--optimizer", "rmsprop", "--rmsprop", "0.9,0.9"],
                                  ["--optimizer", "rmsprop", "--rmsprop", "0.9,0.9,0"],
                                  ["--optimizer", "rmsprop", "--rmsprop", "1.0,0.9,1"],
                                  ["--optimizer", "rmsprop", "--rmsprop", "a,b,c"],
                                  ["--rmsprop", "0.9,0.9,1.0"], ["--optimizer", "lamb"],
                                  ["--weight_ema", "1.0"], ["--weight_ema", "-0.1"], ["--weight_ema_no_warm"]])
def test_parser_rejects(argv, capsys):
    import train
    with pytest.raises(SystemExit) as e:
        train.build_parser().parse_args(argv)
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


# ---- evaluate.py
def test_evaluate_averaged_names_the_member_without_an_average(tmp_path, graph, flats):
    import evaluate
    from jr import checkpoint
    flat, ema = flats
    a, b = str(tmp_path / "with"), str(tmp_path / "without")
    checkpoint.save(a, graph, flat, weight_ema={"flat": ema, "decay": 0.9, "warm": True, "updates": 2})
    checkpoint.save(b, graph, flat)
    with pytest.raises(SystemExit) as e:
        evaluate.main(["-o", "--data_dir", str(tmp_path / "none"), "-lm", f"{a},{b}", "--weights", "averaged"])
    msg = str(e.value)
    assert b in msg and "no averaged weights" in msg and "--weight_ema" in msg
    got = evaluate.load_averaged([a], graph)
    assert len(got) == 1 and np.array_equal(got[0], ema)


def test_evaluate_averaged_with_moving_bn_needs_a_calibration_directory(tmp_path):
    import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["-o", "--data_dir", str(tmp_path), "-lm", str(tmp_path / "absent"), "--weights", "averaged",
                       "--bn", "moving"])
    msg = str(e.value)
    assert "--bn_calibrate_dir" in msg and "trained weights" in msg
    assert evaluate.build_parser().parse_args(["-o"]).weights == "trained"
