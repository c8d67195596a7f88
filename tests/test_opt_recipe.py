"""The optimizer recipe's host side (no GPU): the numpy restatement of
jr_opt_prepare against its float64 model, the decay ranges of the internal
parameter layout, the learning-rate schedule, train.py's flags, and argument
validation of the new entry points before any HIP call."""
import math

import numpy as np
import pytest

import opt_ref
from opt_ref import f32

FMAX = float(np.finfo(f32).max)


# ---- jr_opt_prepare: restatement against the float64 model
# four fp32 roundings follow the fp64 sqrt (the cast, two multiplies, one
# division), each at most 2^-24 relative: scale and norm agree with the
# float64 model within 4 * 2^-24 (first order; 5 covers the second-order terms)
PREP_RTOL = 5 * 2.0 ** -24

PREP_CASES = [
    # (S, clip_norm, grad_scale)
    (9.0, 0.0, 1.0),            # clip_norm 0: never clips
    (9.0, 4.0, 1.0),            # norm < clip
    (4.0, 2.0, 1.0),            # norm == clip exactly: no clipping
    (9.0, 2.0, 1.0),            # norm > clip
    (1234.5678, 1.5, 1.0),
    (0.0, 2.0, 1.0),            # S = 0: factor 1, no 0/0
    (0.0, 0.0, 1.0),
    (float("inf"), 2.0, 1.0),
    (float("nan"), 2.0, 1.0),
    (1e80, 2.0, 1.0),           # finite fp64 sum whose root overflows fp32: skipped
    (1e76, 2.0, 0.5),           # sqrt = 1e38 fits fp32
    (9.0, 2.0, 0.5),            # grad_scale 0.5: norm 1.5 < clip
    (64.0, 2.0, 0.5),           # grad_scale 0.5: norm 4 > clip
    (16.0, 2.0, 0.5),           # grad_scale 0.5: norm == clip
]


@pytest.mark.parametrize("S,clip,gs", PREP_CASES)
def test_prepare_restatement_against_float64(S, clip, gs):
    scale, gn, skipped = opt_ref.prepare_ref(S, clip, gs)
    scale64, gn64, skipped64 = opt_ref.prepare_f64(S, clip, gs)
    assert scale.dtype == f32 and gn.dtype == f32
    assert skipped == skipped64
    if skipped:
        assert scale == 0 and not np.isfinite(gn)
        return
    assert abs(float(gn) - gn64) <= PREP_RTOL * abs(gn64)
    assert abs(float(scale) - scale64) <= PREP_RTOL * abs(scale64)


def test_prepare_decisions():
    assert opt_ref.prepare_ref(4.0, 2.0, 1.0) == (f32(1), f32(2), 0)            # norm == clip: factor 1
    assert opt_ref.prepare_ref(0.0, 2.0, 1.0) == (f32(1), f32(0), 0)            # no 0/0
    assert opt_ref.prepare_ref(16.0, 2.0, 1.0) == (f32(0.5), f32(4), 0)
    assert opt_ref.prepare_ref(16.0, 0.0, 1.0) == (f32(1), f32(4), 0)
    assert opt_ref.prepare_ref(64.0, 2.0, 0.5) == (f32(0.25), f32(4), 0)        # scale = grad_scale * factor
    for S in (float("inf"), float("nan"), 1e80, 4.0 * FMAX * FMAX):
        scale, gn, skipped = opt_ref.prepare_ref(S, 2.0, 1.0)
        assert skipped == 1 and scale == 0 and scale.dtype == f32
    assert opt_ref.prepare_ref(1e80, 0.0, 1.0)[2] == 1                          # skipped without clipping too


# ---- decay_ranges
@pytest.fixture(scope="module", params=[107, 299])
def planned(request):
    from jr.inception import build_inception_v3
    from jr.plan import build_plan
    g = build_inception_v3(request.param, request.param, 1)
    return g, build_plan(g)


def _runs(mask):
    """[(begin, end)] of the non-zero runs of a vector."""
    d = np.diff(np.concatenate([[0], (mask != 0).astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def test_decay_ranges_are_the_kernels_of_the_internal_layout(planned):
    from jr.init import param_layout
    from jr.plan import decay_ranges
    g, plan = planned
    ranges = decay_ranges(plan)
    assert ranges and all(isinstance(b, int) and isinstance(e, int) for b, e in ranges)
    assert all(0 <= b < e <= plan.nparam for b, e in ranges)
    assert all(ranges[i][1] < ranges[i + 1][0] for i in range(len(ranges) - 1))     # sorted, disjoint, merged
    keras, total = param_layout(g.params)
    kmask = np.zeros(total, np.float32)
    for name, _, off, size in keras:
        if name.endswith("/kernel"):
            kmask[off:off + size] = 1
    assert ranges == _runs(plan.to_internal(g, kmask))
    # no beta and no bias element in any range
    other = np.zeros(total, np.float32)
    names = set()
    for name, _, off, size in keras:
        if not name.endswith("/kernel"):
            other[off:off + size] = 1
            names.add(name.split("/")[-1])
    assert names == {"beta", "bias"}
    inside = opt_ref.decay_mask(plan.nparam, ranges)
    assert not np.any(inside & (plan.to_internal(g, other) != 0))
    assert int(inside.sum()) == int(kmask.sum())


# ---- jr.schedule.learning_rate
def test_learning_rate_plain_and_repeatable():
    from jr.schedule import learning_rate
    lr = learning_rate(7, 3e-3)
    assert isinstance(lr, np.float32) and lr == f32(3e-3)
    a = [learning_rate(s, 3e-3, (0.94, 5), 4) for s in range(40)]
    b = [learning_rate(s, 3e-3, (0.94, 5), 4) for s in range(40)]
    assert all(isinstance(v, np.float32) for v in a)
    assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_learning_rate_staircase_boundaries():
    from jr.schedule import learning_rate
    base, rate = f32(0.1), f32(0.94)
    for step, k in ((0, 0), (4, 0), (5, 1), (9, 1), (10, 2), (14, 2), (15, 3)):
        p = f32(1)
        for _ in range(k):
            p = f32(p * rate)
        got = learning_rate(step, 0.1, (0.94, 5))
        assert got == f32(base * p), step
        assert abs(float(got) - 0.1 * 0.94 ** k) <= (k + 2) * 2.0 ** -24 * 0.1
    with pytest.raises(ValueError):
        learning_rate(0, 0.1, (0.94, 0))
    with pytest.raises(ValueError):
        learning_rate(-1, 0.1)


def test_learning_rate_warmup_ends_exactly_at_base():
    from jr.schedule import learning_rate
    base = f32(3e-3)
    assert learning_rate(0, 3e-3, warmup=4) == f32(base * f32(f32(1) / f32(4)))     # base / warmup
    vals = [learning_rate(s, 3e-3, warmup=4) for s in range(8)]
    assert all(vals[i] < vals[i + 1] for i in range(3))
    assert all(v == base for v in vals[3:])                                        # exactly base from step warmup - 1
    assert learning_rate(0, 3e-3, warmup=1) == base and learning_rate(0, 3e-3, warmup=0) == base
    # warmup multiplies the staircase
    assert learning_rate(1, 0.1, (0.5, 1), 4) == f32(f32(f32(0.1) * f32(0.5)) * f32(f32(2) / f32(4)))


# ---- train.py's flags
def test_parser_recipe_off_by_default():
    import train
    args = train.build_parser().parse_args([])
    assert train.opt_recipe(args) is None
    assert train.opt_engine_kwargs(args) == {}


def test_parser_recipe_flags():
    import train
    args = train.build_parser().parse_args(["--lr_decay", "0.94,2"])
    assert args.lr_decay == (0.94, 2)
    assert train.opt_recipe(args) == {"learning_rate": train.LEARNING_RATE, "lr_decay": [0.94, 2], "lr_warmup": 0,
                                      "weight_decay": 0.0, "clip_norm": None}
    assert train.opt_engine_kwargs(args) == {"weight_decay": 0.0, "clip_norm": None, "device_lr": True}
    args = train.build_parser().parse_args(["--learning_rate", "0.01"])          # bare: no device path
    assert train.opt_recipe(args)["learning_rate"] == 0.01
    assert train.opt_engine_kwargs(args) == {}
    args = train.build_parser().parse_args(["--weight_decay", "4e-5", "--clip_norm", "2", "--lr_warmup", "3"])
    assert train.opt_engine_kwargs(args) == {"weight_decay": 4e-5, "clip_norm": 2.0, "device_lr": True}
    assert train.opt_recipe(args)["lr_warmup"] == 3


@pytest.mark.parametrize("argv", [
    ["--lr_decay", "0.94"], ["--lr_decay", "0.94,0"], ["--lr_decay", "a,2"], ["--lr_decay", "0.94,2,3"],
    ["--lr_decay", "-0.5,2"], ["--lr_decay", "0.94,1.5"], ["--lr_warmup", "-1"], ["--lr_warmup", "2.5"],
    ["--weight_decay", "-1e-5"], ["--weight_decay", "nan"], ["--clip_norm", "0"], ["--clip_norm", "inf"],
    ["--learning_rate", "0"], ["--learning_rate", "x"]])
def test_parser_rejects_malformed_values(argv, capsys):
    import train
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(argv)
    capsys.readouterr()
    # ... while the flag itself is known: a well-formed value parses
    good = {"--lr_decay": "0.94,2", "--lr_warmup": "0", "--weight_decay": "0", "--clip_norm": "1e-3",
            "--learning_rate": "1e-4"}[argv[0]]
    args = train.build_parser().parse_args([argv[0], good])
    assert getattr(args, argv[0][2:]) is not None and train.opt_recipe(args) is not None


# ---- argument validation before any HIP call (no GPU present)
def test_new_entry_points_validate_without_gpu():
    from jr import _ffi
    L = _ffi.load()
    P = 4096        # any non-null, 16-byte aligned address: validation fails before it is used
    assert L.jr_opt_set_hyper(None, 0.1, 0.0, 0.0, 1.0, None) == -1
    assert "opt_set_hyper" in _ffi.last_error()
    assert L.jr_grad_sqnorm_workspace_size(-1) == 0
    assert L.jr_grad_sqnorm_workspace_size(0) == 8 == L.jr_grad_sqnorm_workspace_size(1024)
    assert L.jr_grad_sqnorm_workspace_size(1025 + 3) == 16
    assert L.jr_grad_sqnorm_workspace_size(21770401) == 8 * 1024 == L.jr_grad_sqnorm_workspace_size(2 ** 40)
    assert L.jr_grad_sqnorm(None, 8, P, 8, None) == -1
    assert L.jr_grad_sqnorm(P, 8, None, 8, None) == -1
    assert L.jr_grad_sqnorm(P, -1, P, 8, None) == -1
    assert L.jr_grad_sqnorm(P, 4096, P, 8, None) == -1
    assert "workspace too small" in _ffi.last_error()
    assert L.jr_opt_prepare(None, 8, P, P, None) == -1
    assert L.jr_opt_prepare(P, 8, None, P, None) == -1
    assert L.jr_opt_prepare(P, 8, P, None, None) == -1
    assert L.jr_opt_prepare(P, -1, P, P, None) == -1
    for name in ("jr_nesterov_update_ex", "jr_momentum_update_ex"):
        fn = getattr(L, name)
        for args in ((None, P, P, 8, 0.9, P, 1, P, P, None), (P, None, P, 8, 0.9, P, 1, P, P, None),
                     (P, P, None, 8, 0.9, P, 1, P, P, None), (P, P, P, -1, 0.9, P, 1, P, P, None),
                     (P, P, P, 8, 0.9, P, -1, P, P, None), (P, P, P, 8, 0.9, None, 1, P, P, None),
                     (P, P, P, 8, 0.9, P, 1, None, P, None), (P, P, P, 8, 0.9, P, 1, P, None, None),
                     (P + 4, P, P, 8, 0.9, P, 1, P, P, None)):
            assert fn(*args) == -1, (name, args)
    for args in ((None, P, 8, P, 1, P, P, None), (P, None, 8, P, 1, P, P, None), (P, P, -1, P, 1, P, P, None),
                 (P, P, 8, P, -1, P, P, None), (P, P, 8, None, 1, P, P, None), (P, P, 8, P, 1, None, P, None),
                 (P, P, 8, P, 1, P, None, None)):
        assert L.jr_sgd_update_ex(*args) == -1, args
    for args in ((None, P, P, P, 8, 0.9, 0.999, 1e-8, P, 1, P, P, None), (P, None, P, P, 8, 0.9, 0.999, 1e-8, P, 1, P, P, None),
                 (P, P, None, P, 8, 0.9, 0.999, 1e-8, P, 1, P, P, None), (P, P, P, None, 8, 0.9, 0.999, 1e-8, P, 1, P, P, None),
                 (P, P, P, P, -1, 0.9, 0.999, 1e-8, P, 1, P, P, None), (P, P, P, P, 8, 0.9, 0.999, 1e-8, P, -1, P, P, None),
                 (P, P, P, P, 8, 0.9, 0.999, 1e-8, P, 1, None, P, None), (P, P, P, P, 8, 0.9, 0.999, 1e-8, P, 1, P, None, None)):
        assert L.jr_adam_update_ex(*args) == -1, args
    assert "adam_ex" in _ffi.last_error()


def test_quad_only_updates_refuse_misaligned_buffers():
    """jr_nesterov_update and the four _ex updates move quads only: a buffer at a
    4-byte but not 16-byte aligned address is refused, and the message says why."""
    from jr import _ffi
    L = _ffi.load()
    P = 4096
    calls = {      # what -> (number of buffers, call on them)
        "nesterov": (3, lambda w, g, a: L.jr_nesterov_update(w, g, a, 8, 0.1, 0.9, 1.0, None)),
        "nesterov_ex": (3, lambda w, g, a: L.jr_nesterov_update_ex(w, g, a, 8, 0.9, P, 1, P, P, None)),
        "momentum_ex": (3, lambda w, g, a: L.jr_momentum_update_ex(w, g, a, 8, 0.9, P, 1, P, P, None)),
        "sgd_ex": (2, lambda w, g: L.jr_sgd_update_ex(w, g, 8, P, 1, P, P, None)),
        "adam_ex": (4, lambda w, g, m, v: L.jr_adam_update_ex(w, g, m, v, 8, 0.9, 0.999, 1e-8, P, 1, P, P, None)),
    }
    for what, (nbuf, call) in calls.items():
        for k in range(nbuf):
            bufs = [P] * nbuf
            bufs[k] = P + 4
            assert call(*bufs) == -1, (what, k)
            assert _ffi.last_error().startswith(what + ":") and "16-byte aligned" in _ffi.last_error(), (what, k)
