"""The numpy model of the JR_F32_X6H split (x6h_model.py), checked on the CPU:
pow2_scale and the three-way truncation against what include/jr.h promises,
and, for every case test_gpu_x6h_scales.py runs (the same generated inputs),
that the model itself meets the contract against fp64 and that the case would
notice a wrong kernel: a model with fp16 subnormals flushed, or with an
operand's scale off by a factor of two, differs from the model by at least 4x
the case's bar on at least a tenth of its outputs.  (A GPU case that could not
tell these apart would pass on a kernel that is wrong in exactly the way the
case exists to catch.)"""
import numpy as np
import pytest

from oracle import tf_ops as R

import x6h_model as X

F32 = np.float32


def _f32_grid(e_lo, e_hi, seed):
    """fp32 values of both signs over binades e_lo .. e_hi: the power of two,
    its two neighbours, an all-ones and a single-low-bit significand, and
    random significands."""
    rng = np.random.default_rng(seed)
    out = []
    for e in range(e_lo, e_hi + 1):
        p = F32(2.0) ** F32(e)
        edge = [p, np.nextafter(p, F32(0)), np.nextafter(p, F32(np.inf)), np.nextafter(2 * p, F32(0))]
        out += edge + list((p * rng.uniform(1, 2, 24)).astype(F32))
    v = np.array(out, F32)
    return np.concatenate([v, -v])


# ---------------------------------------------------------------- the scale
def test_pow2_scale_puts_the_magnitude_in_2_14_2_15():
    for eb in range(41, 255):                        # 268 - eb <= 227: no clamp
        p = F32(2.0) ** F32(eb - 127)
        s = X.pow2_scale(p)
        assert np.frexp(s)[0] == 0.5                 # a power of two
        assert float(p) * s == 2.0 ** 14
        if eb < 254:
            for m in (np.nextafter(2 * p, F32(0)), F32(float(p) * 1.37)):
                assert 2.0 ** 14 <= float(m) * X.pow2_scale(m) < 2.0 ** 15, m
        below = np.nextafter(p, F32(0))              # the binade below, all ones
        if eb > 41:
            assert 2.0 ** 14 <= float(below) * X.pow2_scale(below) < 2.0 ** 15


def test_pow2_scale_clamp_and_defaults():
    assert X.pow2_scale(F32(2.0) ** F32(-86)) == 2.0 ** 100          # the last unclamped exponent
    for m in (F32(2.0) ** F32(-87), F32(2.0) ** F32(-100), F32(1e-38), F32(1e-45)):   # down to subnormals
        assert X.pow2_scale(m) == 2.0 ** 100
    assert X.pow2_scale(np.nextafter(F32(np.inf), F32(0))) == 2.0 ** -113
    for m in (0.0, -0.0, -1.0, -np.inf, np.inf, np.nan):
        assert X.pow2_scale(m) == 1.0


# ---------------------------------------------------------------- the split
def test_rtz16_is_fp16_truncation():
    """Against an independent route: numpy's round-to-nearest fp16, stepped
    one fp16 toward zero where it rounded away."""
    v = _f32_grid(-30, 15, 1).astype(np.float64)
    got = X.rtz16(v)
    with np.errstate(over="ignore"):
        rn = v.astype(np.float16)
    away = np.abs(rn.astype(np.float64)) > np.abs(v)
    want = np.where(away, np.nextafter(rn, np.float16(0)), rn).astype(np.float64)
    assert np.array_equal(got, want)
    assert np.array_equal(got.astype(np.float16).astype(np.float64), got)      # representable, subnormals included
    fl = X.rtz16(v, flush=True)
    assert np.array_equal(fl, np.where(np.abs(got) < 2.0 ** -14, 0.0, got))
    assert np.all(X.rtz16(np.array([65520.0, 1e6, -1e6])) == [65504.0, 65504.0, -65504.0])


@pytest.mark.parametrize("s", [1.0, 4.0, 2.0 ** -86, 2.0 ** 100])
def test_split_is_exact_from_2_m1(s):
    xs0 = _f32_grid(-1, 15, 2)
    xs0 = xs0[np.abs(xs0) >= 0.5]                                # |xs| in [2^-1, 2^16)
    x = (xs0.astype(np.float64) / s).astype(F32)
    xs, h, m, l = X.split(x, s)                                  # noqa: E741
    assert np.array_equal(xs, xs0.astype(np.float64))            # (x s is exact: s a power of two)
    assert np.array_equal(h + m + l, xs)
    assert np.array_equal((h + m + l) / s, x.astype(np.float64))


def test_split_below_the_exact_range():
    xs0 = _f32_grid(-40, -2, 3)
    xs, h, m, l = X.split(xs0, 1.0)                              # noqa: E741
    assert np.all(np.abs(xs - (h + m + l)) < 2.0 ** -24)
    assert np.all(np.abs(h) >= np.abs(m)) and np.all(np.abs(m) >= np.abs(l))
    # truncation toward zero: every partial sum stays on xs's side of zero and
    # never passes it, every term has the remainder's sign
    for part in (h, h + m, h + m + l):
        assert np.all(np.abs(part) <= np.abs(xs)) and np.all(part * xs >= 0)
    assert np.all(m * (xs - h) >= 0) and np.all(l * (xs - h - m) >= 0)
    for t in (h, m, l):
        assert np.array_equal(t.astype(np.float16).astype(np.float64), t)
    assert np.any(np.abs(l[l != 0]) < 2.0 ** -14) and np.any(np.abs(m[m != 0]) < 2.0 ** -14)   # subnormals at work
    assert np.all(h[np.abs(xs) < 2.0 ** -24] == 0)


# ------------------------------------------------------------- the wrapper
@pytest.mark.parametrize("op", X.OPS)
@pytest.mark.parametrize("case", [(2, 7, 6, 8, 16, 3, 3, 2, "valid"), (1, 5, 7, 3, 16, 3, 5, 1, "same"),
                                  (2, 9, 8, 4, 16, 5, 3, 2, "valid")])
def test_conv_as_gemm_is_the_oracle(op, case):
    """operands(): A @ B in fp64 is oracle.tf_ops' conv, and S bounds it."""
    n, h, wd, cin, cout, kh, kw, s, pad = case
    _, _, ho, wo = X.geometry(case)
    rng = np.random.default_rng(5)
    x, w, dy = (rng.standard_normal(sh).astype(F32) for sh in ((n, h, wd, cin), (kh, kw, cin, cout), (n, ho, wo, cout)))
    A, B, K, shape = X.operands(op, case, x, w, dy)
    got = (A.astype(np.float64) @ B.astype(np.float64)).reshape(shape)
    _, exact, S, _ = X.conv(op, case, x, w, dy, 1.0, 1.0)
    assert np.max(np.abs(got - exact)) <= 1e-13 * S.max()
    assert np.all(np.abs(exact) <= S * (1 + 1e-12))
    if op == "dgrad":       # the reduction length per stride phase: taps that hit dy at all
        assert set(np.unique(K)) <= {cout * a * b for a in range(kh + 1) for b in range(kw + 1)}
        assert K.max() == cout * -(-kh // s) * -(-kw // s)


# ---------------------------------------------- every GPU case, on the CPU
ALL = X.ladder_cases() + X.mixed_cases() + X.grouped_cases() + X.ordinary_cases()


def _operand_contract(t, s):
    """jr.h: exact for |x s| >= 2^-1, within 2^-24 / s below."""
    xs, h, m, l = X.split(t, s)                                  # noqa: E741
    err = np.abs(t.astype(np.float64) - (h + m + l) / s)
    big = np.abs(xs) >= 0.5
    assert np.all(np.abs(xs) < 2.0 ** 16)                        # the stated magnitude holds (twice it at most)
    assert np.all(err[big] == 0)
    assert np.all(err[~big] < 2.0 ** -24 / s)


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_gpu_case_conditions(case):
    (x, w, dy), stated = case.make()
    sa, sb = X.scales(case.op, stated)
    a, b = {"fwd": (x, w), "dgrad": (dy, w), "wgrad": (x, dy)}[case.op]
    _operand_contract(a, sa)
    _operand_contract(b, sb)
    model, exact, S, K = X.conv(case.op, case.geom, x, w, dy, sa, sb)
    assert np.all(np.isfinite(model))
    # the model against fp64 at the outputs: each operand element is off by
    # less than 2^-24 / s (none where exact), the dropped ml + lm + ll are
    # below 2^-28 |a b| (|m| <= 2^-10 |h|, |l| <= 2^-10 |m|, with room)
    A, B, _, shape = X.operands(case.op, case.geom, x, w, dy)
    allow = ((A != 0).astype(np.float64) @ np.abs(B).astype(np.float64) * 2.0 ** -24 / sa +
             np.abs(A).astype(np.float64) @ (B != 0).astype(np.float64) * 2.0 ** -24 / sb).reshape(shape) + 2.0 ** -28 * S
    assert np.all(np.abs(model - exact) <= allow)
    # every output must be an ordinary fp32 number (or exactly 0): the cases
    # pair tiny with huge magnitudes so that the bar never meets fp32's range
    nz = model != 0
    assert np.all(np.abs(model[nz]) >= 2.0 ** -120) and np.all(S < 2.0 ** 120)
    bar = X.bar(K, S)
    if case.id.startswith("ordinary"):
        # the model leaves the fp32 bars of test_gpu_x6h.py to the kernel's
        # accumulation: it is within 1 % of them itself
        lim = 5e-6 if case.op == "fwd" else 1e-5
        assert np.max(np.abs(model - exact)) <= 0.01 * lim * np.max(np.abs(exact))
    for mut in case.mutations:
        wrong = X.mutated(case.op, case.geom, (x, w, dy), stated, mut)
        seen = np.abs(wrong - model) >= 4 * bar
        print(case.id, mut, "seen on", float(np.mean(seen)))
        assert np.mean(seen) >= 0.1, (mut, float(np.mean(seen)))


def test_ladders_hold_what_the_issue_lists():
    """Rungs -1 .. 40 on rows and columns of every ladder; every way of
    stating a magnitude on both operands; the listed magnitudes."""
    kinds_a = {m[0] for m in X.LADDER_MAGS}
    kinds_b = {m[2] for m in X.LADDER_MAGS}
    assert kinds_a == kinds_b == {"w0", "w31", "w63", "bnd", "zero"}
    vals = {m[1] for m in X.LADDER_MAGS} | {m[3] for m in X.LADDER_MAGS}
    assert {4096.0, 2048.0, 1.0, X.P2(-100), X.P2(100), X.BELOW(4096.0)} <= vals
    for op in X.OPS:
        (x, w, dy), ra, rb = X.ladder_case(op, X.LADDER_MAGS[0])
        assert set(ra) == set(rb) == set(range(-1, 41)) and max(len(ra), len(rb)) >= 64
        A, B, K, _ = X.operands(op, X.LADDER_GEOM[op], x, w, dy)
        assert np.all(np.asarray(K) == 16) and np.all(A > 0) and np.all(B > 0)
        top = (A.max(1) / 4096.0, B.max(0) / 1.0)          # rung k: bound 2^-k U[0.5, 1)
        for t, r in zip(top, (ra, rb)):
            assert np.all(t < 2.0 ** -r.astype(float)) and np.all(t >= 2.0 ** (-r.astype(float) - 1))
        (_, _, _), ra, _ = X.ladder_case(op, ("bnd", X.BELOW(8.0), "bnd", 1.0))
        assert ra.min() == 0                                # no power of two: no rung above the bound
