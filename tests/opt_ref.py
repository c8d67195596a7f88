"""numpy restatements of the device optimizer recipe (TEST ORACLE ONLY).

float32 restatements, one rounding per operation in the order include/jr.h
states, of jr_opt_prepare and of the four jr_*_update_ex kernels (weight
decay inside the decay ranges, the step's scale, the skip), plus the float64
model of the prepare step and the exact sum of squares the norm is held to.
"""
import math

import numpy as np

f32 = np.float32


def exact_sqsum(g) -> float:
    """sum g_i^2, exactly rounded once (math.fsum of the exact fp64 squares)."""
    g = np.asarray(g, np.float64).ravel()
    return math.fsum((g * g).tolist())       # an fp32 value squared is exact in fp64


def sqsum_bound(n: int, S: float) -> float:
    """|S_dev - S| <= n * 2^-53 * S: the a-priori bound of ANY summation order
    of n non-negative fp64 terms (each of the n - 1 additions rounds by at most
    2^-53 of a partial sum that never exceeds S(1 + ...); the squares are exact)."""
    return n * 2.0 ** -53 * S


def prepare_ref(S, clip_norm, grad_scale):
    """jr_opt_prepare from the fp64 sum of squares S: (scale, grad_norm, skipped)."""
    with np.errstate(all="ignore"):
        gs, clip = f32(grad_scale), f32(clip_norm)
        n32 = f32(np.sqrt(np.float64(S)))
        gn = f32(n32 * gs)
        factor = f32(clip / gn) if (clip > 0 and gn > clip) else f32(1)
        scale = f32(gs * factor)
        if not np.isfinite(gn):
            return f32(0), gn, 1
        return scale, gn, 0


def prepare_f64(S, clip_norm, grad_scale):
    """The same step in float64 with fp32 range: (scale, grad_norm, skipped)."""
    S, clip, gs = float(S), float(clip_norm), float(grad_scale)
    gn = math.sqrt(S) * gs if S == S and S >= 0 else float("nan")
    if not (abs(gn) <= float(np.finfo(f32).max)):          # inf, NaN, or past the fp32 range
        return 0.0, gn, 1
    factor = clip / gn if (clip > 0 and gn > clip) else 1.0
    return gs * factor, gn, 0


def decay_mask(n, ranges):
    m = np.zeros(n, bool)
    for b, e in ranges:
        m[b:e] = True
    return m


def update_ref(opt, w, g, state, scale, lr, weight_decay, mask, skipped=0, momentum=0.9, beta1=0.9, beta2=0.999,
               eps=1e-8):
    """One jr_<opt>_update_ex step.  state: (accum,) for nesterov / momentum,
    () for sgd, (m, v) for adam; lr: hyper->lr (adam: the step's alpha).
    Returns (w, state) as new float32 arrays."""
    w = np.array(w, f32)
    state = tuple(np.array(s, f32) for s in state)
    if skipped:
        return w, state
    scale, lr, wd = f32(scale), f32(lr), f32(weight_decay)
    with np.errstate(all="ignore"):
        g = np.asarray(g, f32) * scale
        if wd != 0:
            g = np.where(mask, g + wd * w, g).astype(f32)
        if opt == "nesterov":
            m = f32(momentum)
            a = state[0] * m + g
            return (w - (g * lr + (a * m) * lr)).astype(f32), (a.astype(f32),)
        if opt == "momentum":
            a = state[0] * f32(momentum) + g
            return (w - a * lr).astype(f32), (a.astype(f32),)
        if opt == "sgd":
            return (w - g * lr).astype(f32), ()
        b1, b2 = f32(beta1), f32(beta2)
        m1 = state[0] + (g - state[0]) * (f32(1) - b1)
        v1 = state[1] + (g * g - state[1]) * (f32(1) - b2)
        return (w - (m1 * lr) / (np.sqrt(v1) + f32(eps))).astype(f32), (m1.astype(f32), v1.astype(f32))


def adam_alpha(lr, t, beta1=0.9, beta2=0.999):
    """The host's alpha of Adam step t (1-based): fp32, fp32 beta powers (Engine._adam_alpha)."""
    b1p, b2p = f32(beta1), f32(beta2)
    for _ in range(t - 1):
        b1p, b2p = f32(b1p * f32(beta1)), f32(b2p * f32(beta2))
    return f32(f32(lr) * np.sqrt(f32(1) - b2p)) / (f32(1) - b1p)
