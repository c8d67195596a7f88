"""numpy restatements of RMSProp and the weight average (TEST ORACLE ONLY).

float32 restatements, one rounding per operation in the order include/jr.h
states, of jr_rmsprop_update / jr_rmsprop_update_ex, jr_ema_set /
jr_ema_prepare and jr_ema_update, plus a float64 model that carries an
a-priori bound of the fp32 evaluation's error through every operation (Err).
"""
import numpy as np

from opt_ref import f32

U = 2.0 ** -24          # the unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -150      # half the smallest fp32 denormal: the absolute error of a result that underflows


def rmsprop_ref(w, g, mom, ms, scale, lr, weight_decay=0.0, mask=None, skipped=0, rho=0.9, momentum=0.9, eps=1.0):
    """One jr_rmsprop_update_ex step (jr_rmsprop_update: scale = grad_scale,
    weight decay 0).  Returns (w, mom, ms) as new float32 arrays."""
    w, mom, ms = (np.array(v, f32) for v in (w, mom, ms))
    if skipped:
        return w, mom, ms
    scale, lr, wd = f32(scale), f32(lr), f32(weight_decay)
    with np.errstate(all="ignore"):
        g = np.asarray(g, f32) * scale
        if wd != 0:
            g = np.where(mask, g + wd * w, g).astype(f32)
        ms = (ms + (g * g - ms) * (f32(1) - f32(rho))).astype(f32)
        mom = (mom * f32(momentum) + (g * lr) / np.sqrt(ms + f32(eps))).astype(f32)
        return (w - mom).astype(f32), mom, ms


def ema_set_ref(decay, warm=True, updates=0):
    """jr_ema_set: the jr_ema_state as a dict."""
    return {"decay": f32(decay), "one_minus_decay": f32(f32(1) - f32(decay)), "updates": int(updates),
            "warm": int(bool(warm))}


def warm_decay(decay, updates, warm=True):
    """The decay of update number `updates` (0-based; scalars or arrays): min(decay, (1 + t) / (10 + t))."""
    decay = f32(decay)
    if not warm:
        return decay
    t = np.asarray(updates).astype(f32)
    return np.minimum(decay, ((f32(1) + t) / (f32(10) + t)).astype(f32))


def ema_prepare_ref(state, skipped=0):
    """jr_ema_prepare: the next jr_ema_state."""
    st = dict(state)
    if skipped:
        st["one_minus_decay"] = f32(0)
        return st
    st["one_minus_decay"] = f32(f32(1) - warm_decay(st["decay"], st["updates"], st["warm"]))
    st["updates"] = st["updates"] + 1
    return st


def ema_update_ref(shadow, w, one_minus_decay, skipped=0):
    """jr_ema_update: shadow - (shadow - w) * one_minus_decay as a new float32 array."""
    shadow = np.array(shadow, f32)
    if skipped:
        return shadow
    with np.errstate(all="ignore"):
        return (shadow - (shadow - np.asarray(w, f32)) * f32(one_minus_decay)).astype(f32)


def ema_step_ref(shadow, w, state, skipped=0):
    """prepare + update: (shadow, state)."""
    state = ema_prepare_ref(state, skipped)
    return ema_update_ref(shadow, w, state["one_minus_decay"], skipped), state


class Err:
    """A float64 value `v` of an expression and a bound `e` of |fp32 evaluation - v|.

    Every fp32 operation returns the exact result of its (already inexact)
    operands times (1 + d), |d| <= U, or within TINY when it underflows; the
    operands' errors go through the operation by the first-order rules below
    with their second-order terms kept, so `e` is a bound, not an estimate.
    (The float64 arithmetic of v itself rounds by 2^-53 per operation: 2^-29
    of the fp32 roundings counted here, covered by the factor 1 + 2^-20.)"""

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, np.float64), np.asarray(e, np.float64) + np.zeros_like(v, np.float64)

    def _rounded(self, v, e):
        return Err(v, (e + U * (np.abs(v) + e) + TINY) * (1 + 2.0 ** -20))

    def __add__(self, o):
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        v = self.v / o.v
        lo = np.abs(o.v) - o.e
        assert np.all(lo > 0), "divisor not bounded away from zero"
        return self._rounded(v, (self.e + np.abs(v) * o.e) / lo)

    def sqrt(self):
        lo = self.v - self.e
        assert np.all(lo > 0), "sqrt argument not bounded away from zero"
        return self._rounded(np.sqrt(self.v), self.e / (2 * np.sqrt(lo)))     # |sqrt x - sqrt y| <= |x - y| / (2 sqrt(min))


def rmsprop_model(w, g, mom, ms, scale, lr, rho=0.9, momentum=0.9, eps=1.0):
    """One undecayed RMSProp step on exact fp32 inputs: (w, mom, ms) as Err."""
    c = lambda x: Err(np.float64(f32(x)))     # noqa: E731  (a constant: its fp32 value, exactly)
    w, g, mom, ms = (Err(np.asarray(x, f32)) for x in (w, g, mom, ms))
    g = g * c(scale)
    ms = ms + (g * g - ms) * (c(1) - c(rho))
    mom = mom * c(momentum) + (g * c(lr)) / (ms + c(eps)).sqrt()
    return w - mom, mom, ms
