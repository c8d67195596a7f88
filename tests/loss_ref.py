"""Reference models of the loss recipe and of dropout (include/jr.h; no tests
here: test_loss_recipe.py checks these models on the CPU, test_gpu_loss_recipe.py
checks libjr against them).

* sigmoid_recipe / softmax_recipe: the fp64 models of jr_head_fwd_ex /
  jr_head_bwd_ex (loss, probabilities, dloss/dz), every term from the logit in
  the stable forms jr.h names;
* sigmoid_recipe_loss_f32: the same sigmoid loss restated in numpy float32 --
  the yardstick of the focal term's error bar (an independent fp32 evaluation
  with numpy's power in place of the device's powf);
* philox4x32_10, dropout_state, dropout_mask, dropout_apply: the generator and
  the mask, bit for bit what jr_dropout.hip computes.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


# ------------------------------------------------------------------ the loss
def _softplus(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1 / (1 + e), e / (1 + e))


def _pow(x, g):
    return np.ones_like(x) if g == 0 else np.power(x, g)


def sigmoid_terms(z, y, eps, cw, gamma, dtype=np.float64):
    """Per-element loss and dloss/dz (no mean) of the sigmoid recipe in `dtype`; cw: one weight per unit."""
    z, y = np.asarray(z, dtype), np.asarray(y, dtype)
    eps, gamma, half, one = dtype(eps), dtype(gamma), dtype(0.5), dtype(1)
    c = np.asarray(cw, dtype).reshape(1, -1)
    t = y * (one - eps) + eps * half
    p, q = _sigmoid(z).astype(dtype), _sigmoid(-z).astype(dtype)
    spz, spn = _softplus(z).astype(dtype), _softplus(-z).astype(dtype)
    qg, pg = _pow(q, gamma), _pow(p, gamma)
    loss = c * t * qg * spn + (one - t) * pg * spz
    dz = -c * t * qg * (gamma * p * spn + q) + (one - t) * pg * (gamma * q * spz + p)
    return loss, p, dz


def sigmoid_recipe(z, y, eps=0.0, cw=None, gamma=0.0):
    """fp64: (loss, probs, dloss/dz) of jr_head_fwd_ex / jr_head_bwd_ex, JR_HEAD_SIGMOID; z, y: [n][units]."""
    z = np.asarray(z, np.float64)
    cw = np.ones(z.shape[1]) if cw is None else cw
    loss, p, dz = sigmoid_terms(z, y, eps, cw, gamma)
    return float(loss.mean()), p, dz / z.size


def sigmoid_recipe_loss_f32(z, y, eps=0.0, cw=None, gamma=0.0):
    """The sigmoid loss evaluated in numpy float32 from float32 logits (the mean summed in fp64, as the kernel's)."""
    z = np.asarray(z, np.float32)
    cw = np.ones(z.shape[1]) if cw is None else cw
    loss, _, _ = sigmoid_terms(z, y, eps, cw, gamma, dtype=np.float32)
    assert loss.dtype == np.float32
    return float(loss.astype(np.float64).mean())


def softmax_recipe(z, y, eps=0.0, cw=None):
    """fp64: (loss, probs, dloss/dz) of the softmax recipe; z, y: [n][units]."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    n, units = z.shape
    c = np.ones(units) if cw is None else np.asarray(cw, np.float64)
    zm = z - z.max(axis=1, keepdims=True)
    se = np.exp(zm).sum(axis=1, keepdims=True)
    p, lse = np.exp(zm) / se, np.log(se)
    t = y * (1 - eps) + eps / units
    s = (y * c).sum(axis=1, keepdims=True)
    loss = float(np.mean(s * np.sum(t * (lse - zm), axis=1, keepdims=True)))
    dz = s * (p * t.sum(axis=1, keepdims=True) - t) / n
    return loss, p, dz


# -------------------------------------------------------------------- dropout
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32
    scalars -> the four output words, uint32 arrays of that shape."""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) for v in counter]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(v, shape).copy() for v in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]        # < 2^64: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK32]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def dropout_state(key0, key1, rate, step=0):
    """What jr_dropout_set stores: rate travels as a C float."""
    rate = float(np.float32(rate))
    assert 0.0 <= rate < 1.0
    threshold = int(np.floor(rate * 2.0 ** 32))
    scale = np.float32(1.0 / (1.0 - threshold / 2.0 ** 32))
    return {"key": (int(key0) & 0xFFFFFFFF, int(key1) & 0xFFFFFFFF), "step": int(step) & 0xFFFFFFFF,
            "threshold": threshold, "scale": scale}


def dropout_advance(state):
    return dict(state, step=(state["step"] + 1) & 0xFFFFFFFF)


def dropout_mask(n, state):
    """keep[i] of elements 0..n-1: word i & 3 of philox((lo32(i >> 2), hi32(i >> 2), step, 0), key) >= threshold."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((q & _MASK32, q >> np.uint64(32), np.uint64(state["step"]), np.uint64(0)), state["key"])
    r = np.stack(words, axis=1).reshape(-1)[:n]
    return r >= np.uint32(state["threshold"]) if state["threshold"] else np.ones(n, bool)


def dropout_apply(x, state):
    """keep ? x * scale : 0.0f, one float32 multiply per element."""
    x = np.asarray(x, np.float32)
    keep = dropout_mask(x.size, state).reshape(x.shape)
    return np.where(keep, x * state["scale"], np.float32(0.0)).astype(np.float32)
