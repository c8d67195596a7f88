"""numpy restatement of the training augmentation of include/jr.h
(jr_image_u8_augment_nhwc), formula for formula, in the dtype asked for: the
fp64 run is the tests' reference, the fp32 run sets their error bar.

Stage 0 (u8 -> f32(u8) * f32(1/255)) is always done in fp32, as the kernel
does it; every later stage runs in `dtype`.
"""
import numpy as np


def convert(u8):
    """Stage 0: [.., 3] uint8 -> float32."""
    return u8.astype(np.float32) * np.float32(1 / 255)


def _mod6(x, six):
    """floor-mod 6 with the result in [0, 6) also after rounding."""
    r = np.fmod(x, six)
    r = np.where(r < 0, r + six, r)
    return np.where(r >= six, r - six, r)


def hue_sat(x, hue_delta, sat_factor, dtype):
    """Stage 2 on [h, w, 3] of `dtype`."""
    T = dtype
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(r, np.maximum(g, b))
    m = np.minimum(r, np.minimum(g, b))
    c = v - m
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, c / v, T(0))
        h6 = np.where(c == 0, T(0),
                      np.where(v == r, (g - b) / c,
                               np.where(v == g, (b - r) / c + T(2), (r - g) / c + T(4))))
    h6 = h6.astype(T)
    h = _mod6(h6 + T(6) * T(hue_delta), T(6)).astype(T)
    s2 = np.clip(s * T(sat_factor), T(0), T(1)).astype(T)

    def f(n):
        k = _mod6(h + T(n), T(6))
        return v - v * s2 * np.clip(np.minimum(k, T(4) - k), T(0), T(1))

    return np.stack([f(5), f(3), f(1)], axis=-1).astype(T)


def augment_image(u8, p, dtype=np.float64):
    """One [h, w, 3] uint8 image with one parameter record p (fields of
    jr.augment.PARAM_DTYPE) -> [h, w, 3] of `dtype`, clamped to [0, 1]."""
    T = np.dtype(dtype).type
    x = convert(u8)
    flags = int(p["flags"])
    if flags & 1:
        x = x[:, ::-1]
    if flags & 2:
        x = x[::-1]
    x = x.astype(T)
    hd, sf = np.float32(p["hue_delta"]), np.float32(p["sat_factor"])
    cf, bd = np.float32(p["contrast_factor"]), np.float32(p["brightness_delta"])
    if not (hd == 0 and sf == 1):
        x = hue_sat(x, hd, sf, T)
    if cf != 1:
        mean = x.reshape(-1, 3).mean(axis=0, dtype=T)
        x = (x - mean) * T(cf) + mean
    if bd != 0:
        x = x + T(bd)
    return np.clip(x, T(0), T(1)).astype(T)


def augment_batch(u8, table, dtype=np.float64):
    """[n, h, w, 3] uint8 and an [n] parameter table -> [n, h, w, 3] of `dtype`."""
    return np.stack([augment_image(u8[i], table[i], dtype) for i in range(len(u8))])
