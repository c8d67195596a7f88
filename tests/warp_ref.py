"""numpy restatement of jr_image_u8_warp_augment_nhwc (include/jr.h), formula
for formula, in the dtype asked for: stage 1 (flip, source position, outside
test, four guarded taps, two lerps) here, stages 2 - 5 as tests/augment_ref.py
has them.  The fp64 run is the tests' reference, the fp32 run sets their bar.

Stage 0 (u8 -> f32(u8) * f32(1/255)) is always done in fp32, as the kernel
does it; the matrix entries are the table's float32 values; everything after
them runs in `dtype`, every operation rounded on its own.
"""
import numpy as np

import augment_ref


def warp_stage(u8, flags, m, dtype=np.float64):
    """Stage 1 of one [h, w, 3] uint8 image -> ([h, w, 3] of `dtype`, the
    [h, w] mask of destination pixels that passed the outside test)."""
    T = np.dtype(dtype).type
    h, w, _ = u8.shape
    src = augment_ref.convert(u8).astype(T)
    m = [T(np.float32(v)) for v in m]
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    if flags & 1:
        x = w - 1 - x
    if flags & 2:
        y = h - 1 - y
    xf, yf = x.astype(T), y.astype(T)
    with np.errstate(all="ignore"):
        u = (m[0] * xf + m[1] * yf) + m[2]
        v = (m[3] * xf + m[4] * yf) + m[5]
        inside = (u > -1) & (u < w) & (v > -1) & (v < h)        # False for NaN and +-inf
        u, v = np.where(inside, u, T(0)), np.where(inside, v, T(0))
    x0f, y0f = np.floor(u), np.floor(v)
    fx, fy = (u - x0f)[..., None], (v - y0f)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)

    def tap(i, j):
        xs, ys = x0 + i, y0 + j
        ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
        p = src[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)]
        return np.where(ok[..., None], p, T(0))

    p00, p10, p01, p11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
    top = p00 + fx * (p10 - p00)
    bot = p01 + fx * (p11 - p01)
    out = top + fy * (bot - top)
    return np.where(inside[..., None], out, T(0)).astype(T), inside


def warp_image(u8, p, wp, dtype=np.float64):
    """One [h, w, 3] uint8 image with its jr_augment_param p and jr_warp_param
    wp -> [h, w, 3] of `dtype`, clamped to [0, 1]."""
    T = np.dtype(dtype).type
    x, _ = warp_stage(u8, int(p["flags"]), wp["m"], T)
    hd, sf = np.float32(p["hue_delta"]), np.float32(p["sat_factor"])
    cf, bd = np.float32(p["contrast_factor"]), np.float32(p["brightness_delta"])
    if not (hd == 0 and sf == 1):
        x = augment_ref.hue_sat(x, hd, sf, T)
    if cf != 1:
        mean = x.reshape(-1, 3).mean(axis=0, dtype=T)      # over every destination pixel, fill included
        x = (x - mean) * T(cf) + mean
    if bd != 0:
        x = x + T(bd)
    return np.clip(x, T(0), T(1)).astype(T)


def warp_batch(u8, table, warps, dtype=np.float64):
    """[n, h, w, 3] uint8, an [n] parameter table and an [n] warp table -> [n, h, w, 3] of `dtype`."""
    return np.stack([warp_image(u8[i], table[i], warps[i], dtype) for i in range(len(u8))])


def inside_fraction(u8, table, warps):
    """Per image, the share of destination pixels sampled from inside the source (fp64)."""
    return np.array([warp_stage(u8[i], int(table[i]["flags"]), warps[i]["m"], np.float64)[1].mean()
                     for i in range(len(u8))])
