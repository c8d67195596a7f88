"""numpy float32 restatement of jr_grad_accumulate (include/jr.h) and of the
group planner jr.schedule.accum_groups (no tests here; see test_accum.py and
test_gpu_accum.py).

    dst[i] = first ? src[i] : dst[i] + src[i]

one correctly rounded fp32 add per element (numpy's float32 add is IEEE:
denormals kept, round to nearest even), `first` a copy that never reads dst.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

f32 = np.float32


def accumulate(dst: np.ndarray, src: np.ndarray, first: bool) -> np.ndarray:
    """What jr_grad_accumulate leaves in dst."""
    dst, src = np.asarray(dst, f32), np.asarray(src, f32)
    assert dst.shape == src.shape
    if first:
        return src.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        return (dst + src).astype(f32)


def closed_gradient(grads) -> np.ndarray:
    """The gradient a group's closing step hands the optimizer: acc <- g0,
    acc <- acc + g1, ..., g <- g_last + acc -- by commutativity the left-to-right
    sum ((g0 + g1) + g2) + ... in micro-batch order."""
    grads = [np.asarray(g, f32) for g in grads]
    if len(grads) == 1:
        return grads[0].copy()
    acc = accumulate(np.full_like(grads[0], np.nan), grads[0], True)
    for g in grads[1:-1]:
        acc = accumulate(acc, g, False)
    return accumulate(grads[-1], acc, False)


def groups(batches: int, accum_steps: int) -> Tuple[List[int], int]:
    """(group sizes in order, number of updates) of an epoch of `batches`
    micro-batches: full groups of accum_steps, then the remainder if any."""
    sizes, left = [], int(batches)
    while left > 0:
        sizes.append(min(int(accum_steps), left))
        left -= sizes[-1]
    return sizes, len(sizes)


def special_values(n: int, seed: int, nans: int = 4) -> np.ndarray:
    """n float32 values for the kernel test: normal draws over many binades,
    with +-0, +-denormals, +-inf and exactly `nans` NaNs where n leaves room
    (the specials are dropped from the end as n shrinks; NaNs only from n >= 16)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(f32)
    specials = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, np.inf, -np.inf]
    if n >= 16:
        pos = rng.choice(n, size=len(specials) + nans, replace=False)
        x[pos[:len(specials)]] = np.array(specials, f32)
        x[pos[len(specials):]] = np.nan
    else:
        k = min(n, len(specials))
        x[:k] = np.array(specials[:k], f32)
    return x
