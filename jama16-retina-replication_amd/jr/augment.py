"""Parameter tables of the on-device training augmentation
(jr_image_u8_augment_nhwc, include/jr.h): one jr_augment_param per image.

The transform itself runs in libjr (csrc/jr_augment.hip) inside the uint8 ->
float input conversion; this module only draws its per-image parameters on
the host.  The reference trains unaugmented, so nothing here is on unless
train.py gets --augment.
"""
from __future__ import annotations

from dataclasses import asdict, dataclass
from typing import Tuple

import numpy as np

# include/jr.h: struct jr_augment_param (32 bytes)
PARAM_DTYPE = np.dtype([("hue_delta", "<f4"), ("sat_factor", "<f4"), ("contrast_factor", "<f4"),
                        ("brightness_delta", "<f4"), ("flags", "<u4"), ("reserved", "<u4", (3,))])
assert PARAM_DTYPE.itemsize == 32

FLIP_LR, FLIP_UD = 1, 2


@dataclass(frozen=True)
class AugmentSpec:
    """Ranges of the per-image draws, all uniform: hue_delta in [-hue, hue]
    (turns of the colour circle), sat_factor and contrast_factor in their
    (lo, hi), brightness_delta in [-brightness, brightness] (of the [0, 1]
    pixel range); each flip with probability 1/2 when flip is on."""
    flip: bool = True
    hue: float = 0.2
    saturation: Tuple[float, float] = (0.5, 1.5)
    contrast: Tuple[float, float] = (0.5, 1.5)
    brightness: float = 0.125

    def __post_init__(self):
        if self.hue < 0 or self.brightness < 0:
            raise ValueError("hue and brightness ranges must be >= 0")
        for name in ("saturation", "contrast"):
            lo, hi = getattr(self, name)
            if not 0 <= lo <= hi:
                raise ValueError(f"{name} range must satisfy 0 <= lo <= hi")
            object.__setattr__(self, name, (float(lo), float(hi)))

    def to_meta(self) -> dict:
        """JSON-able form (the checkpoint .meta)."""
        d = asdict(self)
        d["saturation"], d["contrast"] = list(self.saturation), list(self.contrast)
        return d


def identity(n: int) -> np.ndarray:
    """[n] table that changes nothing (bitwise jr_image_u8_to_nhwc)."""
    t = np.zeros(n, PARAM_DTYPE)
    t["sat_factor"] = 1.0
    t["contrast_factor"] = 1.0
    return t


def _inside(x, lo: float, hi: float) -> np.ndarray:
    """float32 of the float64 draws x, kept inside [lo, hi] as real numbers
    (rounding to float32 can step one ulp past a bound)."""
    y = x.astype(np.float32)
    y = np.where(y.astype(np.float64) > hi, np.nextafter(y, np.float32(-np.inf)), y)
    return np.where(y.astype(np.float64) < lo, np.nextafter(y, np.float32(np.inf)), y)


def draw(spec: AugmentSpec, rng: np.random.Generator, n: int) -> np.ndarray:
    """[n] table of jr_augment_param drawn from `spec`.  The draws are made
    in a fixed order and number whatever the spec (a switched-off flip still
    consumes its bits), so the stream of a seed is stable."""
    t = identity(n)
    t["hue_delta"] = _inside(rng.uniform(-spec.hue, spec.hue, n), -spec.hue, spec.hue)
    t["sat_factor"] = _inside(rng.uniform(spec.saturation[0], spec.saturation[1], n), *spec.saturation)
    t["contrast_factor"] = _inside(rng.uniform(spec.contrast[0], spec.contrast[1], n), *spec.contrast)
    t["brightness_delta"] = _inside(rng.uniform(-spec.brightness, spec.brightness, n), -spec.brightness,
                                    spec.brightness)
    flags = rng.integers(0, 4, n, dtype=np.uint32)
    t["flags"] = flags if spec.flip else 0
    return t


def as_table(augment, n: int) -> np.ndarray:
    """Validate a caller's table: [n] of PARAM_DTYPE, or its [n, 8] uint32 view."""
    a = np.asarray(augment)
    if a.dtype != PARAM_DTYPE:
        if a.dtype != np.uint32 or a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("augment must be a jr.augment table ([n] jr_augment_param or its [n, 8] uint32 view)")
        a = np.ascontiguousarray(a).view(PARAM_DTYPE).reshape(-1)
    a = np.ascontiguousarray(a.reshape(-1))
    if a.shape[0] != n:
        raise ValueError(f"augment table has {a.shape[0]} entries for a batch of {n}")
    if np.any(a["reserved"] != 0) or np.any(a["flags"] > 3):
        raise ValueError("augment table: reserved words must be 0 and flags <= 3")
    return a
