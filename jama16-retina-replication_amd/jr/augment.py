"""Parameter tables of the on-device training augmentation
(jr_image_u8_augment_nhwc, include/jr.h): one jr_augment_param per image.

The transform itself runs in libjr (csrc/jr_augment.hip) inside the uint8 ->
float input conversion; this module only draws its per-image parameters on
the host.  The reference trains unaugmented, so nothing here is on unless
train.py gets --augment.

The second half holds the tables of jr_image_u8_warp_augment_nhwc (one
jr_warp_param per image: rotation, zoom, shift), drawn for training by
train.py --augment_rotate / --augment_zoom / --augment_shift, and the fixed
views of test-time augmentation (evaluate.py --tta).
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


# ---------------------------------------------------------------- geometry
# jr_image_u8_warp_augment_nhwc: one jr_warp_param per image beside the
# jr_augment_param, a 2 x 3 matrix from destination pixel (x, y) to the source
# position (u, v) that the kernel samples bilinearly (include/jr.h)

# include/jr.h: struct jr_warp_param (32 bytes)
WARP_DTYPE = np.dtype([("m", "<f4", (6,)), ("reserved", "<u4", (2,))])
assert WARP_DTYPE.itemsize == 32

IDENTITY_MATRIX = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def warp_identity(n: int) -> np.ndarray:
    """[n] warp table that resamples nothing (bitwise jr_image_u8_augment_nhwc)."""
    t = np.zeros(n, WARP_DTYPE)
    t["m"] = IDENTITY_MATRIX
    return t


def as_warp_table(warp, n: int) -> np.ndarray:
    """Validate a caller's warp table: [n] of WARP_DTYPE, or its [n, 8] uint32 view."""
    a = np.asarray(warp)
    if a.dtype != WARP_DTYPE:
        if a.dtype != np.uint32 or a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("warp must be a jr.augment warp table ([n] jr_warp_param or its [n, 8] uint32 view)")
        a = np.ascontiguousarray(a).view(WARP_DTYPE).reshape(-1)
    a = np.ascontiguousarray(a.reshape(-1))
    if a.shape[0] != n:
        raise ValueError(f"warp table has {a.shape[0]} entries for a batch of {n}")
    if np.any(a["reserved"] != 0):
        raise ValueError("warp table: reserved words must be 0")
    return a


def batch_tables(n: int, augment=None, warp=None) -> tuple:
    """(colour table, warp table or None) of a batch of n as an upload takes them, validated;
    (None, None) without either.  A warp alone goes with the identity colour table."""
    if augment is None and warp is None:
        return None, None
    return identity(n) if augment is None else as_table(augment, n), None if warp is None else as_warp_table(warp, n)


def warp_matrix(h: int, w: int, degrees: float = 0.0, zoom: float = 1.0, dx: float = 0.0, dy: float = 0.0) -> np.ndarray:
    """float32[6] matrix of a rotation by `degrees` and a magnification by
    `zoom` about the image centre c = ((w-1)/2, (h-1)/2), the content then
    moved by (dx, dy) pixels: source = A (dest - c - d) + c with A = R(degrees)
    / zoom, R = [[cos, -sin], [sin, cos]].  Computed in fp64, rounded once.
    Multiples of 90 degrees use cos, sin in {0, +-1} exactly, so on a square
    image degrees = 90 k is np.rot90(image, k), a pure permutation."""
    if not zoom > 0:
        raise ValueError("zoom must be > 0")
    q = float(degrees) / 90.0
    if q == round(q):
        cos, sin = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(round(q)) % 4]
    else:
        cos, sin = np.cos(np.deg2rad(float(degrees))), np.sin(np.deg2rad(float(degrees)))
    a00, a01, a10, a11 = cos / zoom, -sin / zoom, sin / zoom, cos / zoom
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    tx, ty = cx + float(dx), cy + float(dy)
    m = np.array([a00, a01, cx - (a00 * tx + a01 * ty), a10, a11, cy - (a10 * tx + a11 * ty)], np.float64)
    return (m + 0.0).astype(np.float32)      # (+ 0.0: no negative zeros, the identity is the identity's bytes)


@dataclass(frozen=True)
class WarpSpec:
    """Ranges of the per-image geometric draws, all uniform: the rotation in
    [-rotate, rotate] degrees, the zoom in its (lo, hi), each shift in
    [-shift, shift] as a fraction of that side of the image."""
    rotate: float = 180.0
    zoom: Tuple[float, float] = (0.9, 1.1)
    shift: float = 0.05

    def __post_init__(self):
        if self.rotate < 0 or self.shift < 0:
            raise ValueError("rotate and shift ranges must be >= 0")
        lo, hi = self.zoom
        if not 0 < lo <= hi:
            raise ValueError("zoom range must satisfy 0 < lo <= hi")
        object.__setattr__(self, "zoom", (float(lo), float(hi)))

    def to_meta(self) -> dict:
        """JSON-able form (the checkpoint .meta)."""
        d = asdict(self)
        d["zoom"] = list(self.zoom)
        return d


def draw_warp(spec: WarpSpec, rng: np.random.Generator, n: int, h: int, w: int) -> np.ndarray:
    """[n] table of jr_warp_param drawn from `spec` for h x w images: n
    rotations, n zooms, n x shifts, n y shifts, in that order and number
    whatever the spec.  `rng` is the caller's generator for the geometry
    alone: draw() and its stream are not involved."""
    deg = rng.uniform(-spec.rotate, spec.rotate, n)
    zoom = rng.uniform(spec.zoom[0], spec.zoom[1], n)
    dx = rng.uniform(-spec.shift, spec.shift, n) * w
    dy = rng.uniform(-spec.shift, spec.shift, n) * h
    t = warp_identity(n)
    for i in range(n):
        t["m"][i] = warp_matrix(h, w, deg[i], zoom[i], dx[i], dy[i])
    return t


def d4_views(h: int, w: int) -> list:
    """The 8 (flags, matrix) views of the dihedral group of a square image:
    quarter turns 0, 90, 180, 270, then the same four with flags = FLIP_LR.
    View k of a batch x is np.rot90(x, k % 4, axes=(1, 2)), mirrored left-right
    when k >= 4; every view is a pure permutation of the pixels."""
    if h != w:
        raise ValueError(f"the quarter turns need a square image, got {h} x {w}")
    return [(flags, warp_matrix(h, w, 90.0 * k)) for flags in (0, FLIP_LR) for k in range(4)]


def flip_views() -> list:
    """The 4 (flags, matrix) views of the two flips: flags 0, 1, 2, 3 with the identity matrix."""
    return [(flags, np.array(IDENTITY_MATRIX, np.float32)) for flags in range(4)]


def view_tables(view, n: int) -> tuple:
    """(augment table, warp table) that show one (flags, matrix) view of a batch of n, colours untouched."""
    flags, matrix = view
    tab, warp = identity(n), warp_identity(n)
    tab["flags"] = flags
    warp["m"] = matrix
    return tab, warp
