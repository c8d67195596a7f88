"""Geometric augmentation and test-time views, the parts that need no GPU:
argument validation of jr_image_u8_warp_augment_nhwc, the warp tables of
jr.augment, train.py's flags and the numpy restatement tests/warp_ref.py on
the matrices that must be pure permutations."""
import ctypes

import numpy as np
import pytest

import warp_ref


def _call(L, src=16, dst=16, dtype=0, n=2, h=13, w=21, c=3, ds=4, params=16, warps=16, ws=16, ws_bytes=1 << 20):
    return L.jr_image_u8_warp_augment_nhwc(src, dst, dtype, n, h, w, c, ds, params, warps, ws, ws_bytes, None)


def test_abi_validation_without_gpu():
    from jr import _ffi
    L = _ffi.load()
    for kw, text in (({"src": None}, "null"), ({"dst": None}, "null"), ({"params": None}, "null"),
                     ({"warps": None}, "null"), ({"ws": None}, "null"), ({"c": 4}, "c must be 3"),
                     ({"c": 1}, "c must be 3"), ({"ds": 2}, "dst_stride"), ({"dtype": 2}, "dtype"),
                     ({"dtype": 4}, "dtype"), ({"dtype": -1}, "dtype"), ({"ws_bytes": 0}, "workspace")):
        assert _call(L, **kw) == -1, kw
        assert text in _ffi.last_error() and "image_u8_warp_augment" in _ffi.last_error(), (kw, _ffi.last_error())
    need = L.jr_augment_workspace_size(2, 13, 21)
    assert _call(L, ws_bytes=need - 1) == -1 and "workspace" in _ffi.last_error()
    assert _call(L, n=0) == 0       # nothing to do, nothing launched


def test_warp_layout_matches_the_header():
    from jr import _ffi, augment
    assert augment.WARP_DTYPE.itemsize == 32 == ctypes.sizeof(_ffi.WarpParam)
    for name, _ in _ffi.WarpParam._fields_:
        assert augment.WARP_DTYPE.fields[name][1] == getattr(_ffi.WarpParam, name).offset
    assert "jr_image_u8_warp_augment_nhwc" in _ffi.EXPORTED


def test_identity_and_as_warp_table():
    from jr import augment
    t = augment.warp_identity(3)
    assert t.dtype.itemsize == 32 and np.all(t["reserved"] == 0)
    assert np.array_equal(t["m"], np.tile(np.float32([1, 0, 0, 0, 1, 0]), (3, 1)))
    assert augment.as_warp_table(t.view(np.uint32).reshape(3, 8), 3).tobytes() == t.tobytes()
    with pytest.raises(ValueError):
        augment.as_warp_table(t, 2)
    with pytest.raises(ValueError):
        augment.as_warp_table(augment.identity(3), 3)       # the colour table is not a warp table
    bad = t.copy()
    bad["reserved"][1, 0] = 1
    with pytest.raises(ValueError):
        augment.as_warp_table(bad, 3)
    for kw in (dict(zoom=(1.1, 0.9)), dict(zoom=(0.0, 1.0)), dict(rotate=-1.0), dict(shift=-0.1)):
        with pytest.raises(ValueError):
            augment.WarpSpec(**kw)
    assert augment.WarpSpec().to_meta() == {"rotate": 180.0, "zoom": [0.9, 1.1], "shift": 0.05}


@pytest.mark.parametrize("size", [17, 64])
def test_lattice_matrices_have_integer_entries(size):
    from jr import augment
    mats = [augment.warp_matrix(size, size, 90.0 * k) for k in range(-1, 6)]
    mats += [m for _, m in augment.d4_views(size, size)] + [m for _, m in augment.flip_views()]
    mats += [np.float32([-1, 0, size - 1, 0, 1, 0]), np.float32([1, 0, 0, 0, -1, size - 1])]   # the two flips
    for m in mats:
        assert m.dtype == np.float32 and m.shape == (6,)
        assert np.array_equal(m, np.round(m)) and np.all(np.abs(m[[0, 1, 3, 4]]) <= 1), m
    assert np.array_equal(augment.warp_matrix(size, size), np.float32([1, 0, 0, 0, 1, 0]))
    assert np.array_equal(augment.warp_matrix(size, size, 180.0), np.float32([-1, 0, size - 1, 0, -1, size - 1]))
    assert np.array_equal(augment.warp_matrix(size, size, 450.0), augment.warp_matrix(size, size, 90.0))


@pytest.mark.parametrize("size", [17, 64])
def test_d4_and_flip_views_are_pure_permutations(size):
    """Through the fp32 restatement the views are bitwise np.rot90 / [:, ::-1] of the plain conversion."""
    from jr import augment
    rng = np.random.default_rng(size)
    u8 = rng.integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    plain = u8.astype(np.float32) * np.float32(1 / 255)
    views = augment.d4_views(size, size)
    assert [f for f, _ in views] == [0, 0, 0, 0, 1, 1, 1, 1]
    for k, view in enumerate(views):
        tab, warp = augment.view_tables(view, 2)
        got = warp_ref.warp_batch(u8, tab, warp, np.float32)
        want = np.rot90(plain, k % 4, axes=(1, 2))
        if k >= 4:
            want = want[:, :, ::-1]
        assert got.dtype == np.float32 and np.array_equal(got, want), k
    assert [f for f, _ in augment.flip_views()] == [0, 1, 2, 3]
    for flags, view in enumerate(augment.flip_views()):
        tab, warp = augment.view_tables(view, 2)
        want = plain[:, :, ::-1] if flags & 1 else plain
        want = want[:, ::-1] if flags & 2 else want
        assert np.array_equal(warp_ref.warp_batch(u8, tab, warp, np.float32), want), flags
    # the flip matrices are the flag flips
    for flags, m in ((1, [-1, 0, size - 1, 0, 1, 0]), (2, [1, 0, 0, 0, -1, size - 1])):
        tab, warp = augment.view_tables((0, np.float32(m)), 2)
        ftab, fwarp = augment.view_tables((flags, np.float32(augment.IDENTITY_MATRIX)), 2)
        assert np.array_equal(warp_ref.warp_batch(u8, tab, warp, np.float32),
                              warp_ref.warp_batch(u8, ftab, fwarp, np.float32))
    with pytest.raises(ValueError):
        augment.d4_views(13, 21)


def test_ref_identity_composes_with_the_colour_stages():
    """At the identity matrix the restatement is tests/augment_ref.py's, bit for bit, in both dtypes."""
    import augment_ref
    from jr import augment
    rng = np.random.default_rng(2)
    u8 = rng.integers(0, 256, (4, 17, 13, 3), dtype=np.uint8)
    tab = augment.draw(augment.AugmentSpec(), np.random.Generator(np.random.PCG64([1, 0])), 4)
    for dt in (np.float32, np.float64):
        assert np.array_equal(warp_ref.warp_batch(u8, tab, augment.warp_identity(4), dt),
                              augment_ref.augment_batch(u8, tab, dt))


def _decompose(t, h, w):
    """(degrees, zoom, dx, dy) of the matrices of a warp table (the inverse of jr.augment.warp_matrix)."""
    m = t["m"].astype(np.float64)
    deg = np.degrees(np.arctan2(m[:, 3], m[:, 0]))
    zoom = 1.0 / np.hypot(m[:, 0], m[:, 3])
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    out = []
    for i in range(len(m)):
        A = np.array([[m[i, 0], m[i, 1]], [m[i, 3], m[i, 4]]])
        out.append(np.linalg.solve(A, np.array([cx - m[i, 2], cy - m[i, 5]])) - (cx, cy))
    d = np.array(out)
    return deg, zoom, d[:, 0], d[:, 1]


def test_draw_warp_is_deterministic_ranked_and_in_range():
    from jr import augment
    spec, h, w = augment.WarpSpec(), 75, 91
    gen = lambda rank: np.random.Generator(np.random.PCG64([7, rank, 1]))  # noqa: E731
    a, b, c = (augment.draw_warp(spec, gen(r), 512, h, w) for r in (0, 0, 1))
    assert a.dtype == augment.WARP_DTYPE and a.shape == (512,)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != c.tobytes()
    eps = 1e-4          # the float32 rounding of the matrix entries, seen through the decomposition
    for t in (a, c):
        assert np.all(t["reserved"] == 0) and np.all(np.isfinite(t["m"]))
        deg, zoom, dx, dy = _decompose(t, h, w)
        assert np.all(np.abs(deg) <= 180 + eps)
        assert np.all((zoom >= 0.9 - eps) & (zoom <= 1.1 + eps))
        assert np.all(np.abs(dx) <= 0.05 * w + eps) and np.all(np.abs(dy) <= 0.05 * h + eps)
    # the ranges are used, not just respected
    deg, zoom, dx, dy = _decompose(a, h, w)
    assert deg.min() < -170 and deg.max() > 170
    assert zoom.min() < 0.91 and zoom.max() > 1.09
    assert dx.min() < -0.045 * w and dx.max() > 0.045 * w and dy.min() < -0.045 * h and dy.max() > 0.045 * h
    # every spec consumes the same draws; the identity spec draws the identity
    narrow = augment.WarpSpec(rotate=0.0, zoom=(1.0, 1.0), shift=0.0)
    g1, g2 = gen(0), gen(0)
    assert augment.draw_warp(narrow, g1, 16, h, w).tobytes() == augment.warp_identity(16).tobytes()
    augment.draw_warp(spec, g2, 16, h, w)
    assert g1.bit_generator.state == g2.bit_generator.state
    # matches warp_matrix on the recovered parameters
    m0 = augment.warp_matrix(h, w, deg[0], zoom[0], dx[0], dy[0])
    assert np.allclose(m0, a["m"][0], atol=1e-3)


def test_draw_warp_leaves_the_colour_stream_alone():
    """train.py draws the geometry from PCG64([seed, rank, 1]): the colour
    table of PCG64([seed, rank]) is byte-identical with and without it."""
    from jr import augment
    spec = augment.AugmentSpec()
    alone = np.random.Generator(np.random.PCG64([3, 0]))
    beside, geo = np.random.Generator(np.random.PCG64([3, 0])), np.random.Generator(np.random.PCG64([3, 0, 1]))
    for _ in range(3):
        want = augment.draw(spec, alone, 64)
        augment.draw_warp(augment.WarpSpec(), geo, 64, 107, 107)
        assert augment.draw(spec, beside, 64).tobytes() == want.tobytes()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_ref_degenerate_matrices_stay_in_range(dt):
    from jr import augment
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (4, 13, 21, 3), dtype=np.uint8)
    tab = augment.identity(4)
    tab["contrast_factor"], tab["brightness_delta"] = 1.3, 0.05
    warp = augment.warp_identity(4)
    warp["m"][0] = 0.0
    warp["m"][1] = np.nan
    warp["m"][2] = [np.inf, 0, -np.inf, 1, np.inf, 0]
    warp["m"][3] = 1e30
    got = warp_ref.warp_batch(u8, tab, warp, dt)
    assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0
    # all-zero matrix: every destination pixel is source pixel (0, 0); NaN / inf / 1e30: all fill
    pure = warp_ref.warp_batch(u8, augment.identity(4), warp, dt)
    assert np.all(pure[0] == (u8[0, 0, 0].astype(np.float32) * np.float32(1 / 255)).astype(dt))
    assert np.all(pure[1:] == 0)


def test_ref_fp32_tracks_fp64():
    """The fp32 restatement against the fp64 one on a generic warp (the figure
    the GPU tests scale their bar with).  Bound: u and v are four roundings
    each of values below 128 (half an ulp of 2^-17 apiece: 2^-16 per
    coordinate), the bilinear surface moves by at most 1 per pixel along each
    axis (2^-15 in all), and the lerps add a few roundings of values <= 1."""
    from jr import augment
    rng = np.random.default_rng(4)
    u8 = rng.integers(0, 256, (2, 75, 91, 3), dtype=np.uint8)
    warp = augment.warp_identity(2)
    warp["m"][0] = augment.warp_matrix(75, 91, 30.0)
    warp["m"][1] = augment.warp_matrix(75, 91, -17.5, 1.1, 2.5, -1.25)
    tab = augment.identity(2)
    e = np.max(np.abs(warp_ref.warp_batch(u8, tab, warp, np.float32).astype(np.float64)
                      - warp_ref.warp_batch(u8, tab, warp, np.float64)))
    print(f"fp32 warp restatement vs fp64: {e:.2e}")
    assert 0 < e < 2.0 ** -15 + 8 * 2.0 ** -24
    assert np.all(warp_ref.inside_fraction(u8, tab, warp) >= 0.5)


def test_train_parser_geometry_flags():
    import train
    from jr import augment
    p = train.build_parser()
    args = p.parse_args([])
    assert args.augment_rotate is None and args.augment_zoom is None and args.augment_shift is None
    assert train.warp_spec(args) is None
    assert train.warp_spec(p.parse_args(["--augment"])) is None        # colour only: no warp table
    for flags in (["--augment_rotate", "30"], ["--augment_zoom", "0.9,1.1"], ["--augment_shift", "0.05"]):
        with pytest.raises(SystemExit):
            p.parse_args(flags)
    args = p.parse_args(["--augment", "--augment_seed", "3", "--augment_rotate", "30", "--augment_zoom", "0.9,1.1"])
    spec = train.warp_spec(args)
    assert spec == augment.WarpSpec(rotate=30.0, zoom=(0.9, 1.1), shift=0.0)
    assert train.augment_spec(args) == augment.AugmentSpec()           # the colour spec does not move
    assert spec.to_meta() == {"rotate": 30.0, "zoom": [0.9, 1.1], "shift": 0.0}
    only_shift = train.warp_spec(p.parse_args(["--augment", "--augment_shift", "0.1"]))
    assert only_shift == augment.WarpSpec(rotate=0.0, zoom=(1.0, 1.0), shift=0.1)


def test_evaluate_parser_tta():
    import evaluate
    p = evaluate.build_parser()
    assert p.parse_args(["-e"]).tta == "none"
    assert p.parse_args(["-e", "--tta", "d4"]).tta == "d4"
    with pytest.raises(SystemExit):
        p.parse_args(["-e", "--tta", "rot45"])
    assert len(evaluate.tta_views("flips", 107, 107)) == 4 and len(evaluate.tta_views("d4", 107, 107)) == 8
