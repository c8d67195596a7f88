"""On-device training augmentation, the parts that need no GPU: argument
validation of the C ABI, the workspace query, the parameter draws of
jr.augment, train.py's flags and the numpy restatement at identity."""
import ctypes

import numpy as np

import augment_ref


def _call(L, src=16, dst=16, dtype=0, n=2, h=13, w=21, c=3, ds=4, params=16, ws=16, ws_bytes=1 << 20):
    return L.jr_image_u8_augment_nhwc(src, dst, dtype, n, h, w, c, ds, params, ws, ws_bytes, None)


def test_abi_validation_without_gpu():
    from jr import _ffi
    L = _ffi.load()
    for kw, text in (({"src": None}, "null"), ({"dst": None}, "null"), ({"params": None}, "null"),
                     ({"ws": None}, "null"), ({"c": 4}, "c must be 3"), ({"c": 1}, "c must be 3"),
                     ({"ds": 2}, "dst_stride"), ({"dtype": 2}, "dtype"), ({"dtype": 4}, "dtype"),
                     ({"dtype": -1}, "dtype"), ({"ws_bytes": 0}, "workspace")):
        assert _call(L, **kw) == -1, kw
        assert text in _ffi.last_error(), (kw, _ffi.last_error())
    need = L.jr_augment_workspace_size(2, 13, 21)
    assert _call(L, ws_bytes=need - 1) == -1 and "workspace" in _ffi.last_error()


def test_workspace_size_positive_and_monotone():
    from jr import _ffi
    L = _ffi.load()
    for h, w in ((13, 21), (75, 91), (299, 299)):
        sizes = [L.jr_augment_workspace_size(n, h, w) for n in range(1, 66)]
        assert sizes[0] > 0
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    # the partial count of an image depends on (h, w) alone
    assert L.jr_augment_workspace_size(64, 299, 299) == 64 * L.jr_augment_workspace_size(1, 299, 299)


def test_param_layout_matches_the_header():
    from jr import _ffi, augment
    assert augment.PARAM_DTYPE.itemsize == 32 == ctypes.sizeof(_ffi.AugmentParam)
    for name, _ in _ffi.AugmentParam._fields_:
        assert augment.PARAM_DTYPE.fields[name][1] == getattr(_ffi.AugmentParam, name).offset


def test_draw_is_deterministic_ranked_and_in_range():
    from jr import augment
    spec = augment.AugmentSpec()
    gen = lambda rank: np.random.Generator(np.random.PCG64([7, rank]))  # noqa: E731
    a, b, c = augment.draw(spec, gen(0), 512), augment.draw(spec, gen(0), 512), augment.draw(spec, gen(1), 512)
    assert a.dtype.itemsize == 32 and a.shape == (512,)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != c.tobytes()
    assert a.view(np.uint32).reshape(512, 8).shape == (512, 8)
    for t in (a, c):
        assert np.all(t["reserved"] == 0)
        assert np.all(np.abs(t["hue_delta"].astype(np.float64)) <= 0.2)
        assert np.all((t["sat_factor"].astype(np.float64) >= 0.5) & (t["sat_factor"].astype(np.float64) <= 1.5))
        assert np.all((t["contrast_factor"].astype(np.float64) >= 0.5) & (t["contrast_factor"].astype(np.float64) <= 1.5))
        assert np.all(np.abs(t["brightness_delta"].astype(np.float64)) <= 0.125)
        assert set(np.unique(t["flags"])) == {0, 1, 2, 3}
    # the ranges are used, not just respected
    assert a["hue_delta"].min() < -0.15 and a["hue_delta"].max() > 0.15
    assert a["sat_factor"].min() < 0.6 and a["contrast_factor"].max() > 1.4
    narrow = augment.AugmentSpec(flip=False, hue=0.0, saturation=(1.0, 1.0), contrast=(1.0, 1.0), brightness=0.0)
    assert augment.draw(narrow, gen(0), 16).tobytes() == augment.identity(16).tobytes()


def test_identity_table_and_as_table():
    import pytest
    from jr import augment
    t = augment.identity(3)
    assert t.dtype.itemsize == 32 and np.all(t["reserved"] == 0) and np.all(t["flags"] == 0)
    assert np.all(t["hue_delta"] == 0) and np.all(t["sat_factor"] == 1)
    assert np.all(t["contrast_factor"] == 1) and np.all(t["brightness_delta"] == 0)
    assert augment.as_table(t.view(np.uint32).reshape(3, 8), 3).tobytes() == t.tobytes()
    with pytest.raises(ValueError):
        augment.as_table(t, 2)
    bad = t.copy()
    bad["reserved"][1, 0] = 1
    with pytest.raises(ValueError):
        augment.as_table(bad, 3)
    with pytest.raises(ValueError):
        augment.AugmentSpec(saturation=(1.5, 0.5))


def test_train_parser_defaults_augment_off():
    import train
    p = train.build_parser()
    args = p.parse_args([])
    assert args.augment is False and args.augment_seed == 0
    assert train.augment_spec(args) is None
    args = p.parse_args(["--augment", "--augment_seed", "3", "--augment_hue", "0.1", "--augment_saturation", "0.8,1.2",
                         "--augment_contrast", "0.9,1.1", "--augment_brightness", "0.05", "--no_augment_flip"])
    spec = train.augment_spec(args)
    assert (spec.flip, spec.hue, spec.saturation, spec.contrast, spec.brightness) == \
        (False, 0.1, (0.8, 1.2), (0.9, 1.1), 0.05)
    from jr import augment
    assert train.augment_spec(p.parse_args(["--augment"])) == augment.AugmentSpec()
    assert augment.AugmentSpec().to_meta() == {"flip": True, "hue": 0.2, "saturation": [0.5, 1.5],
                                               "contrast": [0.5, 1.5], "brightness": 0.125}


def test_ref_identity_is_the_plain_conversion():
    from jr import augment
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (2, 17, 13, 3), dtype=np.uint8)
    u8[0, 0] = 0
    u8[0, 1] = 255
    want = u8.astype(np.float32) * np.float32(1 / 255)
    for dt in (np.float32, np.float64):
        got = augment_ref.augment_batch(u8, augment.identity(2), dt)
        assert got.dtype == dt
        assert np.array_equal(got, want.astype(dt))
    assert want.max() == 1.0   # 255 * f32(1/255) rounds to exactly 1: the clamp leaves it


def test_ref_fp32_tracks_fp64():
    """The fp32 restatement stays within a few fp32 roundings of the fp64 one
    (the figure the GPU tests scale their bar with)."""
    from jr import augment
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, (4, 17, 13, 3), dtype=np.uint8)
    t = augment.draw(augment.AugmentSpec(), np.random.Generator(np.random.PCG64([1, 0])), 4)
    e = np.max(np.abs(augment_ref.augment_batch(u8, t, np.float32).astype(np.float64)
                      - augment_ref.augment_batch(u8, t, np.float64)))
    print(f"fp32 restatement vs fp64: {e:.2e}")
    assert 0 < e < 64 * 2.0 ** -24   # a dozen roundings, the hue in [0, 6) at ulp 2^-22
