"""jr_image_u8_augment_nhwc on the GPU, through the C ABI, against the numpy
restatement tests/augment_ref.py (fp64 = the reference; the same code in fp32
sets the error bar) and against jr_image_u8_to_nhwc, the unaugmented input
conversion whose output the identity table must reproduce bit for bit.

Measured on an MI355X: fp32 worst case 8.7e-7 against
fp64 where the fp32 restatement has 9.9e-7; bf16 within one bf16 ulp of the
bf16-rounded fp64 result.
"""
import functools

import numpy as np
import pytest

import augment_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, BF16 = 0, 1
DS = 4
SHAPES = [(3, 13, 21), (3, 75, 91)]
IDS = ["13x21", "75x91"]


def _ffi():
    from jr import _ffi
    _ffi.init(0)
    return _ffi


@functools.lru_cache(maxsize=None)
def images(n, h, w):
    """Random uint8 pixels plus the HSV corner cases: black rows (v = 0), white
    rows, gray pixels (c = 0) and every two-channel tie."""
    rng = np.random.default_rng(1000 * h + w)
    u8 = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    u8[:, 0] = 0
    u8[:, 1] = 255
    u8[:, 2] = u8[:, 2, :, :1]                       # gray
    hi = rng.integers(1, 256, (n, w), dtype=np.uint8)
    lo = (hi * rng.random((n, w))).astype(np.uint8)  # lo < hi
    for row, (a, b, c) in enumerate([(hi, hi, lo), (lo, hi, hi), (hi, lo, hi), (lo, lo, hi), (hi, lo, lo),
                                     (lo, hi, lo)], start=3):
        u8[:, row] = np.stack([a, b, c], axis=-1)
    u8.setflags(write=False)
    return u8


def table(n, hue=0.0, sat=1.0, con=1.0, bri=0.0, flags=0):
    from jr import augment
    t = augment.identity(n)
    for name, v in (("hue_delta", hue), ("sat_factor", sat), ("contrast_factor", con), ("brightness_delta", bri),
                    ("flags", flags)):
        t[name] = v
    return t


def bits(t):
    """Device tensor -> numpy of its raw bits (float32 as is, bf16 as uint16)."""
    torch.cuda.synchronize()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def bf16_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f64_to_bf16_bits(x):
    """Round-to-nearest-even bf16 of fp64 values in [0, 1] (via fp32, exact
    there for these tests' purposes: a double rounding moves at most the tie)."""
    b = x.astype(np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def run_plain(u8, dt):
    ffi = _ffi()
    n, h, w, _ = u8.shape
    src = torch.as_tensor(np.array(u8)).cuda()
    dst = torch.full((n, h, w, DS), 7.0, device="cuda", dtype=torch.bfloat16 if dt == BF16 else torch.float32)
    ffi.check("plain", ffi.load().jr_image_u8_to_nhwc(src.data_ptr(), dst.data_ptr(), dt, n * h * w, 3, DS, None))
    return bits(dst)


def run_aug(u8, tab, dt, slots=None):
    """The new entry point on a sentinel-filled destination of `slots` images."""
    ffi = _ffi()
    L = ffi.load()
    n, h, w, _ = u8.shape
    slots = slots or n
    src = torch.as_tensor(np.array(u8)).cuda()
    par = torch.as_tensor(np.ascontiguousarray(tab).view(np.uint8)).cuda()
    dst = torch.full((slots, h, w, DS), 7.0, device="cuda", dtype=torch.bfloat16 if dt == BF16 else torch.float32)
    nbytes = L.jr_augment_workspace_size(n, h, w)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    ffi.check("augment", L.jr_image_u8_augment_nhwc(src.data_ptr(), dst.data_ptr(), dt, n, h, w, 3, DS,
                                                    par.data_ptr(), ws.data_ptr(), nbytes, None))
    out = bits(dst)
    del src, par, ws
    return out


def as_f64(out, dt):
    return bf16_to_f64(out) if dt == BF16 else out.astype(np.float64)


@functools.lru_cache(maxsize=None)
def plain(shape, dt):
    out = run_plain(images(*shape), dt)
    out.setflags(write=False)
    return out


def flipped(a, flags):
    """[h, w, ds] flipped as the flag bits say."""
    if flags & 1:
        a = a[:, ::-1]
    if flags & 2:
        a = a[::-1]
    return a


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_identity_is_the_plain_conversion(shape, dt):
    n = shape[0]
    out = run_aug(images(*shape), table(n), dt, slots=n + 1)
    assert np.array_equal(out[:n], plain(shape, dt))
    assert np.all(out[:n, ..., 3] == 0)
    sentinel = bits(torch.full((1,), 7.0, device="cuda", dtype=torch.bfloat16 if dt == BF16 else torch.float32))[0]
    assert np.all(out[n] == sentinel)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_flips_are_pure_indexing(shape, dt):
    n = shape[0]
    base = plain(shape, dt)
    for flags in ([0, 1, 2], [3, 2, 1]):
        out = run_aug(images(*shape), table(n, flags=flags), dt)
        for i, f in enumerate(flags):
            assert np.array_equal(out[i], flipped(base[i], f)), (flags, i)


# name -> per-image parameters (n = 3)
ACCURACY_CASES = {
    "hue_half": dict(hue=[0.5, -0.5, 0.07]),
    "hue_wrap": dict(hue=[0.9, -0.3, 1.75]),                    # wraps past 0 in both directions
    "sat_only": dict(sat=[0.3, 1.7, 4.0]),                      # hue_delta == 0; 1.7 and 4.0 hit the clamp
    "sat_zero": dict(sat=[0.0, 1.0000001, 250.0]),
    "contrast": dict(con=[0.5, 1.5, 3.0]),                      # 3.0 hits both ends of the final clamp
    "contrast_neg": dict(con=[0.0, -1.0, 6.0]),
    "brightness": dict(bri=[0.125, -0.125, 0.9]),               # black pixels under a negative delta
    "brightness_neg": dict(bri=[-0.9, 1.0, -1e-3]),
    "contrast_brightness": dict(con=[8.0, 8.0, 0.25], bri=[0.5, -0.5, 0.3]),
    "all": dict(hue=[0.17, -0.2, 0.5], sat=[0.6, 1.45, 1.2], con=[1.4, 0.55, 1.1], bri=[-0.1, 0.12, 0.05],
                flags=[1, 2, 3]),
    "all_mixed_skips": dict(hue=[0.0, 0.31, 0.0], sat=[1.0, 1.0, 0.8], con=[1.0, 1.3, 0.7], bri=[0.1, 0.0, -0.06],
                            flags=[3, 0, 2]),
}


@functools.lru_cache(maxsize=None)
def reference(shape, case):
    """(fp64 result, max abs error of the fp32 restatement against it)."""
    tab = table(shape[0], **ACCURACY_CASES[case])
    r64 = augment_ref.augment_batch(images(*shape), tab, np.float64)
    r32 = augment_ref.augment_batch(images(*shape), tab, np.float32)
    r64.setflags(write=False)
    return r64, float(np.max(np.abs(r32.astype(np.float64) - r64)))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(ACCURACY_CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_accuracy_against_fp64(shape, case, dt):
    """GPU max abs error against fp64 <= 4 x that of the fp32 restatement on
    the same inputs (4: FMA contraction, another summation order of the
    mean); bf16: against the bf16-rounded fp64 result, plus one bf16 ulp of
    the reference value."""
    n = shape[0]
    r64, e32 = reference(shape, case)
    out = run_aug(images(*shape), table(n, **ACCURACY_CASES[case]), dt)
    got = as_f64(out, dt)
    assert np.all(got[..., 3] == 0)
    if dt == F32:
        err = float(np.max(np.abs(got[..., :3] - r64)))
        print(f"augment {case} {shape} f32: gpu-vs-fp64 {err:.3e}  fp32-restatement-vs-fp64 {e32:.3e}")
        assert err <= 4 * e32
    else:
        rb = f64_to_bf16_bits(r64)
        ref = bf16_to_f64(rb)
        ulp = bf16_to_f64((rb + 1).astype(np.uint16)) - ref
        d = np.abs(got[..., :3] - ref)
        print(f"augment {case} {shape} bf16: gpu-vs-bf16(fp64) {float(d.max()):.3e} "
              f"({int((d > 0).sum())} of {d.size} differ)  fp32-restatement-vs-fp64 {e32:.3e}")
        assert np.all(d <= 4 * e32 + ulp)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_determinism_and_slot_independence(shape, dt):
    n, h, w = shape
    u8 = images(*shape)
    tab = table(n, **ACCURACY_CASES["all"])
    a, b = run_aug(u8, tab, dt), run_aug(u8, tab, dt)
    assert np.array_equal(a, b)
    # image 2 with its parameters alone in slot 0 of a batch of one
    one = run_aug(u8[2:3], tab[2:3], dt)
    assert np.array_equal(one[0], a[2])
    # ... and moved to slot 0 of the same batch size
    swapped = run_aug(u8[::-1], tab[::-1], dt)
    assert np.array_equal(swapped[0], a[2]) and np.array_equal(swapped[2], a[0])
    # contrast on one image only: the others are the plain / flipped conversion
    only = run_aug(u8, table(n, con=[1.0, 1.6, 1.0], flags=[0, 1, 2]), dt)
    base = plain(shape, dt)
    assert np.array_equal(only[0], base[0])
    assert np.array_equal(only[2], flipped(base[2], 2))
    assert not np.array_equal(only[1], flipped(base[1], 1))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_output_range_with_extreme_parameters(shape, dt):
    n = shape[0]
    for kw in (dict(hue=[123.456, -77.7, 1e6], sat=[1e6, 0.0, -3.0], con=[1e4, -50.0, 1e-4], bri=[10.0, -10.0, 0.999]),
               dict(hue=[-1e6, 0.5, 0.0], sat=[1e30, 1e-30, 1.0], con=[-1e6, 1e30, 0.0], bri=[-1e30, 1e30, -1.0],
                    flags=[3, 1, 2])):
        got = as_f64(run_aug(images(*shape), table(n, **kw), dt), dt)
        assert np.all(np.isfinite(got))
        assert got.min() >= 0.0 and got.max() <= 1.0
        assert np.all(got[..., 3] == 0)


def test_engine_set_batch_augment():
    """Engine.set_batch(augment=...) at 107^2, B = 2: the input buffer is the
    direct C-ABI call's output; augment=None is the unaugmented path; a float
    batch is refused; an x6h training step on the augmented batch is finite."""
    from jr import augment, synth
    from jr.engine import Engine
    ffi = _ffi()
    L = ffi.load()
    B, res = 2, 107
    eng = Engine(B, res, res, seed=5, conv_math="x6h")
    u8 = synth.fundus_batch(0, B, res)
    y = np.array([[1.0], [0.0]], np.float32)
    tab = augment.draw(augment.AugmentSpec(), np.random.Generator(np.random.PCG64([3, 0])), B)
    tab["contrast_factor"][0] = 1.25     # the contrast pass runs whatever the draw
    ds, count = eng.in_stride, B * res * res * eng.in_stride
    src = torch.as_tensor(u8).cuda()

    eng.set_batch(u8, y, augment=tab)
    eng.synchronize()
    got = bits(eng.acts[eng.g.input_buf][:count])
    par = torch.as_tensor(tab.view(np.uint8)).cuda()
    nbytes = L.jr_augment_workspace_size(B, res, res)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    want = torch.full((count,), 7.0, device="cuda")
    ffi.check("augment", L.jr_image_u8_augment_nhwc(src.data_ptr(), want.data_ptr(), F32, B, res, res, 3, ds,
                                                    par.data_ptr(), ws.data_ptr(), nbytes, None))
    assert np.array_equal(got, bits(want))
    assert got.min() >= 0.0 and got.max() <= 1.0      # the x6h stem's input bound
    # the [n, 8] uint32 view is the same table
    eng.set_batch(u8, y, augment=tab.view(np.uint32).reshape(B, 8))
    eng.synchronize()
    assert np.array_equal(bits(eng.acts[eng.g.input_buf][:count]), got)

    with pytest.raises(ValueError):
        eng.set_batch(u8.astype(np.float32) / 255, y, augment=tab)
    with pytest.raises(ValueError):
        eng.set_batch(u8, y, augment=tab[:1])

    eng.set_batch(u8, y, augment=tab)
    eng.train_step()
    loss = eng.loss_value()
    assert np.isfinite(loss) and loss > 0
    assert L.jr_device_check() == 0

    eng.set_batch(u8, y)                               # augment=None: today's conversion
    eng.synchronize()
    ffi.check("plain", L.jr_image_u8_to_nhwc(src.data_ptr(), want.data_ptr(), F32, B * res * res, 3, ds, None))
    assert np.array_equal(bits(eng.acts[eng.g.input_buf][:count]), bits(want))
