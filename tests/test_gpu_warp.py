"""jr_image_u8_warp_augment_nhwc on the GPU, through the C ABI: bitwise
against jr_image_u8_augment_nhwc / the plain conversion wherever the matrix
maps the pixel lattice onto itself, and against the numpy restatement
tests/warp_ref.py (fp64 = the reference; the same code in fp32 sets the error
bar) on generic rotations, zooms and shifts.  The helpers, images, shapes and
colour tables are those of tests/test_gpu_augment.py.
"""
import functools

import numpy as np
import pytest

import test_gpu_augment as A
import warp_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, BF16, DS = A.F32, A.BF16, A.DS
SHAPES, IDS = A.SHAPES, A.IDS
SQUARE = (3, 17, 17)                 # the quarter turns need h == w
DTYPES = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])


def warps(n, matrix=None):
    """[n] warp table, every image with `matrix` (a float32[6], or an [n, 6] array; None: the identity)."""
    from jr import augment
    t = augment.warp_identity(n)
    if matrix is not None:
        t["m"] = matrix
    return t


def run_warp(u8, tab, wtab, dt, slots=None):
    """The warp entry point on a sentinel-filled destination of `slots` images."""
    ffi = A._ffi()
    L = ffi.load()
    n, h, w, _ = u8.shape
    slots = slots or n
    src = torch.as_tensor(np.array(u8)).cuda()
    par = torch.as_tensor(np.ascontiguousarray(tab).view(np.uint8)).cuda()
    wrp = torch.as_tensor(np.ascontiguousarray(wtab).view(np.uint8)).cuda()
    dst = torch.full((slots, h, w, DS), 7.0, device="cuda", dtype=torch.bfloat16 if dt == BF16 else torch.float32)
    nbytes = L.jr_augment_workspace_size(n, h, w)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    ffi.check("warp", L.jr_image_u8_warp_augment_nhwc(src.data_ptr(), dst.data_ptr(), dt, n, h, w, 3, DS,
                                                      par.data_ptr(), wrp.data_ptr(), ws.data_ptr(), nbytes, None))
    out = A.bits(dst)
    del src, par, wrp, ws
    return out


@DTYPES
@pytest.mark.parametrize("shape", SHAPES + [SQUARE], ids=IDS + ["17x17"])
def test_identity_warp_is_the_augment_entry_point(shape, dt):
    n = shape[0]
    u8 = A.images(*shape)
    sentinel = A.bits(torch.full((1,), 7.0, device="cuda", dtype=torch.bfloat16 if dt == BF16 else torch.float32))[0]
    for case, kw in A.ACCURACY_CASES.items():
        tab = A.table(n, **kw)
        out = run_warp(u8, tab, warps(n), dt, slots=n + 1)
        assert np.array_equal(out[:n], A.run_aug(u8, tab, dt)), case
        assert np.all(out[:n, ..., 3] == 0), case
        assert np.all(out[n] == sentinel), case


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_flip_matrices_are_the_flag_flips(shape, dt):
    n, h, w = shape
    u8, base = A.images(*shape), A.plain(shape, dt)
    lr, ud = np.float32([-1, 0, w - 1, 0, 1, 0]), np.float32([1, 0, 0, 0, -1, h - 1])
    both = np.float32([-1, 0, w - 1, 0, -1, h - 1])
    out = run_warp(u8, A.table(n), warps(n, np.stack([lr, ud, both])), dt)
    for i, flags in enumerate((1, 2, 3)):
        assert np.array_equal(out[i], A.flipped(base[i], flags)), flags
    # the flag flips with the identity matrix, and a flag flip undone by its matrix
    out = run_warp(u8, A.table(n, flags=[1, 2, 3]), warps(n), dt)
    for i, flags in enumerate((1, 2, 3)):
        assert np.array_equal(out[i], A.flipped(base[i], flags)), flags
    out = run_warp(u8, A.table(n, flags=[1, 2, 3]), warps(n, np.stack([lr, ud, both])), dt)
    assert np.array_equal(out, base)


@DTYPES
def test_d4_and_flip_views_are_the_permuted_plain_conversion(dt):
    from jr import augment
    n, h, w = SQUARE
    u8, base = A.images(*SQUARE), A.plain(SQUARE, dt)
    for k, view in enumerate(augment.d4_views(h, w)):
        want = np.rot90(base, k % 4, axes=(1, 2))
        if k >= 4:
            want = want[:, :, ::-1]
        assert np.array_equal(run_warp(u8, *augment.view_tables(view, n), dt), want), k
    for flags, view in enumerate(augment.flip_views()):
        want = np.stack([A.flipped(base[i], flags) for i in range(n)])
        assert np.array_equal(run_warp(u8, *augment.view_tables(view, n), dt), want), flags


# (degrees, zoom, dx, dy)
WARP_CASES = [(30, 1, 0, 0), (-17.5, 1.1, 2.5, -1.25), (137, 0.9, -3, 4), (45, 2, 0, 0), (0, 1, 0.5, 0.5)]
WARP_IDS = ["rot30", "rot-17.5_zoom_shift", "rot137_zoomout_shift", "rot45_zoom2", "half_pixel"]
COLOURS = {"pure": {}, "all": A.ACCURACY_CASES["all"]}


def case_tables(shape, case, colour):
    from jr import augment
    n, h, w = shape
    return A.table(n, **COLOURS[colour]), warps(n, augment.warp_matrix(h, w, *case))


@functools.lru_cache(maxsize=None)
def reference(shape, case, colour):
    """(fp64 result, max abs error of the fp32 restatement against it, the
    per-image share of destination pixels sampled inside the source)."""
    tab, wtab = case_tables(shape, case, colour)
    r64 = warp_ref.warp_batch(A.images(*shape), tab, wtab, np.float64)
    r32 = warp_ref.warp_batch(A.images(*shape), tab, wtab, np.float32)
    r64.setflags(write=False)
    return r64, float(np.max(np.abs(r32.astype(np.float64) - r64))), warp_ref.inside_fraction(A.images(*shape), tab, wtab)


@DTYPES
@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("case", WARP_CASES, ids=WARP_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_accuracy_against_fp64(shape, case, colour, dt):
    """GPU max abs error against fp64 <= 4 x that of the fp32 restatement on
    the same inputs; bf16: against the bf16-rounded fp64 result, plus one bf16
    ulp of the reference value (the bars of tests/test_gpu_augment.py).  Every
    case samples at least half of its destination pixels inside the source."""
    r64, e32, inside = reference(shape, case, colour)
    assert np.all(inside >= 0.5), inside
    tab, wtab = case_tables(shape, case, colour)
    got = A.as_f64(run_warp(A.images(*shape), tab, wtab, dt), dt)
    assert np.all(got[..., 3] == 0)
    if dt == F32:
        err = float(np.max(np.abs(got[..., :3] - r64)))
        print(f"warp {case} {colour} {shape} f32: gpu-vs-fp64 {err:.3e}  fp32-restatement-vs-fp64 {e32:.3e}  "
              f"inside {inside.min():.2f}")
        assert err <= 4 * e32
    else:
        rb = A.f64_to_bf16_bits(r64)
        ref = A.bf16_to_f64(rb)
        ulp = A.bf16_to_f64((rb + 1).astype(np.uint16)) - ref
        d = np.abs(got[..., :3] - ref)
        print(f"warp {case} {colour} {shape} bf16: gpu-vs-bf16(fp64) {float(d.max()):.3e} "
              f"({int((d > 0).sum())} of {d.size} differ)  fp32-restatement-vs-fp64 {e32:.3e}")
        assert np.all(d <= 4 * e32 + ulp)


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_outside_pixels_of_a_pure_warp_are_zero(shape, dt):
    """137 degrees, zoomed out: the corners of the destination see nothing.
    Wherever the outside test fails in the fp32 restatement (the kernel's own
    arithmetic) the output is exactly 0; some inside pixel is not."""
    n = shape[0]
    u8 = A.images(*shape)
    tab, wtab = case_tables(shape, WARP_CASES[2], "pure")
    out = run_warp(u8, tab, wtab, dt)
    for i in range(n):
        inside = warp_ref.warp_stage(u8[i], 0, wtab[i]["m"], np.float32)[1]
        assert 0.05 < 1 - inside.mean() < 0.5
        assert np.all(out[i][~inside] == 0)
        assert np.any(out[i][inside] != 0)


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_degenerate_matrices_give_finite_output(shape, dt):
    ffi = A._ffi()
    n = shape[0]
    inf = np.inf
    for mats, kw in (([[np.nan] * 6, [inf, 0, -inf, 1, inf, 0], [1e30] * 6], {}),
                     ([[0.0] * 6, [1, 0, np.nan, 0, 1, 0], [-1e30, 1e30, 0, 1e30, -1e30, 5]], A.ACCURACY_CASES["all"]),
                     ([[1, 0, 2.0 ** 31, 0, 1, 0], [1, 0, 0, 0, 1, -2.0 ** 31], [3e9, 0, -1.5, 0, 3e9, -1.5]],
                      dict(con=[1.5, 0.5, 2.0]))):
        got = A.as_f64(run_warp(A.images(*shape), A.table(n, **kw), warps(n, np.float32(mats)), dt), dt)
        assert np.all(np.isfinite(got))
        assert got.min() >= 0.0 and got.max() <= 1.0
        assert np.all(got[..., 3] == 0)
    torch.cuda.synchronize()
    assert ffi.load().jr_device_check() == 0


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_determinism_and_slot_independence(shape, dt):
    from jr import augment
    n, h, w = shape
    u8 = A.images(*shape)
    tab = A.table(n, **A.ACCURACY_CASES["all"])
    wtab = warps(n, np.stack([augment.warp_matrix(h, w, *c) for c in WARP_CASES[:3]]))
    a, b = run_warp(u8, tab, wtab, dt), run_warp(u8, tab, wtab, dt)
    assert np.array_equal(a, b)
    # image 2 with its parameters alone in slot 0 of a batch of one
    one = run_warp(u8[2:3], tab[2:3], wtab[2:3], dt)
    assert np.array_equal(one[0], a[2])
    # contrast on one image only: the others are the pure warp
    pure = run_warp(u8, A.table(n), wtab, dt)
    only = run_warp(u8, A.table(n, con=[1.0, 1.6, 1.0]), wtab, dt)
    assert np.array_equal(only[0], pure[0]) and np.array_equal(only[2], pure[2])
    assert not np.array_equal(only[1], pure[1])


def test_engines_set_batch_warp():
    """Engine.set_batch and EnsembleEngine.set_batch (augment=, warp=) at
    107^2, B = 2: the input buffer (every member's) is the direct C-ABI call's
    output, from a host array and from a device tensor; warp alone uses the
    identity colour table; augment alone is the existing entry point's buffer;
    float batches are refused; an x6h training step on a warped batch is finite."""
    from jr import augment, synth
    from jr.engine import Engine
    from jr.ensemble import EnsembleEngine
    from jr.init import init_params
    ffi = A._ffi()
    L = ffi.load()
    B, res = 2, 107
    eng = Engine(B, res, res, seed=5, conv_math="x6h")
    ens = EnsembleEngine([init_params(eng.g, 40 + m) for m in range(2)], B, res, res)
    u8 = synth.fundus_batch(0, B, res)
    y = np.array([[1.0], [0.0]], np.float32)
    tab = augment.draw(augment.AugmentSpec(), np.random.Generator(np.random.PCG64([3, 0])), B)
    tab["contrast_factor"][0] = 1.25     # the contrast pass runs whatever the draw
    wtab = augment.draw_warp(augment.WarpSpec(), np.random.Generator(np.random.PCG64([3, 0, 1])), B, res, res)
    ds, count = eng.in_stride, B * res * res * eng.in_stride
    assert ens.in_stride == ds
    src = torch.as_tensor(u8).cuda()
    nbytes = L.jr_augment_workspace_size(B, res, res)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)

    def direct(t, wt):
        want = torch.full((count,), 7.0, device="cuda")
        par = torch.as_tensor(t.view(np.uint8)).cuda()
        if wt is None:
            ffi.check("augment", L.jr_image_u8_augment_nhwc(src.data_ptr(), want.data_ptr(), F32, B, res, res, 3, ds,
                                                            par.data_ptr(), ws.data_ptr(), nbytes, None))
        else:
            wrp = torch.as_tensor(wt.view(np.uint8)).cuda()
            ffi.check("warp", L.jr_image_u8_warp_augment_nhwc(src.data_ptr(), want.data_ptr(), F32, B, res, res, 3, ds,
                                                              par.data_ptr(), wrp.data_ptr(), ws.data_ptr(), nbytes,
                                                              None))
        return A.bits(want)

    def buffers(e):
        e.synchronize()
        full = A.bits(e.acts[e.g.input_buf])
        stride = e.act_ms[e.g.input_buf]
        return [full[m * stride:m * stride + count] for m in range(e.members)]

    both, warp_only, colour_only = direct(tab, wtab), direct(augment.identity(B), wtab), direct(tab, None)
    assert not np.array_equal(both, warp_only) and not np.array_equal(both, colour_only)
    for e in (eng, ens):
        for batch in (u8, src):                            # a host array, a device uint8 tensor
            e.set_batch(batch, y, augment=tab, warp=wtab)
            assert all(np.array_equal(b, both) for b in buffers(e))
        e.set_batch(u8, y, augment=tab.view(np.uint32).reshape(B, 8), warp=wtab.view(np.uint32).reshape(B, 8))
        assert all(np.array_equal(b, both) for b in buffers(e))
        e.set_batch(u8, y, warp=wtab)                      # the identity colour table
        assert all(np.array_equal(b, warp_only) for b in buffers(e))
        e.set_batch(u8, y, augment=tab)                    # warp=None: the existing entry point
        assert all(np.array_equal(b, colour_only) for b in buffers(e))
        for kw in (dict(warp=wtab), dict(augment=tab), dict(augment=tab, warp=wtab)):
            with pytest.raises(ValueError):
                e.set_batch(u8.astype(np.float32) / 255, y, **kw)
        with pytest.raises(ValueError):
            e.set_batch(u8, y, warp=wtab[:1])
    assert both.min() >= 0.0 and both.max() <= 1.0         # the x6h stem's input bound

    eng.set_batch(u8, y, augment=tab, warp=wtab)
    eng.train_step()
    loss = eng.loss_value()
    assert np.isfinite(loss) and loss > 0
    assert L.jr_device_check() == 0
    ens.set_batch(src, y, warp=wtab)
    ens.forward(B)
    assert np.all(np.isfinite(ens.predictions(B)))
