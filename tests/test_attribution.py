"""The attribution surface without a GPU: the float32 restatements of
tests/attribution_ref.py against fp64 (the image gradient within the
sequential-sum bound gamma_(c_out + T) * sum |dy| |w|, every uncovered pixel
exactly 0), the validation errors of every new entry point before any HIP
call, and evaluate.py's flag refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import PKG

import attribution_ref as R

IMG_CASES = [  # (n, h, w, c_in, c_out, k, stride, pad)
    (2, 11, 9, 3, 32, 3, 2, 0), (1, 12, 10, 3, 32, 3, 2, 0), (1, 13, 10, 4, 16, 3, 1, 1), (2, 13, 10, 1, 48, 7, 2, 3)]


def _img_inputs(case, seed):
    n, h, w, cin, cout, k, s, pad = case
    rng = np.random.default_rng(seed)
    ho, wo = R.out_size(h, k, s, pad), R.out_size(w, k, s, pad)
    dy = rng.standard_normal((n, ho, wo, cout)).astype(np.float32)
    wt = (rng.standard_normal((k, k, cin, cout)) * 0.3).astype(np.float32)
    return dy, wt


@pytest.mark.parametrize("case", IMG_CASES)
def test_image_gradient_restatement_within_the_sequential_sum_bound(case):
    n, h, w, cin, cout, k, s, pad = case
    dy, wt = _img_inputs(case, sum(case))
    got = R.conv_bwd_image_ref(dy, wt, h, w, s, pad)
    ref, mag, taps = R.conv_bwd_image_fp64(dy, wt, h, w, s, pad)
    assert got.dtype == np.float32 and got.shape == (n, h, w, cin)
    bound = np.array([R.gamma(cout + t) for t in range(k * k + 1)])[taps][..., None] * mag
    assert np.all(np.abs(got.astype(np.float64) - ref) <= bound)
    assert np.any(got != 0)
    # a pixel no output covers is exactly 0 (the even sizes leave a last row and column)
    assert np.all(got[taps == 0] == 0)
    if s == 2 and pad == 0 and h % 2 == 0:
        assert np.all(taps[:, -1] == 0) and np.all(taps[:, :, -1] == 0) and np.all(got[:, -1] == 0)


def test_image_gradient_restatement_is_the_adjoint_of_the_forward():
    """<conv(x), dy> == <x, bwd_image(dy)> in fp64 arithmetic of the fp64 reference."""
    import torch
    import torch.nn.functional as F
    case = (2, 11, 9, 3, 32, 3, 2, 0)
    dy, wt = _img_inputs(case, 5)
    x = np.random.default_rng(6).standard_normal((2, 11, 9, 3))
    y = F.conv2d(torch.as_tensor(x).permute(0, 3, 1, 2), torch.as_tensor(wt.astype(np.float64)).permute(3, 2, 0, 1),
                 stride=2).permute(0, 2, 3, 1).numpy()
    ref, _, _ = R.conv_bwd_image_fp64(dy, wt, 11, 9, 2, 0)
    assert abs(np.sum(y * dy) - np.sum(x * ref)) <= 1e-9 * np.sum(np.abs(y * dy))


def test_frozen_bn_backward_restatement():
    rng = np.random.default_rng(3)
    m, c = 37, 16
    x = rng.standard_normal((m, c)).astype(np.float32)
    mean, beta = rng.standard_normal(c).astype(np.float32), (rng.standard_normal(c) * 0.5).astype(np.float32)
    invstd = (1 / np.sqrt(rng.uniform(0.5, 2, c))).astype(np.float32)
    dy = rng.standard_normal((m, c)).astype(np.float32)
    x[0], dy[0] = mean - beta / invstd, np.nan                      # pre ~ 0 or tiny: whatever the gate, no NaN leaks
    x[1, :] = mean
    beta0 = beta.copy()
    beta0[:] = 0                                                    # row 1 with beta 0: pre == 0 exactly, gate closed
    dy[1] = np.inf
    dx = R.bn_relu_bwd_frozen_ref(x, dy, mean, invstd, beta0)
    assert np.all(dx[1] == 0)
    y = R.bn_relu_apply_ref(x, mean, invstd, beta0)
    ok = np.isfinite(dy)
    assert np.array_equal((dx != 0) & ok, (y > 0) & ok & (dy * invstd != 0))
    ref = np.where(y > 0, dy.astype(np.float64) * invstd.astype(np.float64), 0.0)
    assert np.allclose(dx[ok], ref[ok], rtol=2.0 ** -23, atol=0)
    b = R.bn_relu_bwd_frozen_ref(R.to_bf16(x), R.to_bf16(dy), R.to_bf16(mean), invstd, beta0, bf16=True)
    assert np.array_equal(b[1:], R.to_bf16(b)[1:]) and np.all(b[1] == 0)     # (row 0 carries the NaNs)


def test_elementwise_restatements():
    rng = np.random.default_rng(9)
    w = rng.standard_normal((7, 5)).astype(np.float32)
    d = R.head_logit_bwd_ref(w, [0, 4, 5, -1], 4)
    assert np.array_equal(d[0], w[:, 0]) and np.array_equal(d[1], w[:, 4]) and not d[2:].any()
    assert np.array_equal(R.head_logit_bwd_ref(w, None, 2), np.stack([w[:, 0]] * 2))
    a = rng.standard_normal((6, 4)).astype(np.float32)
    x = rng.standard_normal((6, 4)).astype(np.float32)
    assert np.array_equal(R.scale_input_ref(a, np.float32(0.5)), a * np.float32(0.5))
    acc = R.accumulate_ref(a, np.full_like(a, np.nan), 2.0, True)
    assert np.array_equal(acc, a * np.float32(2))
    assert np.array_equal(R.accumulate_ref(x, acc, 0.25, False), acc + x * np.float32(0.25))
    assert np.array_equal(R.map_ref(0, a), np.abs(a[:, :3]).max(axis=1))
    assert np.allclose(R.map_ref(1, a, x), np.sum(a[:, :3].astype(np.float64) * x[:, :3], axis=1), atol=1e-5)


def test_validation_errors_without_gpu():
    from jr import _ffi
    L = _ffi.load()
    INV, UNS = _ffi.JR_ERR_INVALID, _ffi.JR_ERR_UNSUPPORTED
    seg = (_ffi.BnSeg * 1)(_ffi.BnSeg(16, 0, 8, 8, 16, None))      # (dbeta NULL is fine)
    args = (ctypes.byref(seg), 16, 0, 8, 10, 8, 16, 16, 16, None)
    for bad in (2, 3, 4, 7):                                         # the conv-only dtypes, an unknown one
        assert L.jr_bn_relu_bwd_frozen(bad, 1, *args) == INV
    assert L.jr_bn_relu_bwd_frozen(0, 0, *args) == INV and "segments" in _ffi.last_error()
    assert L.jr_bn_relu_bwd_frozen(0, 1, ctypes.byref(seg), None, 0, 8, 10, 8, 16, 16, 16, None) == INV
    assert L.jr_bn_relu_bwd_frozen(0, 1, ctypes.byref(seg), 16, 4, 8, 10, 8, 16, 16, 16, None) == INV   # x slice
    assert L.jr_bn_relu_bwd_frozen(0, 1, ctypes.byref(seg), 16, 0, 16, 10, 16, 16, 16, 16, None) == INV  # sum c
    nodY = (_ffi.BnSeg * 1)(_ffi.BnSeg(None, 0, 8, 8, 16, None))
    assert L.jr_bn_relu_bwd_frozen(0, 1, ctypes.byref(nodY), 16, 0, 8, 10, 8, 16, 16, 16, None) == INV
    assert L.jr_bn_relu_bwd_frozen(0, 1, ctypes.byref(seg), 16, 0, 2048, 10, 2048, 16, 16, 16, None) in (INV, UNS)

    def desc(h=11, w=9, cin=3, cout=32, k=3, s=2, pad=0, yoff=0, ystride=None, ho=None):
        oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
        return _ffi.ConvDesc(2, h, w, cin, cout, k, k, s, s, pad, pad, oh if ho is None else ho, ow, 0, 4, yoff,
                             ystride or cout)
    img = L.jr_conv2d_bwd_image
    assert img(None, 0, 16, 16, 16, 4, None) == INV and "null descriptor" in _ffi.last_error()
    assert img(ctypes.byref(desc()), 0, None, 16, 16, 4, None) == INV
    for bad in (2, 3, 4, 9):
        assert img(ctypes.byref(desc()), bad, 16, 16, 16, 4, None) == INV and "storage" in _ffi.last_error()
    assert img(ctypes.byref(desc(ho=7)), 0, 16, 16, 16, 4, None) == INV and "ho/wo" in _ffi.last_error()
    assert img(ctypes.byref(desc()), 0, 16, 16, 16, 2, None) == INV                       # dx_c_stride < c_in
    assert img(ctypes.byref(desc(yoff=40, ystride=64)), 0, 16, 16, 16, 4, None) == INV    # slice past the stride
    assert img(ctypes.byref(desc(yoff=4, ystride=64)), 1, 16, 16, 16, 4, None) == INV     # bf16: offsets % 8
    assert img(ctypes.byref(desc(cin=8)), 0, 16, 16, 16, 8, None) == UNS
    assert img(ctypes.byref(desc(h=21, w=21, k=9)), 0, 16, 16, 16, 4, None) == UNS
    assert img(ctypes.byref(desc(h=21, w=21, s=3)), 0, 16, 16, 16, 4, None) == UNS
    assert img(ctypes.byref(desc(cout=24)), 0, 16, 16, 16, 4, None) == UNS
    assert img(ctypes.byref(desc(cout=2048, k=7, pad=3)), 0, 16, 16, 16, 4, None) == UNS and "LDS" in _ffi.last_error()

    assert L.jr_head_logit_bwd(None, None, 2, 8, 1, 16, None) == INV
    assert L.jr_head_logit_bwd(16, None, 2, 8, 1, None, None) == INV
    assert L.jr_head_logit_bwd(16, None, 0, 8, 1, 16, None) == INV
    assert L.jr_head_logit_bwd(16, None, 2, 8, 17, 16, None) == INV
    assert L.jr_attr_scale_input(2, 16, 16, 10, 0.5, None) == INV
    assert L.jr_attr_scale_input(0, None, 16, 10, 0.5, None) == INV
    assert L.jr_attr_scale_input(0, 16, 16, 0, 0.5, None) == INV
    assert L.jr_attr_accumulate(None, 16, 10, 1.0, 1, None) == INV
    assert L.jr_attr_accumulate(16, 16, -1, 1.0, 1, None) == INV
    assert L.jr_attr_map(2, 16, 4, 16, 0, 4, 10, 3, 16, None) == INV
    assert L.jr_attr_map(0, 16, 4, None, 4, 4, 10, 3, 16, None) == INV                    # dtype
    assert L.jr_attr_map(1, 16, 4, None, 0, 4, 10, 3, 16, None) == INV                    # mode 1 needs x
    assert L.jr_attr_map(0, 16, 2, None, 0, 4, 10, 3, 16, None) == INV                    # stride < c
    assert L.jr_attr_map(0, 16, 4, None, 0, 4, 10, 4, 16, None) == UNS and "c must be 3" in _ffi.last_error()
    assert L.jr_attr_map(0, None, 4, None, 0, 4, 10, 3, 16, None) == INV


def test_evaluate_refuses_attribution_without_frozen_bn_or_with_tta(capsys):
    sys.path.insert(0, PKG)
    import evaluate
    p = evaluate.build_parser()
    base = ["-o", "--data_dir", "x"]
    a = p.parse_args(base + ["--bn", "moving", "--attribution", "integrated", "--attribution_dir", "d"])
    assert (a.attribution, a.attribution_steps, a.attribution_dir) == ("integrated", 16, "d")
    assert p.parse_args(base).attribution is None
    for extra, word in ((["--attribution", "gradient", "--attribution_dir", "d"], "--bn moving"),
                        (["--bn", "moving", "--tta", "flips", "--attribution", "gradient", "--attribution_dir", "d"],
                         "--tta"),
                        (["--bn", "moving", "--attribution", "gradient"], "--attribution_dir"),
                        (["--bn", "moving", "--attribution", "integrated", "--attribution_dir", "d",
                          "--attribution_steps", "0"], "--attribution_steps"),
                        (["--bn", "moving", "--attribution", "smooth", "--attribution_dir", "d"], "invalid choice")):
        with pytest.raises(SystemExit) as ei:
            p.parse_args(base + extra)
        assert ei.value.code == 2
        assert word in capsys.readouterr().err


def test_new_symbols_are_declared_bound_and_documented():
    from conftest import ROOT
    from jr import _ffi
    names = ("jr_bn_relu_bwd_frozen", "jr_conv2d_bwd_image", "jr_head_logit_bwd", "jr_attr_scale_input",
             "jr_attr_accumulate", "jr_attr_map")
    header = open(os.path.join(ROOT, "include", "jr.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in names:
        assert s in _ffi.EXPORTED and s + "(" in header and s in doc
