"""The guarded frozen forward of x6h, the part that needs no GPU: every
*_guard entry point refuses a limit that is not finite and > 0 before any HIP
call (other arguments valid or null alike), jr_absmax_reset refuses a null
pointer and a negative count, and evaluate.py's parser refuses --x6h_frozen
outside --bn moving / --dtype f32 / --conv_math x6h."""
import ctypes
import os
import sys

import pytest

from conftest import PKG

BAD_LIMITS = [0.0, -1.0, float("inf"), float("nan")]
P = 4096        # a non-null "pointer": never dereferenced, the limit is checked first


def _lib():
    from jr import _ffi
    return _ffi, _ffi.load()


def _guarded_calls(ffi, L, limit, null):
    """(name, status) of each guarded entry point with `limit`; null: every pointer NULL."""
    p = None if null else P
    pd = ffi.PoolDesc(2, 9, 9, 8, 4, 4, 0, 8, 0, 8)
    d = None if null else ctypes.byref(pd)
    seg = ffi.BnApplySeg(p, 0, 16, 16, p)
    segs = None if null else ctypes.byref(seg)
    return [
        ("jr_bn_relu_apply_guard",
         L.jr_bn_relu_apply_guard(ffi.JR_F32, p, 0, 16, 5, 16, p, p, p, p, 0, 16, limit, None)),
        ("jr_bn_relu_apply_multi_guard",
         L.jr_bn_relu_apply_multi_guard(ffi.JR_F32, 1, segs, p, 0, 16, 5, 16, p, p, limit, None)),
        ("jr_bn_relu_apply_grouped_guard",
         L.jr_bn_relu_apply_grouped_guard(ffi.JR_F32, 3, p, 0, 16, 80, 5, 16, p, p, 16, p, 16, p, 0, 16, 80, limit,
                                          None)),
        ("jr_bn_relu_maxpool3x3s2_fwd_guard",
         L.jr_bn_relu_maxpool3x3s2_fwd_guard(d, ffi.JR_F32, p, p, p, p, p, p, limit, None)),
        ("jr_bn_relu_maxpool3x3s2_fwd_grouped_guard",
         L.jr_bn_relu_maxpool3x3s2_fwd_grouped_guard(d, ffi.JR_F32, 1, p, p, p, 8, p, 8, p, p, limit, None)),
    ]


@pytest.mark.parametrize("null", [False, True])
@pytest.mark.parametrize("limit", BAD_LIMITS)
def test_guarded_entry_points_refuse_a_bad_limit_before_any_hip_call(limit, null):
    ffi, L = _lib()
    for name, rc in _guarded_calls(ffi, L, limit, null):
        assert rc == ffi.JR_ERR_INVALID, (name, limit, rc)
        assert "limit must be finite and > 0" in ffi.last_error(), (name, ffi.last_error())


def test_a_good_limit_leaves_the_unguarded_validation():
    """With a valid limit the refusals are the unguarded call's (null pointers here)."""
    ffi, L = _lib()
    for name, rc in _guarded_calls(ffi, L, 4096.0, True):
        assert rc == ffi.JR_ERR_INVALID, (name, rc)
        assert "limit" not in ffi.last_error(), (name, ffi.last_error())
    # x6h is conv-only for the guarded apply too; c % 4
    assert L.jr_bn_relu_apply_guard(ffi.JR_F32_X6H, P, 0, 8, 10, 8, P, P, P, P, 0, 8, 1.0, None) == ffi.JR_ERR_INVALID
    assert L.jr_bn_relu_apply_guard(ffi.JR_F32, P, 0, 6, 10, 6, P, P, P, P, 0, 6, 1.0, None) == ffi.JR_ERR_INVALID


def test_absmax_reset_refusals():
    ffi, L = _lib()
    assert L.jr_absmax_reset(None, 64, None) == ffi.JR_ERR_INVALID
    assert L.jr_absmax_reset(None, 0, None) == ffi.JR_ERR_INVALID
    assert L.jr_absmax_reset(P, -1, None) == ffi.JR_ERR_INVALID
    assert L.jr_absmax_reset(P, 0, None) == ffi.JR_OK          # nothing to zero: no HIP call
    assert L.jr_bn_relu_bwd_frozen_absmax(ffi.JR_F32, 1, None, None, 0, 16, 5, 16, None, None, None, None,
                                          None) == ffi.JR_ERR_INVALID


def _parser():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    cwd = os.getcwd()
    import evaluate
    assert os.getcwd() == cwd
    return evaluate.build_parser()


@pytest.mark.parametrize("argv", [
    ["-e", "--x6h_frozen"],                                              # without --bn moving
    ["-e", "--bn", "moving", "--x6h_frozen", "--dtype", "bf16"],
    ["-e", "--bn", "moving", "--x6h_frozen", "--conv_math", "x8"],
    ["-e", "--bn", "moving", "--x6h_frozen", "--conv_math", "f32"],
])
def test_parser_refuses_the_flag_out_of_place(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _parser().parse_args(argv)
    assert e.value.code == 2
    assert "--x6h_frozen requires" in capsys.readouterr().err


def test_parser_accepts_the_flag_and_defaults_to_off():
    p = _parser()
    assert p.parse_args(["-e", "--bn", "moving", "--x6h_frozen"]).x6h_frozen is True
    assert p.parse_args(["-e", "--bn", "moving"]).x6h_frozen is False
    assert p.parse_args(["-e"]).x6h_frozen is False
