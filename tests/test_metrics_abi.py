"""jr_metrics_accumulate, jr_metrics_reset and jr_step_log_append refuse bad
arguments with JR_ERR_INVALID before any HIP call: no GPU needed (as
test_abi.py does for the others).  The pointers are never dereferenced."""
import pytest

P = 4096        # a non-null, aligned address that no refused call touches


def lib():
    from jr import _ffi
    return _ffi.load()


def test_header_and_binding_carry_the_new_entry_points():
    from jr import _ffi
    from test_abi import header_symbols
    for name in ("jr_metrics_accumulate", "jr_metrics_reset", "jr_step_log_append"):
        assert name in header_symbols() and name in _ffi.EXPORTED
    import ctypes
    assert ctypes.sizeof(_ffi.StepRec) == 16


@pytest.mark.parametrize("args", [
    (None, P, 8, P, 4, P, P, 3),        # null probs
    (P, None, 8, P, 4, P, P, 3),        # null labels
    (P, P, 8, None, 4, P, P, 1),        # counts asked for, no thresholds
    (P, P, 8, P, 4, None, P, 3),        # counts asked for, no counts
    (P, P, 8, P, 4, P, None, 2),        # brier asked for, no brier
    (P, P, 8, P, 4, P, None, 3),
    (P, P, 0, P, 4, P, P, 3),           # n <= 0
    (P, P, -1, P, 4, P, P, 3),
    (P, P, 8, P, 0, P, P, 3),           # T outside 1..1024
    (P, P, 8, P, 1025, P, P, 3),
    (P, P, 8, P, -3, P, P, 2),
    (P, P, 8, P, 4, P, P, 0),           # which outside 1..3
    (P, P, 8, P, 4, P, P, 4),
    (P, P, 8, P, 4, P, P, -1),
])
def test_metrics_accumulate_refuses(args):
    from jr import _ffi
    assert lib().jr_metrics_accumulate(*args, None) == _ffi.JR_ERR_INVALID
    assert "metrics_accumulate" in _ffi.last_error()


def test_metrics_reset_and_step_log_refuse():
    from jr import _ffi
    L = lib()
    assert L.jr_metrics_reset(P, 0, None, None) == _ffi.JR_ERR_INVALID
    assert L.jr_metrics_reset(P, 1025, P, None) == _ffi.JR_ERR_INVALID
    assert L.jr_metrics_reset(None, 0, None, None) == _ffi.JR_OK       # nothing to zero: nothing is called
    for args in ((None, 2, P, P, None), (P, 2, None, P, None), (P, 2, P, None, None), (P, 0, P, P, P)):
        assert L.jr_step_log_append(*args, None) == _ffi.JR_ERR_INVALID
        assert "step_log_append" in _ffi.last_error()
