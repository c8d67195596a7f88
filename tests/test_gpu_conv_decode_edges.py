"""The conv kernels' row, tap, column and stream-K decode (division-free:
reciprocals from the planner, tests/test_conv_fastdiv.py) at shapes where every
decode wraps INSIDE one tile:

  (3, 7, 11, 16, 32, 3, 3, 1, same)   batch and row carries inside one 128-row tile, ho*wo = 77
  (2, 9, 1, 32, 32, 7, 1, 1, same)    wo = 1
  (2, 13, 9, 16, 48, 3, 3, 2, valid)  four ragged DGRAD stride phases
  (5, 5, 5, 64, 32, 1, 1, 1, same)    M = 125: one partial tile

for JR_F32_X6H and JR_F32_X8, fwd / dgrad / wgrad, at the planner's config id
and at one stream-K id with split field 3 (a 384-block grid cut down to the
work: tiles are cut between blocks and handed off wherever the GEMM has two
blocks' worth of K-tiles).  Judged against the fp64 reference at the bars of
test_gpu_x6h.py / test_gpu_ops.py (5e-6 of max |ref| for fwd and dgrad, 1e-5
for wgrad); two runs of each must be byte-equal."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import tf_ops as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

X6H, X8 = 4, 2
SK_ID = 31 | (3 << 8)      # the stream-K grid of tile 3 (128 x 64, BK 16), split field 3
CASES = [(3, 7, 11, 16, 32, 3, 3, 1, "same"), (2, 9, 1, 32, 32, 7, 1, 1, "same"),
         (2, 13, 9, 16, 48, 3, 3, 2, "valid"), (5, 5, 5, 64, 32, 1, 1, 1, "same")]
BARS = (5e-6, 5e-6, 1e-5)  # fwd, dgrad, wgrad


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs, device copies and the fp64 references of a case (computed once, shared, never written)."""
    from test_gpu_x6h import _lib, _setup
    ffi = _lib()
    n, h, w, cin, cout, kh, kw, s, pad = case
    d, (x, wt, dy), dev, keep = _setup(ffi, case, 1000 + CASES.index(case))
    refs = (R.conv2d(x, wt, s, pad), R.conv2d_bwd_data(dy, wt, x.shape, s, pad),
            R.conv2d_bwd_filter(x, dy, wt.shape, s, pad))
    return ffi, d, dev, keep, refs


@pytest.mark.parametrize("cfg", [-1, SK_ID], ids=["planned", "streamk3"])
@pytest.mark.parametrize("dtype", [X6H, X8], ids=["x6h", "x8"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_decode_edges(case, dtype, cfg):
    from test_gpu_x6h import relerr
    ffi, d, (X, W, DY), keep, refs = _case(case)
    L = ffi.load()
    s = case[7]
    ref = ctypes.byref(d)
    phases = {0: 1, 1: s * s, 2: 1}
    try:
        for op in range(3):
            for ph in range(phases[op]):
                ffi.check("set", L.jr_conv2d_set_config(ref, op, dtype, ph, cfg))
        wsb = max(L.jr_conv2d_workspace_size(ref, op, dtype) for op in range(3))
        ws = torch.zeros(wsb // 4 + 4, device="cuda")
        P = lambda t: t.data_ptr()  # noqa: E731
        calls = (lambda o: L.jr_conv2d_fwd(ref, dtype, P(X), P(W), P(o), P(ws), wsb, None),
                 lambda o: L.jr_conv2d_bwd_data(ref, dtype, P(DY), P(W), P(o), 0, P(ws), wsb, None),
                 lambda o: L.jr_conv2d_bwd_filter(ref, dtype, P(X), P(DY), P(o), P(ws), wsb, None))
        for op, (call, want, bar) in enumerate(zip(calls, refs, BARS)):
            cs = X.shape[-1]      # dx carries the padded channel stride of x
            size = want.size if op != 1 else want.size // want.shape[-1] * cs
            runs = []
            for fill in (0.0, 7.0):                       # a second run over other old contents
                out = torch.full((size,), fill, device="cuda")
                ffi.check(("fwd", "dgrad", "wgrad")[op], call(out))
                torch.cuda.synchronize()
                runs.append(out.cpu().numpy())
            got = runs[0] if op != 1 else runs[0].reshape(want.shape[:-1] + (cs,))[..., :want.shape[-1]]
            err = relerr(got.reshape(want.shape), want)
            print(f"{case} dtype {dtype} cfg {cfg} op {op}: rel err {err:.2e} (bar {bar:.0e})")
            assert err < bar, (op, err)
            assert runs[0].tobytes() == runs[1].tobytes(), op
        ffi.device_check()
    finally:
        for op in range(3):
            for ph in range(phases[op]):
                ffi.check("reset", L.jr_conv2d_set_config(ref, op, dtype, ph, -1))
