"""The hard-channel generator of test_gpu_bn_stats_hard.py (bn_hard_gen.py),
checked on the fp64 oracle's output, no GPU: classes C and D are exactly
constant and exactly zero, class B has |mean| = 256 x spread, class A mean 0
and spread 1, and every aligned group of 4 output channels (and so every
32-column block) holds at least two classes."""
import numpy as np
import pytest

from oracle import tf_ops as R

import bn_hard_gen as G

CASES = [(2, 18, 18, 32, 96, 3, 3, 1, "valid"), (1, 15, 17, 32, 96, 3, 3, 1, "valid"),
         (2, 37, 37, 3, 32, 3, 3, 2, "valid"), (1, 64, 64, 4, 16, 1, 1, 1, "same"),
         (1, 64, 64, 8, 16, 1, 1, 1, "same")]


@pytest.mark.parametrize("case", CASES)
def test_hard_channel_classes(case):
    n, h, w, cin, cout, kh, kw, s, pad = case
    x, wt, cls = G.hard_case(*case, seed=5)
    assert x.dtype == np.float32 and wt.dtype == np.float32
    assert np.all(x[..., 0] == 1.0) and np.all(x >= 0)
    y = R.conv2d(x, wt, s, pad).reshape(-1, cout)
    mu, sd = y.mean(0), y.std(0)
    c, d, a, b = (cls == G.C), (cls == G.D), (cls == G.A), (cls == G.B)
    assert np.all(y[:, d] == 0.0)
    assert np.all(y[:, c] == y[0, c]) and np.all(y[0, c] != 0.0)
    # (the weights are rounded to fp32 after the fp64 calibration: 1e-6 relative)
    assert np.all(np.abs(sd[a | b] - 1.0) < 1e-5)
    assert np.all(np.abs(mu[a]) < 1e-5)
    assert np.all(np.abs(np.abs(mu[b]) / sd[b] - G.RATIO) < 1e-2)
    assert (mu[b] > 0).any() and (mu[b] < 0).any()
    for g in range(0, cout, 4):
        assert len(set(cls[g:g + 4])) >= 2
    for g in range(0, cout, 32):
        assert len(set(cls[g:g + 32])) == 4
    # the bf16 path rounds both operands: C and D stay exact, B stays hard
    import torch
    rb = lambda t: torch.as_tensor(t).to(torch.bfloat16).double().numpy()  # noqa: E731
    yb = R.conv2d(rb(x), rb(wt), s, pad).reshape(-1, cout)
    assert np.all(yb[:, d] == 0.0) and np.all(yb[:, c] == y[0, c])
    assert np.all(np.abs(yb[:, b].mean(0)) / yb[:, b].std(0) > 200)
