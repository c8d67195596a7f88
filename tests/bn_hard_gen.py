"""Conv inputs whose OUTPUT channels are hard for BN statistics (shared by
test_bn_stats_hard_gen.py, which checks the construction on the CPU, and
test_gpu_bn_stats_hard.py, which feeds it to every statistics path).

Input channel 0 is the constant 1, the others post-ReLU-like noise
max(N(0, 1), 0).  The weight from channel 0 sits on the centre tap only, so on
a 1x1 'same' or a k x k 'valid' conv it adds one chosen offset to every pixel
of an output channel.  Output channel co is of class (co + co // 4) % 4, so
every aligned group of 4 channels (one float4 of the epilogue) holds all four
classes and every 32-column MFMA block a mix:

  A  mean 0, spread 1 (the noise weights are scaled by the fp64 spread of the
     noise part and the offset cancels its mean);
  B  |mean| = 256 x spread (class A plus an offset of +-256, the sign
     alternating with co // 4);
  C  exactly constant and non-zero: no noise weights, offset +-(2 + k / 4),
     k = co % 8 (exact in bf16, and so in every operand split);
  D  exactly zero: no weights at all.
"""
import numpy as np

from oracle import tf_ops as R

A, B, C, D = 0, 1, 2, 3
RATIO = 256.0


def classes(cout):
    co = np.arange(cout)
    return (co + co // 4) % 4


def hard_case(n, h, w, cin, cout, kh, kw, stride, pad, seed):
    """(x [n,h,w,cin] float32, wt [kh,kw,cin,cout] float32, cls [cout])."""
    assert cin >= 2 and (pad == "valid" or (kh == 1 and kw == 1))
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0)
    x[..., 0] = 1.0
    x = x.astype(np.float32)
    cls = classes(cout)
    wt = rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * (cin - 1))
    wt[:, :, 0, :] = 0.0
    wt[..., (cls == C) | (cls == D)] = 0.0
    y0 = R.conv2d(x, wt, stride, pad).reshape(-1, cout)        # the noise part, fp64
    noisy = (cls == A) | (cls == B)
    wt[..., noisy] /= y0.std(0)[noisy]
    off = np.zeros(cout)
    off[noisy] = -(y0.mean(0) / np.where(noisy, y0.std(0), 1.0))[noisy]
    sign = np.where((np.arange(cout) // 4) % 2 == 0, 1.0, -1.0)
    off[cls == B] += (RATIO * sign)[cls == B]
    off[cls == C] = (sign * (2.0 + (np.arange(cout) % 8) / 4.0))[cls == C]
    wt[kh // 2, kw // 2, 0, :] = off
    return x, wt.astype(np.float32), cls
