"""Test references for the moving BN statistics (no GPU, no libjr).

* update_ref / freeze_ref: the formulas of include/jr.h (jr_bn_moving_update,
  jr_bn_moving_freeze) restated in numpy, rounding for rounding: fp64 where
  the header says double, fp32 where it says float.  eps reaches the kernels
  as a C float, so its fp64 value is np.float64(np.float32(1e-3)).
* BNStatsRef: the functional model of oracle/inception_ref.py with conv2d_bn
  overridden -- it records every layer's batch mean and biased variance, or,
  given per-layer (mean, variance), normalises with those instead (frozen BN).
  fp64 is the reference, fp32 the independent implementation whose deviation
  sets the envelope.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.inception_ref import EPS, InceptionV3Ref

EPS32 = np.float32(1e-3)
EPS64 = np.float64(EPS32)


def batch_var_ref(invstd, rows):
    """Steps 1-4 of jr_bn_moving_update: the unbiased batch variance, as fp32."""
    s = np.asarray(invstd, np.float32).astype(np.float64)
    v = 1.0 / (s * s) - EPS64
    v = np.where(v < 0.0, 0.0, v)
    v = v * (np.float64(rows) / np.float64(rows - 1))
    return v.astype(np.float32)


def update_ref(mm, mv, mean_b, invstd, rows, momentum):
    """Step 5: (moving_mean, moving_var) after one update, fp32, every operation rounded on its own."""
    mm, mv, mean_b = (np.asarray(a, np.float32) for a in (mm, mv, mean_b))
    var_b = batch_var_ref(invstd, rows)
    d = np.float32(np.float32(1.0) - np.float32(momentum))
    mm2 = (mm - ((mm - mean_b) * d).astype(np.float32)).astype(np.float32)
    mv2 = (mv - ((mv - var_b) * d).astype(np.float32)).astype(np.float32)
    return mm2, mv2


def freeze_ref(mm, mv):
    """(frozen_mean, frozen_invstd) of jr_bn_moving_freeze."""
    mv = np.asarray(mv, np.float32).astype(np.float64)
    return np.asarray(mm, np.float32).copy(), (1.0 / np.sqrt(mv + EPS64)).astype(np.float32)


class BNStatsRef(InceptionV3Ref):
    """fixed: None (batch statistics, recorded in self.stats[k] = (mean,
    biased variance, rows) of layer k = 1..94), or {k: (mean, variance)} to
    normalise with."""

    def __init__(self, params, dtype=torch.float64, fixed=None, requires_grad=False):
        super().__init__(params, dtype, requires_grad=requires_grad)
        self.fixed = fixed
        self.stats = {}

    def conv2d_bn(self, x, filters, num_row, num_col, padding="same", strides=(1, 1)):
        self._k += 1
        k = self._k
        w = self.P[f"conv2d_{k}/kernel"]
        beta = self.P[f"batch_normalization_{k}/beta"]
        pad = ((num_row - 1) // 2, (num_col - 1) // 2) if padding == "same" else (0, 0)
        y = F.conv2d(x, w.permute(3, 2, 0, 1), stride=strides, padding=pad)
        if self.fixed is None:
            mean = y.mean(dim=(0, 2, 3), keepdim=True)
            var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)      # biased
            self.stats[k] = (mean.detach().reshape(-1).numpy().copy(), var.detach().reshape(-1).numpy().copy(),
                             y.shape[0] * y.shape[2] * y.shape[3])
        else:
            mean, var = (torch.as_tensor(np.asarray(a), dtype=self.dtype).view(1, -1, 1, 1) for a in self.fixed[k])
        y = (y - mean) / torch.sqrt(var + EPS) + beta.view(1, -1, 1, 1)
        return F.relu(y)

    def unbiased(self):
        """{k: (mean, unbiased variance)} of the recorded batch: what one
        update with momentum 0 leaves in the moving statistics."""
        return {k: (m, v * (rows / (rows - 1.0))) for k, (m, v, rows) in self.stats.items()}


def moving_trajectory(params, dtype, batches, momentum):
    """Moving statistics {k: (mean, var)} after one training step per batch
    (x, y) of the functional model in `dtype` (Nesterov, the engine's
    defaults), started from mean 0 / variance 1 and updated in that dtype."""
    ref = BNStatsRef(params, dtype, requires_grad=True)
    state, mov = {}, None
    for x, y in batches:
        ref.train_step(x, y, state)
        cur = ref.unbiased()
        if mov is None:
            mov = {k: (np.zeros_like(m), np.ones_like(v)) for k, (m, v) in cur.items()}
        t = ref.stats[1][0].dtype.type
        mov = {k: (mov[k][0] - (mov[k][0] - cur[k][0]) * t(1 - momentum),
                   mov[k][1] - (mov[k][1] - cur[k][1]) * t(1 - momentum)) for k in cur}
    return mov
