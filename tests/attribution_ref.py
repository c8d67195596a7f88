"""numpy / torch restatements of the attribution surface (TEST ORACLE ONLY).

float32 restatements, one rounding per operation as include/jr.h states them,
of jr_bn_relu_bwd_frozen (on the BN apply's pre-activation), jr_conv2d_bwd_image,
jr_head_logit_bwd, jr_attr_scale_input, jr_attr_accumulate and jr_attr_map; an
fp64 transposed convolution with the sequential-sum error bound of the image
gradient; and the masked-linear model of the whole chain (the network with
every ReLU replaced by a given mask and every max-pool by a gather at given
argmaxes, under given frozen BN statistics: linear in the image, so autograd
gives its exact backward).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.inception_ref import EPS, InceptionV3Ref

f32 = np.float32


def to_bf16(a):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    return torch.as_tensor(np.ascontiguousarray(a, f32)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_bits(a):
    """The uint16 patterns of to_bf16(a)."""
    return (to_bf16(a).view(np.uint32) >> 16).astype(np.uint16)


# ---- BN + ReLU under given statistics
def bn_pre_ref(x, mean, invstd, beta):
    """The pre-activation as the apply forms it: ((x - mean) * invstd) + beta, every operation fp32."""
    x, mean, invstd, beta = (np.asarray(v, f32) for v in (x, mean, invstd, beta))
    with np.errstate(all="ignore"):
        return ((x - mean) * invstd) + beta


def bn_relu_apply_ref(x, mean, invstd, beta, bf16=False):
    y = np.maximum(bn_pre_ref(x, mean, invstd, beta), f32(0))
    return to_bf16(y) if bf16 else y


def bn_relu_bwd_frozen_ref(x, dy, mean, invstd, beta, bf16=False):
    """dx = T(g * invstd), g = pre > 0 ? dy : 0 (a select)."""
    pre = bn_pre_ref(x, mean, invstd, beta)
    g = np.where(pre > 0, np.asarray(dy, f32), f32(0))
    with np.errstate(all="ignore"):
        dx = g * np.asarray(invstd, f32)
    return to_bf16(dx) if bf16 else dx


# ---- the image gradient
def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def conv_bwd_image_ref(dy, w, h, wd, stride, pad):
    """dy [n, ho, wo, c_out] fp32 (bf16 values widened), w [kh, kw, c_in, c_out]
    fp32 -> dx [n, h, wd, c_in] fp32: per tap p = 0, p = p + dy * w over c_out
    ascending; dx = ((0 + p(first)) + p(next)) ... over the valid taps in
    (r, s) ascending order."""
    dy, w = np.asarray(dy, f32), np.asarray(w, f32)
    n, ho, wo, cout = dy.shape
    kh, kw, cin, _ = w.shape
    dx = np.zeros((n, h, wd, cin), f32)
    oy, ox = np.arange(ho), np.arange(wo)
    for r in range(kh):
        iy = oy * stride + r - pad
        vy = (iy >= 0) & (iy < h)
        for s in range(kw):
            ix = ox * stride + s - pad
            vx = (ix >= 0) & (ix < wd)
            p = np.zeros((n, ho, wo, cin), f32)
            for co in range(cout):
                p = p + dy[..., co, None] * w[r, s, :, co]
            sub = p[:, vy][:, :, vx]
            tgt = np.ix_(np.arange(n), iy[vy], ix[vx])
            dx[tgt] = dx[tgt] + sub
    return dx


def conv_bwd_image_fp64(dy, w, h, wd, stride, pad):
    """(dx, sum |dy| |w|, valid taps T) per element from an fp64 conv_transpose."""
    dy64 = torch.as_tensor(np.asarray(dy, np.float64)).permute(0, 3, 1, 2)
    w64 = torch.as_tensor(np.asarray(w, np.float64)).permute(3, 2, 0, 1)        # [c_out, c_in, kh, kw]
    kh, kw = w.shape[:2]
    ho, wo = dy.shape[1:3]
    oph, opw = h - ((ho - 1) * stride - 2 * pad + kh), wd - ((wo - 1) * stride - 2 * pad + kw)

    def tr(a, b):
        # (output_padding < stride; the rest of an uncovered border is zero padding)
        eh, ew = max(oph - (stride - 1), 0), max(opw - (stride - 1), 0)
        o = F.conv_transpose2d(a, b, stride=stride, padding=pad, output_padding=(oph - eh, opw - ew))
        return F.pad(o, (0, ew, 0, eh)).permute(0, 2, 3, 1).numpy()
    dx = tr(dy64, w64)
    mag = tr(dy64.abs(), w64.abs())
    taps = tr(torch.ones_like(dy64[:, :1]), torch.ones(1, 1, kh, kw, dtype=torch.float64))[..., 0]
    return dx, mag, np.rint(taps).astype(np.int64)


def gamma(k):
    u = k * 2.0 ** -24
    return u / (1.0 - u)


# ---- head and the elementwise passes
def head_logit_bwd_ref(w, target, n):
    """w [c, units] -> dfeat [n, c] = w[:, t_i]; zeros for a t_i outside [0, units)."""
    w = np.asarray(w, f32)
    c, units = w.shape
    out = np.zeros((n, c), f32)
    for i in range(n):
        t = 0 if target is None else int(target[i])
        if 0 <= t < units:
            out[i] = w[:, t]
    return out


def scale_input_ref(src, alpha, bf16=False):
    with np.errstate(all="ignore"):
        y = np.asarray(src, f32) * f32(alpha)
    return to_bf16(y) if bf16 else y


def accumulate_ref(dx, acc, weight, first):
    with np.errstate(all="ignore"):
        a = np.zeros_like(np.asarray(dx, f32)) if first else np.asarray(acc, f32)
        return a + np.asarray(dx, f32) * f32(weight)


def map_ref(mode, acc, x=None):
    """acc [..., >= 3], x [..., >= 3] (fp32 values) -> [...]"""
    acc = np.asarray(acc, f32)
    with np.errstate(all="ignore"):
        if mode == 0:
            return np.maximum(np.maximum(np.abs(acc[..., 0]), np.abs(acc[..., 1])), np.abs(acc[..., 2]))
        x = np.asarray(x, f32)
        return ((acc[..., 0] * x[..., 0]) + (acc[..., 1] * x[..., 1])) + (acc[..., 2] * x[..., 2])


# ---- the whole chain
class MaskedLinearRef(InceptionV3Ref):
    """Inception-v3 with every conv2d_bn's ReLU replaced by masks[k] ([B, C, H, W]
    of 0 / 1, k = 1..94), every max-pool by a gather at argmax[j] ([B, C, Ho,
    Wo] window positions 0..8, in network order) and BN by the frozen
    statistics `stats` (Keras names): linear in the image."""

    def __init__(self, params, stats, masks, argmax, dtype=torch.float64, emulate_bf16=False):
        super().__init__(params, dtype, requires_grad=False, emulate_bf16=emulate_bf16)
        self.stats, self.masks, self.argmax = stats, masks, argmax
        self._pool = 0

    def conv2d_bn(self, x, filters, num_row, num_col, padding="same", strides=(1, 1)):
        self._k += 1
        k = self._k
        w, beta = self.P[f"conv2d_{k}/kernel"], self.P[f"batch_normalization_{k}/beta"]
        pad = ((num_row - 1) // 2, (num_col - 1) // 2) if padding == "same" else (0, 0)
        y = self._r(F.conv2d(x, self._r(w).permute(3, 2, 0, 1), stride=strides, padding=pad))
        mean = torch.as_tensor(self.stats[f"batch_normalization_{k}/moving_mean"], dtype=self.dtype)
        var = torch.as_tensor(self.stats[f"batch_normalization_{k}/moving_variance"], dtype=self.dtype)
        eps = torch.tensor(EPS, dtype=torch.float32).to(self.dtype)     # (the fp32 constant the library adds)
        invstd = 1.0 / torch.sqrt(var + eps)
        y = (y - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        return self._r(y * torch.as_tensor(self.masks[k], dtype=self.dtype))

    def maxpool(self, x):
        am = torch.as_tensor(self.argmax[self._pool].astype(np.int64))
        self._pool += 1
        b, c, ho, wo = am.shape
        oy = torch.arange(ho).view(1, 1, ho, 1)
        ox = torch.arange(wo).view(1, 1, 1, wo)
        idx = (2 * oy + am // 3) * x.shape[3] + (2 * ox + am % 3)
        return x.flatten(2).gather(2, idx.flatten(2)).view(b, c, ho, wo)

    def input_gradient(self, x_nhwc, target=None):
        """d sum_i logit_{t_i}(i) / d x -> [B, h, w, 3] (float64 array)."""
        self._pool = 0
        x = torch.tensor(np.asarray(x_nhwc), dtype=self.dtype, requires_grad=True)
        logits = self.features(x) @ self.P["dense/kernel"] + self.P["dense/bias"]
        t = torch.zeros(len(x), dtype=torch.int64) if target is None else torch.as_tensor(target, dtype=torch.int64)
        logits.gather(1, t.view(-1, 1)).sum().backward()
        return x.grad.double().numpy()
