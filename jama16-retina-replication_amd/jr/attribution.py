"""Per-image saliency maps: which pixels moved this score?

What is differentiated is the LOGIT of one class of one image (not the loss,
not the probability), with respect to that image, under frozen BN
(Engine.freeze_bn + forward(bn="frozen")): with batch statistics the gradient
of one image's logit leaks into the whole batch; with frozen statistics
d logit_i / d x_i is a property of image i.

  attribute(engine, "gradient")     max_c |d logit / d x_c| per pixel
  attribute(engine, "integrated")   integrated gradients from the black image
                                    (Sundararajan et al. 2017), midpoint rule:
                                    sum_c x_c * mean_k d logit / d x_c (alpha_k x)

Every step is a libjr call (jr.h: jr_attr_scale_input, jr_attr_accumulate,
jr_attr_map) around Engine.forward(bn="frozen") and Engine.input_gradient;
their fp32 arithmetic is stated there and restated in tests/attribution_ref.py.

conv_math="x6h" engines need x6h_frozen=True (jr.Engine) and then work
unchanged: integrated gradients scale the image by alpha <= 1, which stays
inside the image bound x_bound = 1 of the first conv, and every forward is the
guarded one.  The x6h data gradients scale each layer's dy by its measured
per-batch maximum (a gradient has no a-priori bound), so an x6h map of an image
depends on the rest of its batch within the x6h error class -- not bitwise
independent, as the x8 / f32 maps and the x6h predictions are.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ffi

METHODS = ("gradient", "integrated")


def _accumulate(e, n: int, weight: float, first: bool) -> None:
    _ffi.check("jr_attr_accumulate", e.lib.jr_attr_accumulate(
        e.dinput.data_ptr(), e.attr_acc.data_ptr(), n, float(weight), 1 if first else 0, e._s))


def attribute(engine, method: str, steps: int = 16, target=None, B=None) -> torch.Tensor:
    """A device tensor [B, h, w] (fp32) for the batch of the last set_batch
    (B: its size, default the engine's).  The engine needs input_grad=True and
    frozen BN statistics (freeze_bn).  Afterwards the engine's logits and
    predictions are those of a plain frozen forward of the batch."""
    if method not in METHODS:
        raise ValueError(f"attribute: unknown method {method!r} (one of {', '.join(METHODS)})")
    if method == "integrated" and int(steps) < 1:
        raise ValueError("attribute: steps must be at least 1")
    e = engine
    if not getattr(e, "input_grad", False):
        raise ValueError("attribute needs an engine built with input_grad=True")
    B = B or e.batch
    ib = e.g.bufs[e.g.input_buf]
    pixels = B * ib.h * ib.w
    with torch.cuda.stream(e.stream):
        out = torch.empty(pixels, dtype=torch.float32, device=e.device)
    if method == "gradient":
        e.forward(B, bn="frozen")
        e.input_gradient(B, target)
        _accumulate(e, 4 * pixels, 1.0, True)
        _ffi.check("jr_attr_map", e.lib.jr_attr_map(_ffi.JR_ATTR_ABSMAX, e.attr_acc.data_ptr(), 4, None, e.dt,
                                                    e.in_stride, pixels, ib.c, out.data_ptr(), e._s))
    else:
        steps = int(steps)
        e._check_frozen("frozen")       # (before the input buffer is touched)
        x, n_in = e.acts[e.g.input_buf], pixels * e.in_stride
        with torch.cuda.stream(e.stream):
            e.x0[:n_in].copy_(x[:n_in])
        try:
            for k in range(steps):
                alpha = np.float32((k + 0.5) / steps)
                _ffi.check("jr_attr_scale_input", e.lib.jr_attr_scale_input(
                    e.dt, e.x0.data_ptr(), x.data_ptr(), n_in, float(alpha), e._s))
                e.forward(B, bn="frozen")
                e.input_gradient(B, target)
                _accumulate(e, 4 * pixels, np.float32(1.0 / steps), k == 0)
        finally:        # the unscaled batch again, and its logits and predictions
            with torch.cuda.stream(e.stream):
                x[:n_in].copy_(e.x0[:n_in])
            e.forward(B, bn="frozen")
        _ffi.check("jr_attr_map", e.lib.jr_attr_map(_ffi.JR_ATTR_DOT_INPUT, e.attr_acc.data_ptr(), 4, e.x0.data_ptr(),
                                                    e.dt, e.in_stride, pixels, ib.c, out.data_ptr(), e._s))
    # the caller's stream sees the finished map
    torch.cuda.current_stream(e.device).wait_stream(e.stream)
    out.record_stream(torch.cuda.current_stream(e.device))
    return out.view(B, ib.h, ib.w)
