"""Executor for the Inception-v3 training step / inference on libjr kernels.

The reference runs one `sess.run([global_step, mean_xentropy, train_op,
update_brier])` per batch (train.py:231-232): forward of the 94 conv2d_bn
blocks, head + loss, backward, and 190 ApplyMomentum updates.  This module is
that step, MI355X-native:

* All device memory is planned once per (batch, resolution): one NHWC buffer
  per block output (concat-free slices), a raw pre-BN buffer per conv launch
  (kept for the BN backward), one gradient buffer per activation buffer, a
  flat fp32 parameter / gradient / momentum buffer (so one optimizer launch
  and one all-reduce bucket walk cover all 190 tensors).  PyTorch tensors are
  used only as owners of that memory; every op is a libjr C-ABI call.
* Conv launches follow jr.plan: sibling 1x1 layers reading one buffer run as
  one fused GEMM (their kernels stored side by side), each member keeping its
  own BN, beta and output slice.
* Calls are pre-bound (ctypes function + argument tuple) into call lists, so a
  step is a flat loop of C calls on one HIP stream, and the whole step can be
  captured into a HIP graph (jr_graph_*) and replayed.  One routine enqueues
  a step's lists in order (Engine._enqueue_step, its tail _finish_update) for
  train_step, every micro-batch of an accumulation group and capture; one
  settles the host's books after it (Engine._settle).
* Optional (bn_moving=momentum): one more launch per step keeps Keras-style
  moving averages of every BN layer's batch statistics (jr_bn_moving_update);
  freeze_bn() + forward(bn="frozen") then normalise with fixed statistics, so
  an image's output depends on that image alone.  conv_math="x6h" takes part
  only with x6h_frozen=True: the frozen lists then store every activation
  through the guarded entry points (Replica._frozen_guard: a constant scale,
  predictions bitwise batch-independent, an activation above the bound raises
  JRError(JR_ERR_DEVICE) at the next synchronize() / predictions()).
* Optional (weight_ema=decay): two more launches per step keep a moving
  average of the weights (jr_ema_prepare, jr_ema_update; the counter and the
  warm-up decay live on the device); averaged_weights() runs forwards on it.
* Optional (label_smoothing / class_weight / focal_gamma): the head calls of
  every list are jr_head_fwd_ex / jr_head_bwd_ex with the loss recipe; and
  (dropout=rate) the lists of a training step -- _build_calls(training=True):
  train_step, capture, replay -- drop the pooled features before the dense
  layer (jr_dropout_fwd / _bwd / _advance; key, counter, threshold and scale
  in device memory, so a replay draws the next mask).  No other forward drops.
* Optional (accum_steps=K > 1): K micro-batches per optimizer update.  A
  micro-step that does not close its group ends with jr_grad_accumulate into
  one more flat buffer (acc <- g, then acc <- acc + g) instead of the
  optimizer; the closing one folds it back (g <- g + acc) ahead of today's
  update phase, whose grad_scale becomes 1 / (k * world).
* Optional (metrics_init / step_log_enable / set_batch(staged=True); DESIGN.md
  §15): the streaming metrics and a ring of per-step records live in device
  memory (jr_metrics_accumulate, jr_step_log_append, enqueued on self.stream
  BEHIND the step's call lists, never inside them), and uint8 batches arrive
  through two pinned slots on a feed stream, so a loop needs the host only
  once in a while (their state: jr.runahead; staged or not, one routine
  launches the conversion kernel: Replica._u8_to_input).
* Optional (input_grad=True): a third call list, the data-gradient chain of
  one logit per image down to the image after a frozen forward
  (input_gradient: jr_head_logit_bwd, jr_bn_relu_bwd_frozen, the data
  gradients, jr_conv2d_bwd_image) -- what jr.attribution builds saliency maps
  from.  No filter gradients, no optimizer, no training buffers.  On x6h
  (x6h_frozen=True) the frozen BN backward also measures max |dx| per launch
  (jr_bn_relu_bwd_frozen_absmax, the dy scale of its data gradient): that
  gradient is batch-independent within the x6h error class, not bitwise.
* Data parallel: gradients are all-reduced (torch.distributed backend 'nccl' =
  RCCL over xGMI) in buckets issued during the backward pass, in reverse layer
  order, so communication overlaps the remaining backward kernels.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import json
import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _ffi
from . import augment as _augment
from .inception import BN_EPS, Graph, PoolNode, build_inception_v3
from .init import ALIGN, init_params
from .lanes import Build, Call, Lanes, node_lanes, schedule
from .plan import ConvUnit, bn_batch_groups, bn_moving_segments, build_plan, decay_ranges
from .runahead import STEP_REC, Feed, Metrics, StepLog

DTYPES = {"f32": _ffi.JR_F32, "bf16": _ffi.JR_BF16}


_PINNED = None


def fusable_pools(g: Graph, plan) -> Dict[int, int]:
    """max-pool node index -> its input buffer, for every max-pool whose
    input is the whole output of ONE single-member conv launch and read by
    nothing else (the stem's conv2d_3 and conv2d_5): BN + ReLU then run
    inside the pool (jr_bn_relu_maxpool3x3s2_fwd)."""
    out = {}
    for i, n in enumerate(g.nodes):
        if n.kind != "maxpool":
            continue
        prod = [m for m in g.nodes if m.y.buf == n.x]
        readers = [m for m in g.nodes if m.x == n.x]
        if len(prod) != 1 or len(readers) != 1 or prod[0].kind != "conv":
            continue
        u = plan.unit_of[prod[0].idx]
        if len(u.members) == 1 and prod[0].y.c_off == 0 and prod[0].cout == g.bufs[n.x].c:
            out[i] = n.x
    return out


def pinned_tile_table(conv_math: str, batch: int, height: int, width: int, train: bool) -> Optional[dict]:
    """The committed tile table (jr/tiles_mi355x.json) of this workload, or None."""
    global _PINNED
    if _PINNED is None:
        # (JR_TILE_TABLES: another table file, for A/B runs of re-tuned tables)
        env = os.environ.get("JR_TILE_TABLES")
        if env and not os.path.exists(env):
            raise FileNotFoundError(f"JR_TILE_TABLES={env}: no such tile table file")
        p = env or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tiles_mi355x.json")
        _PINNED = json.load(open(p))["tables"] if os.path.exists(p) else []
    for t in _PINNED:
        if (t["conv_math"], t["batch"], t["height"], t["width"], t["train"]) == (conv_math, batch, height, width,
                                                                              train):
            return t
    return None


class MagRows:
    """The layout of the JR_F32_X6H magnitude words, rows of ROW floats in one
    tensor (Replica.absmax) -- the one place that knows it.  One row per (conv
    launch, member) for its filter block, the members of a launch contiguous
    (the grouped conv's convention); then, with dgrad, one row per launch for
    its raw-output gradient.  The betas' maxima land in the LAST row: a row of
    their own where there are no gradient rows (jr.EnsembleEngine); else
    (jr.Engine) the last gradient row, zeroed again by the same prep and raised
    by the first BN backward only after it: harmless, a larger bound; conv2d_1's
    data gradient is never used (a row of their own there
    too is `self.rows = ... + 1` below)."""
    ROW = 64

    def __init__(self, order: Dict[int, int], members: int, dgrad: bool):
        launches = self._k = order          # launch -> its place in plan order
        self.members, self.filt_rows = members, len(launches) * members
        self.dgrad_rows = len(launches) if dgrad else 0
        self.rows = self.filt_rows + (self.dgrad_rows or 1)
        self.beta = self.rows - 1
        self.size = self.ROW * self.rows

    def filt(self, uid: int, m: int = 0) -> int:
        """Row of member m's filter block of launch uid."""
        return self._k[uid] * self.members + m

    def dgrad(self, uid: int) -> int:
        """Row of launch uid's raw-output gradient."""
        if not self.dgrad_rows:
            raise KeyError("no data-gradient magnitude rows")
        return self.filt_rows + self._k[uid]

    def span(self, row: int, rows: int = 1) -> Tuple[int, int]:
        """(first float, float count) of `rows` rows from `row` on."""
        return self.ROW * row, self.ROW * rows


@dataclasses.dataclass(frozen=True)
class Region:
    """Elements start + r * stride + j (r < rows, j < width) of the flat tensor `name` (Replica.regions)."""
    name: str
    start: int
    width: int
    rows: int = 1
    stride: int = 0

    def contains(self, elem: int) -> bool:
        e = elem - self.start
        if e < 0:
            return False
        if self.rows == 1:
            return e < self.width
        return e // self.stride < self.rows and e % self.stride < self.width


class Replica:
    """What jr.Engine and jr.EnsembleEngine (jr.ensemble) share: the device
    and library, arithmetic codes, the launch plan, the lanes, and the
    tables and uploads both build the same way (members: tensors are
    member-major; jr.Engine is one member)."""
    members = 1

    def __init__(self, graph: Graph, device, dtype: str, conv_math: Optional[str], maths: Tuple[str, ...], head: str,
                 fuse_siblings: bool, fuse_pool: Optional[bool], lanes: int, priorities=(), x6h_frozen: bool = False):
        if dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}")
        if conv_math is None:            # fp32 default: x8 (fp32-accurate, on the bf16 matrix cores)
            conv_math = "x8" if dtype == "f32" else "bf16"
        if conv_math not in (maths if dtype == "f32" else ("bf16",)):
            raise ValueError(f"conv_math: one of {maths} for dtype f32 (x8 = JR_F32_X8, x8p = JR_F32_X8P on pre-split "
                             "operand planes, x6h = JR_F32_X6H scaled fp16 split, f32 = fp32 MFMA); 'bf16' for bf16")
        if x6h_frozen and conv_math != "x6h":
            raise ValueError("x6h_frozen=True is the guarded frozen forward of conv_math='x6h' "
                             f"(this engine: conv_math={conv_math!r})")
        if not torch.cuda.is_available():
            raise RuntimeError(f"jr.{type(self).__name__} needs a ROCm GPU (libjr has no CPU path)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        _ffi.init(self.device.index or 0)
        self.lib = _ffi.load()
        self.g, self.units = graph, graph.units
        self.dtype, self.dt = dtype, DTYPES[dtype]
        # dtype code of the convolution calls: JR_F32_X8 keeps every tensor
        # fp32 and forms the GEMM products on the bf16 matrix cores from an
        # exact three-way split (jr.h); everything else runs self.dt
        self.conv_math = conv_math
        self.x8p = conv_math == "x8p"
        # JR_F32_X6H: every conv operand's power-of-two scale from its largest
        # magnitude -- filters and data gradients measured on the device
        # (jr_absmax_prep once per step, the BN backward's fused max), the
        # activations from the bound |relu(xhat + beta)| <= sqrt(N - 1) +
        # max |beta| (Samuelson), beta guarded on the device (jr.h)
        self.x6h = conv_math == "x6h"
        # x6h_frozen (opt-in): frozen-BN forwards (and the input gradient) run on
        # x6h too.  Samuelson's bound does not hold for values normalised with
        # fixed statistics, so the frozen call lists store every activation
        # through the *_guard entry points instead (_frozen_guard), which keep
        # the constant scale of act_bound and report an activation above it
        # through jr_device_check (synchronize / predictions: JR_ERR_DEVICE)
        self.x6h_frozen = bool(x6h_frozen)
        self.cdt = {"x8": _ffi.JR_F32_X8, "x8p": _ffi.JR_F32_X8P, "x6h": _ffi.JR_F32_X6H}.get(conv_math, self.dt)
        # activation dtype: fp32, or bf16 (parameters, gradients, momentum,
        # BN statistics and the head stay fp32 master copies either way)
        self.act_dtype = torch.bfloat16 if self.dt == _ffi.JR_BF16 else torch.float32
        self.esz = 2 if self.dt == _ffi.JR_BF16 else 4
        self._vw = 16 // self.esz       # channels per 16-byte vector (one launch: <= 256 per row)
        # the image buffer is kept one 16 B DMA piece wide per pixel (4 fp32 /
        # 8 bf16 channels, zeros past c = 3): conv1's c_in = 3 runs on libjr's
        # virtual channel padding
        self.in_stride = (self.g.bufs[self.g.input_buf].c + self._vw - 1) // self._vw * self._vw
        self.head_mode = _ffi.JR_HEAD_SIGMOID if head == "sigmoid" else _ffi.JR_HEAD_SOFTMAX
        # lanes (jr.lanes): lane 0 is self.stream, where every step starts and
        # ends; every lane has its OWN conv workspace (split-K slabs, stream-K
        # partial slots, statistics partials), the resource ("ws", lane)
        self.lanes = Lanes(self.lib, self.device, lanes, priorities)
        self.lane_streams, self.nlanes, self.precise_waits = self.lanes.streams, self.lanes.n, self.lanes.precise_waits
        self.stream, self._s = self.lanes.streams[0], self.lanes.handles[0]
        self.plan = build_plan(self.g, fuse_siblings)
        self.cunits, self.nparam = self.plan.units, self.plan.nparam
        # conv2d_bn outputs read only by a max-pool (the stem's conv2d_3 and
        # conv2d_5): BN + ReLU run inside the pool (jr_bn_relu_maxpool3x3s2_fwd)
        # and the full-resolution activation is never written
        if fuse_pool is None:           # (JR_FUSE_POOL=0: the separate apply + max-pool, for A/B runs)
            fuse_pool = os.environ.get("JR_FUSE_POOL", "1") != "0"
        self.pool_fused = fusable_pools(self.g, self.plan) if fuse_pool else {}
        self.fused_bufs = set(self.pool_fused.values())
        # resources (jr.lanes.schedule): the channel slices of every buffer
        slices: Dict[int, set] = {self.g.input_buf: {0}}
        for n in self.g.nodes:
            slices.setdefault(n.y.buf, set()).add(n.y.c_off)
        self.slices = {b: sorted(o) for b, o in slices.items()}
        self._aug_ws = None             # the augmented upload's workspace and tables, at first use

    def _after_fill(self, t: torch.Tensor) -> torch.Tensor:
        """The stream-ordering rule of every allocation (DESIGN.md "Step
        audit"): a buffer is allocated and filled on torch's current stream,
        and lane 0 -- where every step starts, and which the other lanes
        fork from -- then waits for that stream.  The lanes are streams of
        their own and order nothing with the current stream implicitly:
        without the wait a fill that lands late overwrites what a lane wrote
        (the zero fill of `moving` after _reset_bn_moving's mean 0 / variance
        1).  The one place: _t, _table and _dev_bytes all end here."""
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)
        return t

    def _t(self, n: int, dtype=torch.float32) -> torch.Tensor:
        return self._after_fill(torch.zeros(int(n), dtype=dtype, device=self.device))

    def _dev_bytes(self, data: bytes) -> torch.Tensor:
        return self._after_fill(torch.frombuffer(bytearray(data), dtype=torch.uint8).to(self.device))

    def _table(self, struct, rows) -> torch.Tensor:
        """A device copy of a ctypes struct array."""
        return self._dev_bytes(bytes((struct * len(rows))(*rows)))

    def _a_all(self, b: int) -> list:
        return [("a", b, o) for o in self.slices[b]]

    def _p(self, name: str, m: int = 0) -> int:
        return self.params.data_ptr() + 4 * (m * self.nparam + self.plan.poff[name])

    def _beta(self, n, m: int = 0) -> int:
        return self._p(f"batch_normalization_{n.idx + 1}/beta", m)

    def _pool_producer(self, n: PoolNode):
        """The conv2d_bn layer whose BN + ReLU a fused max-pool applies."""
        return next(m for m in self.g.nodes if m.y.buf == n.x)

    def _alloc_forward(self, dgrad_rows: bool) -> None:
        """What a forward of self.members members reads and writes, member-major
        with member strides (act_ms, raw_ms, stats_ms; batch, units, nparam for
        the head's and the parameters)."""
        g, B, M, at = self.g, self.batch, self.members, self.act_dtype
        if self.x6h:
            # (first: every conv descriptor points into it; the ensemble's filters
            # never change in inference: measured at load_params)
            self._alloc_absmax(B, dgrad_rows)
        self.act_ms = [B * b.h * b.w * (self.in_stride if b.id == g.input_buf else b.c) for b in g.bufs]
        self.acts = [self._t(M * n, at) for n in self.act_ms]
        # raw (pre-BN) output and BN statistics per conv launch; a fused
        # group's members see channel slices of them
        self.raw_ms = {u.first.idx: B * u.ho * u.wo * u.cout for u in self.cunits}
        self.raw_unit = {k: self._t(M * n, at) for k, n in self.raw_ms.items()}
        self.stats_ms = self.plan.stats_size
        self.stats = self._t(M * self.stats_ms)
        self._alloc_bn_moving()
        self.feat = self._t(M * B * g.bufs[g.output_buf].c)
        self.logits = self._t(M * B * self.units)
        self.probs = self._t(M * B * self.units)
        self.labels = self._t(B * self.units)
        self.loss = self._t(4 * M)
        self.params = self._t(M * self.nparam)

    def _alloc_ws(self, nbytes: int) -> None:
        """Every lane's own conv workspace of nbytes."""
        self.ws_bytes = int(nbytes)
        self.ws_lane = [self._t((self.ws_bytes + 15) // 4 + 4) for _ in range(self.nlanes)]
        self.ws = self.ws_lane[0]

    def _alloc_bf16_filters(self, planes: int = 1, hwio: bool = True) -> None:
        """bf16 operand copies of every conv launch's kernel (block) of every
        member, written from the fp32 master parameters by ONE
        jr_conv_weights_bf16_multi launch: HWIO (bwd_data; hwio) and W^T
        [co][kh][kw][c8] (fwd).  planes = 3 (JR_F32_X8P): each copy is the
        three bf16 planes of the exact split, jr_conv_weights_x8p_multi."""
        M = self.members
        self.wplanes = planes
        per, tiles, ho, to = [], 0, 0, 0
        self.wb_hwio_off, self.wb_t_off = {}, {}
        for u in self.cunits:
            c8 = (u.cin + 7) // 8 * 8
            per.append((u, ho if hwio else 0, to, tiles))
            self.wb_hwio_off[u.first.idx], self.wb_t_off[u.first.idx] = ho, to
            tiles += self.lib.jr_conv_weights_bf16_tiles(u.kh, u.kw, u.cin, u.cout)
            # 16 B-aligned starts (8 bf16); x8p: three planes per layer, plane
            # stride = the layer's element count (jr.h)
            ho += (planes * u.kh * u.kw * u.cin * u.cout + 7) // 8 * 8
            to += planes * u.cout * u.kh * u.kw * c8
        self.wt_ms = (to + 7) // 8 * 8          # member stride of the W^T copies
        layers = [_ffi.WPrep(m * self.nparam + u.koff, o_h, m * self.wt_ms + o_t, u.kh, u.kw, u.cin, u.cout,
                             m * tiles + t0, 0) for m in range(M) for u, o_h, o_t, t0 in per]
        self.wprep_table = self._table(_ffi.WPrep, layers)
        self.wprep_layers, self.wprep_tiles = len(layers), M * tiles
        self.w_hwio = self._t(ho, torch.bfloat16) if hwio else None
        self.w_t = self._t(M * self.wt_ms, torch.bfloat16)

    def _alloc_absmax(self, B: int, dgrad_rows: bool) -> None:
        """The JR_F32_X6H magnitude words (MagRows) and the jr_absmax_prep
        table: the filters, then every BN beta with the activation guard."""
        M = self.members
        self._arow = {u.first.idx: k for k, u in enumerate(self.cunits)}    # launch -> its place in plan order
        self.mag = MagRows(self._arow, M, dgrad_rows)
        self.absmax = self._t(self.mag.size)
        nmax = max(B * u.ho * u.wo for u in self.cunits)
        # activations are BN + ReLU outputs (or pools of them): |y| <= sqrt(N-1)
        # + max |beta|; bound = a power of two >= sqrt(N_max) + 1024, beta
        # guarded at that bound, so |y| <= 2 bound < the 4 bound the scale
        # keeps representable
        self.act_bound = float(2 ** int(np.ceil(np.log2(np.sqrt(nmax) + 1024))))
        segs = [_ffi.AbsmaxSeg(m * self.nparam + u.koff, u.kh * u.kw * u.cin * u.cout, self.mag.filt(u.first.idx, m),
                               0.0) for u in self.cunits for m in range(M)]
        segs += [_ffi.AbsmaxSeg(m * self.nparam + self.plan.poff[f"batch_normalization_{n.idx + 1}/beta"], n.cout,
                                self.mag.beta, self.act_bound)
                 for m in range(M) for u in self.cunits for n in u.members]
        self.absmax_table = self._table(_ffi.AbsmaxSeg, segs)
        self.absmax_nseg = len(segs)

    def _frozen_guard(self) -> Optional[float]:
        """The limit of the guarded BN applies and fused stem pools of a frozen
        call list (x6h_frozen), or None: the unguarded entry points.

        limit = 2 * act_bound.  act_bound is a power of two m, so the convs'
        activation scale is exactly 2^14 / m (jr.h): values up to 2 m still
        split exactly and fp16 saturates only near 4 m -- the margin the beta
        guard of _alloc_absmax keeps for the batch-statistics forward.  Every
        conv input is covered: the image is <= 1 (x_bound = 1); every BN + ReLU
        output is stored by a guarded call; and the max- and average-pools
        (mixed3 / mixed8 included) read non-negative guarded values, whose
        maximum or mean never exceeds them, so the pools need no guard of
        their own.  The scale is a constant, not a measurement: a frozen x6h
        prediction stays bitwise independent of the other images of the batch."""
        return 2.0 * self.act_bound if self.x6h and self.x6h_frozen else None

    @staticmethod
    def _frozen_reads(b: Build) -> list:
        """A frozen call list's BN applies and fused pools read self.frozen, not the batch statistics."""
        return [("frozen",)] if b.stats_shift else []

    def _wmax(self, u: ConvUnit) -> int:
        """The magnitude rows of a launch's filters, member 0's first (w_absmax)."""
        return self.absmax.data_ptr() + 4 * self.mag.span(self.mag.filt(u.first.idx))[0]

    def _dmax(self, u: ConvUnit) -> int:
        """The magnitude row of a launch's raw-output gradient (dy_absmax)."""
        return self.absmax.data_ptr() + 4 * self.mag.span(self.mag.dgrad(u.first.idx))[0]

    # ---- the statistics: addresses in the plan's layout (Plan.stats_size, ConvUnit.soff)
    def _mean(self, u: ConvUnit, co: int = 0, m: int = 0) -> int:
        """Member m's batch mean of a launch's channels from column co on (frozen: the caller adds stats_shift)."""
        return self.stats.data_ptr() + 4 * (m * self.stats_ms + u.soff + co)

    def _invstd(self, u: ConvUnit, co: int = 0, m: int = 0) -> int:
        return self._mean(u, u.cout + co, m)

    def _A(self, bid: int, m: int = 0) -> int:
        return self.acts[bid].data_ptr() + self.esz * m * self.act_ms[bid]

    def _conv_desc(self, u: ConvUnit, B: int) -> _ffi.ConvDesc:
        if self.x8p:          # x describes the operand planes: channel radix padded to 8
            xs = (u.cin + 7) // 8 * 8
        else:
            xs = self.in_stride if u.x == self.g.input_buf else u.cin
        d = _ffi.ConvDesc(B, u.h, u.w, u.cin, u.cout, u.kh, u.kw, u.stride, u.stride,
                          u.pad_h, u.pad_w, u.ho, u.wo, 0, xs, 0, u.cout)
        if self.x6h:
            d.x_bound = 1.0 if u.x == self.g.input_buf else self.act_bound    # images: f32(k) * f32(1/255) <= 1
            d.w_absmax = self._wmax(u)
        return d

    def _upload(self, images, labels, B: int, augment=None, warp=None) -> None:
        """A batch (NHWC float32, or uint8 to be scaled by 1/255; a host array
        or a device tensor) into the first member's input buffer and the
        labels, on self.stream.  augment / warp: jr.augment tables (one
        jr_augment_param / jr_warp_param per image) for a uint8 batch, which
        _u8_to_input converts from this upload's own device copies."""
        ib = self.g.bufs[self.g.input_buf]
        x, pixels = torch.as_tensor(images), B * ib.h * ib.w
        tab, wtab = _augment.batch_tables(B, augment, warp)
        if x.dtype == torch.uint8:
            if tab is not None:     # device copies of the host tables
                self._aug_buffers()
                self._aug_tab[:tab.nbytes].copy_(torch.from_numpy(tab.view(np.uint8)), non_blocking=True)
                if wtab is not None:
                    self._warp_tab[:wtab.nbytes].copy_(torch.from_numpy(wtab.view(np.uint8)), non_blocking=True)
            xd = x.to(self.device, non_blocking=True).reshape(-1)
            self._u8_to_input(xd.data_ptr(), B, None if tab is None else self._aug_tab.data_ptr(),
                              None if wtab is None else self._warp_tab.data_ptr())
            self._keep_u8 = xd
        elif tab is not None:
            raise ValueError("augment / warp need a uint8 batch (float batches are not augmented)")
        else:
            v = self.acts[self.g.input_buf][:pixels * self.in_stride].view(pixels, self.in_stride)
            v[:, ib.c:].zero_()
            v[:, :ib.c].copy_(x.to(torch.float32).reshape(pixels, ib.c).to(self.device, non_blocking=True))
        if labels is not None:
            y = torch.as_tensor(labels, dtype=torch.float32).reshape(-1)
            self._check_labels(y, B)
            self.labels[:y.numel()].copy_(y, non_blocking=True)

    def _aug_buffers(self) -> torch.Tensor:
        """The augmenting kernels' workspace (returned) and _upload's device tables: at first use, for
        the planned batch."""
        if self._aug_ws is None:
            ib = self.g.bufs[self.g.input_buf]
            self._aug_ws, self._aug_tab, self._warp_tab = (
                torch.empty(int(n), dtype=torch.uint8, device=self.device)
                for n in (self.lib.jr_augment_workspace_size(self.batch, ib.h, ib.w),
                          self.batch * _augment.PARAM_DTYPE.itemsize, self.batch * _augment.WARP_DTYPE.itemsize))
        return self._aug_ws

    def _u8_to_input(self, x: int, B: int, tab: Optional[int] = None, wtab: Optional[int] = None) -> None:
        """uint8 pixels at device address x -> the first member's input buffer (times 1/255), on
        self.stream: plain, through the colour table at device address tab, or the warp table at wtab too."""
        ib, dst = self.g.bufs[self.g.input_buf], self.acts[self.g.input_buf].data_ptr()
        if tab is None:
            name, args = "jr_image_u8_to_nhwc", (x, dst, self.dt, B * ib.h * ib.w, ib.c, self.in_stride)
        else:
            ws = self._aug_buffers()
            args = (x, dst, self.dt, B, ib.h, ib.w, ib.c, self.in_stride, tab)
            if wtab is None:
                name, args = "jr_image_u8_augment_nhwc", args + (ws.data_ptr(), ws.numel())
            else:
                name, args = "jr_image_u8_warp_augment_nhwc", args + (wtab, ws.data_ptr(), ws.numel())
        _ffi.check(name, getattr(self.lib, name)(*args, self._s))

    def _check_labels(self, y, B: int) -> None:
        if len(y) != B * self.units:
            raise ValueError("labels must have batch*units elements")

    def _check_images(self, images, B: int) -> None:
        ib = self.g.bufs[self.g.input_buf]
        if B > self.batch or B <= 0:
            raise ValueError(f"batch {B} outside 1..{self.batch}")
        if tuple(images.shape[1:]) != (ib.h, ib.w, ib.c):
            raise ValueError(f"images must be [B,{ib.h},{ib.w},{ib.c}] NHWC, got {tuple(images.shape)}")

    # ------------------------------------------- moving BN statistics, frozen BN
    def _alloc_bn_moving(self) -> None:
        """Beside self.stats (the plan's statistics layout, member stride
        self.stats_ms): `moving` (mean 0 and variance 1 as Keras initialises
        them) and `frozen` (what a frozen forward reads)."""
        self.moving = self._t(self.members * self.stats_ms)
        self.frozen = self._t(self.members * self.stats_ms)
        self._bn_tables: Dict[int, tuple] = {}
        self._reset_bn_moving()
        self.frozen_source = None       # what freeze_bn last froze ("moving" / "batch")
        self.updates = 0                # jr_bn_moving_update launches since the statistics were set

    def _reset_bn_moving(self, var: float = 1.0) -> None:
        """moving_mean = 0, moving_var = var, on self.stream (in order with the launches that update them)."""
        host = np.zeros((self.members, self.stats_ms), np.float32)
        for n, _, ov in self.plan.bn_layers():
            host[:, ov:ov + n.cout] = var
        with torch.cuda.stream(self.stream):
            self.moving.copy_(torch.from_numpy(host.reshape(-1)).to(self.device))

    def _bn_table(self, B: int) -> tuple:
        """(device segment table, nseg, max_c) of the jr_bn_moving_* launches at batch B."""
        if B not in self._bn_tables:
            segs = [_ffi.BnMovingSeg(so, mo, rows, c, 0) for so, mo, rows, c in bn_moving_segments(self.cunits, B)]
            self._bn_tables[B] = (self._table(_ffi.BnMovingSeg, segs), len(segs), max(u.cout for u in self.cunits))
        return self._bn_tables[B]

    def _bn_update_args(self, B: int, momentum: float, s) -> tuple:
        table, nseg, max_c = self._bn_table(B)
        return (table.data_ptr(), nseg, max_c, self.members, self.stats.data_ptr(), self.stats_ms,
                self.moving.data_ptr(), self.stats_ms, float(momentum), BN_EPS, s)

    def _bn_moving_get(self) -> List[dict]:
        self.synchronize()
        host = self.moving.cpu().numpy().reshape(self.members, self.stats_ms)
        out = []
        for m in range(self.members):
            d = {}
            for n, om, ov in sorted(self.plan.bn_layers(), key=lambda t: t[0].idx):
                d[f"batch_normalization_{n.idx + 1}/moving_mean"] = host[m, om:om + n.cout].copy()
                d[f"batch_normalization_{n.idx + 1}/moving_variance"] = host[m, ov:ov + n.cout].copy()
            out.append(d)
        return out

    def _bn_moving_set(self, dicts) -> None:
        if len(dicts) != self.members:
            raise ValueError(f"expected {self.members} members' BN statistics, got {len(dicts)}")
        host = np.zeros((self.members, self.stats_ms), np.float32)
        for m, d in enumerate(dicts):
            for n, om, ov in self.plan.bn_layers():
                for key, o, kind in ((f"batch_normalization_{n.idx + 1}/moving_mean", om, "mean"),
                                     (f"batch_normalization_{n.idx + 1}/moving_variance", ov, "var")):
                    if key not in d:
                        raise ValueError(f"BN statistics lack {key}")
                    v = np.asarray(d[key], np.float32).reshape(-1)
                    if v.size != n.cout:
                        raise ValueError(f"{key}: {v.size} values, the layer has {n.cout} channels")
                    if not np.all(np.isfinite(v)):
                        raise ValueError(f"{key}: non-finite values")
                    if kind == "var" and np.any(v < 0):
                        raise ValueError(f"{key}: negative variance")
                    host[m, o:o + n.cout] = v
        with torch.cuda.stream(self.stream):
            self.moving.copy_(torch.from_numpy(host.reshape(-1)).to(self.device))
        self.stream.synchronize()

    def freeze_bn(self, source: str = "moving") -> None:
        """Fill the statistics a frozen forward (forward(bn="frozen"))
        normalises with: "moving" = from the moving averages
        (jr_bn_moving_freeze), "batch" = a device copy of the batch statistics
        of the last forward (bit for bit what that forward applied)."""
        if source == "moving":
            table, nseg, max_c = self._bn_table(self.batch)
            _ffi.check("jr_bn_moving_freeze", self.lib.jr_bn_moving_freeze(
                table.data_ptr(), nseg, max_c, self.members, self.moving.data_ptr(), self.stats_ms,
                self.frozen.data_ptr(), self.stats_ms, BN_EPS, self._s))
        elif source == "batch":
            with torch.cuda.stream(self.stream):
                self.frozen.copy_(self.stats)
        else:
            raise ValueError("freeze_bn: source is 'moving' or 'batch'")
        self.frozen_source = source

    def calibrate_bn(self, batches) -> int:
        """Moving statistics for parameters trained without them: a forward
        with batch statistics over every batch of `batches` (image arrays, or
        (images, labels) pairs), and after batch k one jr_bn_moving_update with
        momentum 1 - 1/k -- the cumulative mean of the batches' means and
        unbiased variances (started from zero, so the first batch's statistics
        are taken exactly).  Eager.  Returns the number of batches."""
        self._reset_bn_moving(0.0)
        k = 0
        for item in batches:
            images = item[0] if isinstance(item, (tuple, list)) else item
            B = self.set_batch(images)
            self.forward(B)
            k += 1
            _ffi.check("jr_bn_moving_update",
                       self.lib.jr_bn_moving_update(*self._bn_update_args(B, 1.0 - 1.0 / k, self._s)))
        if k == 0:
            self._reset_bn_moving()
            raise ValueError("calibrate_bn: no batches")
        self.updates = k
        return k

    def _check_frozen(self, bn: str) -> bool:
        """forward's bn argument -> frozen?; the refusals of the frozen mode."""
        if bn == "batch":
            return False
        if bn != "frozen":
            raise ValueError("forward: bn is 'batch' or 'frozen'")
        if self.x6h and not self.x6h_frozen:
            raise ValueError("bn='frozen' is not available with conv_math='x6h': its activation scale rests on the "
                             "bound |relu(xhat + beta)| <= sqrt(N - 1) + max |beta| of values standardised by their "
                             "own batch, which frozen statistics void; use x8, x8p, f32 or bf16")
        if getattr(self, "fold_stats", False):
            raise ValueError("bn='frozen' is not available with fold_stats=True: that BN apply computes the batch "
                             "statistics itself")
        if self.frozen_source is None:
            raise ValueError("bn='frozen' before freeze_bn()")
        return True

    # ----- the resource map: what memory the keys of the call lists name
    # keys that name whole tensors (those the engine has), and tensors of a list or dict by index
    _WHOLE = {"p": ("params",), "acc": ("accum", "adam_v"), "w16": ("w_hwio", "w_t"), "feat": ("feat",),
              "head": ("logits", "probs", "loss"), "lab": ("labels",), "dfeat": ("dfeat",), "draw2": ("draw_stem2",),
              "wss": ("ws_stem",), "gnorm": ("opt_partials", "opt_step_dev", "opt_hyper"), "bn_moving": ("moving",),
              "frozen": ("frozen",), "target": ("ig_target",), "dinput": ("dinput",), "gacc": ("gacc",),
              "ema": ("ema", "ema_state"), "drop": ("drop_state",), "feat_drop": ("feat_drop",)}
    _INDEXED = {"draw": "draw_lane", "drawp": "drawp_lane", "ws": "ws_lane", "ap": "aplanes", "am": "argmax"}

    @staticmethod
    def _keep_of(lists) -> list:
        """The kept objects of a _build_calls tuple (jr.Engine's five, jr.EnsembleEngine's two)."""
        return lists[3] if len(lists) > 2 else lists[1]

    @classmethod
    def _slab_arena(cls, lists) -> Optional[torch.Tensor]:
        """The deferred filter-gradient arena of one call-list build."""
        return next((t for t in cls._keep_of(lists) if isinstance(t, torch.Tensor) and t.dtype == torch.float32), None)

    def _slice_regions(self, name: str, t: torch.Tensor, buf: int, c_off: int, C: int) -> List[Region]:
        """A channel slice (up to the next slice of self.slices) of every member's part of buffer t, C channels wide."""
        offs = self.slices[buf]
        k = offs.index(c_off)
        width = (offs[k + 1] if k + 1 < len(offs) else C) - c_off
        ms = t.numel() // self.members
        return [Region(name, m * ms + c_off, width, ms // C, C) for m in range(self.members)]

    def regions(self, key, lists=None) -> List[Region]:
        """The memory a resource key of the call lists names (member-major
        tensors: every member's part).  `lists`: the _build_calls tuple the key
        comes from (needed for ("slab", uid): the arena belongs to one build).
        Total over what the builders emit; an unknown key raises KeyError."""
        kind, g = key[0], self.g
        if kind == "a":
            C = self.in_stride if key[1] == g.input_buf else g.bufs[key[1]].c
            return self._slice_regions(f"acts[{key[1]}]", self.acts[key[1]], key[1], key[2], C)
        if kind == "d":
            return self._slice_regions(f"dacts[{key[1]}]", self.dacts[key[1]], key[1], key[2], g.bufs[key[1]].c)
        if kind == "r":
            u = self.plan.unit_of[key[1]]
            return [Region(f"raw[{key[1]}]", 0, self.raw_unit[key[1]].numel()),
                    Region("stats", u.soff, 2 * u.cout, self.members, self.stats_ms)]
        if kind == "g":
            # a tensor's resource includes the alignment padding behind it (jr.init.ALIGN):
            # the optimizer walks the whole flat buffer, so the ("g", ...) keys together
            # are all of `grads`
            pad = lambda n: (n + ALIGN - 1) // ALIGN * ALIGN     # noqa: E731
            if key[1] == "dense":
                sizes = {name: (off, pad(size)) for name, _, off, size in self.plan.layout}
                return [Region("grads", *sizes["dense/kernel"]), Region("grads", *sizes["dense/bias"])]
            u = self.plan.unit_of[key[1]]
            betas = [self.plan.poff[f"batch_normalization_{m.idx + 1}/beta"] for m in u.members]
            return [Region("grads", u.koff, pad(u.kh * u.kw * u.cin * u.cout))] + [
                Region("grads", o, pad(m.cout)) for o, m in zip(betas, u.members)]
        if kind == "wmax":
            return [Region("absmax", *self.mag.span(0, self.mag.filt_rows))]
        if kind == "dmax":
            return [Region("absmax", *self.mag.span(self.mag.dgrad(key[1])))]
        if kind == "drawb":
            return [Region(f"drawb[{key[1]}][{key[2]}]", 0, self.drawb[key[1]][key[2]].numel())]
        if kind == "slab":
            # read from the bound jr_conv2d_bwd_filter_slabs call (arena pointer and byte count)
            c = next(c for c in lists[1] if key in c.writes and c.fn.__name__ == "jr_conv2d_bwd_filter_slabs")
            off = int(c.args[4]) - self._slab_arena(lists).data_ptr()
            return [Region("slab_arena", off // 4, int(c.args[5]) // 4)]
        if kind in self._INDEXED:
            name = self._INDEXED[kind]
            return [Region(f"{name}[{key[1]}]", 0, getattr(self, name)[key[1]].numel())]
        out = [Region(n, 0, getattr(self, n).numel()) for n in self._WHOLE.get(kind, ())
               if getattr(self, n, None) is not None]
        if not out:
            raise KeyError(f"regions: unknown resource key {key!r}")
        return out

    def universe(self, lists=None) -> Dict[str, torch.Tensor]:
        """Every device tensor the engine owns, by the names regions() uses; with
        `lists` (a _build_calls tuple) also that build's slab arena and device tables."""
        out = {}

        def put(name, t):
            if isinstance(t, torch.Tensor):
                out[name] = t

        for name in ("stats", "moving", "frozen", "feat", "logits", "probs", "labels", "loss", "params", "grads",
                     "accum", "adam_v", "dfeat", "draw_stem2", "w_hwio", "w_t", "wprep_table", "absmax", "absmax_table",
                     "ws_stem", "dinput", "x0", "attr_acc", "ig_target", "opt_partials", "opt_hyper", "opt_step_dev",
                     "_opt_ranges_dev", "_aug_ws", "_aug_tab", "_warp_tab", "gacc", "ema", "ema_state", "drop_state",
                     "feat_drop"):
            put(name, getattr(self, name, None))
        for name in ("acts", "dacts", "draw_lane", "drawp_lane", "ws_lane"):
            for k, t in enumerate(getattr(self, name, None) or ()):
                put(f"{name}[{k}]", t)
        for name, short in (("raw_unit", "raw"), ("argmax", "argmax"), ("aplanes", "aplanes")):
            for k, t in (getattr(self, name, None) or {}).items():
                put(f"{short}[{k}]", t)
        for s, row in enumerate(getattr(self, "drawb", None) or ()):
            for k, t in enumerate(row):
                put(f"drawb[{s}][{k}]", t)
        for B, tab in (getattr(self, "_bn_tables", None) or {}).items():
            put(f"bn_table[{B}]", tab[0])
        if lists is not None:
            arena = self._slab_arena(lists)
            put("slab_arena", arena)
            k = 0
            for t in self._keep_of(lists):
                if isinstance(t, torch.Tensor) and t is not arena:
                    put(f"keep_table[{k}]", t)
                    k += 1
        return out


class Engine(Replica):
    """One model replica on one GPU (one process per GPU)."""

    def __init__(self, batch: int, height: int = 299, width: int = 299, units: int = 1,
                 device: int | torch.device = 0, dtype: str = "f32", train: bool = True,
                 optimizer: str = "nesterov", lr: float = 3e-3, momentum: float = 0.9,
                 head: str = "sigmoid", seed: int = 0, graph: Optional[Graph] = None,
                 autotune: bool = False, tiles: str = "pinned", fuse_siblings: bool = True, lanes: int = 2,
                 conv_math: Optional[str] = None, defer_wgrad: Optional[bool] = None, fuse_pool: Optional[bool] = None,
                 fold_stats: Optional[bool] = None, bn_moving: Optional[float] = None, input_grad: bool = False,
                 x6h_frozen: bool = False, weight_decay: float = 0.0, clip_norm: Optional[float] = None,
                 device_lr: bool = False, rmsprop_rho: float = 0.9, rmsprop_momentum: float = 0.9,
                 rmsprop_eps: float = 1.0, weight_ema: Optional[float] = None, weight_ema_warm: bool = True,
                 label_smoothing: float = 0.0, class_weight=None, focal_gamma: float = 0.0,
                 dropout: Optional[float] = None, dropout_seed: int = 0, dropout_stream: int = 0,
                 accum_steps: int = 1):
        # the optimizer recipe with its scalars in device memory (jr.h: jr_opt_*;
        # off by default, on when any of the three is set): L2 weight decay on
        # the filters and the dense kernel, clipping of the global gradient
        # norm (None: none), and a learning rate set_lr may change between
        # steps and between replays of a captured step
        if not (float(weight_decay) >= 0.0 and np.isfinite(weight_decay)):
            raise ValueError("weight_decay: a finite value >= 0")
        if clip_norm is not None and not (float(clip_norm) > 0.0 and np.isfinite(clip_norm)):
            raise ValueError("clip_norm: None or a finite norm > 0")
        self.weight_decay = float(weight_decay)
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.opt_ex = bool(train) and (self.weight_decay != 0.0 or self.clip_norm is not None or bool(device_lr))
        # weight_ema: None, or the decay in [0, 1) of the moving average of the
        # weights every training step then updates (jr.h: jr_ema_*; TF
        # ExponentialMovingAverage, 0.9999 in the published Inception-v3 recipe);
        # weight_ema_warm: decay = min(decay, (1 + t) / (10 + t)) at update t
        if weight_ema is not None and not 0.0 <= float(weight_ema) < 1.0:
            raise ValueError("weight_ema: None or a decay in [0, 1)")
        self.weight_ema = None if weight_ema is None or not train else float(weight_ema)
        self.weight_ema_warm = bool(weight_ema_warm)
        self.ema, self.ema_state, self._averaged = None, None, False
        # the loss recipe (jr.h jr_loss_spec; off by default, on when any of the
        # three is set): label smoothing, per-unit class weights (None: ones; one
        # positive weight per unit), the focal exponent (sigmoid head only).  The
        # head calls are then jr_head_fwd_ex / jr_head_bwd_ex in every forward, so
        # loss_value() after a validation forward is the training objective
        self.loss_spec = self._loss_spec(units, head, label_smoothing, class_weight, focal_gamma)
        # dropout: None, or the rate in [0, 1) of the dropout between the global
        # average pool and the dense layer in the forward of a TRAINING step alone
        # (jr.h jr_dropout_*: the mask is a function of (dropout_seed,
        # dropout_stream), the device's step counter and the element index;
        # data-parallel replicas pass their rank as dropout_stream)
        if dropout is not None and not 0.0 <= float(dropout) < 1.0:
            raise ValueError("dropout: None or a rate in [0, 1)")
        self.dropout = None if dropout is None or not train else float(dropout)
        self.dropout_key = (int(dropout_seed) & 0xFFFFFFFF, int(dropout_stream) & 0xFFFFFFFF)
        self.feat_drop, self.drop_state = None, None
        # accum_steps: micro-batches per optimizer update (1: every batch updates, nothing
        # below exists).  K > 1: every train_step still runs the forward, the backward, the
        # BN moving averages and the dropout counter, but only the K-th of a group runs the
        # optimizer, on the sum of the group's gradients scaled by 1 / (k * world) -- K
        # virtual data-parallel ranks, each under its own BN statistics (jr.h
        # jr_grad_accumulate; `gacc` holds the open group's sum, _pending counts it)
        if isinstance(accum_steps, bool) or int(accum_steps) != accum_steps or int(accum_steps) < 1:
            raise ValueError("accum_steps: a whole number of micro-batches >= 1")
        self.accum_steps = int(accum_steps) if train else 1
        self.gacc, self._pending = None, 0
        # bn_moving: None, or the momentum of the moving averages of the BN
        # statistics every training step then updates (Keras: 0.99)
        if bn_moving is not None and not 0.0 <= float(bn_moving) <= 1.0:
            raise ValueError("bn_moving: None or a momentum in [0, 1]")
        self.bn_momentum = None if bn_moving is None else float(bn_moving)
        # input_grad: the buffers of the data-gradient chain down to the image
        # (input_gradient, jr.attribution), with or without train
        self.input_grad = bool(input_grad)
        if self.input_grad and conv_math == "x8p":
            raise ValueError("input_grad=True is not available with conv_math='x8p': the input-gradient call list "
                             "does not write its operand planes; use x8, f32 or bf16")
        # JR_LANE_PRIORITY="p0,p1,...": HIP stream priority per lane (lower =
        # higher priority). Default: lane 0 (the trunk) high for fp32 steps,
        # measured 0.1 ms/step faster over 6 interleaved rounds on two boxes
        # (profiles/r05_ab_prio_f32*.txt); all normal for bf16, where it
        # measured neutral. Priority moves no result: scheduling only.
        prio = os.environ.get("JR_LANE_PRIORITY", "-1,0" if dtype == "f32" else "")
        super().__init__(graph or build_inception_v3(height, width, units), device, dtype, conv_math,
                         ("x8", "x8p", "x6h", "f32"), head, fuse_siblings, fuse_pool, lanes,
                         [int(v) for v in prio.split(",") if v.strip()], x6h_frozen=x6h_frozen)
        self.batch, self.train_mode = batch, train
        self._data_grads = train or self.input_grad     # gradient buffers and data-gradient plans exist
        self._frozen_fwd = None         # batch size of the frozen forward since the last set_batch, if any
        if optimizer not in ("nesterov", "momentum", "sgd", "adam", "rmsprop"):
            raise ValueError(f"unknown optimizer {optimizer}")
        self.optimizer = optimizer
        self.lr, self.momentum = float(lr), float(momentum)
        # Adam (north-star extra; TF AdamOptimizer defaults): accum holds m;
        # beta1_power / beta2_power are fp32 variables initialised to beta1 /
        # beta2 and multiplied by them (fp32) after every step, as TF's
        # AdamOptimizer._finish does
        self.adam_b1, self.adam_b2, self.adam_eps, self.adam_t = 0.9, 0.999, 1e-8, 0
        self.adam_b1p, self.adam_b2p = np.float32(self.adam_b1), np.float32(self.adam_b2)
        # RMSProp (TF RMSPropOptimizer; the published Inception-v3 recipe: 0.9,
        # 0.9, 1.0): accum holds mom (from zeros), adam_v holds ms (from ones).
        # No per-step host scalar: it captures and follows set_lr like momentum
        self.rmsprop_rho, self.rmsprop_momentum, self.rmsprop_eps = (float(rmsprop_rho), float(rmsprop_momentum),
                                                                     float(rmsprop_eps))
        # backward order per conv launch: the data gradient (the critical
        # path to the next layer's BN backward) before the filter gradient
        # (JR_DGRAD_FIRST=0: filter gradient first)
        self.dgrad_first = os.environ.get("JR_DGRAD_FIRST", "1") != "0"
        # a fused sibling launch's members' BN + ReLU in one launch
        # (JR_APPLY_MULTI=0: one launch per member, for A/B runs)
        self.apply_multi = os.environ.get("JR_APPLY_MULTI", "1") != "0"
        # the BN-statistics finalize folded into the BN apply for launches whose
        # partials are single-stage and at most JR_FOLD_MAX_P per channel
        # (jr_conv2d_fwd_bn_partials + jr_bn_relu_apply_stats: a kernel
        # boundary fewer per layer; bitwise the separate finalize).  Opt-in
        # (JR_FOLD_STATS=1): measured neutral, f32 and bf16
        # (profiles/r05_ab_rows_{bf16,f32}.txt)
        if fold_stats is None:
            fold_stats = os.environ.get("JR_FOLD_STATS", "0") == "1"
        self.fold_stats = bool(fold_stats)
        self.fold_max_p = int(os.environ.get("JR_FOLD_MAX_P", "512"))
        # fp32: the fused stem pools' backward carries the BN reduce (bf16
        # keeps the separate kernels, whose batch-of-rows fp32 sums it would
        # not reproduce bit for bit; JR_FUSE_POOL_BWD=0: separate for fp32 too)
        self.pool_bwd = (self.pool_fused if self.dt == _ffi.JR_F32 and os.environ.get("JR_FUSE_POOL_BWD", "1") != "0"
                         else {})
        # the stem's filter gradients on lane 1 (JR_STEM_WGRAD_LANE=0: on lane 0 with the rest of the stem)
        self.stem_wgrad_lane = os.environ.get("JR_STEM_WGRAD_LANE", "1") != "0"
        # the block-output BN backwards batched per block (jr_bn_relu_bwd_batch,
        # opt-in JR_BN_BATCH=1: bitwise the per-layer launch sets, measured
        # neutral -- bf16 9.343 -> 9.359, f32 24.85 -> 24.90 ms, the per-layer
        # sets already overlap on the two lanes)
        self.bn_batch_on = not self.x8p and not self.x6h and os.environ.get("JR_BN_BATCH", "0") == "1"
        # a captured graph's edges are the producer waits; JR_GRAPH_PRECISE=0:
        # tail waits (bf16 replay 10.04 vs 9.28 ms per step, eager 9.31:
        # profiles/r05_graph_probe.txt)
        self.graph_precise = os.environ.get("JR_GRAPH_PRECISE", "1") != "0"
        readers: Dict[int, int] = {}
        for q in self.g.nodes:
            readers[q.x] = readers.get(q.x, 0) + 1
        # the stem: the layers before the first buffer with several readers
        self._stem_end = next((j for j, q in enumerate(self.g.nodes) if readers[q.x] > 1), 0)
        self.layout = self.plan.layout
        self._calls: Dict[Tuple[int, int], tuple] = {}
        self._retired: list = []        # call sets a captured graph may still reference
        # filter gradients of split-K wgrad GEMMs: slabs kept per layer and
        # summed by ONE jr_wgrad_reduce launch per flush point (the end of the
        # backward, and each gradient bucket's issue point: set_flush_points)
        # Default (None): deferred for bf16; fp32 reduces each layer's slabs
        # right after its filter-gradient GEMM (bitwise the same sums), which
        # with producer waits overlaps the other lane: 24.30 -> 24.06 ms per
        # step, bf16 9.25 -> 9.30 the other way (profiles/r05_ab_defer*.txt).
        # JR_DEFER_WGRAD=0/1 overrides the default.
        if defer_wgrad is None:
            env = os.environ.get("JR_DEFER_WGRAD", "")
            defer_wgrad = env == "1" if env in ("0", "1") else self.dt != _ffi.JR_F32
        self.defer_wgrad = bool(defer_wgrad)
        self._flush_points: List[int] = []
        self._graphs: Dict[object, int] = {}     # batch (accum_steps > 1: (batch, phase)) -> executable
        self.bucket_hooks: List[Tuple[int, Callable]] = []
        # opt-in, nothing exists until asked for: the device metrics
        # (metrics_init), the step log (step_log_enable), the staged input feed
        # (set_batch(staged=True))
        self._metrics, self._log, self._feed = None, None, None
        self._alloc()
        self.load_params(init_params(self.g, seed))
        self._choose_tiles("autotune" if autotune else tiles)

    @staticmethod
    def _loss_spec(units: int, head: str, label_smoothing: float, class_weight, focal_gamma: float):
        """The jr_loss_spec of the loss keywords, or None when none is set (the plain head calls)."""
        eps, gamma = float(label_smoothing), float(focal_gamma)
        if not 0.0 <= eps < 1.0:
            raise ValueError("label_smoothing: a value in [0, 1)")
        if not (gamma >= 0.0 and np.isfinite(gamma)):
            raise ValueError("focal_gamma: a finite value >= 0")
        if gamma != 0.0 and head != "sigmoid":
            raise ValueError("focal_gamma is for head='sigmoid'")
        if class_weight is None:
            if eps == 0.0 and gamma == 0.0:
                return None
            cw = [1.0] * units
        else:
            cw = [float(v) for v in np.asarray(class_weight, np.float64).reshape(-1)]
            if len(cw) != units or not all(v > 0.0 and np.isfinite(v) for v in cw):
                raise ValueError(f"class_weight: None or {units} finite weights > 0 (one per unit)")
        spec = _ffi.LossSpec(eps, gamma)
        for u in range(16):
            spec.class_weight[u] = cw[u] if u < units else 1.0
        return spec

    def _choose_tiles(self, tiles: str) -> None:
        """Conv tiles: "pinned" = the committed MI355X table for this workload
        (jr/tiles_mi355x.json, tools/make_tile_tables.py) when there is one,
        else the planner heuristic -- both deterministic, so every run on
        every box sums in the same order; "autotune" (or autotune=True)
        times the candidates on this box (fastest, box-dependent order)."""
        if tiles not in ("pinned", "heuristic", "autotune"):
            raise ValueError("tiles: 'pinned', 'heuristic' or 'autotune'")
        self.tiles = "heuristic"
        self._clear_configs()           # libjr's per-geometry overrides are process-wide
        if tiles == "autotune":
            self.autotune()
            self.tiles = "autotune"
        elif tiles == "pinned":
            t = pinned_tile_table(self.conv_math, self.batch, self.g.height, self.g.width, self.train_mode)
            if t is not None and all(u.name in t["configs"] for u in self.cunits):
                self.set_tile_table(t)
                self.tiles = "pinned"
        self._own_tiles()

    # ------------------------------------------------------------------ memory
    def _alloc(self) -> None:
        g, B, at = self.g, self.batch, self.act_dtype
        self._alloc_forward(dgrad_rows=True)
        # per-layer views of a launch's raw output and statistics (tests/test_gpu_layerwise.py)
        self.raw, self.mean, self.invstd = {}, {}, {}
        for u in self.cunits:
            r = self.raw_unit[u.first.idx].view(B * u.ho * u.wo, u.cout)
            for n, co in zip(u.members, u.col_off):
                self.raw[n.idx] = r[:, co:co + n.cout]
        for n, om, oi in self.plan.bn_layers():
            self.mean[n.idx], self.invstd[n.idx] = self.stats[om:om + n.cout], self.stats[oi:oi + n.cout]
        self.argmax = {}
        for i, n in enumerate(g.nodes):
            if n.kind == "maxpool":
                self.argmax[i] = self._t(B * n.ho * n.wo * n.c, torch.uint8)
        feat_c = g.bufs[g.output_buf].c
        self.draw_stem2, self.bn_batch, self.drawb = None, [], []
        if self.train_mode:
            self.grads = self._t(self.nparam)
            self.accum = self._t(self.nparam)
            self.adam_v = self._t(self.nparam) if self.optimizer in ("adam", "rmsprop") else None
            if self.weight_ema is not None:
                # the averaged weights (internal layout, padding included) and jr_ema_state
                self.ema, self.ema_state = self._t(self.nparam), self._t(4)
            if self.dropout is not None:
                # the dropped features the head reads in a training step, and jr_dropout_state
                self.feat_drop, self.drop_state = self._t(B * feat_c), self._t(8)
                self._dropout_set(0)
            if self.accum_steps > 1:
                self.gacc = self._t(self.nparam)    # the open group's gradient sum, resource ("gacc",)
            if self.opt_ex:
                # the norm's per-block partials, jr_opt_hyper, jr_opt_step (zeroed: skipped_total
                # counts from here) and the decay ranges of the internal layout
                self.opt_partials = self._t(self.lib.jr_grad_sqnorm_workspace_size(self.nparam) // 8, torch.float64)
                self.opt_hyper, self.opt_step_dev = self._t(4), self._t(4)
                self.opt_ranges = decay_ranges(self.plan)
                self._opt_ranges_dev = self._table(_ffi.OptRange, [_ffi.OptRange(b, e) for b, e in self.opt_ranges])
                self._hyper_dev = None      # the scalars last enqueued for opt_hyper
                self._push_hyper(self.lr, 1.0)
        if self._data_grads:
            self.dacts = [self._t(B * b.h * b.w * b.c, at) if b.id != g.input_buf else None
                          for b in g.bufs]
            # per-lane scratch for the raw-output gradient of the launch in flight
            self.draw_lane = [self._t(max(B * u.ho * u.wo * u.cout for u in self.cunits), at)
                              for _ in range(self.nlanes)]
            # the stem's filter gradients run on lane 1 beside its single-lane
            # data-gradient chain: a second raw-gradient buffer for lane 0 (the
            # next stem layer's BN backward must not overwrite what that
            # filter gradient still reads)
            self.draw_stem2 = (self._t(max(B * u.ho * u.wo * u.cout for u in self.cunits), at)
                               if self.train_mode and self.nlanes > 1 and not self.x8p else None)
            self.draw = self.draw_lane[0]
            self.dfeat = self._t(B * feat_c)
            # the batched block-output BN backwards' raw gradients live in two
            # alternating sets of per-layer buffers
            self.bn_batch = (bn_batch_groups(g, self.plan, B, self._vw, self.fused_bufs)
                             if self.bn_batch_on and self.train_mode else [])
            slots = max((len(grp) for grp in self.bn_batch), default=0)
            self.drawb = [[self._t(max(B * grp[k].ho * grp[k].wo * grp[k].cout
                                       for grp in self.bn_batch if k < len(grp)), at) for k in range(slots)]
                          for _ in range(2 if slots else 0)]
        if self.input_grad:
            ib = g.bufs[g.input_buf]
            # the image gradient (fp32, 4 channels per pixel: c = 3 and a zero), the
            # unscaled input kept for scaled passes, the drivers' accumulator, the targets
            self.dinput = self._t(B * ib.h * ib.w * 4)
            self.x0 = self._t(B * ib.h * ib.w * self.in_stride, at)
            self.attr_acc = self._t(B * ib.h * ib.w * 4)
            self.ig_target = self._t(B, torch.int32)
        if self.dt == _ffi.JR_BF16 or self.x8p:
            self._alloc_bf16_filters(planes=3 if self.x8p else 1)
        if self.x8p:
            self._alloc_planes()
        ws = 0
        for u in self.cunits:
            d = self._conv_desc(u, B)
            ops = (_ffi.JR_CONV_FWD, _ffi.JR_CONV_BWD_DATA, _ffi.JR_CONV_BWD_FILTER)
            for op in (ops if self.train_mode else ops[:2] if self.input_grad else ops[:1]):
                ws = max(ws, self.lib.jr_conv2d_workspace_size(ctypes.byref(d), op, self.cdt))
            ws = max(ws, self.lib.jr_bn_workspace_size(B * u.ho * u.wo, u.cout))   # one backward per launch (or less)
        for grp in self.bn_batch:                        # one batched BN backward per block
            ws = max(ws, sum((self.lib.jr_bn_workspace_size(B * u.ho * u.wo, u.cout) + 255) // 256 * 256
                             for u in grp))
        for i in self.pool_fused:                      # the fused max-pool + BN backward's partials
            ws = max(ws, self.lib.jr_bn_relu_bwd_maxpool_workspace_size(ctypes.byref(self._pool_desc(g.nodes[i], B))))
        self._alloc_ws(ws)
        # the stem filter gradients' own workspace on lane 1
        self.ws_stem = self._t((self.ws_bytes + 15) // 4 + 4) if self.draw_stem2 is not None else None
        # launch -> its group of batched BN backwards
        self._in_batch = {u.first.idx: grp for grp in self.bn_batch for u in grp}

    def _alloc_planes(self) -> None:
        """JR_F32_X8P operand planes (jr.h): the exact bf16 h/m/l split of
        every conv input buffer (written once per step by jr_split_x8p when
        the buffer is complete, read by the forward and the filter-gradient
        GEMMs) and of each lane's raw-output gradient scratch (dgrad and
        wgrad operand).  Channel radices are padded to 8 (the image: 3 -> 8)."""
        g, B = self.g, self.batch
        bf = torch.bfloat16
        self.plane_c = {}
        self.aplanes = {}
        for u in self.cunits:
            b = g.bufs[u.x]
            if u.x in self.aplanes:
                continue
            cp = (b.c + 7) // 8 * 8
            self.plane_c[u.x] = cp
            self.aplanes[u.x] = self._t(3 * B * b.h * b.w * cp, bf)
        if self.train_mode:
            n = max(B * u.ho * u.wo * u.cout for u in self.cunits)
            self.drawp_lane = [self._t(3 * n, bf) for _ in range(self.nlanes)]

    def _wprep_call(self, stream=None):
        fn = self.lib.jr_conv_weights_x8p_multi if self.wplanes == 3 else self.lib.jr_conv_weights_bf16_multi
        return (fn,
                (self.wprep_table.data_ptr(), self.wprep_layers, self.wprep_tiles, self.params.data_ptr(),
                 self.w_hwio.data_ptr(), self.w_t.data_ptr(), stream or self._s), "wprep_bf16")

    def _wf(self, u: ConvUnit) -> int:
        """Filter operand of conv fwd: fp32 HWIO master block, or its bf16 W^T copy (planes)."""
        if self.dt == _ffi.JR_BF16 or self.x8p:
            return self.w_t.data_ptr() + 2 * self.wb_t_off[u.first.idx]
        return self.params.data_ptr() + 4 * u.koff

    def _wd(self, u: ConvUnit) -> int:
        """Filter operand of conv bwd_data: fp32 HWIO master block, or its bf16 copy (planes)."""
        if self.dt == _ffi.JR_BF16 or self.x8p:
            return self.w_hwio.data_ptr() + 2 * self.wb_hwio_off[u.first.idx]
        return self.params.data_ptr() + 4 * u.koff

    def autotune(self, progress: Optional[Callable[[str], None]] = None) -> None:
        """jr_conv2d_autotune every conv launch of the planned batch (cudnnFind
        style: times each tile configuration on this engine's own buffers and
        caches the fastest in libjr).  Runs before any data is loaded: it
        overwrites raw / gradient buffers."""
        L, B = self.lib, self.batch
        self._drop_calls()
        ws, wsb = ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_size_t(self.ws_bytes)
        s = self._s
        if self.dt == _ffi.JR_BF16 or self.x8p:
            fn, args, name = self._wprep_call()
            _ffi.check(name, fn(*args))
        for u in self.cunits:
            if progress is not None:
                progress(u.name)
            d = self._conv_desc(u, B)
            x = (self.aplanes[u.x] if self.x8p else self.acts[u.x]).data_ptr()
            draw = (self.drawp_lane[0] if self.x8p else self.draw).data_ptr() if self._data_grads else 0
            raw = self.raw_unit[u.first.idx].data_ptr()
            _ffi.check("autotune fwd", L.jr_conv2d_autotune(ctypes.byref(d), _ffi.JR_CONV_FWD, self.cdt, x,
                                                             self._wf(u), raw, ws, wsb, s))
            if self.train_mode:
                _ffi.check("autotune wgrad", L.jr_conv2d_autotune(
                    ctypes.byref(d), _ffi.JR_CONV_BWD_FILTER, self.cdt, x, draw,
                    self.grads.data_ptr() + 4 * u.koff, ws, wsb, s))
            if self._data_grads and u.x != self.g.input_buf:
                _ffi.check("autotune dgrad", L.jr_conv2d_autotune(
                    ctypes.byref(d), _ffi.JR_CONV_BWD_DATA, self.cdt, draw, self._wd(u),
                    self.dacts[u.x].data_ptr(), ws, wsb, s))
        self.synchronize()
        if self.train_mode:
            with torch.cuda.stream(self.stream):
                self.grads.zero_()
        self._own_tiles()

    def conv_configs(self) -> dict:
        """{conv launch name: (fwd cfg, wgrad cfg, [dgrad cfg per phase])} in use."""
        out = {}
        for u in self.cunits:
            d = self._conv_desc(u, self.batch)
            f = self.lib.jr_conv2d_get_config(ctypes.byref(d), _ffi.JR_CONV_FWD, self.cdt, 0)
            wg = self.lib.jr_conv2d_get_config(ctypes.byref(d), _ffi.JR_CONV_BWD_FILTER, self.cdt, 0)
            dg = [self.lib.jr_conv2d_get_config(ctypes.byref(d), _ffi.JR_CONV_BWD_DATA, self.cdt, p)
                  for p in range(u.stride * u.stride)]
            out[u.name] = (f, wg, dg)
        return out

    def tile_table(self) -> dict:
        """The conv tile configuration of every launch, as saved in checkpoint
        meta (jr.checkpoint) and accepted back by set_tile_table: with the
        same table two runs sum in the same order (bitwise-equal steps on any
        MI355X).  Keyed by conv math, batch and resolution."""
        return {"conv_math": self.conv_math, "batch": self.batch, "height": self.g.height,
                "width": self.g.width, "configs": {k: [f, wg, list(dg)] for k, (f, wg, dg) in
                                                   self.conv_configs().items()}}

    def _drop_calls(self) -> None:
        """Forget the bound call lists (tile plans or flush points changed);
        their buffers stay alive for graphs captured from them."""
        self._retired.extend(self._calls.values())
        self._calls.clear()

    def set_flush_points(self, points) -> None:
        """Flat-gradient offsets at which a consumer (jr.dist.BucketAllReduce)
        needs every gradient at offsets >= the point final: the deferred
        filter-gradient slabs are reduced before the param_ready hook of the
        first launch whose offset is <= the point."""
        self._flush_points = sorted((int(p) for p in points), reverse=True)
        self._drop_calls()

    def set_tile_table(self, table: dict) -> None:
        """Pin every conv launch to the configs of `table` (tile_table())."""
        self._drop_calls()
        if (table.get("conv_math"), table.get("batch"), table.get("height"), table.get("width")) != \
                (self.conv_math, self.batch, self.g.height, self.g.width):
            raise ValueError("tile table is for another conv math / batch / resolution")
        self._apply_configs(table["configs"])
        self._own_tiles()

    def _own_tiles(self) -> None:
        """Record the configs this engine's call lists are bound to (libjr's
        overrides are process-wide: another engine or caller of the same
        geometry may change them; _ensure_tiles puts these back)."""
        self._tile_cfgs = self.tile_table()["configs"]
        self._tile_gen = self.lib.jr_conv2d_config_generation()

    def _ensure_tiles(self) -> None:
        """Re-apply this engine's configs if libjr's overrides changed since it
        applied them (the deferred filter-gradient segments bind
        the split count of the plan at call-list build time)."""
        if self.lib.jr_conv2d_config_generation() != self._tile_gen:
            self._apply_configs(self._tile_cfgs)     # the same plans the call lists were built with
            self._tile_gen = self.lib.jr_conv2d_config_generation()

    def _apply_configs(self, cfgs: dict) -> None:
        for u in self.cunits:
            f, wg, dg = cfgs[u.name]
            d = self._conv_desc(u, self.batch)
            _ffi.check("set_config", self.lib.jr_conv2d_set_config(ctypes.byref(d), _ffi.JR_CONV_FWD, self.cdt, 0, f))
            if self.train_mode:
                _ffi.check("set_config", self.lib.jr_conv2d_set_config(ctypes.byref(d), _ffi.JR_CONV_BWD_FILTER,
                                                                       self.cdt, 0, wg))
            if self._data_grads and u.x != self.g.input_buf:
                for p, c in enumerate(dg):
                    _ffi.check("set_config", self.lib.jr_conv2d_set_config(ctypes.byref(d), _ffi.JR_CONV_BWD_DATA,
                                                                           self.cdt, p, c))

    def clear_tile_table(self) -> None:
        """Back to the deterministic planner heuristic for every conv launch
        (drops autotuned or pinned configs of this engine's geometries)."""
        self._clear_configs()
        self._own_tiles()

    def _clear_configs(self) -> None:
        self._drop_calls()
        for u in self.cunits:
            d = self._conv_desc(u, self.batch)
            ops = [(_ffi.JR_CONV_FWD, 0)]
            if self.train_mode:
                ops.append((_ffi.JR_CONV_BWD_FILTER, 0))
            if self._data_grads and u.x != self.g.input_buf:
                ops += [(_ffi.JR_CONV_BWD_DATA, p) for p in range(u.stride * u.stride)]
            for op, p in ops:
                _ffi.check("set_config", self.lib.jr_conv2d_set_config(ctypes.byref(d), op, self.cdt, p, -1))

    # ------------------------------------------------------------ parameters
    def load_params(self, flat: np.ndarray) -> None:
        """Keras-layout flat parameters (jr.init.param_layout order)."""
        host = torch.from_numpy(self.plan.to_internal(self.g, flat))
        with torch.cuda.stream(self.stream):     # in order with the steps that read and update them
            self.params.copy_(host.to(self.device))
            if self.train_mode:
                self.accum.zero_()
                self.grads.zero_()
                # optimizer state restarts with the parameters: Adam's v slot and
                # its fp32 beta powers (TF initialises beta1_power / beta2_power to
                # beta1 / beta2 with the slots)
                if self.adam_v is not None:
                    self.adam_v.fill_(1.0 if self.optimizer == "rmsprop" else 0.0)    # (RMSProp's ms starts at ones)
                if self.ema is not None:
                    # the average restarts at the new parameters, its counter at zero
                    self.ema.copy_(self.params)
                    self._ema_set(0)
        # (and a caller's torch work on these tensors, on its own stream, sees the new values)
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        if self.train_mode:
            self.adam_t = 0
            self.adam_b1p, self.adam_b2p = np.float32(self.adam_b1), np.float32(self.adam_b2)
            self._pending = 0       # an open group of micro-batches is discarded (its sum is overwritten by the next)

    def _ema_set(self, updates: int) -> None:
        _ffi.check("jr_ema_set", self.lib.jr_ema_set(self.ema_state.data_ptr(), self.weight_ema,
                                                     int(self.weight_ema_warm), int(updates), self._s))

    def _dropout_set(self, step: int) -> None:
        _ffi.check("jr_dropout_set", self.lib.jr_dropout_set(self.drop_state.data_ptr(), *self.dropout_key, self.dropout,
                                                             int(step) & 0xFFFFFFFF, self._s))

    def dropout_steps(self) -> int:
        """Training steps enqueued so far, modulo 2^32: the device counter the next mask is drawn with."""
        if self.drop_state is None:
            raise ValueError("no dropout: Engine(dropout=rate) keeps its state")
        self.synchronize()
        return int(self.drop_state.cpu()[2:3].view(torch.int32)[0]) & 0xFFFFFFFF

    def _need_ema(self) -> None:
        if self.ema is None:
            raise ValueError("no averaged weights: Engine(weight_ema=decay) keeps them")

    def ema_numpy(self) -> np.ndarray:
        """The moving average of the weights in the Keras layout."""
        self._need_ema()
        torch.cuda.synchronize(self.device)
        return self.plan.to_keras(self.g, self.ema.cpu().numpy())

    def load_ema(self, flat: np.ndarray, updates: int = 0) -> None:
        """A saved average (Keras layout, ema_numpy / jr.checkpoint.load_ema)
        and the number of updates it has seen."""
        self._need_ema()
        if self._averaged:
            raise RuntimeError("load_ema inside averaged_weights()")
        host = torch.from_numpy(self.plan.to_internal(self.g, flat))
        with torch.cuda.stream(self.stream):
            self.ema.copy_(host.to(self.device))
            self._ema_set(updates)
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def ema_updates(self) -> int:
        """The device's count of averaged steps (skipped steps are not counted)."""
        self._need_ema()
        self.synchronize()
        return int(self.ema_state.cpu()[2:3].view(torch.int32)[0])

    def _swap_ema(self) -> None:
        with torch.cuda.stream(self.stream):
            tmp = self.params.clone()
            self.params.copy_(self.ema)
            self.ema.copy_(tmp)

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside: `params` holds the averaged weights and `ema` the trained
        ones (the CONTENTS are swapped on the engine's stream -- the call
        lists hold addresses -- and swapped back on exit); a forward runs on
        the averaged weights, its own prep rebuilding the filter copies and
        scales.  Does not nest; no update, training step or replay inside."""
        self._need_ema()
        if self._averaged:
            raise RuntimeError("averaged_weights() does not nest")
        self._swap_ema()
        self._averaged = True
        try:
            yield self
        finally:
            self._averaged = False
            self._swap_ema()

    def _no_update_on_average(self, what: str) -> None:
        if self._averaged:
            raise RuntimeError(f"{what} inside averaged_weights(): params hold the averaged weights")

    def params_numpy(self) -> np.ndarray:
        """Parameters in the Keras layout (checkpoints, the oracle)."""
        torch.cuda.synchronize(self.device)
        return self.plan.to_keras(self.g, self.params.cpu().numpy())

    def bn_moving_numpy(self) -> dict:
        """The moving BN statistics by Keras name, per conv2d_bn layer
        (batch_normalization_k/moving_mean, .../moving_variance)."""
        return self._bn_moving_get()[0]

    def load_bn_moving(self, stats: dict, updates: int = 0) -> None:
        """Moving BN statistics by Keras name (bn_moving_numpy, jr.checkpoint);
        non-finite values and negative variances are refused."""
        self._bn_moving_set([stats])
        self.updates = int(updates)

    def grads_numpy(self) -> np.ndarray:
        """Gradients of the last backward in the Keras layout."""
        torch.cuda.synchronize(self.device)
        return self.plan.to_keras(self.g, self.grads.cpu().numpy())

    def _gp(self, name: str) -> int:
        return self.grads.data_ptr() + 4 * self.plan.poff[name]

    # ------------------------------------------------------------ descriptors
    def _conv_desc(self, u: ConvUnit, B: int) -> _ffi.ConvDesc:
        d = super()._conv_desc(u, B)
        if self.x6h:
            d.dy_absmax = self._dmax(u)
        return d

    def _pool_desc(self, n: PoolNode, B: int) -> _ffi.PoolDesc:
        yb = self.g.bufs[n.y.buf]
        return _ffi.PoolDesc(B, n.h, n.w, n.c, n.ho, n.wo, 0, n.c, n.y.c_off, yb.c)

    # ------------------------------------------------------------- call lists
    def _bn_groups(self, u: ConvUnit):
        """BN backward launch sets of a conv launch: all members at once while
        the launch's channels fit one 256-thread row (jr_bn: <= 256 vectors of
        4 fp32 / 8 bf16), else one set per member.  [(member, col_off), ...]"""
        groups = [list(zip(u.members, u.col_off))]
        if not _ffi.bn_one_launch(self.dt, u.cout):
            groups = [[mc] for mc in groups[0]]
        return groups

    def _build_calls(self, B: int, nl: Optional[int] = None, frozen: bool = False, training: bool = False,
                     accum: Optional[str] = None):
        """Pre-bound Calls (jr.lanes) for forward, backward, update on nl
        lanes (default self.nlanes), with their cross-lane waits:
        (fwd, bwd, opt, keep, None).  frozen: the forward alone, every BN
        apply and fused stem pool reading self.frozen (its own key).
        training: the lists of a training step (train_step, capture); they are
        the default lists unless dropout is on, which adds jr_dropout_fwd between
        the pool and the head, jr_dropout_bwd behind the head's backward and
        jr_dropout_advance at the end of the update.
        accum (accum_steps > 1 only): where the micro-batch sits in its group --
        "open" / "inside": the update phase is jr_grad_accumulate(acc <- g, first
        = 1 / acc <- acc + g) and what runs once per batch (the BN moving
        averages, the dropout counter); "close": jr_grad_accumulate(g <- g +
        acc), then the default update phase.  None: the default lists (a group
        closed under data parallelism, where jr.dist folds per bucket)."""
        if accum is not None and (self.gacc is None or frozen or accum not in ("open", "inside", "close")):
            raise ValueError("accum: 'open', 'inside' or 'close', with accum_steps > 1")
        self._ensure_tiles()
        nl = self.nlanes if nl is None else max(1, min(int(nl), self.nlanes))
        training = bool(training) and self.dropout is not None and not frozen
        key = (B, nl, "frozen") if frozen else (B, nl, "training") if training else (B, nl)
        if accum is not None:
            key += ("accum", accum)
        if key in self._calls:
            return self._calls[key]
        if accum == "inside":
            # the opening lists with first = 0: the same calls, schedule and buffers
            fwd, bwd, opt, keep, _ = self._build_calls(B, nl, training=training, accum="open")
            a = opt[0].args
            opt = [dataclasses.replace(opt[0], args=a[:3] + (0,) + a[4:])] + list(opt[1:])
            self._calls[key] = (fwd, bwd, opt, keep, None)
            return self._calls[key]
        if B > self.batch or B <= 0:
            raise ValueError(f"batch {B} outside 1..{self.batch}")
        g, unit_of = self.g, self.plan.unit_of
        b = Build(B, self.lanes, nl, self.ws_lane, self.ws_bytes, node_lanes(g, self.plan, nl), self._flush_points)
        if frozen:
            b.stats_shift = self.frozen.data_ptr() - self.stats.data_ptr()
            b.guard = self._frozen_guard()
        b.training = training
        b.accum = accum
        self._fwd_prep(b)
        for i, n in enumerate(g.nodes):
            if n.kind != "conv":
                self._fwd_pool(b, i, n)
            elif unit_of[n.idx].first is n:     # a group is emitted with its first member
                self._fwd_conv(b, b.lane_of[i], unit_of[n.idx])
        self._fwd_head(b)
        if self.train_mode and not frozen:
            if self.defer_wgrad:
                self._bwd_slab_arena(b)
            self._bwd_head(b)
            for i in range(len(g.nodes) - 1, -1, -1):
                n = g.nodes[i]
                if n.kind != "conv":
                    self._bwd_pool(b, i, n)
                elif unit_of[n.idx].first is n:     # a group runs at its first member: every member's dy is final then
                    self._bwd_conv(b, i, unit_of[n.idx])
            self._bwd_flush(b)
            self._opt_update(b)
        schedule(b.seq)
        self._calls[key] = (b.fwd, b.bwd, b.opt, b.keep, None)
        return self._calls[key]

    # resources and operands of the calls: activations, their gradients, and
    # what a conv reads -- x8p: the split planes of its input buffer, written
    # once (by the lane of its first consumer) when the buffer is complete;
    # its filters (w16: their bf16 copies); x6h: their magnitude words too
    def _D(self, bid: int) -> int:
        return self.dacts[bid].data_ptr()

    def _d_all(self, bid: int) -> list:
        return [("d", bid, o) for o in self.slices[bid]]

    def _AX(self, bid: int) -> int:
        return (self.aplanes[bid] if self.x8p else self.acts[bid]).data_ptr()

    def _ax_reads(self, bid: int) -> list:
        return [("ap", bid)] if self.x8p else self._a_all(bid)

    def _w_reads(self) -> list:
        return [("w16",) if (self.dt == _ffi.JR_BF16 or self.x8p) else ("p",)] + ([("wmax",)] if self.x6h else [])

    def _dmax_reads(self, u: ConvUnit) -> list:
        """x6h: the data- and filter-gradient GEMMs scale dy by the launch's magnitude row."""
        return [("dmax", u.first.idx)] if self.x6h else []

    def _dbeta(self, m) -> int:
        return self._gp(f"batch_normalization_{m.idx + 1}/beta")

    def _bn_segs(self, members) -> list:
        """Per member: its upstream gradient slice, beta and dbeta."""
        return [_ffi.BnSeg(self._D(m.y.buf), m.y.c_off, self.g.bufs[m.y.buf].c, m.cout, self._beta(m), self._dbeta(m))
                for m in members]

    # ---- forward
    def _fwd_prep(self, b: Build) -> None:
        if self.dt == _ffi.JR_BF16 or self.x8p:
            b.add(b.fwd, *self._wprep_call(b.S[0]), 0, [("p",)], [("w16",)])
        if self.x6h:
            # the filters' magnitudes (and the beta guard), and every
            # gradient row zeroed, before the first conv of the step
            b.add(b.fwd, self.lib.jr_absmax_prep,
                  (self.params.data_ptr(), self.absmax_table.data_ptr(), self.absmax_nseg, self.absmax.data_ptr(),
                   self.absmax.numel(), b.S[0]), "absmax_prep", 0,
                  [("p",)], [("wmax",)] + [("dmax", u.first.idx) for u in self.cunits], nbytes=4 * self.nparam)

    def _fwd_conv(self, b: Build, ln: int, u: ConvUnit) -> None:
        """A conv launch with the BN batch statistics of its raw output, and
        its members' BN + ReLU."""
        L, g, dt, B, s, ws = self.lib, self.g, self.dt, b.B, b.S[ln], b.WS[ln]
        d = self._conv_desc(u, B)
        b.keep.append(d)
        M, uid = B * u.ho * u.wo, u.first.idx
        raw, mean, invstd = self.raw_unit[uid].data_ptr(), self._mean(u), self._invstd(u)
        if self.x8p and u.x not in b.split_done:
            b.split_done.add(u.x)
            xb, cp = g.bufs[u.x], self.plane_c[u.x]
            rows = B * xb.h * xb.w
            b.add(b.fwd, L.jr_split_x8p, (self._A(u.x), rows, xb.c, 0, self.in_stride if u.x == g.input_buf else xb.c,
                                          self._AX(u.x), cp, 0, cp, self.batch * xb.h * xb.w * cp, s),
                  "split_x8p", ln, self._a_all(u.x), [("ap", u.x)], nbytes=rows * (4 * xb.c + 6 * cp))
        reads = self._ax_reads(u.x) + self._w_reads()
        unfused = not any(m.y.buf in self.fused_bufs for m in u.members)
        lay = None
        if self.fold_stats and unfused:
            lay = _ffi.BnPartials()
            _ffi.check("jr_conv2d_bn_partials_layout",
                       L.jr_conv2d_bn_partials_layout(ctypes.byref(d), self.cdt, ctypes.byref(lay)))
            if not lay.single_stage or lay.P > self.fold_max_p:
                lay = None
        if lay is not None:
            # conv + the statistics partials; each member's BN apply
            # combines its channels' partials (and stores mean / invstd)
            b.add(b.fwd, L.jr_conv2d_fwd_bn_partials,
                  (ctypes.byref(d), self.cdt, self._AX(u.x), self._wf(u), raw, ws, b.wsb, s),
                  "conv_fwd", ln, reads, [("r", uid), ("ws", ln)])
            part = ws.value + lay.ws_offset
            for m, co in zip(u.members, u.col_off):
                b.add(b.fwd, L.jr_bn_relu_apply_stats,
                      (dt, raw, co, u.cout, M, m.cout, part, lay.P, lay.R, u.cout, co, BN_EPS,
                       mean + 4 * co, invstd + 4 * co, self._beta(m), self._A(m.y.buf),
                       m.y.c_off, g.bufs[m.y.buf].c, s),
                      "bn_relu", ln, [("r", uid), ("ws", ln), ("p",)], [("a", m.y.buf, m.y.c_off), ("r", uid)],
                      nbytes=2 * M * m.cout * self.esz)
            return
        b.add(b.fwd, L.jr_conv2d_fwd_bn_stats,
              (ctypes.byref(d), self.cdt, self._AX(u.x), self._wf(u), raw, BN_EPS, mean, invstd, ws, b.wsb, s),
              "conv_fwd", ln, reads, [("r", uid), ("ws", ln)])
        if self.apply_multi and len(u.members) > 1 and _ffi.bn_one_launch(self.dt, u.cout) and unfused:
            # every member's BN + ReLU in one launch (jr_bn_relu_apply_multi)
            segs = (_ffi.BnApplySeg * len(u.members))(*[
                _ffi.BnApplySeg(self._A(m.y.buf), m.y.c_off, g.bufs[m.y.buf].c, m.cout, self._beta(m))
                for m in u.members])
            b.keep.append(segs)
            fn, lim = ((L.jr_bn_relu_apply_multi, ()) if b.guard is None
                       else (L.jr_bn_relu_apply_multi_guard, (b.guard,)))
            b.add(b.fwd, fn,
                  (dt, len(u.members), ctypes.byref(segs), raw, 0, u.cout, M, u.cout, mean + b.stats_shift,
                   invstd + b.stats_shift) + lim + (s,),
                  "bn_relu", ln, [("r", uid), ("p",)] + self._frozen_reads(b),
                  [("a", m.y.buf, m.y.c_off) for m in u.members], nbytes=2 * M * u.cout * self.esz)
            return
        for m, co in zip(u.members, u.col_off):
            if m.y.buf in self.fused_bufs:
                continue        # applied inside its max-pool
            fn, lim = (L.jr_bn_relu_apply, ()) if b.guard is None else (L.jr_bn_relu_apply_guard, (b.guard,))
            b.add(b.fwd, fn,
                  (dt, raw, co, u.cout, M, m.cout, mean + 4 * co + b.stats_shift,
                   invstd + 4 * co + b.stats_shift, self._beta(m), self._A(m.y.buf), m.y.c_off,
                   g.bufs[m.y.buf].c) + lim + (s,),
                  "bn_relu", ln, [("r", uid), ("p",)] + self._frozen_reads(b), [("a", m.y.buf, m.y.c_off)],
                  nbytes=2 * M * m.cout * self.esz)

    def _fwd_pool(self, b: Build, i: int, n: PoolNode) -> None:
        L, dt, B, ln = self.lib, self.dt, b.B, b.lane_of[i]
        s, d = b.S[ln], self._pool_desc(n, B)
        b.keep.append(d)
        out = [("a", n.y.buf, n.y.c_off)]
        if i in self.pool_fused:
            pn = self._pool_producer(n)
            d.x_c_off, d.x_c_stride = 0, pn.cout                       # its raw output
            pu = self.plan.unit_of[pn.idx]          # (a launch of its own: fusable_pools)
            puid = pu.first.idx
            fn, lim = ((L.jr_bn_relu_maxpool3x3s2_fwd, ()) if b.guard is None
                       else (L.jr_bn_relu_maxpool3x3s2_fwd_guard, (b.guard,)))
            b.add(b.fwd, fn,
                  (ctypes.byref(d), dt, self.raw_unit[puid].data_ptr(), self._mean(pu) + b.stats_shift,
                   self._invstd(pu) + b.stats_shift, self._beta(pn), self._A(n.y.buf),
                   self.argmax[i].data_ptr()) + lim + (s,),
                  "bn_relu_maxpool_fwd", ln, [("r", puid), ("p",)] + self._frozen_reads(b), out + [("am", i)],
                  nbytes=B * n.c * (n.h * n.w * self.esz + n.ho * n.wo * (self.esz + 1)))
        elif n.kind == "maxpool":
            b.add(b.fwd, L.jr_maxpool3x3s2_fwd,
                  (ctypes.byref(d), dt, self._A(n.x), self._A(n.y.buf), self.argmax[i].data_ptr(), s),
                  "maxpool_fwd", ln, self._a_all(n.x), out + [("am", i)],
                  nbytes=B * n.c * (n.h * n.w * self.esz + n.ho * n.wo * (self.esz + 1)))
        else:
            b.add(b.fwd, L.jr_avgpool3x3s1_fwd, (ctypes.byref(d), dt, self._A(n.x), self._A(n.y.buf), s),
                  "avgpool_fwd", ln, self._a_all(n.x), out, nbytes=B * n.c * (n.h * n.w + n.ho * n.wo) * self.esz)

    def _fwd_head(self, b: Build) -> None:
        g, s0 = self.g, b.S[0]
        ob = g.bufs[g.output_buf]
        b.add(b.fwd, self.lib.jr_gap_fwd,
              (self.dt, self._A(g.output_buf), b.B, ob.h * ob.w, ob.c, self.feat.data_ptr(), s0),
              "gap_fwd", 0, self._a_all(g.output_buf), [("feat",)])
        feat, fkey = self.feat.data_ptr(), ("feat",)
        if b.training:
            # a training step's head reads the dropped features (a new mask per step: jr.h)
            b.add(b.fwd, self.lib.jr_dropout_fwd, (feat, self.feat_drop.data_ptr(), b.B * ob.c,
                                                   self.drop_state.data_ptr(), s0),
                  "dropout_fwd", 0, [("feat",), ("drop",)], [("feat_drop",)], nbytes=8 * b.B * ob.c)
            feat, fkey = self.feat_drop.data_ptr(), ("feat_drop",)
        args = (feat, self._p("dense/kernel"), self._p("dense/bias"), self.labels.data_ptr(), b.B, ob.c, self.units,
                self.logits.data_ptr(), self.probs.data_ptr(), self.loss.data_ptr(), s0)
        if self.loss_spec is not None:
            b.add(b.fwd, self.lib.jr_head_fwd_ex, (self.head_mode, ctypes.byref(self.loss_spec)) + args,
                  "head_fwd_ex", 0, [fkey, ("p",), ("lab",)], [("head",)])
        else:
            b.add(b.fwd, self.lib.jr_head_fwd, (self.head_mode,) + args,
                  "head_fwd", 0, [fkey, ("p",), ("lab",)], [("head",)])

    # ---- backward
    def _bwd_slab_arena(self, b: Build) -> None:
        """Deferred filter gradients: per-layer slab regions of one arena."""
        off = 0
        for u in self.cunits:
            d = self._conv_desc(u, b.B)
            b.keep.append(d)
            sg = _ffi.WgradSeg()
            _ffi.check("jr_conv2d_wgrad_seg", self.lib.jr_conv2d_wgrad_seg(ctypes.byref(d), self.cdt, ctypes.byref(sg)))
            if sg.splits > 1:
                nb = 4 * sg.splits * sg.m * sg.n
                sg.dw = self.grads.data_ptr() + 4 * u.koff
                b.defer[u.first.idx] = (sg, off, nb)
                off += (nb + 255) // 256 * 256
        arena = self._t(off // 4 + 64)
        b.keep.append(arena)
        for sg, o, _ in b.defer.values():
            sg.slabs = arena.data_ptr() + o
        self.slab_bytes = off

    def _bwd_flush(self, b: Build) -> None:
        """One jr_wgrad_reduce over every pending layer (lane 0)."""
        if not b.pending:
            return
        arr = (_ffi.WgradSeg * len(b.pending))()
        blocks = 0
        for k, (sg, _) in enumerate(b.pending):
            arr[k] = sg
            arr[k].block0 = blocks
            blocks += sg.blocks
        table = self._dev_bytes(bytes(arr))
        b.keep.append(table)
        nbytes = sum(4 * sg.m * sg.n * (sg.splits + 1) for sg, _ in b.pending)
        b.add(b.bwd, self.lib.jr_wgrad_reduce, (table.data_ptr(), len(b.pending), blocks, b.S[0]), "wgrad_reduce", 0,
              [("slab", uid) for _, uid in b.pending], [("g", uid) for _, uid in b.pending], nbytes=nbytes)
        b.pending.clear()

    def _bwd_head(self, b: Build) -> None:
        g, s0 = self.g, b.S[0]
        ob = g.bufs[g.output_buf]
        drop = b.training
        feat, fkey = (self.feat_drop.data_ptr(), ("feat_drop",)) if drop else (self.feat.data_ptr(), ("feat",))
        args = (feat, self._p("dense/kernel"), self.probs.data_ptr(), self.labels.data_ptr(), b.B, ob.c, self.units,
                self.dfeat.data_ptr(), self._gp("dense/kernel"), self._gp("dense/bias"), s0)
        if self.loss_spec is not None:
            b.add(b.bwd, self.lib.jr_head_bwd_ex,
                  (self.head_mode, ctypes.byref(self.loss_spec), self.logits.data_ptr()) + args,
                  "head_bwd_ex", 0, [fkey, ("p",), ("head",), ("lab",)], [("dfeat",), ("g", "dense")])
        else:
            b.add(b.bwd, self.lib.jr_head_bwd, (self.head_mode,) + args,
                  "head_bwd", 0, [fkey, ("p",), ("head",), ("lab",)], [("dfeat",), ("g", "dense")])
        if drop:
            # the forward's mask again, recomputed from the state (the counter advances after the update)
            b.add(b.bwd, self.lib.jr_dropout_bwd, (self.dfeat.data_ptr(), b.B * ob.c, self.drop_state.data_ptr(), s0),
                  "dropout_bwd", 0, [("drop",)], [("dfeat",)], nbytes=8 * b.B * ob.c)
        b.add(b.bwd, self.lib.jr_gap_bwd,
              (self.dt, self.dfeat.data_ptr(), b.B, ob.h * ob.w, ob.c, self._D(g.output_buf), s0),
              "gap_bwd", 0, [("dfeat",)], self._d_all(g.output_buf))

    def _bwd_conv(self, b: Build, i: int, u: ConvUnit) -> None:
        """A conv launch's backward: the BN backward of its members into the
        raw-output gradient, the data and the filter gradient, and the
        param_ready hook (with a flush of the deferred filter gradients where
        a flush point falls)."""
        ln, uid = b.lane_of[i], u.first.idx
        acc = 1 if u.x in b.written else 0
        d = self._conv_desc(u, b.B)
        b.keep.append(d)
        draw, dkey, wl = self.draw_lane[ln].data_ptr(), ("draw", ln), ln
        if (len(b.S) > 1 and self.draw_stem2 is not None and self.stem_wgrad_lane
                and i < self._stem_end and ln == 0):    # the stem: filter gradient on lane 1
            if b.sbuf:
                draw, dkey = self.draw_stem2.data_ptr(), ("draw2", 0)
            b.sbuf ^= 1
            wl = 1
        if uid in self._in_batch and uid not in b.batch_draw:
            self._bwd_bn_batch(b, ln, self._in_batch[uid])
        pool_i = next((j for j, buf in self.pool_bwd.items() if buf == u.first.y.buf), None)
        if uid in b.batch_draw:
            draw, dkey = b.batch_draw[uid]
        if pool_i is not None:
            self._bwd_bn_pool(b, ln, u, pool_i, draw, dkey)
        elif uid not in b.batch_draw:
            self._bwd_bn_groups(b, ln, u, draw, dkey)
        if self.x8p:             # the raw-output gradient as split planes (dgrad and wgrad operand)
            M, drawp = b.B * u.ho * u.wo, self.drawp_lane[ln].data_ptr()
            b.add(b.bwd, self.lib.jr_split_x8p,
                  (draw, M, u.cout, 0, u.cout, drawp, u.cout, 0, u.cout, M * u.cout, b.S[ln]),
                  "split_x8p", ln, [("draw", ln)], [("drawp", ln)], nbytes=10 * M * u.cout)
            draw, dkey = drawp, ("drawp", ln)
        if self.dgrad_first:
            self._bwd_dgrad(b, ln, u, d, draw, dkey, acc)
        self._bwd_wgrad(b, ln, wl, u, d, draw, dkey)
        if not self.dgrad_first:
            self._bwd_dgrad(b, ln, u, d, draw, dkey, acc)
        if b.flush_at and b.flush_at[0] >= u.koff:      # a flush point falls here
            while b.flush_at and b.flush_at[0] >= u.koff:
                b.flush_at.pop(0)
            self._bwd_flush(b)
        b.bwd.append(Call("param_ready", u.koff, "hook", 0))

    def _bwd_bn_batch(self, b: Build, ln: int, grp) -> None:
        """The batched BN backward of a block's launches: issued where the
        group's first launch comes up (its upstream gradients are final
        there), on that launch's lane, into the raw-gradient set b.bset."""
        B = b.B
        layers = (_ffi.BnBwdLayer * len(grp))()
        reads, writes = [("r", v.first.idx) for v in grp] + [("p",)], [("ws", ln)]
        for k, v in enumerate(grp):
            vid = v.first.idx
            ptr = self.drawb[b.bset][k].data_ptr()
            b.batch_draw[vid] = (ptr, ("drawb", b.bset, k))
            segs = self._bn_segs(v.members)
            layers[k].nseg = len(segs)
            for j, sgm in enumerate(segs):
                layers[k].segs[j] = sgm
            layers[k].x = self.raw_unit[vid].data_ptr()
            layers[k].x_c_off, layers[k].x_c_stride = 0, v.cout
            layers[k].m, layers[k].c = B * v.ho * v.wo, v.cout
            layers[k].mean, layers[k].invstd = self._mean(v), self._invstd(v)
            layers[k].dx = ptr
            reads += [("d", m.y.buf, m.y.c_off) for m in v.members]
            writes += [("drawb", b.bset, k), ("g", vid)]
        b.keep.append(layers)
        b.add(b.bwd, self.lib.jr_bn_relu_bwd_batch, (self.dt, len(grp), ctypes.byref(layers), b.WS[ln], b.wsb, b.S[ln]),
              "bn_relu_bwd", ln, reads, writes, nbytes=sum(3 * B * v.ho * v.wo * v.cout * self.esz for v in grp))
        b.bset ^= 1

    def _bwd_bn_pool(self, b: Build, ln: int, u: ConvUnit, pool_i: int, draw: int, dkey) -> None:
        """The max-pool backward adds the BN reduce's sums (a fused stem pool)."""
        uid, pn, m0 = u.first.idx, self.g.nodes[pool_i], u.first
        pd = self._pool_desc(pn, b.B)
        b.keep.append(pd)
        args = (self.dt, ctypes.byref(pd), self.argmax[pool_i].data_ptr(), self._D(pn.y.buf), self._D(pn.x),
                self.raw_unit[uid].data_ptr(), u.cout, self._mean(u), self._invstd(u), self._beta(m0), draw,
                self._dbeta(m0), b.WS[ln], b.wsb)
        fn = self.lib.jr_bn_relu_bwd_maxpool
        if self.x6h:    # also the raw-output gradient's magnitude (dy_absmax of its GEMMs)
            fn, args = self.lib.jr_bn_relu_bwd_maxpool_absmax, args + (self._dmax(u),)
        b.add(b.bwd, fn, args + (b.S[ln],),
              "bn_relu_bwd", ln, [("d", pn.y.buf, pn.y.c_off), ("am", pool_i), ("r", uid), ("p",)],
              self._d_all(pn.x) + [dkey, ("g", uid), ("ws", ln)] + ([("dmax", uid)] if self.x6h else []),
              nbytes=4 * b.B * u.ho * u.wo * u.cout * self.esz)

    def _bwd_bn_groups(self, b: Build, ln: int, u: ConvUnit, draw: int, dkey) -> None:
        """One backward launch set per group of members (_bn_groups)."""
        uid, M = u.first.idx, b.B * u.ho * u.wo
        for grp in self._bn_groups(u):
            co0 = grp[0][1]
            cg = sum(m.cout for m, _ in grp)
            segs = (_ffi.BnSeg * len(grp))(*self._bn_segs(m for m, _ in grp))
            b.keep.append(segs)
            args = (self.dt, len(grp), ctypes.byref(segs), self.raw_unit[uid].data_ptr(), co0, u.cout, M, cg,
                    self._mean(u, co0), self._invstd(u, co0), draw, b.WS[ln], b.wsb)
            fn = self.lib.jr_bn_relu_bwd_multi
            if self.x6h:
                fn, args = self.lib.jr_bn_relu_bwd_multi_absmax, args + (self._dmax(u),)
            b.add(b.bwd, fn, args + (b.S[ln],),
                  "bn_relu_bwd", ln, [("d", m.y.buf, m.y.c_off) for m, _ in grp] + [("r", uid), ("p",)],
                  [dkey, ("g", uid), ("ws", ln)] + ([("dmax", uid)] if self.x6h else []), nbytes=3 * M * cg * self.esz)

    def _bwd_dgrad(self, b: Build, ln: int, u: ConvUnit, d, draw: int, dkey, acc: int) -> None:
        if u.x == self.g.input_buf:
            return
        b.add(b.bwd, self.lib.jr_conv2d_bwd_data,
              (ctypes.byref(d), self.cdt, draw, self._wd(u), self._D(u.x), acc, b.WS[ln], b.wsb, b.S[ln]),
              "conv_dgrad", ln, [dkey] + self._w_reads() + self._dmax_reads(u), self._d_all(u.x) + [("ws", ln)])
        b.written.add(u.x)

    def _bwd_wgrad(self, b: Build, ln: int, wl: int, u: ConvUnit, d, draw: int, dkey) -> None:
        """The filter gradient on lane wl: deferred (split-K slabs kept for
        the next jr_wgrad_reduce) or final; the stem's on lane 1 (wl != ln)
        use their own workspace."""
        uid, reads = u.first.idx, self._ax_reads(u.x) + [dkey] + self._dmax_reads(u)
        if uid in b.defer:
            sg, _, nb = b.defer[uid]
            b.add(b.bwd, self.lib.jr_conv2d_bwd_filter_slabs,
                  (ctypes.byref(d), self.cdt, self._AX(u.x), draw, sg.slabs, nb, b.S[wl]),
                  "conv_wgrad", wl, reads, [("slab", uid)])
            b.pending.append((sg, uid))
            return
        ws, wskey = (ctypes.c_void_p(self.ws_stem.data_ptr()), ("wss",)) if wl != ln else (b.WS[ln], ("ws", ln))
        b.add(b.bwd, self.lib.jr_conv2d_bwd_filter,
              (ctypes.byref(d), self.cdt, self._AX(u.x), draw, self.grads.data_ptr() + 4 * u.koff, ws, b.wsb, b.S[wl]),
              "conv_wgrad", wl, reads, [("g", uid), wskey])

    def _bwd_pool(self, b: Build, i: int, n: PoolNode, plain: bool = False) -> None:
        if i in self.pool_bwd and not plain:
            return              # with its producer's BN backward (jr_bn_relu_bwd_maxpool)
        L, dt, B, ln = self.lib, self.dt, b.B, b.lane_of[i]
        acc = 1 if n.x in b.written else 0
        d = self._pool_desc(n, B)
        b.keep.append(d)
        if n.kind == "maxpool":
            b.add(b.bwd, L.jr_maxpool3x3s2_bwd,
                  (ctypes.byref(d), dt, self.argmax[i].data_ptr(), self._D(n.y.buf), self._D(n.x), acc, b.S[ln]),
                  "maxpool_bwd", ln, [("am", i), ("d", n.y.buf, n.y.c_off)], self._d_all(n.x),
                  nbytes=B * n.c * (n.ho * n.wo * (self.esz + 1) + n.h * n.w * self.esz * (1 + acc)))
        else:
            b.add(b.bwd, L.jr_avgpool3x3s1_bwd, (ctypes.byref(d), dt, self._D(n.y.buf), self._D(n.x), acc, b.S[ln]),
                  "avgpool_bwd", ln, [("d", n.y.buf, n.y.c_off)], self._d_all(n.x),
                  nbytes=B * n.c * (n.ho * n.wo + n.h * n.w * (1 + acc)) * self.esz)
        b.written.add(n.x)

    # ---- input gradient (frozen BN)
    def _build_input_grad(self, B: int, nl: Optional[int] = None) -> list:
        """The data-gradient chain of ONE logit per image down to the image,
        after a frozen forward of the same batch: head (jr_head_logit_bwd) and
        GAP, then in reverse node order the pool backwards and, per conv
        launch, the frozen BN backward (jr_bn_relu_bwd_frozen, reading the
        frozen statistics) and the data gradient -- jr_conv2d_bwd_image into
        self.dinput for the image layer.  Fused stem pools: the plain max-pool
        backward from the stored argmax, then the frozen BN backward.  No
        filter gradient, no hook, no optimizer.  Its own key and schedule.
        x6h (x6h_frozen): the list starts with one jr_absmax_reset of the
        data-gradient magnitude rows on lane 0, and every frozen BN backward
        is jr_bn_relu_bwd_frozen_absmax into its launch's row."""
        self._ensure_tiles()
        nl = self.nlanes if nl is None else max(1, min(int(nl), self.nlanes))
        key = (B, nl, "input_grad")
        if key in self._calls:
            return self._calls[key][1]
        if B > self.batch or B <= 0:
            raise ValueError(f"batch {B} outside 1..{self.batch}")
        g, unit_of = self.g, self.plan.unit_of
        b = Build(B, self.lanes, nl, self.ws_lane, self.ws_bytes, node_lanes(g, self.plan, nl))
        b.stats_shift = self.frozen.data_ptr() - self.stats.data_ptr()
        ob, s0 = g.bufs[g.output_buf], b.S[0]
        if self.x6h:
            # x6h (x6h_frozen): every frozen BN backward raises its launch's
            # data-gradient row (the dy_absmax of its dgrad), so those rows
            # start from zero on EVERY run -- two input_gradient calls after one
            # forward give the same bits as one.  (The last of them also held the
            # betas' maxima of the forward's jr_absmax_prep: their guard was
            # evaluated inside that launch, nothing reads them afterwards.)
            first, n = self.mag.span(self.mag.filt_rows, self.mag.dgrad_rows)
            b.add(b.bwd, self.lib.jr_absmax_reset, (self.absmax.data_ptr() + 4 * first, n, s0),
                  "absmax_reset", 0, [], [("dmax", u.first.idx) for u in self.cunits], nbytes=4 * n)
        b.add(b.bwd, self.lib.jr_head_logit_bwd,
              (self._p("dense/kernel"), self.ig_target.data_ptr(), B, ob.c, self.units, self.dfeat.data_ptr(), s0),
              "head_logit_bwd", 0, [("p",), ("target",)], [("dfeat",)])
        b.add(b.bwd, self.lib.jr_gap_bwd,
              (self.dt, self.dfeat.data_ptr(), B, ob.h * ob.w, ob.c, self._D(g.output_buf), s0),
              "gap_bwd", 0, [("dfeat",)], self._d_all(g.output_buf))
        for i in range(len(g.nodes) - 1, -1, -1):
            n = g.nodes[i]
            if n.kind != "conv":
                self._bwd_pool(b, i, n, plain=True)
            elif unit_of[n.idx].first is n:
                self._ig_conv(b, i, unit_of[n.idx])
        schedule(b.seq)
        self._calls[key] = (None, b.bwd, None, b.keep, None)
        return b.bwd

    def _ig_conv(self, b: Build, i: int, u: ConvUnit) -> None:
        ln, uid, M = b.lane_of[i], u.first.idx, b.B * u.ho * u.wo
        acc = 1 if u.x in b.written else 0
        d = self._conv_desc(u, b.B)
        b.keep.append(d)
        draw, dkey = self.draw_lane[ln].data_ptr(), ("draw", ln)
        for grp in self._bn_groups(u):
            co0 = grp[0][1]
            cg = sum(m.cout for m, _ in grp)
            segs = (_ffi.BnSeg * len(grp))(*[
                _ffi.BnSeg(self._D(m.y.buf), m.y.c_off, self.g.bufs[m.y.buf].c, m.cout, self._beta(m), None)
                for m, _ in grp])
            b.keep.append(segs)
            # x6h: also the raw-output gradient's magnitude, the dy_absmax of the
            # dgrad below (which reads dkey, written here: ordered behind it)
            fn, amax = ((self.lib.jr_bn_relu_bwd_frozen_absmax, (self._dmax(u),)) if self.x6h
                        else (self.lib.jr_bn_relu_bwd_frozen, ()))
            b.add(b.bwd, fn,
                  (self.dt, len(grp), ctypes.byref(segs), self.raw_unit[uid].data_ptr(), co0, u.cout, M, cg,
                   self._mean(u, co0) + b.stats_shift, self._invstd(u, co0) + b.stats_shift, draw) + amax + (b.S[ln],),
                  "bn_relu_bwd_frozen", ln, [("d", m.y.buf, m.y.c_off) for m, _ in grp] + [("r", uid), ("p",)],
                  [dkey] + ([("dmax", uid)] if self.x6h else []), nbytes=3 * M * cg * self.esz)
        if u.x != self.g.input_buf:
            self._bwd_dgrad(b, ln, u, d, draw, dkey, acc)
            return
        ib = self.g.bufs[u.x]
        b.add(b.bwd, self.lib.jr_conv2d_bwd_image,
              (ctypes.byref(d), self.dt, draw, self.params.data_ptr() + 4 * u.koff, self.dinput.data_ptr(), 4, b.S[ln]),
              "conv_bwd_image", ln, [dkey, ("p",)], [("dinput",)],
              nbytes=M * u.cout * self.esz + 16 * b.B * ib.h * ib.w)

    def input_gradient(self, B: Optional[int] = None, target=None) -> None:
        """Enqueue d logit_t(i) / d image_i for every image i of the batch into
        self.dinput (fp32 [B, h, w, 4], channel 3 zero).  target: None (logit 0)
        or one class index per image.  Needs Engine(..., input_grad=True) and a
        forward(B, bn="frozen") of the current batch: under frozen BN the
        gradient of an image's logit is a property of that image alone (bit
        for bit on x8 / f32 / bf16; on x6h, whose dy scales are measured per
        batch, to within the x6h error class)."""
        if not self.input_grad:
            raise ValueError("input_gradient needs an engine built with input_grad=True")
        self._check_frozen("frozen")
        B = B or self.batch
        if self._frozen_fwd != B:
            raise ValueError(f"input_gradient({B}) needs a forward({B}, bn='frozen') of the current batch first "
                             "(none since the last set_batch / batch-statistics forward)")
        calls = self._build_input_grad(B)
        with torch.cuda.stream(self.stream):
            if target is None:
                self.ig_target[:B].zero_()
            else:
                t = torch.as_tensor(target, dtype=torch.int32).reshape(-1)
                if t.numel() != B:
                    raise ValueError("target must have one class index per image")
                self.ig_target[:B].copy_(t, non_blocking=True)
        self.lanes.fork()
        self.lanes.run(calls)
        self.lanes.join()

    def input_gradient_numpy(self, B: Optional[int] = None) -> np.ndarray:
        """[B, h, w, 3]: the result of the last input_gradient."""
        B = B or self.batch
        ib = self.g.bufs[self.g.input_buf]
        self.synchronize()
        return self.dinput[:B * ib.h * ib.w * 4].view(B, ib.h, ib.w, 4)[..., :ib.c].cpu().numpy()

    # ---- optimizer
    def _opt_desc(self) -> tuple:
        """self.optimizer's update: (by-value function, _ex function, state
        buffers, hyper-parameters passed by value, written resources, nbytes).
        Both functions take (params, grads, *state, n, ...; stream last): by value
        (lr, *hyper, grad_scale), _ex (*hyper, ranges, nranges, hyper and step struct)."""
        L, acc, pa = self.lib, self.accum.data_ptr(), [("p",), ("acc",)]
        if self.optimizer == "nesterov":
            return L.jr_nesterov_update, L.jr_nesterov_update_ex, (acc,), (self.momentum,), pa, 20 * self.nparam
        if self.optimizer == "momentum":
            return L.jr_momentum_update, L.jr_momentum_update_ex, (acc,), (self.momentum,), pa, 0
        if self.optimizer == "sgd":
            return L.jr_sgd_update, L.jr_sgd_update_ex, (), (), [("p",)], 0
        if self.optimizer == "adam":
            return (L.jr_adam_update, L.jr_adam_update_ex, (acc, self.adam_v.data_ptr()),
                    (self.adam_b1, self.adam_b2, self.adam_eps), pa, 0)
        return (L.jr_rmsprop_update, L.jr_rmsprop_update_ex, (acc, self.adam_v.data_ptr()),
                (self.rmsprop_rho, self.rmsprop_momentum, self.rmsprop_eps), pa, 28 * self.nparam)

    def _by_value_args(self, lr: float, grad_scale: float) -> tuple:
        """The by-value update's arguments (lr: Adam's alpha of the step)."""
        _, _, state, hyper, _, _ = self._opt_desc()
        return (self.params.data_ptr(), self.grads.data_ptr(), *state, self.nparam, lr, *hyper, grad_scale, self._s)

    def _opt_update(self, b: Build) -> None:
        L, s0, n, G = self.lib, b.S[0], self.nparam, self.grads.data_ptr()
        fn, fn_ex, state, hyper, writes, nbytes = self._opt_desc()
        greads = [("g", u.first.idx) for u in self.cunits] + [("g", "dense")]
        ph = b.accum
        if ph is not None:
            # the group's sum (jr.h jr_grad_accumulate): acc <- g / acc <- acc + g on a micro-step that
            # leaves the group open, g <- g + acc on the closing one, g <- acc when accum_flush
            # closes a partial group.  ("inside" is "open" with first = 0: _build_calls)
            A = self.gacc.data_ptr()
            if ph == "open":
                b.add(b.opt, L.jr_grad_accumulate, (A, G, n, 1, s0), "grad_accumulate", 0, greads, [("gacc",)],
                      nbytes=8 * n)
            else:
                b.add(b.opt, L.jr_grad_accumulate, (G, A, n, int(ph == "flush"), s0), "grad_accumulate", 0,
                      [("gacc",)], greads, nbytes=(8 if ph == "flush" else 12) * n)
        # what runs once per update, and what runs once per micro-batch
        updating, per_batch = ph in (None, "close", "flush"), ph != "flush"
        if not updating:
            pass        # the group stays open
        elif self.opt_ex:
            # norm of the (reduced) raw gradient -> scale / skip of this step -> the
            # update reading lr, weight decay, scale and skip from device memory
            part, hy, st = self.opt_partials.data_ptr(), self.opt_hyper.data_ptr(), self.opt_step_dev.data_ptr()
            R, nr = self._opt_ranges_dev.data_ptr(), len(self.opt_ranges)
            b.add(b.opt, L.jr_grad_sqnorm, (G, n, part, ctypes.c_size_t(8 * self.opt_partials.numel()), s0),
                  "grad_sqnorm", 0, greads, [("gnorm",)], nbytes=4 * n)
            b.add(b.opt, L.jr_opt_prepare, (part, n, hy, st, s0), "opt_prepare", 0, [("gnorm",)], [("gnorm",)])
            b.add(b.opt, fn_ex, (self.params.data_ptr(), G, *state, n, *hyper, R, nr, hy, st, s0),
                  self.optimizer + "_update_ex", 0, greads + [("gnorm",)], writes, nbytes=nbytes)
        else:   # (adam: apply_update binds the step's alpha in place of self.lr)
            b.add(b.opt, fn, self._by_value_args(self.lr, 1.0), self.optimizer, 0, greads, writes, nbytes=nbytes)
        if self.ema is not None and updating:
            # the moving average of the updated weights, a pass of its own;
            # the device path hands it the step struct: a skipped step is neither averaged nor counted
            es, st = self.ema_state.data_ptr(), (self.opt_step_dev.data_ptr() if self.opt_ex else None)
            gn = [("gnorm",)] if self.opt_ex else []
            b.add(b.opt, L.jr_ema_prepare, (es, st, s0), "ema_prepare", 0, gn, [("ema",)])
            b.add(b.opt, L.jr_ema_update, (self.ema.data_ptr(), self.params.data_ptr(), n, es, st, s0), "ema_update", 0,
                  [("p",), ("ema",)] + gn, [("ema",)], nbytes=12 * n)
        if self.bn_momentum is not None and per_batch:
            # the moving averages of this step's batch statistics (one launch; jr.h)
            b.add(b.opt, L.jr_bn_moving_update, self._bn_update_args(b.B, self.bn_momentum, s0), "bn_moving", 0,
                  [("r", u.first.idx) for u in self.cunits], [("bn_moving",)], nbytes=4 * 2 * self.stats_ms)
        if b.training and per_batch:
            # the next step's mask: the counter counts enqueued steps, a skipped one included (jr.h)
            b.add(b.opt, L.jr_dropout_advance, (self.drop_state.data_ptr(), s0), "dropout_advance", 0, [], [("drop",)])

    def fence_lanes(self, stream) -> None:
        """`stream` (the gradient all-reduce's) waits for the work enqueued on
        EVERY lane so far; the lanes themselves wait for nothing.  Used by
        jr.dist.BucketAllReduce at each bucket's issue point instead of
        joining the lanes onto lane 0."""
        self.lanes.fence(stream)

    # ------------------------------------------------------------------- data
    def set_batch(self, images, labels=None, n: Optional[int] = None, augment=None, warp=None,
                  staged: bool = False) -> int:
        """Copy a batch (NHWC float32, or uint8 to be scaled by 1/255) into the
        input buffer.  Returns the batch size.  augment, warp: jr.augment
        tables (one jr_augment_param / jr_warp_param per image) -- the uint8
        batch then goes through the augmenting conversion kernel or, with a
        warp, the warping one (None, None: no augmentation; _u8_to_input).
        staged: a uint8 host batch goes through the two-slot pinned feed
        (_upload_staged: the copy runs on a stream of its own and the host never
        waits for the step it feeds); anything else takes the path above."""
        B = int(images.shape[0]) if n is None else n
        self._check_images(images, B)
        self._frozen_fwd = None
        if staged and not isinstance(images, torch.Tensor) and np.asarray(images).dtype == np.uint8:
            self._upload_staged(np.asarray(images), labels, B, augment, warp)
        else:
            with torch.cuda.stream(self.stream):
                self._upload(images, labels, B, augment, warp)
        return B

    # ---- the staged input feed
    def _upload_staged(self, images: np.ndarray, labels, B: int, augment, warp) -> None:
        """_upload for a uint8 host batch without a pageable copy and without a
        host wait for the step it feeds: the batch goes through the free slot
        of the feed (jr.runahead.Feed.load, built here at first use), then the
        unchanged conversion kernel (_u8_to_input) reads pixels and tables
        inside the slot, and the labels are copied out of it, on self.stream."""
        ib = self.g.bufs[self.g.input_buf]
        tab, wtab = _augment.batch_tables(B, augment, warp)
        y = None if labels is None else np.asarray(labels, np.float32).reshape(-1)
        if y is not None:
            self._check_labels(y, B)
        f = self._feed = self._feed or Feed(self.device, self.batch, self.units, ib.h * ib.w * ib.c)
        dev = f.load(self.stream, images, y, tab, wtab)
        base = dev.data_ptr()
        self._u8_to_input(base + f.off_x, B, None if tab is None else base + f.off_a,
                          None if wtab is None else base + f.off_w)
        if y is not None:
            with torch.cuda.stream(self.stream):
                self.labels[:y.size].copy_(dev[f.off_y:f.off_y + 4 * y.size].view(torch.float32))

    # ------------------------------------------------------------------- runs
    def forward(self, B: Optional[int] = None, bn: str = "batch", training: bool = False) -> None:
        """bn="frozen": normalise with the statistics of freeze_bn() instead
        of this batch's (every image's output then depends on that image alone).
        training: the forward of a training step (train_step's lists): with
        dropout on it drops, and backward / apply_update of that step take
        training=True too.  Every other forward never drops."""
        frozen = self._check_frozen(bn)
        fwd = self._build_calls(B or self.batch, frozen=frozen, training=training)[0]
        self._frozen_fwd = (B or self.batch) if frozen else None
        self.lanes.fork()
        self.lanes.run(fwd)
        self.lanes.join()

    def backward(self, B: Optional[int] = None, hook=None, training: bool = False) -> None:
        self.lanes.run(self._build_calls(B or self.batch, training=training)[1], hook)
        self.lanes.join()

    def _adam_alpha(self) -> float:
        """TF ApplyAdam (training_ops.cc): alpha = lr * sqrt(1 - beta2_power)
        / (1 - beta1_power) of the next step, evaluated in the variable dtype
        (fp32, left to right; np.sqrt of a float32 is correctly rounded like
        Eigen's), from fp32 beta powers, which it then advances."""
        f = np.float32
        self.adam_t += 1
        alpha = f(f(self.lr) * np.sqrt(f(1) - self.adam_b2p)) / (f(1) - self.adam_b1p)
        self.adam_b1p = f(self.adam_b1p * f(self.adam_b1))
        self.adam_b2p = f(self.adam_b2p * f(self.adam_b2))
        return float(f(alpha))

    def _push_hyper(self, lr: float, grad_scale: float) -> None:
        """Enqueue jr_opt_set_hyper on the engine's stream when a scalar differs
        from what the device holds (by value: nothing for the host to keep alive)."""
        want = (float(lr), self.weight_decay, self.clip_norm or 0.0, float(grad_scale))
        if want != self._hyper_dev:
            _ffi.check("jr_opt_set_hyper", self.lib.jr_opt_set_hyper(self.opt_hyper.data_ptr(), *want, self._s))
            self._hyper_dev = want

    def set_lr(self, lr: float) -> None:
        """The learning rate of the steps enqueued from here on, replays of a
        captured step included (device path only: the default path binds the
        rate into its call lists and captured graphs)."""
        if not self.opt_ex:
            raise ValueError("set_lr needs the device optimizer path: Engine(device_lr=True) "
                             "(or weight_decay / clip_norm)")
        self.lr = float(lr)
        # (grad_scale stays what the last apply_update set; the next apply_update / replay sets its own)
        if self.optimizer != "adam":    # Adam: apply_update writes the step's alpha
            self._push_hyper(self.lr, self._hyper_dev[3])

    def opt_step(self) -> Tuple[float, float, int, int]:
        """(grad_norm, scale, skipped, skipped_total) of the last step (jr.h
        jr_opt_step), after a synchronise."""
        if not self.opt_ex:
            raise ValueError("opt_step needs the device optimizer path (weight_decay, clip_norm or device_lr)")
        self.synchronize()
        raw = self.opt_step_dev.cpu()
        scale, norm = (float(v) for v in raw[:2])
        skipped, total = (int(v) for v in raw[2:].view(torch.int32))
        return norm, scale, skipped, total

    def _bound(self, opt, grad_scale: float) -> list:
        """An update list with this update's scalars: the device path writes them
        ahead of it (_push_hyper); by value, the optimizer's call is rebound when
        they differ from what the list holds (self.lr, 1.0)."""
        if self.opt_ex:
            # (a skipped step still counts as a step on the host: Adam's t and beta powers,
            # and the BN moving averages and self.updates, advance; only the device
            # write of weights and optimizer state is withheld -- jr.h)
            self._push_hyper(self._adam_alpha() if self.optimizer == "adam" else self.lr, grad_scale)
        elif grad_scale != 1.0 or self.optimizer == "adam":
            # (so Adam steps run eagerly: the scalar changes every step)
            lr = self._adam_alpha() if self.optimizer == "adam" else self.lr
            i = next(j for j, c in enumerate(opt) if c.name == self.optimizer)
            opt = list(opt)
            opt[i] = dataclasses.replace(opt[i], args=self._by_value_args(lr, grad_scale))
        return opt

    def apply_update(self, B: Optional[int] = None, grad_scale: float = 1.0, training: bool = False) -> None:
        self._no_update_on_average("apply_update")
        opt = self._build_calls(B or self.batch, training=training)[2]
        self.lanes.run(self._bound(opt, grad_scale))
        self._settle()

    # ---- the step driver: one routine enqueues a step, one settles the host's books after it
    def _enqueue_step(self, lists, allreduce=None, fold: bool = False, denom: Optional[int] = None) -> None:
        """A step's call lists (_build_calls) on the lanes: fork, forward, join,
        [allreduce.begin], backward [with the bucket hook], join -- every lane
        back on self.stream -- then _finish_update.  Without `allreduce` (a
        micro-step that leaves its group open, a capture) nothing is exchanged."""
        fwd, bwd, opt = lists[:3]
        ln = self.lanes
        ln.fork()
        ln.run(fwd)
        ln.join()
        if allreduce is None:
            ln.run(bwd)
        else:
            allreduce.begin(self, fold=True) if fold else allreduce.begin(self)
            ln.run(bwd, allreduce.param_ready)
        ln.join()
        self._finish_update(opt, allreduce, denom)

    def _finish_update(self, opt, allreduce, denom: Optional[int]) -> None:
        """The tail that closes an update: [allreduce.finish -> the exchange's
        scale], then the update list with grad_scale = scale / denom bound
        (_bound: after finish() has returned the scale).  denom None: the list
        as it stands -- a group stays open, or a capture, whose scalars were
        bound before jr_graph_begin, never inside it."""
        scale = 1.0 if allreduce is None else allreduce.finish(self)
        self.lanes.run(opt if denom is None else self._bound(opt, scale / denom))

    def _settle(self, batch: bool = True, closed: Optional[bool] = None, log: bool = False) -> None:
        """The host's books after what a step enqueued -- the one place where
        `updates`, `_pending` and the step log move.  batch: a micro-batch ran
        (and with bn_moving its jr_bn_moving_update); closed: whether it closed
        its group (None: no group is touched -- apply_update on its own); log:
        one record, of an update when the group closed."""
        if batch and self.bn_momentum is not None:
            self.updates += 1
        if closed is not None:
            self._pending = 0 if closed else self._pending + 1
        if log:
            self._log_append(bool(closed))

    def train_step(self, B: Optional[int] = None, allreduce=None) -> None:
        """fwd + bwd (+ bucketed all-reduce) + optimizer, enqueued on the lanes
        (_enqueue_step).  accum_steps = K > 1: one micro-batch -- forward and
        backward as ever, then the group's sum; the exchange and the optimizer
        run on the K-th call only, with grad_scale 1 / (k * world).  Closing
        under data parallelism runs the DEFAULT lists: BucketAllReduce folds
        `gacc` into each bucket on its own stream just before it issues it
        (begin(fold=True))."""
        B = B or self.batch
        self._no_update_on_average("train_step")
        ph = self._accum_phase()
        closing = ph in (None, "close")
        exchange = allreduce if closing else None
        lists = self._build_calls(B, training=True, accum=None if exchange is not None else ph)
        self._frozen_fwd = None
        self._enqueue_step(lists, exchange, fold=ph is not None, denom=self._pending + 1 if closing else None)
        self._settle(closed=closing, log=True)

    # ---- gradient accumulation (accum_steps = K > 1)
    def accum_pending(self) -> int:
        """Micro-batches in the open group (0: the last train_step, replay or accum_flush closed one)."""
        return self._pending

    def _accum_phase(self) -> Optional[str]:
        """Where the next micro-batch sits in its group (_build_calls' accum); None: accum_steps = 1."""
        k, K = self._pending, self.accum_steps
        return None if K == 1 else "close" if k + 1 == K else "inside" if k else "open"

    def _flush_calls(self) -> list:
        """accum_flush's list: jr_grad_accumulate(g <- acc, first = 1), then what
        runs once per update (the optimizer, the weight average) -- what runs
        once per micro-batch already ran with each of them."""
        key = ("accum", "flush")
        if key not in self._calls:
            b = Build(self.batch, self.lanes, 1, self.ws_lane, self.ws_bytes, {})
            b.accum = "flush"
            self._opt_update(b)
            schedule(b.seq)
            self._calls[key] = ([], [], b.opt, b.keep, None)
        return self._calls[key][2]

    def accum_flush(self, allreduce=None) -> bool:
        """Close a partial group of k < K micro-batches (the end of an epoch):
        g <- acc, the exchange (every bucket at once: no backward to overlap), the
        update with grad_scale 1 / (k * world) (_finish_update).  Nothing is
        pending: nothing happens.  Returns whether an update ran.  Collective
        under data parallelism: every rank holds the same k."""
        self._no_update_on_average("accum_flush")
        k = self._pending
        if k == 0:
            return False
        opt = self._flush_calls()
        self.lanes.run(opt[:1])
        if allreduce is not None:
            allreduce.begin(self)
        self._finish_update(opt[1:], allreduce, k)
        self._settle(batch=False, closed=True, log=True)    # (the loss is the last micro-batch's: no forward ran here)
        return True

    # ---- device metrics (jr.h jr_metrics_*; state: jr.runahead.Metrics)
    def metrics_init(self, thresholds) -> None:
        """Device state of the streaming metrics: the fp32 threshold table, the
        uint32 [4][T] counts (tp, fp, fn, tn) and the Brier double[2], zeroed."""
        self._metrics = Metrics(self, thresholds)

    def _need_metrics(self) -> Metrics:
        if self._metrics is None:
            raise ValueError("the device metrics are off: call metrics_init(thresholds) first")
        return self._metrics

    def metrics_update(self, B: Optional[int] = None, counts: bool = True, brier: bool = True) -> None:
        """Enqueue jr_metrics_accumulate over the probabilities and labels of the
        forward (or step) enqueued last, on self.stream behind it: no host wait."""
        self._need_metrics().accumulate(self.probs.data_ptr(), self.labels.data_ptr(), (B or self.batch) * self.units,
                                        counts, brier, self._s)

    def metrics_reset(self) -> None:
        self._need_metrics().reset(self._s)

    def metrics_read(self) -> Tuple[np.ndarray, float, float]:
        """(uint32 [4, T] counts, the Brier sum, the sample count) after a synchronise."""
        m = self._need_metrics()
        self.synchronize()
        return m.read()

    # ---- the step log (jr.h jr_step_log_append; state: jr.runahead.StepLog)
    STEP_REC = STEP_REC

    def step_log_enable(self, capacity: int) -> None:
        """From here on train_step (each micro-batch of an accumulation group) and
        accum_flush append one jr_step_rec to a device ring of `capacity` records:
        the loss, and on the device optimizer path the update's grad_norm, scale
        and skip flag.  step_log_read() fetches them.  A device failure
        (jr_device_check) of a logged step shows at the next synchronise, up to
        `capacity` steps late."""
        self._log = StepLog(self, capacity)

    def _log_append(self, updated: bool) -> None:
        if self._log is not None:
            step = self.opt_step_dev.data_ptr() if (self.opt_ex and updated) else None
            self._log.append(self.loss.data_ptr(), step, self._s)

    def step_log_read(self) -> np.ndarray:
        """The records appended since the last read, oldest first, as a STEP_REC
        array (flags bit 0: an update ran and grad_norm / scale are its own; bit 1:
        the non-finite guard skipped it).  One synchronise."""
        if self._log is None:
            raise ValueError("the step log is off: call step_log_enable(capacity) first")
        self.synchronize()
        return self._log.take()

    def capture(self, B: Optional[int] = None) -> None:
        """Capture fwd+bwd+update for batch B into a HIP graph (single GPU;
        not for Adam, whose step scalar changes every step); the two lane
        streams are captured (fork/join by events) and become parallel
        branches of the graph, the producer waits its edges.  At most two
        lanes: on ROCm 7.2, cross-waits among three or more captured streams
        (waits on events recorded mid-stream) crashed hipGraphInstantiate
        (DESIGN.md §3); more lanes run eagerly.  accum_steps = K > 1: one graph
        each for the micro-step that opens a group, one inside it (K > 2) and
        the one that closes it, grad_scale 1 / K.  The host's books (_settle)
        stay as they are: nothing ran."""
        B = B or self.batch
        self._no_update_on_average("capture")
        if self.optimizer == "adam":
            raise ValueError("Adam steps run eagerly (the step's alpha is a host scalar)")
        if self.nlanes > 2:
            raise ValueError("HIP graph capture supports at most two lanes (more lanes run eagerly)")
        K = self.accum_steps
        for ph in ([None] if K == 1 else ["open"] + ["inside"] * (K > 2) + ["close"]):
            fwd, bwd, opt, _, _ = self._build_calls(B, training=True, accum=ph)
            if ph in (None, "close"):
                # the graph reads the device scalars: written ahead of it, never inside it
                # (by value: the group's 1 / K is bound into the captured call)
                opt = self._bound(opt, 1.0 / K)
            torch.cuda.synchronize(self.device)
            _ffi.check("jr_graph_begin", self.lib.jr_graph_begin(self._s))
            self.lanes.capturing = not self.graph_precise
            try:
                self._enqueue_step((fwd, bwd, opt))
            finally:
                self.lanes.capturing = False
                ex = ctypes.c_void_p()
                _ffi.check("jr_graph_end", self.lib.jr_graph_end(self._s, ctypes.byref(ex)))
            self._graphs[B if ph is None else (B, ph)] = ex.value

    def replay(self, B: Optional[int] = None) -> None:
        B = B or self.batch
        self._no_update_on_average("replay")
        ph = self._accum_phase()        # (choosing the graph is the only host work)
        if self.opt_ex:     # a captured step is single-GPU: grad_scale 1 / K, whatever an eager update left
            self._push_hyper(self.lr, 1.0 / self.accum_steps)
        _ffi.check("jr_graph_launch",
                   self.lib.jr_graph_launch(ctypes.c_void_p(self._graphs[B if ph is None else (B, ph)]), self._s))
        self._settle(closed=ph in (None, "close"))

    def synchronize(self) -> None:
        """Wait for every lane, then jr_device_check: a device-side failure
        of any launch since the last check (a stream-K hand-off count word not
        left zero) raises JRError here instead of leaving wrong numbers.
        A loop that runs ahead (device metrics, the step log, the staged feed)
        synchronises once in N steps, so a failure is reported up to N steps
        late -- but always before anything read after a synchronise is used:
        metrics_read, step_log_read, params_numpy (a checkpoint) all end here."""
        for st in self.lane_streams:
            st.synchronize()
        _ffi.device_check()

    def loss_value(self) -> float:
        self.synchronize()
        return float(self.loss[0].item())

    def predictions(self, B: Optional[int] = None) -> np.ndarray:
        B = B or self.batch
        self.synchronize()
        return self.probs[:B * self.units].cpu().numpy().reshape(B, self.units)

    def close(self) -> None:
        """Destroy this engine's HIP graph executables (also on collection)."""
        graphs = getattr(self, "_graphs", None)
        if not graphs:
            return
        for ex in graphs.values():
            self.lib.jr_graph_destroy(ctypes.c_void_p(ex))
        graphs.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone
            pass
