"""Grouped ensemble inference: every member of an evaluate.py -lm ensemble in
ONE launch per layer.

The reference restores and runs each ensemble member in turn
(evaluate.py:166-211), and jr.Engine runs one member per engine.  At the
eval batch of 32 (evaluate.py:25) most GEMMs of one member are too small to
fill the 256 CUs (the 8x8 layers are M = 2,048 GEMMs), so members' forwards
were underfilled launches one after another.  EnsembleEngine keeps M members
resident as ONE replica with a member dimension: every tensor is member-major
([member][batch ...], fixed member strides), and each layer is

  * one grouped conv + BN-statistics launch (jr_conv2d_fwd_bn_stats_grouped:
    member = blockIdx.y, each with its own weights and statistics);
  * one grouped BN+ReLU apply per conv2d_bn layer (jr_bn_relu_apply_grouped);
  * pools and the global average pool over M x B images (the member-major
    activation buffers are simply a batch of M x B images);
  * the dense / sigmoid head per member (tiny).

Every member sees exactly its own batch-statistics BN (App. C Q1) and the
per-member tile plan, so its predictions are BITWISE those of a jr.Engine of
that member (tests/test_gpu_ensemble.py).  Inference only (train=False).

forward(bn="frozen") normalises with fixed statistics (freeze_bn).  On
conv_math="x6h" that needs x6h_frozen=True: the frozen list then stores every
activation through the guarded entry points (jr_bn_relu_apply_grouped_guard,
jr_bn_relu_maxpool3x3s2_fwd_grouped_guard; limit 2 * act_bound, one error word
for all members), the conv scales stay constants -- predictions bitwise
independent of the other images of the batch -- and an activation above the
bound raises JRError (JR_ERR_DEVICE) at the next synchronize() / predictions().
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch

from . import _ffi
from .engine import Replica, pinned_tile_table
from .inception import BN_EPS, build_inception_v3
from .lanes import Build, node_lanes, schedule


class EnsembleEngine(Replica):
    """M inference replicas (ensemble members) of one geometry on one GPU."""

    def __init__(self, params: List[np.ndarray], batch: int, height: int = 299, width: int = 299, units: int = 1,
                 device: int | torch.device = 0, dtype: str = "f32", conv_math: Optional[str] = None,
                 tiles: str = "pinned", head: str = "sigmoid", fuse_pool: Optional[bool] = None, lanes: int = 2,
                 x6h_frozen: bool = False):
        # x6h_frozen: forward(bn="frozen") on conv_math="x6h" through the guarded
        # BN applies and fused stem pools (Replica._frozen_guard), as jr.Engine
        if not params:
            raise ValueError("at least one member")
        self.members = len(params)
        # (fuse_pool: the stem's BN + ReLU inside its max-pools, every member in one launch)
        super().__init__(build_inception_v3(height, width, units), device, dtype, conv_math, ("x8", "x6h", "f32"),
                         head, True, fuse_pool, lanes, x6h_frozen=x6h_frozen)
        self.batch = int(batch)
        self._alloc()
        self.load_params(params)
        self.tiles, self._cfgs = "heuristic", None
        if tiles == "pinned":
            t = pinned_tile_table(self.conv_math, self.batch, height, width, False)
            if t is not None and all(u.name in t["configs"] for u in self.cunits):
                self._apply_configs(t["configs"])
                self.tiles = "pinned"
        elif tiles != "heuristic":
            raise ValueError("tiles: 'pinned' or 'heuristic'")
        self._gen = self.lib.jr_conv2d_config_generation()
        self._calls = {}

    # ------------------------------------------------------------------ memory
    def _alloc(self) -> None:
        B, M = self.batch, self.members
        self._alloc_forward(dgrad_rows=False)
        if self.dt == _ffi.JR_BF16:
            # the bf16 W^T operand copies of every member (weights never change
            # in inference: prepared once, at load_params)
            self._alloc_bf16_filters(hwio=False)
        ws = 0
        for u in self.cunits:
            d = self._conv_desc(u, B)
            ws = max(ws, self.lib.jr_conv2d_workspace_size_grouped(ctypes.byref(d), self.cdt, M))
        self._alloc_ws(ws)

    def load_params(self, params: List[np.ndarray]) -> None:
        """Keras-layout flat parameters of every member (jr.checkpoint.load)."""
        if len(params) != self.members:
            raise ValueError(f"expected {self.members} members' parameters, got {len(params)}")
        with torch.cuda.stream(self.stream):     # ordered before the weight prep below
            for m, flat in enumerate(params):
                self.params[m * self.nparam:(m + 1) * self.nparam].copy_(
                    torch.from_numpy(self.plan.to_internal(self.g, flat)).to(self.device))
        if self.dt == _ffi.JR_BF16:
            with torch.cuda.stream(self.stream):
                _ffi.check("wprep", self.lib.jr_conv_weights_bf16_multi(
                    self.wprep_table.data_ptr(), self.wprep_layers, self.wprep_tiles, self.params.data_ptr(), None,
                    self.w_t.data_ptr(), self._s))
        if self.x6h:
            _ffi.check("absmax_prep", self.lib.jr_absmax_prep(
                self.params.data_ptr(), self.absmax_table.data_ptr(), self.absmax_nseg, self.absmax.data_ptr(),
                self.absmax.numel(), self._s))
        self.stream.synchronize()
        if self.x6h:
            _ffi.device_check()       # the beta guard of the activation bound (jr.h jr_absmax_prep)

    def _apply_configs(self, cfgs: dict) -> None:
        """The per-member forward tile of every launch (the eval table's)."""
        self._cfgs = cfgs
        for u in self.cunits:
            d = self._conv_desc(u, self.batch)
            _ffi.check("set_config", self.lib.jr_conv2d_set_config(ctypes.byref(d), _ffi.JR_CONV_FWD, self.cdt, 0,
                                                                   cfgs[u.name][0]))

    # ------------------------------------------------------------- call list
    def _build_calls(self, B: int, frozen: bool = False):
        """(calls, keep): the forward of every member as Calls (jr.lanes) --
        resources: activation channel slices, a launch's raw output +
        statistics, the lane's workspace.  frozen: every BN apply and fused
        stem pool reads self.frozen (a list of its own)."""
        if self._cfgs is not None and self.lib.jr_conv2d_config_generation() != self._gen:
            self._apply_configs(self._cfgs)        # another caller moved this geometry's tiles
            self._calls.clear()
            self._gen = self.lib.jr_conv2d_config_generation()
        key = (B, "frozen") if frozen else B
        if key in self._calls:
            return self._calls[key]
        if B > self.batch or B <= 0:
            raise ValueError(f"batch {B} outside 1..{self.batch}")
        b = Build(B, self.lanes, self.nlanes, self.ws_lane, self.ws_bytes, node_lanes(self.g, self.plan, self.nlanes))
        if frozen:
            b.stats_shift = self.frozen.data_ptr() - self.stats.data_ptr()
            b.guard = self._frozen_guard()
        for i, n in enumerate(self.g.nodes):
            if n.kind != "conv":
                self._fwd_pool(b, i, n)
            elif self.plan.unit_of[n.idx].first is n:
                self._fwd_conv(b, b.lane_of[i], self.plan.unit_of[n.idx])
        self._fwd_head(b)
        schedule(b.seq)
        self._calls[key] = (b.fwd, b.keep)
        return self._calls[key]

    def _fwd_conv(self, b: Build, ln: int, u) -> None:
        """One grouped conv + statistics launch, one grouped BN + ReLU per member layer."""
        L, g, M, B, s = self.lib, self.g, self.members, b.B, b.S[ln]
        d = self._conv_desc(u, B)
        b.keep.append(d)
        uid = u.first.idx
        if self.dt == _ffi.JR_BF16:
            w, w_ms = self.w_t.data_ptr() + 2 * self.wb_t_off[uid], self.wt_ms
        else:
            w, w_ms = self.params.data_ptr() + 4 * u.koff, self.nparam
        raw = self.raw_unit[uid].data_ptr()
        mean, inv = self._mean(u), self._invstd(u)
        b.add(b.fwd, L.jr_conv2d_fwd_bn_stats_grouped,
              (ctypes.byref(d), self.cdt, M, self._A(u.x), self.act_ms[u.x], w, w_ms, raw, self.raw_ms[uid], BN_EPS,
               mean, inv, self.stats_ms, b.WS[ln], b.wsb, s),
              "conv_fwd", ln, self._a_all(u.x), [("r", uid), ("ws", ln)])
        rows = B * u.ho * u.wo
        for mem, co in zip(u.members, u.col_off):
            if mem.y.buf in self.fused_bufs:
                continue        # applied inside its max-pool
            fn, lim = ((L.jr_bn_relu_apply_grouped, ()) if b.guard is None
                       else (L.jr_bn_relu_apply_grouped_guard, (b.guard,)))
            b.add(b.fwd, fn,
                  (self.dt, M, raw, co, u.cout, self.raw_ms[uid], rows, mem.cout, mean + 4 * co + b.stats_shift,
                   inv + 4 * co + b.stats_shift, self.stats_ms, self._beta(mem), self.nparam, self._A(mem.y.buf),
                   mem.y.c_off, g.bufs[mem.y.buf].c, self.act_ms[mem.y.buf]) + lim + (s,),
                  "bn_relu", ln, [("r", uid)] + self._frozen_reads(b), [("a", mem.y.buf, mem.y.c_off)])

    def _fwd_pool(self, b: Build, i: int, n) -> None:
        """Pools: the member-major buffers of a full batch are one batch of
        M * B images (one launch); a partial last batch (B < planned: members
        sit `batch` images apart) runs per member."""
        L, M, B, ln = self.lib, self.members, b.B, b.lane_of[i]
        s, yb, full = b.S[ln], self.g.bufs[n.y.buf], B == self.batch
        for m in range(1 if full else M):
            d = _ffi.PoolDesc(M * B if full else B, n.h, n.w, n.c, n.ho, n.wo, 0, n.c, n.y.c_off, yb.c)
            b.keep.append(d)
            xi, yo, out = self._A(n.x, m), self._A(n.y.buf, m), [("a", n.y.buf, n.y.c_off)]
            if i in self.pool_fused:    # BN + ReLU of the producing layer on the fly
                pn = self._pool_producer(n)
                pu = self.plan.unit_of[pn.idx]
                puid = pu.first.idx
                mean, inv = self._mean(pu, 0, m) + b.stats_shift, self._invstd(pu, 0, m) + b.stats_shift
                fn, lim = ((L.jr_bn_relu_maxpool3x3s2_fwd_grouped, ()) if b.guard is None
                           else (L.jr_bn_relu_maxpool3x3s2_fwd_grouped_guard, (b.guard,)))
                b.add(b.fwd, fn,
                      (ctypes.byref(d), self.dt, B, self.raw_unit[puid].data_ptr() + self.esz * m * self.raw_ms[puid],
                       mean, inv, self.stats_ms, self._beta(pn, m), self.nparam, yo, None) + lim + (s,),
                      "bn_relu_maxpool_fwd", ln, [("r", puid)] + self._frozen_reads(b), out)
            elif n.kind == "maxpool":
                b.add(b.fwd, L.jr_maxpool3x3s2_fwd, (ctypes.byref(d), self.dt, xi, yo, None, s), "maxpool_fwd", ln,
                      self._a_all(n.x), out)
            else:
                b.add(b.fwd, L.jr_avgpool3x3s1_fwd, (ctypes.byref(d), self.dt, xi, yo, s), "avgpool_fwd", ln,
                      self._a_all(n.x), out)

    def _fwd_head(self, b: Build) -> None:
        """The global average pool (per member for a partial batch) and each member's head."""
        L, g, M, B, s0 = self.lib, self.g, self.members, b.B, b.S[0]
        ob = g.bufs[g.output_buf]
        feat = [self.feat.data_ptr() + 4 * m * self.batch * ob.c for m in range(M)]
        if B == self.batch:
            b.add(b.fwd, L.jr_gap_fwd, (self.dt, self._A(g.output_buf), M * B, ob.h * ob.w, ob.c, feat[0], s0),
                  "gap_fwd", 0, self._a_all(g.output_buf), [("feat",)])
        else:
            for m in range(M):
                b.add(b.fwd, L.jr_gap_fwd, (self.dt, self._A(g.output_buf, m), B, ob.h * ob.w, ob.c, feat[m], s0),
                      "gap_fwd", 0, self._a_all(g.output_buf), [("feat",)])
        for m in range(M):
            o = 4 * m * self.batch * self.units
            b.add(b.fwd, L.jr_head_fwd, (self.head_mode, feat[m], self._p("dense/kernel", m), self._p("dense/bias", m),
                                         self.labels.data_ptr(), B, ob.c, self.units, self.logits.data_ptr() + o,
                                         self.probs.data_ptr() + o, self.loss.data_ptr() + 16 * m, s0), "head_fwd", 0,
                  [("feat",)], [("head",)])

    # ------------------------------------------------------------------- runs
    def set_batch(self, images, labels=None, augment=None, warp=None) -> int:
        """One batch for every member (NHWC uint8 or float32, host or device).
        augment, warp: jr.augment tables for a uint8 batch (jr.Engine.set_batch)
        -- one view of test-time augmentation."""
        B = int(images.shape[0])
        self._check_images(images, B)
        with torch.cuda.stream(self.stream):
            self._upload(images, labels, B, augment, warp)
            # every member reads the same images: copy member 0's
            ib, dst = self.g.bufs[self.g.input_buf], self.acts[self.g.input_buf]
            n, k = self.act_ms[self.g.input_buf], B * ib.h * ib.w * self.in_stride
            for m in range(1, self.members):
                dst[m * n:m * n + k].copy_(dst[:k])
        return B

    def bn_moving_numpy(self) -> List[dict]:
        """Every member's moving BN statistics by Keras name (jr.Engine.bn_moving_numpy)."""
        return self._bn_moving_get()

    def load_bn_moving(self, stats: List[dict]) -> None:
        """Every member's moving BN statistics (jr.checkpoint.load_bn_moving);
        non-finite values and negative variances are refused."""
        self._bn_moving_set(stats)

    def forward(self, B: Optional[int] = None, bn: str = "batch") -> None:
        calls, _ = self._build_calls(B or self.batch, frozen=self._check_frozen(bn))
        self.lanes.fork()            # every lane after the batch upload on lane 0
        self.lanes.run(calls)
        self.lanes.join()

    def synchronize(self) -> None:
        """Wait for lane 0 (every forward is joined onto it), then
        jr_device_check: device-side failures raise."""
        self.stream.synchronize()
        _ffi.device_check()

    def predictions(self, n: Optional[int] = None) -> np.ndarray:
        """[members, n, units] sigmoid (softmax) outputs of the last forward."""
        n = self.batch if n is None else n
        self.synchronize()
        p = self.probs.cpu().numpy().reshape(self.members, self.batch, self.units)
        return p[:, :n].copy()
