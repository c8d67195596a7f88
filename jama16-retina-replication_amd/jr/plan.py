"""Launch plan of the conv layers and the engine's internal parameter layout.

Sibling fusion: in every Inception block several 1x1 'same' conv2d_bn
layers read the SAME input buffer (mixed0-2: the 64 / 48 / 64 branch heads,
mixed4-7: 192 / c7 / c7, mixed8: 192 / 192, mixed9-10: 320 / 384 / 448; see
SURVEY.md App. A).  They are one GEMM with N = sum of their c_out: the
engine stores their kernels side by side as one [c_in][sum c_out] block, so
one implicit-GEMM launch computes all of them forward, one writes all their
filter gradients, and one computes their summed data gradient (instead of
one accumulate-into-dx launch per layer).  Each member keeps its own
BatchNormalization (per-channel, so the group's statistics are the members'
statistics), its own beta and its own output slice.  The arithmetic per
output element is unchanged: each output channel is still the dot product of
the same input pixel with the same kernel column.

Internal layout: the flat fp32 parameter buffer holds the tensors in Keras
creation order (jr.init.param_layout), except that a fused group's kernel
block and all its members' betas sit together at the position of the group's
first kernel.  Backward visits the layers in reverse order, so every byte at
offsets >= the offset of the layer just finished is final — the invariant
the bucketed all-reduce (jr.dist) relies on — and the group's parameters
all become final at once, when the group's backward runs.  Checkpoints,
params_numpy() and grads_numpy() use the Keras layout; to_internal /
to_keras convert.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from . import _ffi
from .inception import ConvNode, Graph
from .init import ALIGN, param_layout


@dataclass
class ConvUnit:
    """One implicit-GEMM conv launch: one conv2d_bn layer or a fused group."""
    members: List[ConvNode]
    col_off: List[int]
    koff: int = 0                     # internal offset of the kernel block
    soff: int = 0                     # offset of its [mean(c) | invstd(c)] block in the statistics layout

    @property
    def first(self) -> ConvNode:
        return self.members[0]

    @property
    def fused(self) -> bool:
        return len(self.members) > 1

    @property
    def cout(self) -> int:
        return sum(n.cout for n in self.members)

    @property
    def name(self) -> str:
        if not self.fused:
            return self.first.name
        return "conv2d_" + "+".join(str(n.idx + 1) for n in self.members)

    def __getattr__(self, k):          # geometry shared by all members
        if k in ("x", "cin", "kh", "kw", "stride", "padding", "h", "w", "ho", "wo", "pad_h", "pad_w"):
            return getattr(self.members[0], k)
        raise AttributeError(k)

    def macs_per_image(self) -> int:
        return sum(n.macs_per_image() for n in self.members)


@dataclass
class Plan:
    units: List[ConvUnit]
    unit_of: Dict[int, ConvUnit]                  # conv idx -> unit
    layout: List[Tuple[str, tuple, int, int]]     # internal (name, shape, off, size)
    nparam: int
    poff: Dict[str, int]                          # contiguous tensors: betas, dense, unfused kernels
    kview: Dict[str, Tuple[int, int, int, int, int]] = field(default_factory=dict)
    # conv kernel name -> (block offset, row stride, column offset, rows, cols)
    # the statistics layout, per member: one block [mean(c) | invstd(c)] per conv launch at its
    # ConvUnit.soff, launches in plan order.  The batch statistics, `frozen` (the same layout) and
    # `moving` ([moving_mean(c) | moving_var(c)]) all use these offsets; build_plan is their one home
    stats_size: int = 0

    def bn_layers(self):
        """(conv2d_bn layer, offset of its mean / moving_mean, offset of its invstd / moving_var)."""
        for u in self.units:
            for n, co in zip(u.members, u.col_off):
                yield n, u.soff + co, u.soff + u.cout + co

    def to_internal(self, g: Graph, flat: np.ndarray) -> np.ndarray:
        keras, total = param_layout(g.params)
        flat = np.asarray(flat, np.float32)
        if flat.size != total:
            raise ValueError(f"expected {total} parameters (Keras layout), got {flat.size}")
        out = np.zeros(self.nparam, np.float32)
        for name, shape, off, size in keras:
            src = flat[off:off + size]
            if name in self.kview:
                o, ld, co, rows, cols = self.kview[name]
                out[o:o + rows * ld].reshape(rows, ld)[:, co:co + cols] = src.reshape(rows, cols)
            else:
                o = self.poff[name]
                out[o:o + size] = src
        return out

    def to_keras(self, g: Graph, flat: np.ndarray) -> np.ndarray:
        keras, total = param_layout(g.params)
        flat = np.asarray(flat, np.float32)
        out = np.zeros(total, np.float32)
        for name, shape, off, size in keras:
            if name in self.kview:
                o, ld, co, rows, cols = self.kview[name]
                out[off:off + size] = flat[o:o + rows * ld].reshape(rows, ld)[:, co:co + cols].ravel()
            else:
                o = self.poff[name]
                out[off:off + size] = flat[o:o + size]
        return out


def sibling_groups(g: Graph) -> List[List[ConvNode]]:
    """1x1 stride-1 conv2d_bn layers reading the same buffer, >= 2 of them."""
    by_input: Dict[int, List[ConvNode]] = {}
    for n in g.convs:
        if n.kh == 1 and n.kw == 1 and n.stride == 1:
            by_input.setdefault(n.x, []).append(n)
    return [v for v in by_input.values() if len(v) > 1]


def build_plan(g: Graph, fuse_siblings: bool = True) -> Plan:
    groups = sibling_groups(g) if fuse_siblings else []
    unit_of: Dict[int, ConvUnit] = {}
    for mem in groups:
        offs, c = [], 0
        for n in mem:
            offs.append(c)
            c += n.cout
        u = ConvUnit(list(mem), offs)
        for n in mem:
            unit_of[n.idx] = u
    units = []
    for n in g.convs:
        if n.idx not in unit_of:
            unit_of[n.idx] = ConvUnit([n], [0])
        u = unit_of[n.idx]
        if u.first is n:
            units.append(u)

    shapes = dict(g.params)
    layout, poff, kview = [], {}, {}
    off = 0

    def alloc(name, shape, size):
        nonlocal off
        layout.append((name, tuple(shape), off, size))
        o = off
        off += (size + ALIGN - 1) // ALIGN * ALIGN
        return o

    conv_by_name = {n.name: n for n in g.convs}
    done = set()
    for name, shape in g.params:
        if name in done:
            continue
        base = name.split("/")[0]
        n = conv_by_name.get(base)
        if n is not None and unit_of[n.idx].fused:
            u = unit_of[n.idx]
            rows = n.kh * n.kw * n.cin
            u.koff = alloc(u.name + "/kernel", (n.kh, n.kw, n.cin, u.cout), rows * u.cout)
            for m, co in zip(u.members, u.col_off):
                kview[f"{m.name}/kernel"] = (u.koff, u.cout, co, rows, m.cout)
                done.add(f"{m.name}/kernel")
            for m in u.members:
                bname = f"batch_normalization_{m.idx + 1}/beta"
                poff[bname] = alloc(bname, shapes[bname], m.cout)
                done.add(bname)
            continue
        size = int(np.prod(shape))
        o = alloc(name, shape, size)
        poff[name] = o
        if n is not None and name.endswith("/kernel"):
            unit_of[n.idx].koff = o
    soff = 0
    for u in units:
        u.soff = soff
        soff += 2 * u.cout
    return Plan(units, unit_of, layout, off, poff, kview, soff)


def decay_ranges(plan: Plan) -> List[Tuple[int, int]]:
    """Sorted, disjoint element ranges [begin, end) of the internal parameter
    buffer that L2 weight decay covers: every conv filter block (a fused
    group's shared block included) and the dense kernel.  BN betas, the dense
    bias and the alignment padding between tensors are never decayed; blocks
    that touch are merged into one range."""
    out: List[Tuple[int, int]] = []
    for name, _, off, size in sorted(plan.layout, key=lambda e: e[2]):
        if not name.endswith("/kernel") or size == 0:
            continue
        if out and out[-1][1] == off:
            out[-1] = (out[-1][0], off + size)
        else:
            out.append((off, off + size))
    return out


def bn_moving_segments(units: List[ConvUnit], batch: int) -> List[Tuple[int, int, int, int]]:
    """(stats offset, moving offset, rows, c) per conv launch: the segment
    table of jr_bn_moving_update / jr_bn_moving_freeze at this batch.  The
    statistics and the moving layout share their offsets (Plan.stats_size).
    A launch with fewer than two rows (n * ho * wo) has no unbiased variance:
    refused."""
    segs = []
    for u in units:
        rows = int(batch) * u.ho * u.wo
        if rows < 2:
            raise ValueError(f"BN moving statistics need at least 2 rows per channel: {u.name} has "
                             f"{rows} at batch {batch} ({u.ho}x{u.wo} outputs)")
        segs.append((u.soff, u.soff, rows, u.cout))
    return segs


def bn_batch_groups(g: Graph, plan: Plan, batch: int, vec_width: int, fused_bufs) -> List[List[ConvUnit]]:
    """Conv launches whose BN backwards become due together: every member
    writes a slice of one block buffer (several producing launches: the
    branch-final layers of an Inception block), one launch set per launch
    and at most 512 reduce chunks (jr_bn_plan: single_stage), not the stem's
    pooled layers (fused_bufs); blocks with two or more.  vec_width: 4 (fp32)
    or 8 (bf16) channels per 16-byte vector."""
    dtype = _ffi.JR_BF16 if vec_width == 8 else _ffi.JR_F32
    producers: Dict[int, set] = {}
    for u in plan.units:
        for m in u.members:
            producers.setdefault(m.y.buf, set()).add(u.first.idx)
    for n in g.nodes:
        if n.kind != "conv":
            producers.setdefault(n.y.buf, set()).add(("pool", id(n)))
    fused = set(fused_bufs)
    groups: Dict[int, list] = {}
    for u in plan.units:
        bufs = {m.y.buf for m in u.members}
        if len(bufs) != 1:
            continue
        buf = next(iter(bufs))
        p = _ffi.bn_plan(dtype, batch * u.ho * u.wo, u.cout)    # None: more than one launch set
        if len(producers[buf]) < 2 or buf in fused or buf == g.output_buf or p is None or not p.single_stage:
            continue
        groups.setdefault(buf, []).append(u)
    return [grp for grp in groups.values() if len(grp) >= 2]
