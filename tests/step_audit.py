"""Audit helpers for the training step's call lists (no tests here; see
test_step_audit.py for the CPU checks of these helpers and
test_gpu_step_audit.py for the audits of the engine).

jr.lanes.schedule orders the calls of a step by the resources they DECLARE
(Call.reads / Call.writes).  What memory each resource key names and which
device tensors an engine owns is the engines' own knowledge (jr.engine:
Replica.regions, Replica.universe, Region); this module drives a call list one call at a time over a shadow copy of that memory, so a
test can ask which bytes a call really wrote (write-set audit) and whether it
read anything it did not declare (read-set audit, by poisoning everything
else with quiet NaNs).  trace / first_difference digest every declared write
on the call's own lane without synchronising the host, to name the first call
at which two runs of the same step diverge.

Everything works on torch tensors, on the GPU for the engine and on the CPU
(tensors that share memory with numpy arrays) for the unit tests.

Convention, stated once: a declared write implies a read.  schedule() already
orders a writer behind the last writer of the same resource (WAW), which is
all an accumulating call needs (acc = 1 data gradients and pool backwards,
the optimizer on params / accum, the moving averages, the x6h magnitude
maxima), so the call lists name such regions in `writes` alone.  The read-set
audit therefore leaves a call's declared writes unpoisoned.  With
WRITE_IMPLIES_READ = False it poisons them too and every accumulating call
has to list what it reads.
"""
from __future__ import annotations

import bisect
import dataclasses
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from jr.engine import Region

WRITE_IMPLIES_READ = True

# quiet-NaN bit patterns by dtype, as (same-size integer dtype, pattern)
QNAN = {torch.float32: (torch.int32, 0x7FC00000), torch.bfloat16: (torch.int16, 0x7FC0)}
# resource keys of the conv / BN workspaces: scratch whose contents no later
# call relies on (and whose stream-K count words must stay zero: never
# poisoned, never restored, never compared)
SCRATCH_KEYS = ("ws", "wss")
MAX_FINDINGS = 20


# ---------------------------------------------------------------- exclusions
# per-lane raw-gradient scratch: sized for the largest launch, so a digest of
# the whole buffer also sees what earlier launches of THAT lane left behind --
# comparable between two runs of one list, not between a one- and a two-lane list
LANE_SCRATCH = ("draw", "draw2", "drawb", "drawp")


def never_poison(name: str, t: torch.Tensor) -> bool:
    """The read-set audit's exclusions: index and table buffers (a poisoned
    one would form addresses), the parameters, the workspaces (stream-K count
    words), and anything that is not fp32 / bf16."""
    if t.dtype not in QNAN:
        return True
    return name.startswith(("argmax", "params", "ws_lane", "ws_stem", "ig_target", "keep_table", "bn_table")) or \
        "table" in name or name.startswith("_")


def is_scratch(name: str) -> bool:
    return name.startswith(("ws_lane", "ws_stem"))


# ------------------------------------------------------------- shadow memory
class Memory:
    """A set of named flat tensors and byte-exact flat copies of them."""

    def __init__(self, tensors: Dict[str, torch.Tensor], sync: Callable[[], None] = lambda: None):
        self.names = list(tensors)
        self.tensors = [tensors[n].reshape(-1) for n in self.names]
        self.bytes = [t.view(torch.uint8) for t in self.tensors]
        self.esz = {n: t.element_size() for n, t in zip(self.names, self.tensors)}
        self.index = {n: k for k, n in enumerate(self.names)}
        self.off, o = [], 0
        for b in self.bytes:
            self.off.append(o)
            o += (b.numel() + 15) // 16 * 16
        self.total = max(o, 16)
        self.device = self.tensors[0].device
        self.sync = sync

    def new(self, fill: int = 0) -> torch.Tensor:
        return torch.full((self.total,), fill, dtype=torch.uint8, device=self.device)

    def segs(self, flat: torch.Tensor, names: Optional[Iterable[str]] = None) -> list:
        ks = range(len(self.names)) if names is None else [self.index[n] for n in names]
        return [flat[self.off[k]:self.off[k] + self.bytes[k].numel()] for k in ks]

    def snap(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = self.new() if out is None else out
        torch._foreach_copy_(self.segs(out), self.bytes)
        return out

    def write_back(self, flat: torch.Tensor, names: Sequence[str]) -> None:
        torch._foreach_copy_([self.bytes[self.index[n]] for n in names], self.segs(flat, names))

    def view(self, flat: torch.Tensor, r: Region) -> torch.Tensor:
        """The bytes of region r inside a flat copy."""
        k, z = self.index[r.name], self.esz[r.name]
        o = self.off[k] + r.start * z
        end = r.start + (r.rows - 1) * r.stride + r.width
        if end * z > self.bytes[k].numel():
            raise IndexError(f"region {r} runs past {r.name} ({self.bytes[k].numel() // z} elements)")
        if r.rows == 1:
            return flat[o:o + r.width * z]
        return flat.as_strided((r.rows, r.width * z), (r.stride * z, 1), o)

    def locate(self, byte: int) -> Tuple[str, int]:
        """(tensor name, element offset) of a byte of a flat copy."""
        k = bisect.bisect_right(self.off, byte) - 1
        return self.names[k], (byte - self.off[k]) // self.esz[self.names[k]]

    def poison(self, skip: Callable[[str, torch.Tensor], bool]) -> Tuple[torch.Tensor, torch.Tensor]:
        """(flat quiet-NaN image, base keep mask: 0xFF where nothing is ever poisoned)."""
        pois, keep = self.new(), self.new(0xFF)
        for n, t, seg_p, seg_k in zip(self.names, self.tensors, self.segs(pois), self.segs(keep)):
            if skip(n, t):
                continue
            idt, pat = QNAN[t.dtype]
            seg_p.view(idt).fill_(pat)
            seg_k.zero_()
        return pois, keep


def _first_bad(mem: Memory, x64: torch.Tensor, a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor):
    """First byte where a and b differ under mask, given the non-zero word image x64."""
    w = int(torch.nonzero(x64)[0])
    sl = slice(8 * w, 8 * w + 8)
    d = ((a[sl] ^ b[sl]) & mask[sl]).cpu().numpy()
    byte = 8 * w + int(np.nonzero(d)[0][0])
    return mem.locate(byte) + (int(torch.count_nonzero(x64)),)


class SerialAudit:
    """Issue a call list one call at a time, with a full synchronise after
    each, over a shadow copy of `tensors`.

    region_of(key) -> [Region]; calls: objects with fn, args, name, lane,
    idx, reads, writes ("param_ready" entries are skipped).  run() returns
    (write findings, read findings): strings naming the call index, name,
    lane, tensor, first offending element offset and, where one contains it,
    the resource of the call lists that element belongs to."""

    def __init__(self, tensors: Dict[str, torch.Tensor], region_of: Callable, sync: Callable[[], None],
                 skip_poison: Callable[[str, torch.Tensor], bool] = never_poison,
                 scratch: Callable[[str], bool] = is_scratch):
        self.mem = Memory(tensors, sync)
        self.region_of, self.sync = region_of, sync
        self.skip_poison = skip_poison
        self.restorable = [n for n in self.mem.names if not scratch(n)]
        self.scratch = scratch
        self.keys: list = []

    def _regions(self, keys, scratch: bool = True) -> List[Region]:
        out = []
        for k in keys:
            for r in self.region_of(k):
                if scratch or not self.scratch(r.name):
                    out.append(r)
        return out

    def _resource(self, name: str, elem: int) -> str:
        for k in self.keys:
            if any(r.name == name and r.contains(elem) for r in self.region_of(k)):
                return repr(k)
        return "no declared resource"

    def _where(self, c, what: str, name: str, elem: int, words: int) -> str:
        return (f"call {c.idx} {c.name} (lane {c.lane}) {what} {name}[{elem}], resource {self._resource(name, elem)}; "
                f"{words} 8-byte words differ; declared reads {list(c.reads)} writes {list(c.writes)}")

    def run(self, calls: Sequence, poison: bool = True) -> Tuple[List[str], List[str]]:
        mem, sync = self.mem, self.sync
        calls = [c for c in calls if c.fn != "param_ready"]
        seen = {}
        for c in calls:                     # every key must map: an unknown one is an error, here
            for k in tuple(c.reads) + tuple(c.writes):
                if k not in seen:
                    seen[k] = self.region_of(k)
        self.keys = list(seen)
        sync()
        shadow = mem.snap()
        cur, curp, tmp = mem.new(), mem.new(), mem.new()
        deny, chk = mem.new(0xFF), mem.new()
        for k in self.keys:                 # (bounds of every region, before anything runs)
            for r in seen[k]:
                mem.view(deny, r)
        if poison:
            pois, keep0 = mem.poison(self.skip_poison)
            keep, mixed = mem.new(), mem.new()
        i64 = lambda t: t.view(torch.int64)     # noqa: E731
        wfind, rfind = [], []
        for c in calls:
            rc = c.fn(*c.args)
            if rc:
                raise RuntimeError(f"call {c.idx} {c.name} returned {rc}")
            sync()
            mem.snap(cur)
            # a. what changed must lie inside the declared writes
            deny.fill_(0xFF)
            for r in self._regions(c.writes):
                mem.view(deny, r).zero_()
            torch.bitwise_xor(i64(cur), i64(shadow), out=i64(tmp))
            i64(tmp).bitwise_and_(i64(deny))
            if bool(i64(tmp).any()) and len(wfind) < MAX_FINDINGS:
                name, elem, words = _first_bad(mem, i64(tmp), cur, shadow, deny)
                wfind.append(self._where(c, "wrote outside its declared writes:", name, elem, words))
            if poison:
                # b. everything the call does not declare is quiet NaN; its
                # declared writes must come out as they just did
                keep.copy_(keep0)
                for r in self._regions(tuple(c.reads) + (tuple(c.writes) if WRITE_IMPLIES_READ else ())):
                    mem.view(keep, r).fill_(0xFF)
                torch.bitwise_and(i64(shadow), i64(keep), out=i64(mixed))
                i64(keep).bitwise_not_()
                i64(keep).bitwise_and_(i64(pois))
                i64(mixed).bitwise_or_(i64(keep))
                mem.write_back(mixed, self.restorable)
                sync()
                rc = c.fn(*c.args)
                if rc:
                    raise RuntimeError(f"call {c.idx} {c.name} returned {rc} on poisoned memory")
                sync()
                mem.snap(curp)
                chk.zero_()
                for r in self._regions(c.writes, scratch=False):
                    mem.view(chk, r).fill_(0xFF)
                torch.bitwise_xor(i64(cur), i64(curp), out=i64(tmp))
                i64(tmp).bitwise_and_(i64(chk))
                if bool(i64(tmp).any()) and len(rfind) < MAX_FINDINGS:
                    name, elem, words = _first_bad(mem, i64(tmp), cur, curp, chk)
                    rfind.append(self._where(c, "read something it does not declare; differs at", name, elem, words))
                mem.write_back(cur, self.restorable)
                sync()
            shadow, cur = cur, shadow
        return wfind, rfind


def engine_audit(engine, lists, poison: bool = True, phases=(0, 1, 2)) -> Tuple[List[str], List[str]]:
    """SerialAudit over a jr.Engine's call lists (a _build_calls tuple), in issue order."""
    calls = [c for p in phases for c in (lists[p] or ())]
    audit = SerialAudit(engine.universe(lists), lambda k: engine.regions(k, lists), torch.cuda.synchronize)
    return audit.run(calls, poison)


# ---------------------------------------------------- first-divergence trace
@dataclasses.dataclass
class Trace:
    rows: List[tuple]           # (step, call index, call name, lane, resource)
    values: np.ndarray          # int64 digest per row


def digest(v: torch.Tensor, ramp: torch.Tensor) -> torch.Tensor:
    """A 64-bit integer digest of a tensor's bits (position-weighted sum mod 2^64)."""
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[v.element_size()]
    x = v.view(idt).reshape(-1).to(torch.int64)
    return (x * ramp[:x.numel()]).sum()


def region_view(t: torch.Tensor, r: Region) -> torch.Tensor:
    t = t.reshape(-1)
    if r.rows == 1:
        return t[r.start:r.start + r.width]
    return t.as_strided((r.rows, r.width), (r.stride, 1), t.storage_offset() + r.start)


class Tracer:
    """Wraps the calls of a jr.Engine's lists so that each, right after its
    launch and on ITS lane's stream, digests its declared writes (workspaces
    excepted) into a device table; nothing synchronises the host until
    result()."""

    def __init__(self, engine, lists, steps: int):
        self.engine, self.steps, self.step = engine, steps, 0
        uni = engine.universe(lists)
        self.rows, self.phases = [], []
        n = 1
        for p in range(3):
            wrapped = []
            for c in lists[p] or ():
                if c.fn == "param_ready":
                    continue
                views = []
                for k in c.writes:
                    if k[0] in SCRATCH_KEYS:
                        continue
                    vs = [region_view(uni[r.name], r) for r in engine.regions(k, lists)]
                    n = max(n, max(v.numel() for v in vs))
                    views.append((len(self.rows), vs))
                    self.rows.append((c.idx, c.name, c.lane, k))
                wrapped.append(dataclasses.replace(c, fn=self._wrap(c, views)))
            self.phases.append(wrapped)
        dev = engine.device
        self.ramp = 2 * torch.arange(n, dtype=torch.int64, device=dev) + 1
        self.table = torch.zeros(steps * len(self.rows), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

    def _wrap(self, c, views):
        stream = self.engine.lane_streams[c.lane]

        def fn(*args):
            rc = c.fn(*args)
            if rc or not views:
                return rc
            base = self.step * len(self.rows)
            with torch.cuda.stream(stream):
                for row, vs in views:
                    d = digest(vs[0], self.ramp)
                    for v in vs[1:]:
                        d = d * 1000003 + digest(v, self.ramp)
                    self.table[base + row] = d
            return 0
        fn.__name__ = getattr(c.fn, "__name__", "fn")
        return fn

    def run_step(self, serial: bool = False) -> None:
        """One training step: as Engine.train_step issues it (fork, forward,
        join, backward, join, update), or one call at a time with every lane
        synchronised after each."""
        ln = self.engine.lanes
        if serial:
            for p in self.phases:
                for c in p:
                    rc = c.fn(*c.args)
                    if rc:
                        raise RuntimeError(f"call {c.idx} {c.name} returned {rc}")
                    for st in ln.streams:
                        st.synchronize()
        else:
            ln.fork()
            ln.run(self.phases[0])
            ln.join()
            ln.run(self.phases[1])
            ln.join()
            ln.run(self.phases[2])
        self.step += 1

    def result(self) -> Trace:
        self.engine.synchronize()
        torch.cuda.synchronize(self.engine.device)
        rows = [(s,) + r for s in range(self.steps) for r in self.rows]
        return Trace(rows, self.table.cpu().numpy())


def trace(engine, lists, steps: int, feed: Callable[[int], None], serial: bool = False) -> Trace:
    """The trace of `steps` training steps of one call-list build (a
    _build_calls tuple of `engine`): feed(k) uploads step k's batch, the step
    runs on the lanes (serial: one call at a time).  What to run, twice, when
    a bitwise test of the step next fails: first_difference names the call."""
    tr = Tracer(engine, lists, steps)
    for k in range(steps):
        feed(k)
        tr.run_step(serial)
    return tr.result()


def first_difference(t1: Trace, t2: Trace, skip_kinds: Sequence[str] = ()) -> Optional[dict]:
    """None when the traces agree; else the first row (issue order) where
    they do not: step, call index, name, lane and resource of both.  Rows are
    matched by position; a different call name at a position is itself the
    difference (resources and lanes may differ between a one- and a two-lane
    list: only the digests are compared).  skip_kinds: resource kinds whose
    digests are not compared (LANE_SCRATCH between lists of different lane
    counts; what is computed from them is compared)."""
    n = min(len(t1.rows), len(t2.rows))
    for k in range(n):
        a, b = t1.rows[k], t2.rows[k]
        if a[:3] == b[:3] and a[4][0] in skip_kinds and b[4][0] in skip_kinds:
            continue
        if a[:3] != b[:3] or int(t1.values[k]) != int(t2.values[k]):
            return {"step": a[0], "call": a[1], "name": a[2], "lane": (a[3], b[3]), "resource": (a[4], b[4]),
                    "digest": (int(t1.values[k]), int(t2.values[k]))}
    if len(t1.rows) != len(t2.rows):
        return {"step": None, "call": n, "name": "length", "lane": None, "resource": None,
                "digest": (len(t1.rows), len(t2.rows))}
    return None
