"""Branch-level concurrency of the Inception step: lanes (HIP streams) and
the event dependencies between them.

An Inception block runs 3-4 independent branches between its input buffer
and its concat-free output slices, and from mixed4 on the
branch layers are small (17x17, 8x8 at batch 64): a few hundred workgroups
and a few microseconds each, latency- rather than throughput-bound on 256
CUs.  Running the branches on separate streams lets the hardware overlap
them (inside a captured HIP graph the cross-stream event waits become graph
edges).

* node_lanes: a launch that reads a buffer written by exactly one launch
  continues that launch's lane (the first such reader does; further readers
  of the same producer fork onto new lanes); readers of block buffers (several
  producers: the concat-free block outputs) start new lanes round-robin.
  Backward calls of a node run on its forward lane.
* schedule: every call declares the resources it reads and writes
  (activation / gradient channel slices, raw outputs and statistics of a
  launch, per-launch gradient regions, per-lane scratch, ...).  Over the
  whole step's call sequence (forward, backward, update in issue order) each
  call waits for the last writer of what it reads or writes and for the
  readers since that write of what it writes (RAW, WAW, WAR) -- when those run
  on another lane (by waiting for that lane's tail); same-lane order is
  stream order.  (Eager runs wait for the producing call itself instead of
  the other lane's tail: Call.pwaits.)  Accumulating writers of
  one gradient buffer are therefore serialised in issue order, so the result
  is bitwise the single-stream result.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

from . import _ffi


@dataclass
class Call:
    fn: object
    args: tuple
    name: str
    lane: int = 0
    reads: Tuple = ()
    writes: Tuple = ()
    idx: int = -1                                   # position in the step's call sequence
    waits: List[int] = field(default_factory=list)  # lanes whose work so far must finish first
    nbytes: int = 0                                 # algorithmic HBM bytes (memory-bound ops; bench.py)
    # producer waits (eager runs): (lane, call index) pairs -- wait for THAT
    # call of the other lane (an event recorded right after it), not for
    # everything the host had issued there by then; record: this call is
    # such a producer
    pwaits: List[Tuple[int, int]] = field(default_factory=list)
    record: bool = False


def node_lanes(g, plan, nl: int) -> Dict[int, int]:
    """Graph node index -> lane in [0, nl)."""
    if nl <= 1:
        return {i: 0 for i in range(len(g.nodes))}
    index = {id(n): i for i, n in enumerate(g.nodes)}

    def launch_of(i):                      # node that issues node i's launch
        n = g.nodes[i]
        return index[id(plan.unit_of[n.idx].first)] if n.kind == "conv" else i

    producers: Dict[int, set] = {}
    for i, n in enumerate(g.nodes):
        producers.setdefault(n.y.buf, set()).add(launch_of(i))
    lane: Dict[int, int] = {}
    taken = set()
    rr = 0
    for i, n in enumerate(g.nodes):
        li = launch_of(i)
        if li != i:
            lane[i] = lane[li]
            continue
        p = producers.get(n.x, set())
        src = next(iter(p)) if len(p) == 1 else None
        if src is not None and src not in taken:
            taken.add(src)
            lane[i] = lane[src]
        else:
            lane[i] = rr % nl
            rr += 1
    return lane


def schedule(calls: Sequence[Call]) -> None:
    """Number the calls and fill in the lanes each must wait for.  A wait is
    on the TAIL of the other lane at issue time (an event recorded there just
    before the wait), which covers every call issued on that lane so far; a
    lane already waited for at a tail at or past the needed call is skipped.
    (Waiting on an event recorded earlier, while its stream has since moved
    on, made hipGraphInstantiate crash with three or more lanes on ROCm 7.2;
    tail events are also what the fork / join of a step use.)"""
    last_w: Dict[object, int] = {}
    readers: Dict[object, List[int]] = {}
    tail: Dict[int, int] = {}                       # lane -> newest call issued on it
    synced: Dict[Tuple[int, int], int] = {}         # (lane, other lane) -> other lane's tail when last waited for
    psynced: Dict[Tuple[int, int], int] = {}        # the same for the producer waits
    for i, c in enumerate(calls):
        c.idx = i
        c.waits = []
        c.pwaits = []
        c.record = False
    for i, c in enumerate(calls):
        dep = set()
        for k in c.reads:
            if k in last_w:
                dep.add(last_w[k])
        for k in c.writes:
            if k in last_w:
                dep.add(last_w[k])
            dep.update(readers.get(k, ()))
        for k in c.reads:
            readers.setdefault(k, []).append(i)
        for k in c.writes:
            last_w[k] = i
            readers[k] = []
        need: Dict[int, int] = {}
        for j in dep:
            lj = calls[j].lane
            if lj != c.lane:
                need[lj] = max(need.get(lj, -1), j)
        for lj, j in sorted(need.items()):
            if psynced.get((c.lane, lj), -1) < j:   # (a wait for j' >= j on lane lj covers j)
                psynced[(c.lane, lj)] = j
                c.pwaits.append((lj, j))
                calls[j].record = True
            if synced.get((c.lane, lj), -1) >= j:
                continue                            # already waited for a tail at or past j
            synced[(c.lane, lj)] = tail[lj]
            c.waits.append(lj)
        tail[c.lane] = i


class Build:
    """The state of one call-list build: stream and workspace handles per
    lane, the node -> lane map, the ctypes objects the calls point into
    (keep), the phase lists and the step's issue order (seq), and what the
    backward carries from launch to launch."""

    def __init__(self, B: int, lanes: "Lanes", nl: int, ws_lane, ws_bytes: int, lane_of: Dict[int, int],
                 flush_points: Sequence[int] = ()):
        self.B = B
        self.S = lanes.handles[:nl]
        self.WS = [ctypes.c_void_p(w.data_ptr()) for w in ws_lane[:nl]]
        self.wsb = ctypes.c_size_t(ws_bytes)
        self.lane_of = lane_of
        self.keep: list = []
        self.fwd, self.bwd, self.opt, self.seq = [], [], [], []
        self.split_done = set()         # x8p: input buffers whose operand planes are written
        self.written = set()            # gradient buffers written so far (later writers accumulate)
        self.defer: Dict[int, tuple] = {}   # deferred filter gradients: launch -> (WgradSeg, arena offset, bytes)
        self.pending: list = []         # (WgradSeg, launch) awaiting the next jr_wgrad_reduce
        self.flush_at = list(flush_points)
        self.sbuf = self.bset = 0       # alternating raw-gradient buffers: the stem's, the batched BN backwards'
        self.batch_draw: Dict[int, tuple] = {}      # batched BN backwards: launch -> (raw gradient, its resource)
        # frozen BN (forward(bn="frozen")): byte distance from the batch statistics
        # to the frozen ones, added to what every BN apply and fused pool reads
        self.stats_shift = 0
        # ... and, for JR_F32_X6H under frozen statistics, the limit of the guarded
        # BN applies and fused pools (None: the unguarded entry points)
        self.guard = None
        # the lists of a training step with dropout on (Engine._build_calls(training=True))
        self.training = False
        # gradient accumulation (Engine(accum_steps=K > 1)): the update phase of a micro-batch that
        # opens, continues ("inside") or closes its group, or of accum_flush; None: the default one
        self.accum = None

    def add(self, lst, fn, args, name, lane, reads=(), writes=(), nbytes=0) -> None:
        c = Call(fn, args, name, lane, tuple(reads), tuple(writes), nbytes=int(nbytes))
        lst.append(c)
        self.seq.append(c)


class Lanes:
    """The lanes of one engine: their HIP streams (lane 0 is where every step
    starts and ends), the events between them, and the flat loop that issues
    a call list on them."""

    def __init__(self, lib, device, n: int, priorities: Sequence[int] = ()):
        import torch
        self.lib, self.n = lib, max(1, int(n))
        prio = list(priorities) + [0] * self.n
        self.streams = [torch.cuda.Stream(device=device, priority=prio[i]) for i in range(self.n)]
        self.handles = [ctypes.c_void_p(st.cuda_stream) for st in self.streams]
        self._fork_ev = torch.cuda.Event()
        self._join_ev = [torch.cuda.Event() for _ in range(self.n - 1)]
        self._tail_ev = [torch.cuda.Event() for _ in range(self.n)]
        self._fence_ev = [torch.cuda.Event() for _ in range(self.n)]
        # eager runs: a cross-lane consumer waits for its producing call (an
        # event recorded right after it) instead of the other lane's tail
        # (JR_PRECISE_WAITS=0: tail waits; capturing: set while a graph
        # capture is to use tail waits too)
        self.precise_waits = os.environ.get("JR_PRECISE_WAITS", "1") != "0"
        self.capturing = False
        self.join_each = os.environ.get("JR_DP_JOIN_EACH", "0") == "1"
        # producer events by call index: libjr's (no timing, no system-scope
        # fence: cheaper to record), created on first use, or torch's
        # (JR_LANE_EVENTS=torch, for A/B runs)
        self.native_ev = os.environ.get("JR_LANE_EVENTS", "native") != "torch"
        self._prod_ev: Dict[int, object] = {}

    def _new_event(self):
        if not self.native_ev:
            import torch
            return torch.cuda.Event()
        ev = ctypes.c_void_p()
        _ffi.check("jr_event_create", self.lib.jr_event_create(ctypes.byref(ev)))
        weakref.finalize(self, self.lib.jr_event_destroy, ev)
        return ev

    def fork(self) -> None:
        """Every lane waits for the work enqueued on lane 0 so far."""
        if self.n > 1:
            self._fork_ev.record(self.streams[0])
            for st in self.streams[1:]:
                st.wait_event(self._fork_ev)

    def join(self) -> None:
        """Lane 0 waits for every other lane's work enqueued so far."""
        for ev, st in zip(self._join_ev, self.streams[1:]):
            ev.record(st)
            self.streams[0].wait_event(ev)

    def fence(self, stream) -> None:
        """`stream` (a consumer outside the lanes) waits for the work enqueued
        on EVERY lane so far; the lanes themselves wait for nothing."""
        for ev, st in zip(self._fence_ev, self.streams):
            ev.record(st)
            stream.wait_event(ev)

    def run(self, calls: Sequence[Call], hook=None) -> None:
        streams, handles, tail_ev, prod_ev = self.streams, self.handles, self._tail_ev, self._prod_ev
        native, precise = self.native_ev, self.precise_waits and not self.capturing
        for c in calls:
            if c.fn == "param_ready":
                # no join here: the hook fences the lanes onto ITS stream, and
                # only when a bucket is actually issued (fence); lane 0 never
                # waits for lane 1 at a conv unit
                if hook is not None:
                    if self.join_each:      # round-5 behaviour, A/B runs only (JR_DP_JOIN_EACH=1)
                        self.join()
                    hook(c.args)
                continue
            st = streams[c.lane]
            if precise:
                for lj, j in c.pwaits:      # the producing call on the other lane (schedule)
                    ev = prod_ev.get(j)
                    if ev is None:          # producer never run in this process (e.g. backward() first): its tail
                        ev = tail_ev[lj]
                        ev.record(streams[lj])
                        st.wait_event(ev)
                    elif native:
                        _ffi.check("jr_stream_wait_event", self.lib.jr_stream_wait_event(handles[c.lane], ev))
                    else:
                        st.wait_event(ev)
            else:
                for lj in c.waits:          # the other lane's tail (schedule)
                    ev = tail_ev[lj]
                    ev.record(streams[lj])
                    st.wait_event(ev)
            rc = c.fn(*c.args)
            if rc:
                raise _ffi.JRError(c.name, rc, _ffi.last_error())
            if c.record and precise:
                ev = prod_ev.get(c.idx)
                if ev is None:
                    ev = prod_ev[c.idx] = self._new_event()
                if native:
                    _ffi.check("jr_event_record", self.lib.jr_event_record(ev, handles[c.lane]))
                else:
                    ev.record(st)


def _sig_arg(v) -> str:
    if isinstance(v, float) or (isinstance(v, int) and abs(v) < 2 ** 31):
        return repr(v)
    if isinstance(v, ctypes.c_size_t):
        return repr(v.value)
    return "N" if v is None else "P"    # P: pointers, byref, ctypes structs


def signature(calls: Sequence[Call]) -> str:
    """Canonical pointer-free text of a call sequence, one line per Call in
    list order: what is launched, where, after what, with which scalars
    (tests/test_gpu_call_signature.py pins the step's schedule with it)."""
    lines = []
    for c in calls:
        args = c.args if isinstance(c.args, tuple) else (c.args,)
        fn = c.fn if isinstance(c.fn, str) else getattr(c.fn, "__name__", repr(c.fn))
        lines.append(f"{c.name} {fn} lane={c.lane} idx={c.idx} reads={list(c.reads)} writes={list(c.writes)} "
                     f"waits={sorted(c.waits)} pwaits={list(c.pwaits)} record={c.record} nbytes={c.nbytes} "
                     f"args=({','.join(_sig_arg(v) for v in args)})")
    return "\n".join(lines) + "\n"


def check_schedule(calls: Sequence[Call], precise: bool = False) -> None:
    """Test helper: every pair of conflicting calls on different lanes is
    ordered by a chain of same-lane order and tail waits (precise: producer
    waits) -- happens-before."""
    hb: List[Dict[int, int]] = []
    last_on_lane: Dict[int, int] = {}
    for i, c in enumerate(calls):
        known: Dict[int, int] = {}
        prev = last_on_lane.get(c.lane)
        if prev is not None:
            known = dict(hb[prev])
            known[c.lane] = max(known.get(c.lane, -1), prev)
        targets = ([(lj, j) for lj, j in c.pwaits] if precise
                   else [(lj, last_on_lane.get(lj)) for lj in c.waits])
        for lj, t in targets:
            assert lj != c.lane
            if t is None:
                continue
            if precise:
                assert calls[t].lane == lj and calls[t].record and t < i
            for l2, k in hb[t].items():
                known[l2] = max(known.get(l2, -1), k)
            known[lj] = max(known.get(lj, -1), t)
        hb.append(known)
        last_on_lane[c.lane] = i
    for i, ci in enumerate(calls):
        wi, ri = set(ci.writes), set(ci.reads)
        for j in range(i):
            cj = calls[j]
            if cj.lane == ci.lane:
                continue
            if (wi & (set(cj.writes) | set(cj.reads))) or (ri & set(cj.writes)):
                assert hb[i].get(cj.lane, -1) >= j, (cj.name, j, ci.name, i)
