"""The state of a loop that runs ahead of the host: the
streaming metrics on the device (Metrics), the ring of per-step records
(StepLog) and the two-slot pinned input feed (Feed).  The engine builds each
when it is first asked for (Engine.metrics_init, step_log_enable,
set_batch(staged=True)) and keeps what needs the engine: its buffers, its
stream and the synchronise before a read.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _ffi
from .augment import PARAM_DTYPE, WARP_DTYPE

# include/jr.h jr_step_rec
STEP_REC = np.dtype([("loss", "<f4"), ("grad_norm", "<f4"), ("scale", "<f4"), ("flags", "<u4")])


class Metrics:
    """jr_metrics_*: the fp32 threshold table, the uint32 [4][T] counts (tp,
    fp, fn, tn) and the Brier double[2] (sum, samples), zeroed."""

    def __init__(self, eng, thresholds):
        thr = np.ascontiguousarray(np.asarray(thresholds, np.float32).reshape(-1))
        if not 1 <= thr.size <= 1024:
            raise ValueError("metrics_init: 1..1024 thresholds")
        self.lib, self.T = eng.lib, int(thr.size)
        self.thr = eng._after_fill(torch.from_numpy(thr).to(eng.device))
        self.counts, self.brier = eng._t(4 * thr.size, torch.int32), eng._t(2, torch.float64)

    def accumulate(self, probs: int, labels: int, n: int, counts: bool, brier: bool, s) -> None:
        which = int(bool(counts)) | 2 * int(bool(brier))
        if which:
            _ffi.check("jr_metrics_accumulate", self.lib.jr_metrics_accumulate(
                probs, labels, n, self.thr.data_ptr(), self.T, self.counts.data_ptr(), self.brier.data_ptr(), which, s))

    def reset(self, s) -> None:
        _ffi.check("jr_metrics_reset", self.lib.jr_metrics_reset(self.counts.data_ptr(), self.T, self.brier.data_ptr(),
                                                                 s))

    def read(self) -> Tuple[np.ndarray, float, float]:
        """(uint32 [4, T] counts, the Brier sum, the sample count) of what has completed."""
        s, n = (float(v) for v in self.brier.cpu().numpy())
        return self.counts.cpu().numpy().view(np.uint32).reshape(4, self.T), s, n


class StepLog:
    """jr_step_log_append: a device ring of `capacity` jr_step_rec and its
    cursor; the host counts what it appended and what it has read."""

    def __init__(self, eng, capacity: int):
        self.lib, self.cap = eng.lib, int(capacity)
        if self.cap < 1:
            raise ValueError("step_log_enable: capacity >= 1")
        self.ring, self.cursor = eng._t(4 * self.cap, torch.int32), eng._t(1, torch.int32)
        self.appended = self.read = 0

    def append(self, loss: int, step, s) -> None:
        """One record: the loss at `loss`, the jr_opt_step at `step` (None: no update ran)."""
        if self.appended - self.read >= self.cap:
            raise RuntimeError(f"step log full: {self.cap} records unread (call step_log_read() at least every "
                               f"{self.cap} steps, or enable a larger ring)")
        _ffi.check("jr_step_log_append", self.lib.jr_step_log_append(
            self.ring.data_ptr(), self.cap, self.cursor.data_ptr(), loss, step, s))
        self.appended += 1

    def take(self) -> np.ndarray:
        """The records appended since the last take, oldest first (after a synchronise)."""
        idx = np.arange(self.read, self.appended) % self.cap
        self.read = self.appended
        return self.ring.cpu().numpy().view(STEP_REC)[idx].copy()


class Feed:
    """Two slots, each one pinned host buffer and one device staging tensor of
    the same layout: labels, the jr_augment_param and jr_warp_param tables
    (sized for the planned batch, 256-byte aligned), then the uint8 pixels --
    so one copy of the used prefix, on the feed's own stream, moves a batch."""

    def __init__(self, device, batch: int, units: int, image_bytes: int):
        al = lambda v: (v + 255) // 256 * 256   # noqa: E731
        self.off_y = 0
        self.off_a = al(4 * batch * units)
        self.off_w = self.off_a + al(batch * PARAM_DTYPE.itemsize)
        self.off_x = self.off_w + al(batch * WARP_DTYPE.itemsize)
        nbytes = self.off_x + batch * image_bytes
        self.pin = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.host = [p.numpy() for p in self.pin]
        self.dev = [torch.empty(nbytes, dtype=torch.uint8, device=device) for _ in range(2)]
        self.stream = torch.cuda.Stream(device=device)
        self.copied = [torch.cuda.Event() for _ in range(2)]
        # recorded on the consumer's stream after the step that read the slot; waited for before its refill
        self.consumed = [torch.cuda.Event() for _ in range(2)]
        self.busy, self.last = [False, False], None

    def load(self, stream, pixels, labels=None, tab=None, wtab=None) -> torch.Tensor:
        """A batch (uint8 pixels, float32 labels, the two tables; None: absent)
        into the free slot, its copy enqueued, `stream` waiting for the copy;
        returns the slot's device tensor.  What `stream` was given since the
        last load consumed that load's slot, and a slot is refilled only after
        the event recorded behind its consumer: at most two steps in flight."""
        if self.last is not None:
            self.consumed[self.last].record(stream)
            self.busy[self.last] = True
        s = 0 if self.last is None else 1 - self.last
        if self.busy[s]:
            self.consumed[s].synchronize()
            self.busy[s] = False
        host, end = self.host[s], self.off_x + pixels.size
        for off, part in ((self.off_x, pixels), (self.off_y, labels), (self.off_a, tab), (self.off_w, wtab)):
            if part is not None:
                host[off:off + part.nbytes] = np.ascontiguousarray(part).view(np.uint8).reshape(-1)
        with torch.cuda.stream(self.stream):
            self.dev[s][:end].copy_(self.pin[s][:end], non_blocking=True)
        self.copied[s].record(self.stream)
        stream.wait_event(self.copied[s])
        self.last = s
        return self.dev[s]
