"""numpy restatements of the device metrics and the step log (TEST ORACLE ONLY).

jr_metrics_accumulate, jr_metrics_reset and jr_step_log_append as
include/jr.h states them: integer counts (any order gives the same integers),
the Brier sums in the one fp64 order of jr_brier_accumulate, and the ring
record of one step.
"""
import numpy as np

f32 = np.float32

STEP_REC = np.dtype([("loss", "<f4"), ("grad_norm", "<f4"), ("scale", "<f4"), ("flags", "<u4")])
CHUNK = 1024        # include/jr.h JR_METRICS_CHUNK


def counts_ref(probs, labels, thr) -> np.ndarray:
    """uint32 [4, T] (tp, fp, fn, tn) of one call: positive iff p > thr as an
    fp32 comparison (NaN: negative), the label true iff y != 0."""
    p = np.asarray(probs, f32).reshape(-1)
    y = np.asarray(labels, f32).reshape(-1) != f32(0)
    thr = np.asarray(thr, f32).reshape(-1)
    with np.errstate(invalid="ignore"):
        pos = p[None, :] > thr[:, None]                 # [T, n]
    y = y[None, :]
    return np.stack([np.count_nonzero(pos & y, axis=1), np.count_nonzero(pos & ~y, axis=1),
                     np.count_nonzero(~pos & y, axis=1), np.count_nonzero(~pos & ~y, axis=1)]).astype(np.uint32)


def brier_block_sum(probs, labels) -> np.float64:
    """The block's sum of jr_brier_accumulate: thread t adds elements t, t +
    256, ... in ascending order in fp64, then the 256 partials fold as a
    tree (o = 128 .. 1: r[t] += r[t + o])."""
    p = np.asarray(probs, f32).reshape(-1).astype(np.float64)
    y = np.asarray(labels, f32).reshape(-1).astype(np.float64)
    d = p - y
    q = d * d
    n = q.size
    rows = -(-n // 256)
    pad = np.zeros(rows * 256, np.float64)
    pad[:n] = q
    valid = (np.arange(rows * 256) < n).reshape(rows, 256)
    r = np.zeros(256, np.float64)
    with np.errstate(all="ignore"):
        for k, row in enumerate(pad.reshape(rows, 256)):
            r = np.where(valid[k], r + row, r)        # a thread past n adds nothing (not even + 0.0)
        o = 128
        while o:
            r[:o] = r[:o] + r[o:2 * o]
            o >>= 1
    return np.float64(r[0])


def brier_ref(acc, probs, labels) -> np.ndarray:
    """jr_brier_accumulate / which bit 1: the new double[2]."""
    acc = np.array(acc, np.float64)
    with np.errstate(all="ignore"):
        acc[0] = acc[0] + brier_block_sum(probs, labels)
    acc[1] = acc[1] + np.float64(np.asarray(probs).size)
    return acc


def metrics_accumulate_ref(counts, brier, probs, labels, thr, which=3):
    """jr_metrics_accumulate: (counts, brier) after the call, as new arrays."""
    counts, brier = np.array(counts, np.uint32), np.array(brier, np.float64)
    if which & 1:
        counts = counts + counts_ref(probs, labels, thr)        # uint32: wraps like the device add
    if which & 2:
        brier = brier_ref(brier, probs, labels)
    return counts, brier


def metrics_reset_ref(T):
    return np.zeros((4, T), np.uint32), np.zeros(2, np.float64)


def step_log_append_ref(ring, cursor, loss, step=None):
    """jr_step_log_append on a STEP_REC ring: the new cursor (the ring is
    updated in place).  step: None or (scale, grad_norm, skipped)."""
    cap = len(ring)
    slot = cursor % cap
    if step is None:
        ring[slot] = (f32(loss), f32(0), f32(0), 0)
    else:
        scale, norm, skipped = step
        ring[slot] = (f32(loss), f32(norm), f32(scale), 1 | (2 if skipped else 0))
    return (cursor + 1) & 0xFFFFFFFF
