"""Learning-rate schedules (host only).

The value of a step is evaluated in numpy float32 in one stated order, from
integers and the flags alone, so every data-parallel rank computes bitwise the
same rate on any host (no libm pow: the staircase power is a chain of float32
multiplications).  The engine takes the result through Engine.set_lr, which
writes it to device memory ahead of the step (jr_opt_set_hyper).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np


def learning_rate(step: int, base: float, decay: Optional[Tuple[float, int]] = None, warmup: int = 0) -> np.float32:
    """The learning rate of optimizer step `step` (0-based), a numpy float32:

        lr = float32(base)
        decay = (rate, steps):  p = 1; floor(step / steps) times: p = p * float32(rate);  lr = lr * p
                                (an exponential staircase, base * rate ** floor(step / steps))
        step + 1 < warmup:      lr = lr * (float32(step + 1) / float32(warmup))
                                (linear from base / warmup at step 0; the factor is exactly 1 from step
                                warmup - 1 on, where the multiplication is left out)

    every operation rounded to float32."""
    f = np.float32
    step, warmup = int(step), int(warmup)
    if step < 0 or warmup < 0:
        raise ValueError("learning_rate: step and warmup must be >= 0")
    lr = f(base)
    if decay is not None:
        rate, steps = decay
        if int(steps) <= 0:
            raise ValueError("learning_rate: decay steps must be > 0")
        p = f(1)
        for _ in range(step // int(steps)):
            p = f(p * f(rate))
        lr = f(lr * p)
    if step + 1 < warmup:
        lr = f(lr * f(f(step + 1) / f(warmup)))
    return lr


def accum_groups(batches: int, accum_steps: int) -> Tuple[List[int], int]:
    """How an epoch of `batches` micro-batches falls into optimizer updates of
    `accum_steps` micro-batches each: (the group sizes in order, their number).
    Every group is full but the last, which holds the remainder and is closed
    at the end of the epoch (Engine.accum_flush); the number of updates,
    ceil(batches / accum_steps), is the epoch the schedule counts in."""
    batches, k = int(batches), int(accum_steps)
    if batches < 0 or k < 1:
        raise ValueError("accum_groups: batches >= 0 and accum_steps >= 1")
    sizes = [k] * (batches // k) + ([batches % k] if batches % k else [])
    return sizes, len(sizes)
