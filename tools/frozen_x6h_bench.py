"""Frozen-BN forward and input gradient, x8 against guarded x6h, on one GPU.

  python tools/frozen_x6h_bench.py [--members 10] [--batch 32] [--res 299] [--rounds 5] [--calls 12]

One process, the engines of both arithmetics resident and interleaved round
by round (profiles/frozen_x6h.txt is this script's output):
  1. EnsembleEngine, `members` members: forward(bn="frozen"), x8 (what
     evaluate.py --bn moving runs) against x6h with x6h_frozen=True;
  2. one Engine: the same forward;
     (1 and 2 also time forward() with batch statistics, the unguarded lists,
     so the cost of the guard itself can be read off the x6h lines)
  3. one Engine(input_grad=True): input_gradient() after a frozen forward.
Host clock around work that ends in a synchronise of the engine's lane 0 (every
call list is joined onto it); 3 warm-up passes; per round the median of `calls`
calls; the median over rounds and their spread (max - min) are reported.
Random initialisation (seeds 0..members-1), synthetic images, the statistics of
freeze_bn("batch") -- the timing does not depend on the values.  After every
round jr_device_check must be clean (the guard never tripped).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jama16-retina-replication_amd"))


def timed(fn, sync, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def interleave(cases, rounds, calls):
    """cases: name -> (fn, sync, check).  Prints one line per case."""
    for fn, sync, _ in cases.values():
        for _ in range(3):
            fn()
            sync()
    med = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (fn, sync, check) in cases.items():
            med[k].append(timed(fn, sync, calls))
            check()
    for k, v in med.items():
        print(f"  {k:<28} median per round (ms) " + " ".join(f"{t:8.3f}" for t in v) +
              f" -> median {np.median(v):8.3f}, spread {max(v) - min(v):.3f}", flush=True)
    return {k: float(np.median(v)) for k, v in med.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=299)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=12)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("frozen_x6h_bench needs the GPU: nothing is measured without one")
    from jr import synth
    from jr.engine import Engine
    from jr.ensemble import EnsembleEngine
    from jr.inception import build_inception_v3
    from jr.init import init_params
    B, res = a.batch, a.res
    x = synth.fundus_batch(0, B, res)
    maths = {"x8": dict(conv_math="x8"), "x6h guarded": dict(conv_math="x6h", x6h_frozen=True)}
    print(f"{res}^2, B = {B}, conv tiles pinned; 3 warm-ups, median of {a.calls} calls per round, {a.rounds} rounds, "
          "interleaved in one process\n", flush=True)

    g = build_inception_v3(res, res)
    params = [init_params(g, s) for s in range(a.members)]
    cases, batch, keep = {}, {}, []
    for name, kw in maths.items():
        e = EnsembleEngine(params, B, res, res, tiles="pinned", **kw)
        e.set_batch(x)
        e.forward()
        e.freeze_bn("batch")
        e.synchronize()
        keep.append(e)
        cases[name] = ((lambda e=e: e.forward(bn="frozen")), e.stream.synchronize, e.synchronize)
        batch[name] = ((lambda e=e: e.forward()), e.stream.synchronize, e.synchronize)
        print(f"  ({name}: tiles {e.tiles})")
    print(f"EnsembleEngine, {a.members} members: forward() with batch statistics (unguarded, for reference)")
    interleave(batch, a.rounds, a.calls)
    print(f"EnsembleEngine, {a.members} members: forward(bn='frozen')")
    m = interleave(cases, a.rounds, a.calls)
    print(f"  images/s (members x batch / time): x8 {a.members * B / m['x8'] * 1e3:.0f}, "
          f"x6h guarded {a.members * B / m['x6h guarded'] * 1e3:.0f}; x6h / x8 time {m['x6h guarded'] / m['x8']:.4f}\n",
          flush=True)
    del cases, batch, keep, e
    torch.cuda.empty_cache()

    fwd, grad, batch, keep = {}, {}, {}, []
    for name, kw in maths.items():
        e = Engine(B, res, res, seed=0, train=False, tiles="pinned", input_grad=True, **kw)
        e.set_batch(x)
        e.forward()
        e.freeze_bn("batch")
        e.forward(bn="frozen")
        e.synchronize()
        keep.append(e)
        fwd[name] = ((lambda e=e: e.forward(bn="frozen")), e.stream.synchronize, e.synchronize)
        grad[name] = ((lambda e=e: e.input_gradient()), e.stream.synchronize, e.synchronize)
        batch[name] = ((lambda e=e: e.forward()), e.stream.synchronize, e.synchronize)
        print(f"  ({name}: tiles {e.tiles})")
    print("Engine: forward() with batch statistics (unguarded, for reference)")
    interleave(batch, a.rounds, a.calls)
    for e in keep:      # input_gradient needs the frozen forward to be the last one
        e.forward(bn="frozen")
    print("Engine: forward(bn='frozen')")
    m = interleave(fwd, a.rounds, a.calls)
    print(f"  x6h / x8 time {m['x6h guarded'] / m['x8']:.4f}\n")
    print("Engine(input_grad=True): input_gradient() after a frozen forward")
    m = interleave(grad, a.rounds, a.calls)
    print(f"  x6h / x8 time {m['x6h guarded'] / m['x8']:.4f}")


if __name__ == "__main__":
    main()
