"""Gradient accumulation against the step it sits in, on one GPU.

  python tools/accum_bench.py [--batch 64] [--res 299] [--rounds 5] [--calls 12] [--launches 20] [--k 4]

The method of tools/opt_recipe_bench.py (one process, everything resident,
interleaved round by round; profiles/accum.txt is this script's output):
  1. kernels alone at nparam = 21,770,401 floats: jr_grad_accumulate with
     first = 0 (12 B per element) and first = 1 (8 B per element), on 16-byte
     aligned buffers and on a pair off by 4 bytes (the single-element path),
     beside jr_ema_update -- the parent's kernel with the same loop and the
     same 12 B per element, the yardstick.  Device events around `launches`
     back-to-back launches; one launch is reported;
  2. the eager fp32 x6h training step with accum_steps = 1 against the mean
     micro-step of a whole group at accum_steps = K (K - 1 accumulating
     micro-steps and the closing one).  Host clock around steps that end in a
     synchronise of every lane.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jama16-retina-replication_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from opt_recipe_bench import interleave  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--res", type=int, default=299)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--k", type=int, default=4)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench needs the GPU: nothing is measured without one")
    from jr import _ffi, synth
    from jr.engine import Engine
    _ffi.init(0)
    L = _ffi.load()
    n = 21770401
    print(f"n = {n} floats; 3 warm-ups, median of {a.calls} calls per round, {a.rounds} rounds, interleaved in one "
          f"process\n", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    G = torch.randn(n + 4, device="cuda", generator=gen)
    A = torch.randn(n + 4, device="cuda", generator=gen)
    W = torch.randn(n, device="cuda", generator=gen)
    state = torch.zeros(4, device="cuda")
    _ffi.check("ema_set", L.jr_ema_set(state.data_ptr(), 0.9999, 0, 100, None))
    _ffi.check("ema_prepare", L.jr_ema_prepare(state.data_ptr(), None, None))
    p = lambda t, off=0: t.data_ptr() + 4 * off     # noqa: E731

    def events(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.launches
        return run

    def acc(first, off=0):
        return events(lambda: _ffi.check("grad_accumulate", L.jr_grad_accumulate(p(A, off), p(G, off), n, first, None)))
    kernels = {
        "jr_ema_update (12 B / element)": events(lambda: _ffi.check("ema_update", L.jr_ema_update(
            p(A), p(W), n, state.data_ptr(), None, None))),
        "jr_grad_accumulate first=0 (12 B)": acc(0),
        "jr_grad_accumulate first=1 (8 B)": acc(1),
        "  first=0, both off by 4 bytes": acc(0, 1),
        "  first=1, both off by 4 bytes": acc(1, 1),
    }
    print("kernels alone (device events, us per launch)")
    k = interleave(kernels, a.rounds, a.calls, "us")
    ema, add, cp = (k[name] for name in list(kernels)[:3])
    print(f"  accumulate - ema_update = {add[0] - ema[0]:+.3f} us (spreads {add[1]:.3f} / {ema[1]:.3f}); "
          f"12 B x n / median = {12 * n / add[0] / 1e6:.2f} TB/s, the copy {8 * n / cp[0] / 1e6:.2f} TB/s\n", flush=True)

    B, res, K = a.batch, a.res, a.k
    x = synth.fundus_batch(0, B, res)
    y = (np.arange(B) % 2).astype(np.float32).reshape(B, 1)
    steps = {}
    for name, kw, per in (("accum_steps = 1", {}, 1), (f"accum_steps = {K}, mean micro-step", dict(accum_steps=K), K)):
        e = Engine(B, res, res, seed=0, conv_math="x6h", tiles="pinned", lr=1e-4, **kw)
        e.set_batch(x, y)

        def one(e=e, per=per):
            t0 = time.perf_counter()
            for _ in range(per):
                e.train_step()
                e.synchronize()
            return (time.perf_counter() - t0) * 1e3 / per
        steps[name] = one
        print(f"  ({name}: tiles {e.tiles})")
    print(f"eager fp32 x6h training step, {res}^2, B = {B} (host clock, ms per micro-step)")
    s = interleave(steps, a.rounds, a.calls, "ms")
    off, on = (s[name] for name in steps)
    print(f"  K = {K} mean micro-step - K = 1 step = {on[0] - off[0]:+.3f} ms = {100 * (on[0] - off[0]) / off[0]:+.2f} % "
          f"(K = 1 spread {off[1]:.3f} ms)")


if __name__ == "__main__":
    main()
