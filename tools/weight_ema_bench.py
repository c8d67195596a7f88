"""The weight average and RMSProp against the updates they sit beside, on one GPU.

  python tools/weight_ema_bench.py [--batch 64] [--res 299] [--rounds 5] [--calls 12] [--launches 20]

The method of tools/opt_recipe_bench.py (one process, everything resident,
interleaved round by round; profiles/weight_ema.txt is this script's output):
  1. kernels alone at the model's parameter count, with its real decay ranges:
     jr_nesterov_update (20 B per element), jr_ema_prepare + jr_ema_update
     (12 B), jr_adam_update_ex and jr_rmsprop_update_ex (28 B each).  Device
     events around `launches` back-to-back launches; one launch is reported,
     and the achieved bytes per second of each pair;
  2. the eager fp32 x6h training step with the average off and on, and on
     RMSProp with the average on.  Host clock around a step that ends in a
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
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("weight_ema_bench needs the GPU: nothing is measured without one")
    from jr import _ffi, synth
    from jr.engine import Engine
    from jr.inception import build_inception_v3
    from jr.plan import build_plan, decay_ranges
    _ffi.init(0)
    L = _ffi.load()
    plan = build_plan(build_inception_v3(a.res, a.res))
    n, ranges = plan.nparam, decay_ranges(plan)
    print(f"n = {n} parameters, {len(ranges)} decay ranges; 3 warm-ups, median of {a.calls} calls per round, "
          f"{a.rounds} rounds, interleaved in one process\n", flush=True)

    gen = torch.Generator(device="cuda").manual_seed(0)
    W, G = (torch.randn(n, device="cuda", generator=gen) * 0.05 for _ in range(2))
    A, V, S = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda"), torch.zeros(n, device="cuda")
    R = torch.tensor(ranges, dtype=torch.int64, device="cuda")
    ws = L.jr_grad_sqnorm_workspace_size(n)
    part = torch.zeros(ws // 8, dtype=torch.float64, device="cuda")
    hyper, step, ema = (torch.zeros(4, device="cuda") for _ in range(3))
    _ffi.check("set_hyper", L.jr_opt_set_hyper(hyper.data_ptr(), 1e-6, 4e-5, 2.0, 1.0, None))
    _ffi.check("ema_set", L.jr_ema_set(ema.data_ptr(), 0.9999, 1, 0, None))
    p = lambda t: t.data_ptr()     # noqa: E731
    _ffi.check("sqnorm", L.jr_grad_sqnorm(p(G), n, p(part), ws, None))
    _ffi.check("prepare", L.jr_opt_prepare(p(part), n, p(hyper), p(step), None))

    def average():
        _ffi.check("ema_prepare", L.jr_ema_prepare(p(ema), p(step), None))
        _ffi.check("ema_update", L.jr_ema_update(p(S), p(W), n, p(ema), p(step), None))

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
    kernels = {
        "jr_nesterov_update (by value)": (20, events(lambda: _ffi.check("nesterov", L.jr_nesterov_update(
            p(W), p(G), p(A), n, 1e-6, 0.9, 1.0, None)))),
        "jr_ema_prepare + jr_ema_update": (12, events(average)),
        "jr_adam_update_ex (decay on)": (28, events(lambda: _ffi.check("adam_ex", L.jr_adam_update_ex(
            p(W), p(G), p(A), p(V), n, 0.9, 0.999, 1e-8, p(R), len(ranges), p(hyper), p(step), None)))),
        "jr_rmsprop_update_ex (decay on)": (28, events(lambda: _ffi.check("rmsprop_ex", L.jr_rmsprop_update_ex(
            p(W), p(G), p(A), p(V), n, 0.9, 0.9, 1.0, p(R), len(ranges), p(hyper), p(step), None)))),
    }
    print("kernels alone (device events, us per launch)")
    k = interleave({name: fn for name, (_, fn) in kernels.items()}, a.rounds, a.calls, "us")
    rate = {name: b * n / k[name][0] / 1e6 for name, (b, _) in kernels.items()}
    for name, (b, _) in kernels.items():
        print(f"  {name:<34} {b} B per element = {b * n / 1e6:.1f} MB -> {rate[name]:.2f} TB/s")
    nes, avg, adam, rms = (rate[name] for name in kernels)
    print(f"  jr_ema_update / jr_nesterov_update bytes per second = {avg / nes:.3f} (expected >= 0.9)")
    print(f"  jr_rmsprop_update_ex / jr_adam_update_ex bytes per second = {rms / adam:.3f} (expected >= 0.9)\n", flush=True)
    del W, G, A, V, S
    torch.cuda.empty_cache()

    B, res = a.batch, a.res
    x = synth.fundus_batch(0, B, res)
    y = (np.arange(B) % 2).astype(np.float32).reshape(B, 1)
    engines = {"average off": {}, "average on": dict(weight_ema=0.9999),
               "rmsprop recipe, average on": dict(optimizer="rmsprop", weight_decay=4e-5, clip_norm=2.0,
                                                  weight_ema=0.9999)}
    steps = {}
    for name, kw in engines.items():
        e = Engine(B, res, res, seed=0, conv_math="x6h", tiles="pinned", lr=1e-4, **kw)
        e.set_batch(x, y)

        def one(e=e):
            t0 = time.perf_counter()
            e.train_step()
            e.synchronize()
            return (time.perf_counter() - t0) * 1e3
        steps[name] = one
        print(f"  ({name}: tiles {e.tiles})")
    print(f"eager fp32 x6h training step, {res}^2, B = {B} (host clock, ms per step)")
    s = interleave(steps, a.rounds, a.calls, "ms")
    off, on, full = (s[name] for name in engines)
    print(f"  average on - off = {on[0] - off[0]:+.3f} ms = {100 * (on[0] - off[0]) / off[0]:+.2f} % "
          f"(off spread {off[1]:.3f} ms)")
    print(f"  rmsprop recipe with the average - plain step = {full[0] - off[0]:+.3f} ms = "
          f"{100 * (full[0] - off[0]) / off[0]:+.2f} %")


if __name__ == "__main__":
    main()
