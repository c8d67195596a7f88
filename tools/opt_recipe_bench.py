"""The device optimizer recipe against the by-value update, on one GPU.

  python tools/opt_recipe_bench.py [--batch 64] [--res 299] [--rounds 5] [--calls 12] [--launches 20]

One process, everything resident and interleaved round by round
(profiles/opt_recipe.txt is this script's output):
  1. kernels alone at the model's parameter count, with its real decay ranges:
     jr_nesterov_update (by value), jr_nesterov_update_ex (weight decay on,
     and with no range table: the kernel without its lookup),
     jr_grad_sqnorm + jr_opt_prepare.  Device events around `launches`
     back-to-back launches; the time of one launch is reported;
  2. the eager fp32 x6h training step, recipe off against recipe on
     (weight_decay + clip_norm).  Host clock around a step that ends in a
     synchronise of every lane.
3 warm-up passes; per round the median of `calls` calls; the median over rounds
and their spread (max - min) are reported.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jama16-retina-replication_amd"))


def interleave(cases, rounds, calls, unit):
    """cases: name -> fn returning one time.  Prints one line per case."""
    for fn in cases.values():
        for _ in range(3):
            fn()
    med = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            med[k].append(float(np.median([fn() for _ in range(calls)])))
    out = {}
    for k, v in med.items():
        out[k] = (float(np.median(v)), max(v) - min(v))
        print(f"  {k:<34} median per round ({unit}) " + " ".join(f"{t:8.3f}" for t in v) +
              f" -> median {out[k][0]:8.3f}, spread {out[k][1]:.3f}", flush=True)
    return out


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
        raise SystemExit("opt_recipe_bench needs the GPU: nothing is measured without one")
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
    A = torch.zeros(n, device="cuda")
    R = torch.tensor(ranges, dtype=torch.int64, device="cuda")
    ws = L.jr_grad_sqnorm_workspace_size(n)
    part = torch.zeros(ws // 8, dtype=torch.float64, device="cuda")
    hyper, step = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    _ffi.check("set_hyper", L.jr_opt_set_hyper(hyper.data_ptr(), 1e-6, 4e-5, 2.0, 1.0, None))
    p = lambda t: t.data_ptr()

    def norm():
        _ffi.check("sqnorm", L.jr_grad_sqnorm(p(G), n, p(part), ws, None))
        _ffi.check("prepare", L.jr_opt_prepare(p(part), n, p(hyper), p(step), None))
    norm()

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
        "jr_nesterov_update (by value)": events(lambda: _ffi.check("nesterov", L.jr_nesterov_update(
            p(W), p(G), p(A), n, 1e-6, 0.9, 1.0, None))),
        "jr_nesterov_update_ex (decay on)": events(lambda: _ffi.check("nesterov_ex", L.jr_nesterov_update_ex(
            p(W), p(G), p(A), n, 0.9, p(R), len(ranges), p(hyper), p(step), None))),
        "jr_grad_sqnorm + jr_opt_prepare": events(norm),
        "jr_nesterov_update_ex (no ranges)": events(lambda: _ffi.check("nesterov_ex", L.jr_nesterov_update_ex(
            p(W), p(G), p(A), n, 0.9, None, 0, p(hyper), p(step), None))),
    }
    print("kernels alone (device events, us per launch)")
    k = interleave(kernels, a.rounds, a.calls, "us")
    leg, ex, nm = (k[name] for name in list(kernels)[:3])
    print(f"  update: 20 B per element = {20 * n / 1e6:.1f} MB -> by value {20 * n / leg[0] / 1e6:.2f} TB/s, "
          f"_ex {20 * n / ex[0] / 1e6:.2f} TB/s; _ex - by value = {ex[0] - leg[0]:+.3f} us "
          f"(by-value spread {leg[1]:.3f} us)")
    print(f"  norm: {4 * n / 1e6:.1f} MB read -> {4 * n / nm[0] / 1e6:.2f} TB/s\n", flush=True)
    del W, G, A
    torch.cuda.empty_cache()

    B, res = a.batch, a.res
    x = synth.fundus_batch(0, B, res)
    y = (np.arange(B) % 2).astype(np.float32).reshape(B, 1)
    engines = {"recipe off": {}, "recipe on (decay + clip)": dict(weight_decay=4e-5, clip_norm=2.0)}
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
    off, on = (s[name] for name in engines)
    print(f"  recipe on - off = {on[0] - off[0]:+.3f} ms = {100 * (on[0] - off[0]) / off[0]:+.2f} % "
          f"(off spread {off[1]:.3f} ms)")


if __name__ == "__main__":
    main()
