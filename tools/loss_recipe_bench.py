"""Dropout and the loss recipe against the step they sit in, on one GPU.

  python tools/loss_recipe_bench.py [--batch 64] [--res 299] [--rounds 5] [--calls 12] [--launches 20]

The method of tools/opt_recipe_bench.py (one process, everything resident,
interleaved round by round; profiles/loss_recipe.txt is this script's output):
  1. kernels alone at the step's sizes (batch x 2048 features, one unit):
     jr_dropout_fwd, jr_dropout_bwd (8 B per element each), jr_dropout_advance,
     jr_head_fwd + jr_head_bwd and their _ex forms with label smoothing, and
     with a class weight and a focal term.  Device events around `launches`
     back-to-back launches; one launch (pair) is reported;
  2. the eager fp32 x6h training step without the keywords (the call lists of
     an engine that has none: tests/golden/call_signatures.json pins them) and
     with dropout=0.2, label_smoothing=0.1.  Host clock around a step that ends
     in a synchronise of every lane.
"""
import argparse
import ctypes
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
        raise SystemExit("loss_recipe_bench needs the GPU: nothing is measured without one")
    from jr import _ffi, synth
    from jr.engine import Engine
    _ffi.init(0)
    L = _ffi.load()
    B, c, units = a.batch, 2048, 1
    n = B * c
    print(f"n = {B} x {c} = {n} features, {units} unit; 3 warm-ups, median of {a.calls} calls per round, "
          f"{a.rounds} rounds, interleaved in one process\n", flush=True)

    gen = torch.Generator(device="cuda").manual_seed(0)
    F = torch.rand(n, device="cuda", generator=gen)
    FD, DF = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    W = torch.randn(c * units, device="cuda", generator=gen) * 0.05
    bias, Y = torch.zeros(units, device="cuda"), (torch.arange(B * units, device="cuda") % 2).float()
    Z, P, loss = torch.zeros(B * units, device="cuda"), torch.zeros(B * units, device="cuda"), torch.zeros(4, device="cuda")
    DW, DB = torch.zeros(c * units, device="cuda"), torch.zeros(units, device="cuda")
    state = torch.zeros(8, device="cuda")
    _ffi.check("dropout_set", L.jr_dropout_set(state.data_ptr(), 0, 0, 0.2, 0, None))
    p = lambda t: t.data_ptr()     # noqa: E731

    def spec(eps, weight, gamma):
        s = _ffi.LossSpec(eps, gamma)
        for u in range(16):
            s.class_weight[u] = weight if u < units else 1.0
        return s
    smooth, focal = spec(0.1, 1.0, 0.0), spec(0.1, 3.5, 2.0)

    def head():
        _ffi.check("head_fwd", L.jr_head_fwd(0, p(F), p(W), p(bias), p(Y), B, c, units, p(Z), p(P), p(loss), None))
        _ffi.check("head_bwd", L.jr_head_bwd(0, p(F), p(W), p(P), p(Y), B, c, units, p(DF), p(DW), p(DB), None))

    def head_ex(s):
        def run():
            sp = ctypes.byref(s)
            _ffi.check("head_fwd_ex", L.jr_head_fwd_ex(0, sp, p(F), p(W), p(bias), p(Y), B, c, units, p(Z), p(P), p(loss),
                                                       None))
            _ffi.check("head_bwd_ex", L.jr_head_bwd_ex(0, sp, p(Z), p(F), p(W), p(P), p(Y), B, c, units, p(DF), p(DW),
                                                       p(DB), None))
        return run

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
        "jr_dropout_fwd": events(lambda: _ffi.check("dropout_fwd", L.jr_dropout_fwd(p(F), p(FD), n, p(state), None))),
        "jr_dropout_bwd": events(lambda: _ffi.check("dropout_bwd", L.jr_dropout_bwd(p(DF), n, p(state), None))),
        "jr_dropout_advance": events(lambda: _ffi.check("dropout_advance", L.jr_dropout_advance(p(state), None))),
        "jr_head_fwd + jr_head_bwd": events(head),
        "_ex, label smoothing 0.1": events(head_ex(smooth)),
        "_ex, smoothing, weight 3.5, gamma 2": events(head_ex(focal)),
    }
    print("kernels alone (device events, us per launch or pair of launches)")
    k = interleave(kernels, a.rounds, a.calls, "us")
    drop = k["jr_dropout_fwd"][0] + k["jr_dropout_bwd"][0] + k["jr_dropout_advance"][0]
    print(f"  dropout's three launches = {drop:.3f} us; the _ex head with label smoothing - the plain head = "
          f"{k['_ex, label smoothing 0.1'][0] - k['jr_head_fwd + jr_head_bwd'][0]:+.3f} us\n", flush=True)

    res = a.res
    x = synth.fundus_batch(0, B, res)
    y = (np.arange(B) % 2).astype(np.float32).reshape(B, 1)
    engines = {"keywords off": {}, "dropout 0.2, label smoothing 0.1": dict(dropout=0.2, label_smoothing=0.1)}
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
    print(f"  keywords on - off = {on[0] - off[0]:+.3f} ms = {100 * (on[0] - off[0]) / off[0]:+.2f} % "
          f"(off spread {off[1]:.3f} ms)")


if __name__ == "__main__":
    main()
