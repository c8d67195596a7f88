"""The host's driving order of a training step, pinned: for eight scenarios
(eager, data-parallel through a stub all-reduce, accumulated, Adam, captured
and replayed) the sequence of Lanes.fork / join / run, of the stub's begin /
param_ready / finish and of the eager library calls that surround a step
(jr_opt_set_hyper, jr_step_log_append, jr_graph_begin / _end / _launch) must
equal the recorded one in tests/golden/step_traces.json, and so must the
host's bookkeeping after every action (Engine.updates, accum_pending(), and
the update's scale on the device optimizer path).  107^2, B = 4, the sizes of
test_gpu_call_signature.py; a call list is recorded as the sha256 of its
jr.lanes.signature.

Only public seams are wrapped -- the three jr.lanes.Lanes methods and
attributes of the loaded library object -- and every wrapper calls through:
nothing is skipped on the device.

`python tests/test_gpu_step_trace.py` rewrites the fixture from the code as it
stands (a deliberate change of the driving order).
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "step_traces.json")
RES, B = 107, 4
LIB_CALLS = ("jr_opt_set_hyper", "jr_step_log_append", "jr_graph_begin", "jr_graph_end", "jr_graph_launch")

# name -> (constructor keywords, all-reduce stub?, step log capacity or None, actions)
# actions: "step", "flush", "capture", "replay", ("set_lr", value)
SCENARIOS = {
    "a_eager": (dict(), False, None, ["step", "step"]),
    "b_allreduce": (dict(), True, None, ["step", "step"]),
    "c_allreduce_clip_bn_log_lr": (dict(clip_norm=1.0, bn_moving=0.99), True, 8, ["step", ("set_lr", 1e-3), "step"]),
    "d_accum3": (dict(accum_steps=3), False, None, ["step"] * 4 + ["flush"]),
    "e_accum3_allreduce_clip": (dict(accum_steps=3, clip_norm=1.0), True, None, ["step"] * 4 + ["flush"]),
    "f_adam": (dict(optimizer="adam"), False, None, ["step", "step"]),
    "g_capture_replay": (dict(), False, None, ["capture", "replay", "replay"]),
    "h_accum3_clip_capture_replay": (dict(accum_steps=3, clip_norm=1.0), False, None, ["capture"] + ["replay"] * 4),
}


class StubAllReduce:
    """A duck-typed all-reduce of a world of two that exchanges nothing."""

    def __init__(self, events):
        self.events, self.ready = events, 0

    def begin(self, eng=None, fold=False):
        self.ready = 0
        self.events.append(["begin", {"fold": bool(fold)}])

    def param_ready(self, offset):
        self.ready += 1

    def finish(self, eng=None):
        self.events += [["param_ready", self.ready], ["finish"]]
        return 0.5


@contextlib.contextmanager
def recording(lib, events):
    """Wrap the seams; every wrapper records and calls through."""
    from jr import lanes
    saved = [(lanes.Lanes, n, getattr(lanes.Lanes, n)) for n in ("fork", "join", "run")]
    saved += [(lib, n, getattr(lib, n)) for n in LIB_CALLS]
    fork, join, run = (fn for _, _, fn in saved[:3])

    def rec_fork(self):
        events.append(["fork"])
        return fork(self)

    def rec_join(self):
        events.append(["join"])
        return join(self)

    def rec_run(self, calls, hook=None):
        sha = hashlib.sha256(lanes.signature(calls).encode()).hexdigest()
        events.append(["run", sha, hook is not None])
        return run(self, calls, hook)

    def lib_call(name, fn):
        def wrapper(*args):
            if name == "jr_opt_set_hyper":      # (hyper, lr, weight_decay, clip_norm, grad_scale, stream)
                events.append([name, [float(v) for v in args[1:5]]])
            elif name == "jr_step_log_append":  # (ring, capacity, cursor, loss, step, stream)
                events.append([name, {"step_is_null": args[4] is None}])
            else:
                events.append([name])
            return fn(*args)
        return wrapper

    try:
        lanes.Lanes.fork, lanes.Lanes.join, lanes.Lanes.run = rec_fork, rec_join, rec_run
        for _, n, fn in saved[3:]:
            setattr(lib, n, lib_call(n, fn))
        yield
    finally:
        for obj, n, fn in saved:
            setattr(obj, n, fn)


def run_scenario(name):
    """The events of one scenario, as the JSON fixture holds them."""
    from jr import synth
    from jr.engine import Engine
    from test_gpu_call_signature import _clear_overrides
    kw, stub, log_cap, actions = SCENARIOS[name]
    _clear_overrides("f32", "x8", [B])
    e = Engine(B, RES, RES, tiles="heuristic", seed=1, conv_math="x8", **kw)
    if log_cap is not None:
        e.step_log_enable(log_cap)
    e.set_batch(synth.fundus_batch(40, B, RES), synth.labels(40, B, p=0.5))
    events = []
    ar = StubAllReduce(events) if stub else None
    with recording(e.lib, events):
        for act in actions:
            events.append(["action", act if isinstance(act, str) else list(act)])
            if act == "step":
                e.train_step(B, allreduce=ar)
            elif act == "flush":
                e.accum_flush(allreduce=ar)
            elif act == "capture":
                e.capture(B)
            elif act == "replay":
                e.replay(B)
            else:
                e.set_lr(act[1])
            events.append(["state", {"updates": int(e.updates), "pending": int(e.accum_pending()),
                                     "scale": float(e.opt_step()[1]) if e.opt_ex else None}])
    e.synchronize()
    assert np.isfinite(e.loss_value())
    e.close()
    return events


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_step_trace(name):
    pytest.importorskip("torch")
    want = json.load(open(FIXTURE))[name]
    got = json.loads(json.dumps(run_scenario(name)))
    for k, (w, g) in enumerate(zip(want, got)):
        assert w == g, f"{name}: event {k} is {g}, the fixture has {w} (after {got[max(0, k - 3):k]})"
    assert len(got) == len(want), f"{name}: {len(got)} events, the fixture has {len(want)}"


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "jama16-retina-replication_amd")]
    fixture = {}
    for scenario in sorted(SCENARIOS):
        fixture[scenario] = run_scenario(scenario)
        print(scenario, len(fixture[scenario]), "events", flush=True)
    with open(FIXTURE, "w") as f:       # one event per line
        f.write("{\n" + ",\n".join(
            f' "{k}": [\n' + ",\n".join("  " + json.dumps(ev, sort_keys=True) for ev in evs) + "\n ]"
            for k, evs in sorted(fixture.items())) + "\n}\n")
