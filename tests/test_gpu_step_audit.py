"""The training step's declared reads and writes, its stream order against
torch's own work, and a first-divergence trace (tests/step_audit.py).

All at 107^2, B = 4, tiles="heuristic" (the sizes of test_gpu_bn_moving.py),
for bf16 (deferred filter gradients, the stem's filter gradients on lane 1,
the bf16 filter copies, the halo forward), x6h (the magnitude rows) and x8p
(the operand planes).  Every condition is bitwise.

a. Write-set audit: the two-lane call list, one call at a time; after each
   call the bytes that changed lie inside that call's declared writes.
b. Read-set audit: before each call everything it declares neither as a read
   nor as a write is overwritten with quiet NaNs (fp32 0x7FC00000, bf16
   0x7FC0); its declared writes must come out bit for bit as in the
   unpoisoned run of (a), and jr_device_check stays clean.  A declared write
   implies a read (step_audit.WRITE_IMPLIES_READ).  Never
   poisoned: index and table buffers (argmax, the segment / tile / wprep /
   absmax tables: a poisoned table would form addresses), params, and the
   workspaces ws_lane / ws_stem (the stream-K count words, whose "left zero"
   contract test_gpu_streamk.py owns); nor anything that is not fp32 / bf16.
   The frozen forward list is audited the same way (x6h: its keys are mapped
   only, a frozen x6h forward needs x6h_frozen).
c. First-divergence trace: a digest of every declared write, enqueued on the
   call's own lane, no host synchronisation; serial vs serial, one lane vs
   two lanes with producer waits and with tail waits (JR_PRECISE_WAITS=0
   semantics), three steps each; eager vs replayed graph on the final state.
d. torch's current stream stalled (~20 ms) right before each phase that
   allocates or fills: losses, parameters, stats and moving of three steps
   bitwise the unstalled run; moving_variance exactly 1 after construction.
e. The same with the caching allocator handing back 0xFF-filled blocks.
"""
import functools
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RES, B, STEPS = 107, 4, 3
CONFIGS = {"bf16": dict(dtype="bf16"), "x6h": dict(dtype="f32", conv_math="x6h"),
           "x8p": dict(dtype="f32", conv_math="x8p")}
CFGS = sorted(CONFIGS)


def _batch(k):
    from jr import synth
    return synth.fundus_batch(300 + 10 * k, B, RES), synth.labels(300 + 10 * k, B, p=0.5)


def _engine(cfg, **kw):
    from jr.engine import Engine
    return Engine(B, RES, RES, seed=3, lanes=2, tiles="heuristic", bn_moving=0.99, **CONFIGS[cfg], **kw)


def _sync(e):
    e.synchronize()
    torch.cuda.synchronize()


def _bits(t):
    a = t.detach().cpu().contiguous().reshape(-1)
    return a.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]).numpy()


# ------------------------------------------------------ a, b. the two audits
@functools.lru_cache(maxsize=None)
def _audited(cfg):
    """One warm step (so accumulators and statistics hold real values), then
    the serial, shadowed, poisoned run of the next step's two-lane list and of
    the frozen forward list."""
    import step_audit
    from jr import _ffi
    e = _engine(cfg)
    e.set_batch(*_batch(0))
    e.train_step()
    e.set_batch(*_batch(1))
    _sync(e)
    lists = e._build_calls(B)
    assert {c.lane for c in lists[1] if c.fn != "param_ready"} == {0, 1}
    out = {"device": None}
    t0 = time.perf_counter()
    out["train"] = step_audit.engine_audit(e, lists)
    out["calls"] = sum(1 for p in lists[:3] for c in p if c.fn != "param_ready")
    if cfg != "x6h":
        e.freeze_bn("batch")
        _sync(e)
        out["frozen"] = step_audit.engine_audit(e, e._build_calls(B, frozen=True), phases=(0,))
    torch.cuda.synchronize()
    try:
        e.synchronize()
    except _ffi.JRError as err:
        out["device"] = str(err)
    print(f"step audit {cfg}: {out['calls']} calls, {time.perf_counter() - t0:.2f} s")
    e.close()
    return out


TRAIN_KEYS = {"a", "r", "d", "g", "p", "acc", "draw", "ws", "am", "feat", "head", "lab", "dfeat", "bn_moving", "frozen"}
# the keywords of test_gpu_call_signature.py's bf16_accum3_every_call, and label smoothing
EVERY_KEYWORD = dict(dtype="bf16", accum_steps=3, dropout=0.2, clip_norm=1.0, weight_ema=0.999, bn_moving=0.99,
                     label_smoothing=0.1)
BF16_KEYS = TRAIN_KEYS | {"w16", "draw2", "slab"}
MAPPED = {"bf16": BF16_KEYS,
          "x6h": TRAIN_KEYS | {"wmax", "dmax", "draw2", "wss"},
          "x8p": TRAIN_KEYS | {"w16", "ap", "drawp"},
          "every_keyword": (BF16_KEYS - {"frozen"}) | {"gacc", "ema", "drop", "feat_drop", "gnorm"},
          "input_grad": {"target", "dinput", "dmax"},
          "ens_x6h": {"a", "r", "ws", "feat", "head", "frozen"},
          "ens_bf16": {"a", "r", "ws", "feat", "head", "frozen"}}


def _mapped_lists(case):
    """(engine, the _build_calls tuples whose keys the case maps)."""
    from jr.engine import Engine
    if case in CONFIGS:
        e = _engine(case)
        return e, [e._build_calls(B), e._build_calls(B, 1), e._build_calls(B, frozen=True)]
    if case == "every_keyword":
        e = Engine(B, RES, RES, seed=3, lanes=2, tiles="heuristic", **EVERY_KEYWORD)
        lists = [e._build_calls(B, training=True, accum=ph) for ph in ("open", "inside", "close", None)]
        return e, lists + [([], [], e._flush_calls(), [], None)]
    if case == "input_grad":
        e = Engine(B, RES, RES, seed=3, lanes=2, tiles="heuristic", conv_math="x6h", input_grad=True, x6h_frozen=True)
        e._build_input_grad(B)
        return e, [e._calls[(B, 2, "input_grad")]]
    from jr.ensemble import EnsembleEngine
    from jr.inception import build_inception_v3
    from jr.init import init_params
    g = build_inception_v3(RES, RES, 1)
    kw = dict(conv_math="x6h", x6h_frozen=True) if case == "ens_x6h" else dict(dtype="bf16")
    e = EnsembleEngine([init_params(g, 70 + m) for m in range(2)], B, RES, RES, tiles="heuristic", **kw)
    return e, [e._build_calls(B), e._build_calls(B, frozen=True)]


def _inside(r, t):
    """Region r is non-empty and ends inside the flat tensor t."""
    return r.width > 0 and r.rows > 0 and 0 <= r.start and r.start + (r.rows - 1) * r.stride + r.width <= t.numel()


@pytest.mark.parametrize("cfg", sorted(MAPPED))
def test_every_resource_key_maps_to_memory(cfg):
    """Every key of every call of every list a builder can emit -- train (one and
    two lanes) and frozen-forward lists; the four accumulation phases and the
    flush list with every keyword on; the input-gradient list; an ensemble's
    batch-statistics and frozen lists -- maps to one or more regions inside a
    tensor of universe(): an unknown key or a region past its tensor is an
    error.  Only allocates and binds: no kernel of the step runs."""
    import step_audit
    e, all_lists = _mapped_lists(cfg)
    seen = set()
    for lists in all_lists:
        uni = e.universe(lists)
        mem = step_audit.Memory(uni)
        flat = mem.new()
        phases = lists[:3] if len(lists) > 2 else lists[:1]
        for p in phases:
            for c in p or ():
                if c.fn == "param_ready":
                    continue
                for k in tuple(c.reads) + tuple(c.writes):
                    seen.add(k[0])
                    regs = e.regions(k, lists)
                    assert regs, k
                    for r in regs:
                        assert r.name in uni and _inside(r, uni[r.name]), (k, r)
                        assert mem.view(flat, r).numel() > 0, (k, r)
    assert MAPPED[cfg] <= seen, sorted(MAPPED[cfg] - seen)
    if cfg == "ens_x6h":
        # no call of an ensemble's lists names the filters' magnitude rows (measured once, at
        # load_params): the map still covers them, a row per launch and member
        (r,) = e.regions(("wmax",))
        assert _inside(r, uni["absmax"]) and (r.start, r.width) == (0, 64 * len(e.cunits) * e.members)
        assert r.width + 64 == e.absmax.numel()         # and the betas' row behind them
    if hasattr(e, "close"):
        e.close()


@pytest.mark.parametrize("cfg", CFGS)
def test_write_set_audit(cfg):
    out = _audited(cfg)
    for which in ("train", "frozen"):
        if which in out:
            assert not out[which][0], "\n".join([f"{cfg} {which} list:"] + out[which][0])


@pytest.mark.parametrize("cfg", CFGS)
def test_read_set_audit(cfg):
    """Exclusions (never poisoned): argmax, every table, params, ws_lane /
    ws_stem, non-float buffers; a declared write implies a read."""
    out = _audited(cfg)
    for which in ("train", "frozen"):
        if which in out:
            assert not out[which][1], "\n".join([f"{cfg} {which} list:"] + out[which][1])
    assert out["device"] is None, out["device"]


# --------------------------------------------------- c. first-divergence trace
MODES = ("serial", "serial2", "one_lane", "two_lanes", "two_lanes_tail")


@functools.lru_cache(maxsize=None)
def _trace(cfg, mode):
    import step_audit
    e = _engine(cfg)
    if mode == "two_lanes_tail":
        e.lanes.precise_waits = False
    lists = e._build_calls(B, 1) if mode == "one_lane" else e._build_calls(B)
    t0 = time.perf_counter()
    t = step_audit.trace(e, lists, STEPS, lambda k: e.set_batch(*_batch(k)), serial=mode.startswith("serial"))
    print(f"trace {cfg} {mode}: {len(t.rows)} digests, {time.perf_counter() - t0:.2f} s")
    final = {n: _bits(getattr(e, n)) for n in ("params", "accum", "stats", "moving", "loss")}
    e.close()
    return t, final


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("a,b", [("serial", "serial2"), ("one_lane", "two_lanes"), ("one_lane", "two_lanes_tail"),
                                 ("serial", "two_lanes")])
def test_traces_agree(cfg, a, b):
    import step_audit
    (ta, fa), (tb, fb) = _trace(cfg, a), _trace(cfg, b)
    assert len(ta.rows) == len(tb.rows) > 3 * 100
    # (the table is filled: zero digests are zeroed regions, x6h's magnitude rows after jr_absmax_prep)
    assert np.count_nonzero(ta.values) > len(ta.values) // 2
    d = step_audit.first_difference(ta, tb, step_audit.LANE_SCRATCH if "one_lane" in (a, b) else ())
    assert d is None, (cfg, a, b, d)
    for n in fa:
        assert np.array_equal(fa[n], fb[n]), (cfg, a, b, n)


@pytest.mark.parametrize("cfg", CFGS)
def test_replayed_graph_is_the_eager_final_state(cfg):
    """No torch work inside the capture: the final state alone."""
    _, eager = _trace(cfg, "two_lanes")
    e = _engine(cfg)
    for k in range(STEPS):
        e.set_batch(*_batch(k))
        if k == 0:
            e.capture()
        e.replay()
    _sync(e)
    for n in eager:
        got = _bits(getattr(e, n))
        assert np.array_equal(got, eager[n]), (cfg, n, int(np.sum(got != eager[n])))
    e.close()


# ------------------------------------- d, e. order against the current stream
PHASES = ("construct", "set_batch", "first_step", "augment", "load_bn_moving", "freeze_bn", "calibrate_bn")


@functools.lru_cache(maxsize=None)
def _stall_cycles():
    """Cycles of torch.cuda._sleep for roughly 20 ms, from one timed probe."""
    probe = 10_000_000
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    cycles = int(probe * 20.0 / max(ms, 1e-3))
    print(f"stall calibration: {probe} cycles = {ms:.2f} ms; 20 ms = {cycles} cycles")
    return cycles


def _dirty_allocator(sizes):
    """Blocks of the engine's buffer sizes, filled with 0xFF, back in the caching allocator."""
    blocks = [torch.empty(n, dtype=torch.uint8, device="cuda").fill_(0xFF) for n in sizes]
    torch.cuda.synchronize()
    del blocks


@functools.lru_cache(maxsize=None)
def _sizes(cfg):
    e = _engine(cfg)
    e.set_batch(*_batch(0))
    e.train_step()
    _sync(e)
    sizes = sorted({t.numel() * t.element_size() for t in e.universe(e._build_calls(B)).values()})
    e.close()
    return tuple(sizes)


def _scenario(cfg, stall=None, dirty=False):
    """Construction, three training steps (the second on an augmented batch),
    load_bn_moving, freeze_bn, calibrate_bn; `stall`: the phase right before
    which torch's current stream is stalled."""
    from jr import augment

    def at(phase):
        if phase == stall:
            torch.cuda._sleep(_stall_cycles())

    if dirty:
        _dirty_allocator(_sizes(cfg))
    out = {}
    at("construct")
    e = _engine(cfg)
    mv = e.bn_moving_numpy()
    var = np.concatenate([v for k, v in mv.items() if k.endswith("moving_variance")])
    mean = np.concatenate([v for k, v in mv.items() if k.endswith("moving_mean")])
    out["var0"] = (float(var.min()), float(var.max()), float(np.abs(mean).max()))
    for k in range(STEPS):
        x, y = _batch(k)
        if k == 1:
            tab = augment.draw(augment.AugmentSpec(), np.random.Generator(np.random.PCG64([3, 0])), B)
            at("augment")
            e.set_batch(x, y, augment=tab)
        else:
            if k == 0:
                at("set_batch")
            e.set_batch(x, y)
        if k == 0:
            at("first_step")
        e.train_step()
        _sync(e)
        for n in ("loss", "stats", "moving"):
            out[f"{n}[{k}]"] = _bits(getattr(e, n))
    out["params"], out["accum"] = _bits(e.params), _bits(e.accum)
    stats = {k: (v * np.float32(0.5) + np.float32(0.25)) for k, v in e.bn_moving_numpy().items()}
    at("load_bn_moving")
    e.load_bn_moving(stats)
    at("freeze_bn")
    e.freeze_bn("moving")
    _sync(e)
    out["moving_loaded"], out["frozen_loaded"] = _bits(e.moving), _bits(e.frozen)
    at("calibrate_bn")
    e.calibrate_bn([_batch(3)[0]])
    e.freeze_bn("moving")
    _sync(e)
    out["moving_calibrated"], out["frozen_calibrated"] = _bits(e.moving), _bits(e.frozen)
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def _reference(cfg):
    return _scenario(cfg)


def _assert_same(cfg, what, got, want):
    assert got["var0"] == (1.0, 1.0, 0.0), (cfg, what, "moving statistics right after construction "
                                            "(min var, max var, max |mean|)", got["var0"])
    for n in want:
        if n != "var0":
            assert np.array_equal(got[n], want[n]), (cfg, what, n, int(np.sum(got[n] != want[n])))


STALLS = [("bf16", p) for p in PHASES] + [("x6h", "construct"), ("x6h", "first_step"), ("x8p", "construct"),
                                          ("x8p", "first_step")]


@pytest.mark.parametrize("cfg,phase", STALLS)
def test_stalled_current_stream(cfg, phase):
    want = _reference(cfg)
    assert want["var0"] == (1.0, 1.0, 0.0)
    _assert_same(cfg, f"stall before {phase}", _scenario(cfg, stall=phase), want)


def test_stalled_current_stream_ensemble_construction():
    from jr.ensemble import EnsembleEngine
    from jr.inception import build_inception_v3
    from jr.init import init_params
    g = build_inception_v3(RES, RES, 1)
    params = [init_params(g, 70 + m) for m in range(2)]
    x, y = _batch(0)
    got = []
    for stall in (False, True):
        if stall:
            torch.cuda._sleep(_stall_cycles())
        e = EnsembleEngine(params, B, RES, RES, tiles="heuristic", dtype="bf16")
        for mv in e.bn_moving_numpy():
            for k, v in mv.items():
                assert np.all(v == (1.0 if k.endswith("moving_variance") else 0.0)), (stall, k)
        e.set_batch(x, y)
        e.forward()
        got.append(e.predictions())
    assert got[0].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("phase", [None, "construct", "first_step"])
def test_dirty_allocator(cfg, phase):
    _assert_same(cfg, f"dirty allocator, stall before {phase}", _scenario(cfg, stall=phase, dirty=True),
                 _reference(cfg))
