"""The step's schedule, pinned: for a spread of engine configurations the
bound call lists (what is launched, in which order, on which lane, after
which waits, with which scalars and byte counts -- jr.lanes.signature) must
equal the recorded ones in tests/golden/call_signatures.json.  The engines
only allocate and bind here; no kernel of the step runs.  The pointers the
signature leaves out are covered by the bitwise tests (test_gpu_engine,
test_gpu_ensemble, test_gpu_bn_batch, test_gpu_fold, test_gpu_apply_multi).

`python tests/test_gpu_call_signature.py` rewrites the fixture from the code
as it stands (a deliberate change of the schedule).
"""
import collections
import ctypes
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "call_signatures.json")
RES = 107
PHASES = ("fwd", "bwd", "opt")

# name -> (kind, constructor keywords, environment, builds, phases); a build is (batch, lanes or None) or
# (batch, lanes or None, {"training": ..., "accum": ...}) -- further keywords of _build_calls -- or "flush":
# accum_flush's update list
ACCUM = [(4, None, dict(training=True, accum=ph)) for ph in ("open", "inside", "close", None)] + ["flush"]
CASES = {
    "x6h_l2_train": ("engine", dict(conv_math="x6h", lanes=2), {}, [(4, None), (3, None), (4, 1)], PHASES),
    "x8_l4_train": ("engine", dict(conv_math="x8", lanes=4), {}, [(4, None)], PHASES),
    "f32_defer_flush": ("engine", dict(conv_math="f32", defer_wgrad=True), {}, [(4, None)], PHASES),
    "bf16_l2": ("engine", dict(dtype="bf16", lanes=2), {}, [(4, None)], PHASES),
    "x8p_l2": ("engine", dict(conv_math="x8p", lanes=2), {}, [(4, None)], PHASES),
    "x8_fold": ("engine", dict(conv_math="x8", fold_stats=True), {}, [(4, None)], PHASES),
    "x8_b6_bn_batch": ("engine", dict(batch=6, conv_math="x8"), {"JR_BN_BATCH": "1"}, [(6, None)], PHASES),
    "x8_unfused_pool_single_apply": ("engine", dict(conv_math="x8", fuse_pool=False), {"JR_APPLY_MULTI": "0"},
                                     [(4, None)], PHASES),
    "x8_ab_order": ("engine", dict(conv_math="x8"),
                    {"JR_DGRAD_FIRST": "0", "JR_STEM_WGRAD_LANE": "0", "JR_FUSE_POOL_BWD": "0"}, [(4, None)], PHASES),
    "x6h_eval": ("engine", dict(conv_math="x6h", train=False), {}, [(4, None)], PHASES),
    "x8_adam": ("engine", dict(conv_math="x8", optimizer="adam"), {}, [(4, None)], ("opt",)),
    "ens3_x6h_l2": ("ensemble", dict(members=3, conv_math="x6h", lanes=2), {}, [(4, None), (3, None)], ("fwd",)),
    "ens2_bf16": ("ensemble", dict(members=2, dtype="bf16"), {}, [(4, None)], ("fwd",)),
    "x8_decay_clip": ("engine", dict(conv_math="x8", weight_decay=1e-4, clip_norm=1.0), {}, [(4, None)], PHASES),
    "x8_rmsprop_ema": ("engine", dict(conv_math="x8", optimizer="rmsprop", weight_ema=0.999), {}, [(4, None)], PHASES),
    "x8_dropout": ("engine", dict(conv_math="x8", dropout=0.2), {},
                   [(4, None, dict(training=True)), (4, None, dict(training=False))], PHASES),
    "x8_loss_recipe": ("engine", dict(conv_math="x8", label_smoothing=0.1, class_weight=[2.0], focal_gamma=2.0), {},
                       [(4, None)], PHASES),
    "x8_bn_moving": ("engine", dict(conv_math="x8", bn_moving=0.99), {}, [(4, None)], PHASES),
    "x8_accum3": ("engine", dict(conv_math="x8", accum_steps=3), {}, ACCUM, PHASES),
    "bf16_accum3_every_call": ("engine", dict(accum_steps=3, dtype="bf16", dropout=0.2, clip_norm=1.0, weight_ema=0.999,
                                              bn_moving=0.99), {}, ACCUM, PHASES),
}


def _clear_overrides(dtype, conv_math, batches):
    """libjr's per-geometry tile overrides are process-wide (another test may
    have pinned or autotuned this geometry): back to the planner heuristic
    for every conv launch of the case, before its engine sizes anything."""
    from jr import _ffi
    from jr.inception import build_inception_v3
    from jr.plan import build_plan
    _ffi.init(0)
    lib = _ffi.load()
    g = build_inception_v3(RES, RES, 1)
    dt = {"f32": _ffi.JR_F32, "bf16": _ffi.JR_BF16}[dtype]
    cdt = {"x8": _ffi.JR_F32_X8, "x8p": _ffi.JR_F32_X8P, "x6h": _ffi.JR_F32_X6H}.get(conv_math, dt)
    q = 8 if dtype == "bf16" else 4
    in_stride = (g.bufs[g.input_buf].c + q - 1) // q * q
    for u in build_plan(g, True).units:
        if conv_math == "x8p":
            xs = (u.cin + 7) // 8 * 8
        else:
            xs = in_stride if u.x == g.input_buf else u.cin
        for B in batches:
            d = _ffi.ConvDesc(B, u.h, u.w, u.cin, u.cout, u.kh, u.kw, u.stride, u.stride, u.pad_h, u.pad_w,
                              u.ho, u.wo, 0, xs, 0, u.cout)
            ops = [(_ffi.JR_CONV_FWD, 0), (_ffi.JR_CONV_BWD_FILTER, 0)]
            if u.x != g.input_buf:
                ops += [(_ffi.JR_CONV_BWD_DATA, p) for p in range(u.stride * u.stride)]
            for op, p in ops:
                _ffi.check("set_config", lib.jr_conv2d_set_config(ctypes.byref(d), op, cdt, p, -1))


def _describe(calls):
    from jr.lanes import signature
    text = signature(calls)
    counts = collections.Counter(c.name for c in calls)
    return text, {"sha256": hashlib.sha256(text.encode()).hexdigest(), "counts": dict(sorted(counts.items()))}


def build_case(name, setenv):
    """{"B<batch>[_nl<lanes>][_accum_<where>][_training_<flag>]/<phase>" or "flush/opt": (text, {"sha256",
    "counts"})} of one case."""
    from jr.engine import Engine
    from jr.ensemble import EnsembleEngine
    from jr.init import init_params
    kind, kw, env, builds, phases = CASES[name]
    kw = dict(kw)
    for k, v in env.items():
        setenv(k, v)
    dtype = kw.get("dtype", "f32")
    conv_math = kw.get("conv_math") or ("x8" if dtype == "f32" else "bf16")
    batch = kw.pop("batch", 4)
    _clear_overrides(dtype, conv_math, sorted({batch} | {b[0] for b in builds if b != "flush"}))
    out = {}
    if kind == "ensemble":
        from jr.inception import build_inception_v3
        g = build_inception_v3(RES, RES, 1)
        params = [init_params(g, 70 + m) for m in range(kw.pop("members"))]
        e = EnsembleEngine(params, batch, RES, RES, tiles="heuristic", **kw)
        for B, _ in builds:
            out[f"B{B}/fwd"] = _describe(e._build_calls(B)[0])
        return out
    e = Engine(batch, RES, RES, tiles="heuristic", seed=1, **kw)
    if name == "f32_defer_flush":
        n = e.nparam
        e.set_flush_points([n // 2, n // 5, n // 20])
    for build in builds:
        if build == "flush":
            out["flush/opt"] = _describe(e._flush_calls())
            continue
        B, nl, more = (tuple(build) + ({},))[:3]
        lists = e._build_calls(B, **more) if nl is None else e._build_calls(B, nl, **more)
        key = (f"B{B}" if nl is None else f"B{B}_nl{nl}") + "".join(f"_{k}_{v}" for k, v in sorted(more.items()))
        for phase, calls in zip(PHASES, lists[:3]):
            if phase in phases:
                out[f"{key}/{phase}"] = _describe(calls)
    e.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_call_signature(name, monkeypatch, tmp_path):
    pytest.importorskip("torch")
    want = json.load(open(FIXTURE))[name]
    got = build_case(name, monkeypatch.setenv)
    assert sorted(got) == sorted(want)
    for key, (text, desc) in got.items():
        if desc != want[key]:
            path = tmp_path / f"{name}_{key.replace('/', '_')}.txt"
            path.write_text(text)
            diff = {k: (want[key]["counts"].get(k), desc["counts"].get(k))
                    for k in set(want[key]["counts"]) | set(desc["counts"])
                    if want[key]["counts"].get(k) != desc["counts"].get(k)}
            raise AssertionError(f"{name} {key}: call signature differs from the fixture (per-name counts that "
                                 f"differ, (fixture, now): {diff}); full text written to {path}")


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "jama16-retina-replication_amd")]
    dump = sys.argv[1] if len(sys.argv) > 1 else None      # optional: a directory for the full texts
    fixture = {}
    for case in sorted(CASES):
        saved = {k: os.environ.get(k) for k in CASES[case][2]}
        built = build_case(case, os.environ.__setitem__)
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        fixture[case] = {key: desc for key, (_, desc) in built.items()}
        if dump:
            os.makedirs(dump, exist_ok=True)
            for key, (text, _) in built.items():
                open(os.path.join(dump, f"{case}_{key.replace('/', '_')}.txt"), "w").write(text)
        print(case, {k: v["sha256"][:12] for k, v in fixture[case].items()}, flush=True)
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
