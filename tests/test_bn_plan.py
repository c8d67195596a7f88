"""The BN launch planner's output, pinned on the CPU.  What the C ABI reports
must equal the record in tests/golden/bn_plans.json:

* plans/<workload>/dt<d>: every field of jr_bn_plan, fp32 and bf16, for every
  distinct (B*ho*wo, c_out) of the conv launches of Inception-v3 (siblings
  fused) at the three workloads of test_conv_plan, and every member's c at
  the same m;
* edge/dt<d>: the same for c in EDGE_C and m in EDGE_M plus, for each valid
  c, the two m on either side of nchunks = 512 (the single-stage finalize and
  jr_bn_relu_bwd_batch limit) and of nchunks = 1024 (where chunks start to
  grow), derived from the smallest chunk the library itself reports;
* ws: jr_bn_relu_bwd_batch_workspace_size for the layer set of
  test_gpu_bn_batch, for 8 layers, and for n = 0 and 9, and
  jr_bn_relu_bwd_maxpool_workspace_size for the fused stem pools;
* refusals/<entry point>: the calls every BN entry point must refuse before
  any launch, with their status and jr_last_error() text.  Pointers are small
  16-aligned integers that validation never dereferences.  Only refused calls
  are made: none reaches a launch, so no device is needed;
* groups/<workload>/vw<w>: the launches jr.plan.bn_batch_groups batches (the
  engine's JR_BN_BATCH=1 groups), by name.

The fixture keeps one sha256 and one row count per group, and a short digest
per block so that a mismatch can name where it starts.  The walk runs in a
fresh child process without JR_BN_FOLD_ROWS and JR_FOLD_BN_BWD: the library
reads those once per process.

`python tests/test_bn_plan.py [DIR]` rewrites the fixture from the code as it
stands (a deliberate change of the planner) and, with DIR, dumps the full
texts there, so two commits can be diffed.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "bn_plans.json")
WORKLOADS = {"res107_b4": (107, 4), "res299_b64": (299, 64), "res587_b2": (587, 2)}
GROUP_WORKLOADS = {"res107_b6": (107, 6), "res299_b64": (299, 64)}
DTYPES = (0, 1)                          # JR_F32, JR_BF16
EDGE_C = (4, 6, 8, 12, 32, 64, 192, 768, 1024, 1028, 2048, 2056)
EDGE_M = (1, 15, 16, 17)
ENV_DROPPED = ("JR_BN_FOLD_ROWS", "JR_FOLD_BN_BWD")
# tests/test_gpu_bn_batch.py LAYERS: (m, segment channels)
BATCH_LAYERS = [(64 * 17 * 17, (192,)), (64 * 17 * 17, (160,)), (64 * 8 * 8, (384,)), (64 * 35 * 35, (64,)),
                (64 * 8 * 8, (256, 128))]
ENTRY_POINTS = ("jr_bn_plan", "jr_bn_stats", "jr_bn_relu_apply", "jr_bn_relu_apply_multi", "jr_bn_relu_apply_stats",
                "jr_bn_relu_apply_grouped", "jr_bn_relu_bwd", "jr_bn_relu_bwd_multi", "jr_bn_relu_bwd_multi_absmax",
                "jr_bn_relu_bwd_batch", "jr_bn_relu_bwd_maxpool", "jr_bn_relu_bwd_maxpool_absmax")
GROUPS = ([f"plans/{w}/dt{dt}" for w in WORKLOADS for dt in DTYPES] + [f"edge/dt{dt}" for dt in DTYPES] + ["ws"] +
          [f"refusals/{fn}" for fn in ENTRY_POINTS] + [f"groups/{w}/vw{vw}" for w in GROUP_WORKLOADS for vw in (4, 8)])
PLAN_FIELDS = ("vec_width", "rows_per_chunk", "nchunks", "single_stage", "reduce_grid", "finalize_grid",
               "stats_finalize_grid", "apply_grid", "fold_rows", "fold_grid_x", "fold_grid_y", "k1_offset",
               "workspace_size")
PTR = 16                                 # a non-null "pointer" no refused call reads


def _plan_row(lib, ffi, dt, m, c):
    p = ffi.BnLaunchPlan()
    rc = lib.jr_bn_plan(dt, m, c, ctypes.byref(p))
    head = f"dt={dt} m={m} c={c} -> {rc}"
    if rc:
        return f"{head} {ffi.last_error()}", None
    assert p.workspace_size == lib.jr_bn_workspace_size(m, c)
    return head + "".join(f" {n}={getattr(p, n)}" for n in PLAN_FIELDS), p


def _model(res):
    from jr.inception import build_inception_v3
    from jr.plan import build_plan
    g = build_inception_v3(res, res, 1)
    return g, build_plan(g, True)


def _walk_plans(lib, ffi, out):
    for wname, (res, batch) in WORKLOADS.items():
        _, plan = _model(res)
        shapes = {}                      # m -> channel counts, in first-seen order
        for u in plan.units:
            cs = shapes.setdefault(batch * u.ho * u.wo, [])
            for c in [u.cout] + [n.cout for n in u.members]:
                if c not in cs:
                    cs.append(c)
        for dt in DTYPES:
            out[f"plans/{wname}/dt{dt}"] = [(f"m={m}", [_plan_row(lib, ffi, dt, m, c)[0] for c in cs])
                                            for m, cs in shapes.items()]


def _walk_edges(lib, ffi, out):
    for dt in DTYPES:
        blocks = []
        for c in EDGE_C:
            ms = list(EDGE_M)
            _, p = _plan_row(lib, ffi, dt, 1, c)
            if p is not None:            # the smallest chunk: nchunks = ceil(m / it) up to 1024 of them
                ms += [k * p.rows_per_chunk + d for k in (512, 1024) for d in (0, 1)]
            blocks.append((f"c={c}", [_plan_row(lib, ffi, dt, m, c)[0] for m in ms]))
        out[f"edge/dt{dt}"] = blocks


def _batch_layers(ffi, specs, keep):
    layers = (ffi.BnBwdLayer * len(specs))()
    for k, (m, segs) in enumerate(specs):
        c = sum(segs)
        layers[k].nseg = len(segs)
        for j, s in enumerate(segs):
            layers[k].segs[j] = ffi.BnSeg(PTR, 0, s, s, PTR, PTR)
        layers[k].x, layers[k].x_c_off, layers[k].x_c_stride, layers[k].m, layers[k].c = PTR, 0, c, m, c
        layers[k].mean, layers[k].invstd, layers[k].dx = PTR, PTR, PTR
    keep.append(layers)
    return layers


def _pool_descs(ffi, res, batch):
    from jr.engine import fusable_pools
    g, plan = _model(res)
    return [ffi.PoolDesc(batch, n.h, n.w, n.c, n.ho, n.wo, 0, n.c, n.y.c_off, g.bufs[n.y.buf].c)
            for n in (g.nodes[i] for i in fusable_pools(g, plan))]


def _walk_ws(lib, ffi, out):
    keep, rows = [], []
    eight = (BATCH_LAYERS * 2)[:8]
    for name, n, specs in (("layers5", 5, BATCH_LAYERS), ("layers8", 8, eight), ("n0", 0, eight), ("n9", 9, eight + eight[:1])):
        layers = _batch_layers(ffi, specs, keep)
        rows.append(f"bwd_batch {name} -> {lib.jr_bn_relu_bwd_batch_workspace_size(n, ctypes.byref(layers))}")
    rows.append(f"bwd_batch null -> {lib.jr_bn_relu_bwd_batch_workspace_size(2, None)}")
    for wname, (res, batch) in WORKLOADS.items():
        descs = _pool_descs(ffi, res, batch)
        assert len(descs) == 2           # the stem's conv2d_3 and conv2d_5
        for d in descs:
            rows.append(f"bwd_maxpool {wname} {d.n}x{d.h}x{d.w}x{d.c} -> "
                        f"{lib.jr_bn_relu_bwd_maxpool_workspace_size(ctypes.byref(d))}")
    rows.append(f"bwd_maxpool null -> {lib.jr_bn_relu_bwd_maxpool_workspace_size(None)}")
    out["ws"] = [("ws", rows)]


# argument names of every entry point, in call order (include/jr.h)
SPEC = {
    "jr_bn_plan": "dtype m c out",
    "jr_bn_stats": "dtype x m c eps mean invstd ws ws_bytes stream",
    "jr_bn_relu_apply": "dtype x x_c_off x_c_stride m c mean invstd beta y y_c_off y_c_stride stream",
    "jr_bn_relu_apply_multi": "dtype nseg asegs x x_c_off x_c_stride m c mean invstd stream",
    "jr_bn_relu_apply_stats": ("dtype x x_c_off x_c_stride m c part P R n_total stat_c_off eps mean invstd beta y "
                               "y_c_off y_c_stride stream"),
    "jr_bn_relu_apply_grouped": ("dtype members x x_c_off x_c_stride x_member_stride m c mean invstd "
                                 "stats_member_stride beta beta_member_stride y y_c_off y_c_stride y_member_stride stream"),
    "jr_bn_relu_bwd": "dtype dy dy_c_off dy_c_stride x x_c_off x_c_stride m c mean invstd beta dx dbeta ws ws_bytes stream",
    "jr_bn_relu_bwd_multi": "dtype nseg bsegs x x_c_off x_c_stride m c mean invstd dx ws ws_bytes stream",
    "jr_bn_relu_bwd_multi_absmax": "dtype nseg bsegs x x_c_off x_c_stride m c mean invstd dx ws ws_bytes absmax stream",
    "jr_bn_relu_bwd_batch": "dtype n layers ws ws_bytes stream",
    "jr_bn_relu_bwd_maxpool": "dtype d argmax pooled_dy dy x x_c_stride mean invstd beta dx dbeta ws ws_bytes stream",
    "jr_bn_relu_bwd_maxpool_absmax": ("dtype d argmax pooled_dy dy x x_c_stride mean invstd beta dx dbeta ws ws_bytes "
                                      "absmax stream"),
}
POINTERS = ("x", "y", "dy", "dx", "mean", "invstd", "beta", "dbeta", "part", "ws", "argmax", "pooled_dy", "d", "out",
            "asegs", "bsegs", "layers")
REFUSED = (-1, -3, -4)                   # JR_ERR_INVALID, JR_ERR_UNSUPPORTED, JR_ERR_WORKSPACE: all before any launch


def _walk_refusals(lib, ffi, out):
    rows, keep = {fn: [] for fn in ENTRY_POINTS}, []
    M, C = 100, 64
    for dt in DTYPES:
        vw = 4 if dt == 0 else 8
        # (offset, stride) of a c-channel slice: misaligned offset, negative offset, misaligned stride, overrun
        bad_slices = {"offset": (vw // 2, C + vw), "negative": (-vw, C + vw), "stride": (0, C + vw // 2),
                      "overrun": (vw, C)}

        def pool(**kw):
            f = dict(n=2, h=9, w=9, c=C, ho=4, wo=4, x_c_off=0, x_c_stride=C, y_c_off=0, y_c_stride=C)
            f.update(kw)
            d = ffi.PoolDesc(*(f[k] for k in ("n", "h", "w", "c", "ho", "wo", "x_c_off", "x_c_stride", "y_c_off", "y_c_stride")))
            keep.append(d)
            return d

        def asegs(*segs):                # (c, y_c_off, y_c_stride, y, beta)
            arr = (ffi.BnApplySeg * max(1, len(segs)))(*[ffi.BnApplySeg(y, off, st, c, be) for c, off, st, y, be in segs])
            keep.append(arr)
            return ctypes.byref(arr)

        def bsegs(*segs):                # (c, dy_c_off, dy_c_stride, dy, beta, dbeta)
            arr = (ffi.BnSeg * max(1, len(segs)))(*[ffi.BnSeg(dy, off, st, c, be, db) for c, off, st, dy, be, db in segs])
            keep.append(arr)
            return ctypes.byref(arr)

        half = C // 2
        two_a = ((half, 0, half, PTR, PTR), (half, 0, half, PTR, PTR))
        two_b = ((half, 0, half, PTR, PTR, PTR), (half, 0, half, PTR, PTR, PTR))
        ws_of = lib.jr_bn_workspace_size
        base = dict(dtype=dt, m=M, c=C, eps=1e-3, stream=None, x_c_off=0, x_c_stride=C, y_c_off=0, y_c_stride=C,
                    dy_c_off=0, dy_c_stride=C, ws_bytes=ws_of(M, C), P=4, R=32, n_total=C, stat_c_off=0, members=2,
                    x_member_stride=M * C, y_member_stride=M * C, stats_member_stride=C, beta_member_stride=C,
                    nseg=2, asegs=asegs(*two_a), bsegs=bsegs(*two_b), absmax=PTR, n=2,
                    layers=ctypes.byref(_batch_layers(ffi, [(M, (half, half)), (M, (C,))], keep)),
                    d=ctypes.byref(pool()), out=ctypes.byref(ffi.BnLaunchPlan()))
        base.update({p: PTR for p in POINTERS if p not in base})

        def call(fn, case, **over):
            names = SPEC[fn].split()
            assert set(over) <= set(names), (fn, case)
            rc = getattr(lib, fn)(*[over.get(k, base[k]) for k in names])
            assert rc in REFUSED, f"{fn} dt{dt} {case}: status {rc}, not refused before the launch"
            rows[fn].append(f"{fn} dt{dt} {case} -> {rc} {ffi.last_error()}")

        for fn in ENTRY_POINTS:
            names = SPEC[fn].split()
            # what every entry point checks of (dtype, m, c): jr_bn_plan's status
            if "m" in names:
                one_a, one_b = lambda c: asegs((c, 0, c, PTR, PTR)), lambda c: bsegs((c, 0, c, PTR, PTR, PTR))
                for case, over in (("dtype=2", dict(dtype=2)), ("dtype=4", dict(dtype=4)), ("m=0", dict(m=0)),
                                   ("c=0", dict(c=0)), ("c_not_vector", dict(c=C + vw // 2)),
                                   ("c_257_vectors", dict(c=257 * vw))):
                    c = over.get("c", C)
                    wide = {k: v for k, v in dict(x_c_stride=c, y_c_stride=c, dy_c_stride=c, n_total=c, nseg=1,
                                                  asegs=one_a(c), bsegs=one_b(c)).items() if k in names}
                    call(fn, case, **wide, **over)
            for p in POINTERS:
                if p in names:
                    call(fn, f"null_{p}", **{p: None})
            for t in ("x", "y", "dy"):
                if f"{t}_c_off" in names:
                    for kind, (off, stride) in bad_slices.items():
                        call(fn, f"{t}_slice_{kind}", **{f"{t}_c_off": off, f"{t}_c_stride": stride})
            if "ws_bytes" in names and fn != "jr_bn_relu_bwd_batch" and "d" not in names:
                call(fn, "ws_one_byte_short", ws_bytes=ws_of(M, C) - 1)
            if "nseg" in names:
                mk = asegs if "asegs" in names else bsegs
                key = "asegs" if "asegs" in names else "bsegs"
                tail = (PTR, PTR) if mk is asegs else (PTR, PTR, PTR)
                seg = lambda c, off=0, stride=None: (c, off, c if stride is None else stride) + tail  # noqa: E731
                call(fn, "nseg=0", nseg=0)
                call(fn, "nseg=5", nseg=5, **{key: mk(*[seg(16)] * 5)})
                call(fn, "segments_sum_short", **{key: mk(seg(half), seg(half - vw))})
                call(fn, "segments_sum_long", **{key: mk(seg(half), seg(half + vw))})
                call(fn, "segment_c=0", **{key: mk(seg(C), seg(0))})
                call(fn, "segment_c_not_vector", **{key: mk(seg(half + vw // 2), seg(half - vw // 2))})
                for kind, (off, stride) in bad_slices.items():
                    o, s = off, stride - C + half
                    call(fn, f"segment_slice_{kind}", **{key: mk(seg(half), seg(half, o, s))})
                for i in range(len(tail)):
                    nulled = tail[:i] + (None,) + tail[i + 1:]
                    call(fn, f"segment_null_{i}", **{key: mk(seg(half), (half, 0, half) + nulled)})
        call("jr_bn_relu_apply_stats", "P*R<m", P=3, R=33)
        call("jr_bn_relu_apply_stats", "P=0", P=0)
        call("jr_bn_relu_apply_stats", "R=0", R=0)
        call("jr_bn_relu_apply_stats", "stat_c_off+c>n_total", stat_c_off=vw)
        call("jr_bn_relu_apply_stats", "stat_c_off<0", stat_c_off=-vw, n_total=2 * C)
        call("jr_bn_relu_apply_stats", "m=2^31", m=1 << 31, P=1 << 16, R=1 << 16)
        call("jr_bn_relu_apply_grouped", "members=0", members=0)
        call("jr_bn_relu_apply_grouped", "members=65536", members=65536)
        for k in ("x_member_stride", "y_member_stride", "stats_member_stride", "beta_member_stride"):
            call("jr_bn_relu_apply_grouped", f"{k}<0", **{k: -16})
        for k in ("x_member_stride", "y_member_stride"):
            call("jr_bn_relu_apply_grouped", f"{k}_not_16_bytes", **{k: M * C + vw // 4})
        # the batched backward: layer counts, workspace, a layer past 512 chunks, a bad layer
        big = [(64 * 147 * 147, (C,)), (M, (C,))]
        call("jr_bn_relu_bwd_batch", "n=0", n=0)
        call("jr_bn_relu_bwd_batch", "n=9", n=9)
        good = _batch_layers(ffi, [(M, (half, half)), (M, (C,))], keep)
        need = lib.jr_bn_relu_bwd_batch_workspace_size(2, ctypes.byref(good))
        call("jr_bn_relu_bwd_batch", "ws_one_byte_short", layers=ctypes.byref(good), ws_bytes=need - 1)
        lay = _batch_layers(ffi, big, keep)
        call("jr_bn_relu_bwd_batch", "layer_past_512_chunks", layers=ctypes.byref(lay),
             ws_bytes=lib.jr_bn_relu_bwd_batch_workspace_size(2, ctypes.byref(lay)))
        for case, edit in (("layer_nseg=0", lambda L: setattr(L, "nseg", 0)), ("layer_nseg=5", lambda L: setattr(L, "nseg", 5)),
                           ("layer_null_x", lambda L: setattr(L, "x", None)), ("layer_null_dx", lambda L: setattr(L, "dx", None)),
                           ("layer_segments_sum", lambda L: setattr(L.segs[0], "c", half - vw)),
                           ("layer_x_slice_overrun", lambda L: setattr(L, "x_c_off", vw)),
                           ("layer_dtype", None)):
            lay = _batch_layers(ffi, [(M, (half, half)), (M, (C,))], keep)
            if edit:
                edit(lay[1] if "sum" not in case else lay[0])
            call("jr_bn_relu_bwd_batch", case, layers=ctypes.byref(lay), ws_bytes=need, **({} if edit else {"dtype": 2}))
        # the fused max-pool backward: pool geometry, channel count, slices, workspace
        for fn in ("jr_bn_relu_bwd_maxpool", "jr_bn_relu_bwd_maxpool_absmax"):
            pws = lib.jr_bn_relu_bwd_maxpool_workspace_size(ctypes.byref(pool()))
            for case, kw in (("ho_wrong", dict(ho=5)), ("wo_wrong", dict(wo=3)), ("h<3", dict(h=2, ho=0)),
                             ("c=1028", dict(c=1028, x_c_stride=1028, y_c_stride=1028)),
                             ("c=2048", dict(c=2048, x_c_stride=2048, y_c_stride=2048)),
                             ("c_not_vector", dict(c=C + vw // 2, x_c_stride=C + vw // 2, y_c_stride=C + vw // 2)),
                             ("n=0", dict(n=0))):
                c = kw.get("c", C)
                call(fn, case, d=ctypes.byref(pool(**kw)), x_c_stride=c, ws_bytes=max(pws, 4096 * 2 * c * 8 + 8 * c))
            for t in ("x", "y"):
                for kind, (off, stride) in bad_slices.items():
                    call(fn, f"pool_{t}_slice_{kind}", d=ctypes.byref(pool(**{f"{t}_c_off": off, f"{t}_c_stride": stride})),
                         ws_bytes=pws)
            call(fn, "x_c_stride_short", x_c_stride=C - vw, ws_bytes=pws)
            call(fn, "x_c_stride_not_vector", x_c_stride=C + vw // 2, ws_bytes=pws)
            call(fn, "ws_one_byte_short", ws_bytes=pws - 1)
    for fn in ENTRY_POINTS:
        out[f"refusals/{fn}"] = [(fn, rows[fn])]


def _walk_groups(out):
    from jr.engine import fusable_pools
    from jr.plan import bn_batch_groups
    for wname, (res, batch) in GROUP_WORKLOADS.items():
        g, plan = _model(res)
        fused = set(fusable_pools(g, plan).values())
        for vw in (4, 8):
            groups = bn_batch_groups(g, plan, batch, vw, fused)
            out[f"groups/{wname}/vw{vw}"] = [("groups", [" ".join(u.name for u in grp) for grp in groups])]


def walk():
    """{group: [(block head, rows), ...]} -- runs in the child process."""
    from jr import _ffi
    lib = _ffi.load()
    out = {}
    _walk_plans(lib, _ffi, out)
    _walk_edges(lib, _ffi, out)
    _walk_ws(lib, _ffi, out)
    _walk_refusals(lib, _ffi, out)
    _walk_groups(out)
    return out


def _child_main(out_dir):
    from test_conv_plan import _digest
    os.makedirs(out_dir, exist_ok=True)
    summary = {}
    for group, blocks in walk().items():
        text, desc = _digest(blocks)
        desc["heads"] = [h for h, _ in blocks]
        with open(os.path.join(out_dir, group.replace("/", "_") + ".txt"), "w") as f:
            f.write(text)
        summary[group] = desc
    with open(os.path.join(out_dir, "bn_plans.json"), "w") as f:
        json.dump(summary, f)


def run_walk(out_dir):
    """The walk in a fresh child process; full texts under out_dir, returns the summary."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_DROPPED}
    code = (f"import sys; sys.path[:0] = {[HERE, ROOT, os.path.join(ROOT, 'jama16-retina-replication_amd')]!r}; "
            f"import test_bn_plan as t; t._child_main({str(out_dir)!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)
    with open(os.path.join(out_dir, "bn_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    out = tmp_path_factory.mktemp("bn_plans")
    return out, run_walk(out)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_group(recorded):
    assert sorted(recorded) == sorted(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_bn_plans(group, walked, recorded):
    out, got = walked
    want, now = recorded[group], dict(got[group])
    heads = now.pop("heads")
    if now == want:
        return
    path = os.path.join(out, group.replace("/", "_") + ".txt")
    where = "the block or row counts differ"
    for i, (a, b) in enumerate(zip(want["blocks"].split(), now["blocks"].split())):
        if a != b:
            where = f"first differing block {i}: {heads[i]}"
            break
    raise AssertionError(f"{group}: the BN planner's output differs from the fixture ({want['rows']} rows recorded, "
                         f"{now['rows']} now; {where}; the full text is in {path})")


if __name__ == "__main__":
    import tempfile
    dump = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
    fixture = run_walk(dump)
    for desc in fixture.values():
        del desc["heads"]
    print(sum(d["rows"] for d in fixture.values()), "rows in", len(fixture), "groups; full texts in", dump)
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
