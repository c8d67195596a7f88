"""The conv planner's output, pinned on the CPU: for every distinct conv
geometry of Inception-v3 at three workloads, every conv dtype, every op (and
DGRAD stride phase) and every config id -- alone and with split fields 1, 3
and 16 (on a stream-K id the split field is the grid size) -- what the C ABI
reports after jr_conv2d_set_config must equal the record in
tests/golden/conv_plans.json: jr_conv2d_get_config, jr_conv2d_workspace_size,
for WGRAD every integer field of jr_conv2d_wgrad_seg (M, N, the split-K
factor, the reduce lanes and blocks), for FWD every field of
jr_conv2d_bn_partials_layout (the statistics-partials layout and the slab
bytes in front of it).  None of these entry points makes a HIP call, so no
device is needed.  A second, small record covers the stem's first conv with
JR_CONV1_DIRECT=1 (the direct kernel changes the partials layout and the
workspace).

What this record does not see: DGRAD split-K factors show only through
get_config and the workspace size.  They, and the correctness of every id of
every dtype, stay covered by the GPU sweeps against fp64 (test_gpu_ops,
test_gpu_x6h, test_gpu_bf16, test_gpu_x8p, test_gpu_streamk, test_gpu_fused,
test_gpu_fold).

The fixture keeps one sha256 and one row count per (workload, dtype, op), and
a short digest per (conv geometry, phase) block so that a mismatch can name
where it starts.  The walk runs in a fresh child process without
JR_WGRAD_SPLIT_TARGET, JR_WGRAD_SPLIT_KMAX and JR_CONV1_DIRECT: the library
reads those once per process, and tile overrides are process-wide.

`python tests/test_conv_plan.py [DIR]` rewrites the fixture from the code as it
stands (a deliberate change of the planner) and, with DIR, dumps the full
texts there, so two commits can be diffed.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "conv_plans.json")
WORKLOADS = {"res107_b4": (107, 4), "res299_b64": (299, 64), "res587_b2": (587, 2)}
DTYPES = (0, 1, 2, 3, 4)                 # JR_F32, JR_BF16, JR_F32_X8, JR_F32_X8P, JR_F32_X6H
OPS = ("fwd", "dgrad", "wgrad")         # JR_CONV_FWD, JR_CONV_BWD_DATA, JR_CONV_BWD_FILTER
SPLIT_FIELDS = (0, 1, 3, 16)
ENV_DROPPED = ("JR_WGRAD_SPLIT_TARGET", "JR_WGRAD_SPLIT_KMAX", "JR_CONV1_DIRECT")
GROUPS = [f"{w}/dt{dt}/{op}" for w in WORKLOADS for dt in DTYPES for op in OPS]
DIRECT_GROUPS = [f"direct/{w}/dt{dt}/fwd" for w in WORKLOADS for dt in (0, 2)]


def _geometries(res, batch, dtype, stem_only=False):
    """Distinct conv descriptors of the workload as the engine binds them for
    `dtype` (channel padding 8 for bf16 / x8p, else 4), with has_dgrad."""
    from jr import _ffi
    from jr.inception import build_inception_v3
    from jr.plan import build_plan
    g = build_inception_v3(res, res, 1)
    q = 8 if dtype in (_ffi.JR_BF16, _ffi.JR_F32_X8P) else 4
    seen, out = set(), []
    for u in build_plan(g, True).units:
        stem = u.x == g.input_buf
        if stem_only and not stem:
            continue
        pad = (u.cin + q - 1) // q * q
        xs = pad if stem or dtype == _ffi.JR_F32_X8P else u.cin
        key = (batch, u.h, u.w, u.cin, u.cout, u.kh, u.kw, u.stride, u.stride, u.pad_h, u.pad_w, u.ho, u.wo,
               0, xs, 0, u.cout)
        if key not in seen:
            seen.add(key)
            out.append((key, not stem))
    return out


def _block(lib, key, op, dtype, phase):
    """The rows of one (geometry, op, phase): one per config id and split field."""
    from jr import _ffi
    d = _ffi.ConvDesc(*key)
    ref = ctypes.byref(d)
    head = "x".join(map(str, key)) + f" {OPS[op]} p{phase}"
    rows = []
    ids = [-1] + [c | (s << 8) for s in SPLIT_FIELDS for c in range(lib.jr_conv2d_num_configs(dtype))]
    for cfg in ids:
        _ffi.check("set_config", lib.jr_conv2d_set_config(ref, op, dtype, phase, cfg))
        row = [head, f"cfg={cfg}", f"get={lib.jr_conv2d_get_config(ref, op, dtype, phase)}",
               f"ws={lib.jr_conv2d_workspace_size(ref, op, dtype)}"]
        if op == _ffi.JR_CONV_BWD_FILTER:
            seg = _ffi.WgradSeg()
            _ffi.check("wgrad_seg", lib.jr_conv2d_wgrad_seg(ref, dtype, ctypes.byref(seg)))
            row.append("seg=" + ",".join(str(getattr(seg, n)) for n in
                                         ("m", "n", "splits", "c_in", "c_pad", "g", "block0", "blocks")))
        if op == _ffi.JR_CONV_FWD:
            lay = _ffi.BnPartials()
            _ffi.check("bn_partials_layout", lib.jr_conv2d_bn_partials_layout(ref, dtype, ctypes.byref(lay)))
            row.append("bn=" + ",".join(str(getattr(lay, n)) for n in ("ws_offset", "P", "R", "M", "N", "single_stage")))
        rows.append(" ".join(row))
    _ffi.check("set_config", lib.jr_conv2d_set_config(ref, op, dtype, phase, -1))
    return head, rows


def walk(direct=False):
    """{group: [(block head, rows), ...]} -- runs in the child process."""
    from jr import _ffi
    lib = _ffi.load()
    out = {}
    for wname, (res, batch) in WORKLOADS.items():
        for dt in (0, 2) if direct else DTYPES:
            geoms = _geometries(res, batch, dt, stem_only=direct)
            for op, opname in enumerate(OPS):
                if direct and op != _ffi.JR_CONV_FWD:
                    continue
                blocks = []
                for key, has_dgrad in geoms:
                    stride = key[7]
                    if op == _ffi.JR_CONV_BWD_DATA:
                        phases = range(stride * stride) if has_dgrad else ()
                    else:
                        phases = (0,)
                    blocks += [_block(lib, key, op, dt, p) for p in phases]
                out[("direct/" if direct else "") + f"{wname}/dt{dt}/{opname}"] = blocks
    return out


def _digest(blocks):
    text = "".join(r + "\n" for _, rows in blocks for r in rows)
    return text, {"sha256": hashlib.sha256(text.encode()).hexdigest(), "rows": text.count("\n"),
                  "blocks": " ".join(hashlib.sha256("\n".join(rows).encode()).hexdigest()[:8] for _, rows in blocks)}


def _child_main(out_dir, direct):
    os.makedirs(out_dir, exist_ok=True)
    summary = {}
    for group, blocks in walk(direct).items():
        text, desc = _digest(blocks)
        desc["heads"] = [h for h, _ in blocks]
        with open(os.path.join(out_dir, group.replace("/", "_") + ".txt"), "w") as f:
            f.write(text)
        summary[group] = desc
    with open(os.path.join(out_dir, "direct.json" if direct else "plans.json"), "w") as f:
        json.dump(summary, f)


def run_walk(out_dir, direct=False):
    """The walk in a fresh child process; full texts under out_dir, returns the summary."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_DROPPED}
    if direct:
        env["JR_CONV1_DIRECT"] = "1"
    code = (f"import sys; sys.path[:0] = {[HERE, ROOT, os.path.join(ROOT, 'jama16-retina-replication_amd')]!r}; "
            f"import test_conv_plan as t; t._child_main({str(out_dir)!r}, {direct!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)
    with open(os.path.join(out_dir, "direct.json" if direct else "plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    out = tmp_path_factory.mktemp("conv_plans")
    return out, {**run_walk(out), **run_walk(out, direct=True)}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_group(recorded):
    assert sorted(recorded) == sorted(GROUPS + DIRECT_GROUPS)


@pytest.mark.parametrize("group", GROUPS + DIRECT_GROUPS)
def test_conv_plans(group, walked, recorded):
    out, got = walked
    want, now = recorded[group], got[group]
    heads = now.pop("heads")
    if now == want:
        return
    path = os.path.join(out, group.replace("/", "_") + ".txt")
    where = "the block counts differ"
    first = 0
    for i, (a, b) in enumerate(zip(want["blocks"].split(), now["blocks"].split())):
        if a != b:
            per = now["rows"] // len(heads)
            where, first = f"first differing block {i}: {heads[i]}", i * per
            break
    raise AssertionError(f"{group}: the planner's output differs from the fixture ({want['rows']} rows recorded, "
                         f"{now['rows']} now; {where}, from row {first} of the full text written to {path})")


if __name__ == "__main__":
    import tempfile
    dump = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
    fixture = {**run_walk(dump), **run_walk(dump, direct=True)}
    for desc in fixture.values():
        del desc["heads"]
    print(sum(d["rows"] for d in fixture.values()), "rows in", len(fixture), "groups; full texts in", dump)
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
