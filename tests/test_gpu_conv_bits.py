"""The bits of every conv config id, pinned (tests/golden/conv_bits.json).

The every-config sweeps (test_gpu_ops.py, test_gpu_bf16.py, test_gpu_x8p.py,
test_gpu_x6h.py, test_gpu_streamk.py) hold each id to fp64 tolerances.  The
library also promises bitwise reproducible results -- fixed sum order, fixed
split-K slabs and stream-K cut points, no float atomics -- and a change of
index code can keep every tolerance and still move a K-tile to another block.
This test pins the output BYTES of fwd / dgrad / wgrad for all five conv
dtypes, every id of jr_conv2d_num_configs(dt) with split field 0 (the
planner's choice) and 3 (three split-K slabs; on a stream-K id a three-block
grid, so tiles are cut and handed off), halo ids with 0 and 2, on the
smallest shapes of the sweeps at which each address path exists:
  (2,17,17,64,96,3,3,1,same)   wave-uniform tap
  (2,17,17,48,64,3,3,2,valid)  four dgrad stride phases; c_in 48 is not a
                               multiple of every BK: incremental / mixed-radix
  (2,11,11,3,32,3,3,2,valid)   conv1's virtual channel padding (fwd, wgrad)
  bf16 halo ids only: two 8x8 cases whose BM tile spans two images, and one
  with ragged M / N tails.
Operands are the sweeps' own (their helpers, imported).  Every conv runs
twice and the two outputs must be byte-equal BEFORE anything is compared with
the fixture: a nondeterministic kernel shows up as that, not as a moved digest.

Fixture: per (dtype, case) and op one sha256 over the output bytes in config
order, and one 8-hex digest per config in one string, so a mismatch names the
first config id that moved.  `python tests/test_gpu_conv_bits.py` rewrites it
from the code as it stands -- for a deliberate change of arithmetic order
only, never to make a refactor pass.
"""
import ctypes
import hashlib
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_gpu_bf16 as T_BF16  # noqa: E402
import test_gpu_ops as T_OPS  # noqa: E402
import test_gpu_x6h as T_X6H  # noqa: E402
import test_gpu_x8p as T_X8P  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "conv_bits.json")
F32, BF16, X8, X8P, X6H = 0, 1, 2, 3, 4
DT_NAMES = {F32: "f32", BF16: "bf16", X8: "x8", X8P: "x8p", X6H: "x6h"}

SHAPES = [(2, 17, 17, 64, 96, 3, 3, 1, "same"), (2, 17, 17, 48, 64, 3, 3, 2, "valid"),
          (2, 11, 11, 3, 32, 3, 3, 2, "valid")]
HALO_SHAPES = [(2, 8, 8, 384, 384, 1, 3, 1, "same"), (2, 8, 8, 384, 384, 3, 1, 1, "same"),
               (1, 29, 31, 32, 48, 3, 3, 1, "same")]
GROUPS = [(dt, c, False) for dt in (F32, BF16, X8, X8P, X6H) for c in SHAPES] + [(BF16, c, True) for c in HALO_SHAPES]


def _gid(group):
    dt, case, halo = group
    return DT_NAMES[dt] + ("-halo-" if halo else "-") + "x".join(str(v) for v in case)


def _cfgs(L, dt, halo):
    """Config ids in fixture order: tile | split << 8."""
    if halo:
        return [t | (sp << 8) for t in T_BF16.HALO_IDS for sp in (0, 2)]
    return [t | (sp << 8) for t in range(L.jr_conv2d_num_configs(dt))
            for sp in ((0, 2) if dt == BF16 and t in T_BF16.HALO_IDS else (0, 3))]


def _bytes(t):
    torch.cuda.synchronize()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()


def _set_all(ffi, L, d, dt, s, cfg):
    for op in (0, 2):
        ffi.check("set", L.jr_conv2d_set_config(ctypes.byref(d), op, dt, 0, cfg))
    for ph in range(s * s):
        ffi.check("set", L.jr_conv2d_set_config(ctypes.byref(d), 1, dt, ph, cfg))


def _fp32_tensor_outputs(ffi, L, dt, case, cfgs):
    """JR_F32 / JR_F32_X8 (the operands of test_conv_every_tile_config) and
    JR_F32_X6H (those of test_x6h_every_tile_config, with its magnitude words):
    yields, per config, two runs of {op: bytes}."""
    n, h, w, cin, cout, kh, kw, s, pad = case
    if dt == X6H:
        d, (x, wt, dy), (X, W, DY), keep = T_X6H._setup(ffi, case, 7)
        cs = (cin + 3) // 4 * 4
        wsb = max(L.jr_conv2d_workspace_size(ctypes.byref(d), op, dt) for op in range(3))
        wsb += 3 * 4 * max(dy.size, kh * kw * cs * cout, n * h * w * cs)
        ws = torch.zeros(wsb // 4 + 4, device="cuda")
    else:
        d, (x, wt, dy), (X, W, DY), (ws, wsb) = T_OPS._sweep_setup(ffi, L, case, dt)
    try:
        for cfg in cfgs:
            _set_all(ffi, L, d, dt, s if cin % 4 == 0 else 0, cfg)
            runs = []
            for rep in range(2):
                Y, DW = torch.zeros(dy.size, device="cuda"), torch.zeros(wt.size, device="cuda")
                DX = torch.zeros(X.numel(), device="cuda")
                ffi.check("fwd", L.jr_conv2d_fwd(ctypes.byref(d), dt, X.data_ptr(), W.data_ptr(), Y.data_ptr(),
                                                 ws.data_ptr(), wsb, None))
                ffi.check("wgrad", L.jr_conv2d_bwd_filter(ctypes.byref(d), dt, X.data_ptr(), DY.data_ptr(),
                                                          DW.data_ptr(), ws.data_ptr(), wsb, None))
                out = {"fwd": Y, "wgrad": DW}
                if cin % 4 == 0:
                    ffi.check("dgrad", L.jr_conv2d_bwd_data(ctypes.byref(d), dt, DY.data_ptr(), W.data_ptr(),
                                                            DX.data_ptr(), 0, ws.data_ptr(), wsb, None))
                    out["dgrad"] = DX
                runs.append({op: _bytes(t) for op, t in out.items()})
            yield cfg, runs
        ffi.device_check()
    finally:
        _set_all(ffi, L, d, dt, s if cin % 4 == 0 else 0, -1)
        torch.cuda.synchronize()
        T_OPS._KEEP.clear()


def _bf16_operand_outputs(ffi, L, dt, case, cfgs, halo):
    """JR_BF16 (test_gpu_bf16._run_all) and JR_F32_X8P (test_gpu_x8p._run)."""
    n, h, w, cin, cout, kh, kw, s, pad = case
    run = T_BF16._run_all if dt == BF16 else T_X8P._run
    keep = T_BF16._KEEP if dt == BF16 else T_X8P._KEEP
    extra = max(3 * 4 * max(n * h * w * 8 * cout, kh * kw * 8 * cout) * 4, 4 * 4 * n * h * w * 8 * cout)
    c8 = (cin + 7) // 8 * 8
    d = T_BF16._desc(ffi, n, h, w, cin, cout, kh, kw, s, pad, c8)[0]
    try:
        for cfg in cfgs:
            runs = []
            for rep in range(2):
                raw = {}
                run(ffi, L, case, seed=21 if halo else 11, cfg=cfg, extra_ws=extra, raw=raw)
                runs.append({op: _bytes(t) for op, t in raw.items()})
                torch.cuda.synchronize()
                keep.clear()
            yield cfg, runs
        ffi.device_check()
    finally:
        _set_all(ffi, L, d, dt, s if cin % 8 == 0 else 0, -1)


def measure(group):
    """{op: {"sha256", "cfgs"}} of one (dtype, case) group; asserts run-to-run equality."""
    from jr import _ffi as ffi
    ffi.init(0)
    L = ffi.load()
    dt, case, halo = group
    cfgs = _cfgs(L, dt, halo)
    gen = (_bf16_operand_outputs(ffi, L, dt, case, cfgs, halo) if dt in (BF16, X8P)
           else _fp32_tensor_outputs(ffi, L, dt, case, cfgs))
    whole, short = {}, {}
    for cfg, (a, b) in gen:
        for op in a:
            assert a[op] == b[op], f"{_gid(group)} {op}: config {cfg & 0xFF} split {cfg >> 8} differs between two runs"
            whole.setdefault(op, hashlib.sha256()).update(a[op])
            short.setdefault(op, []).append(hashlib.sha256(a[op]).hexdigest()[:8])
    return {op: {"sha256": whole[op].hexdigest(), "cfgs": " ".join(short[op])} for op in sorted(whole)}, cfgs


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_group(recorded):
    assert sorted(recorded) == sorted(_gid(g) for g in GROUPS)


@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_conv_bits(group, recorded):
    got, cfgs = measure(group)
    want = recorded[_gid(group)]
    assert sorted(got) == sorted(want)
    for op in got:
        if got[op] == want[op]:
            continue
        g, w = got[op]["cfgs"].split(), want[op]["cfgs"].split()
        assert len(g) == len(w) == len(cfgs), (op, len(g), len(w), len(cfgs))
        first = next(i for i in range(len(g)) if g[i] != w[i])
        moved = sum(a != b for a, b in zip(g, w))
        raise AssertionError(f"{_gid(group)} {op}: {moved} of {len(g)} configs changed bits; first: config "
                             f"{cfgs[first] & 0xFF} split {cfgs[first] >> 8} ({w[first]} -> {g[first]})")


if __name__ == "__main__":
    fixture = {_gid(g): measure(g)[0] for g in GROUPS}
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
