"""The bits of the BN and pool kernels, pinned (tests/golden/bn_bits.json).

The other BN / pool tests hold these kernels to each other (folded = three
launches, batch = multi, apply_multi = apply, fused pool = two kernels) and to
fp64 tolerances; a change that moves all of them together passes every one.
This test pins the output BYTES of every BN and max-pool entry point, fp32 and
bf16: one sha256 per case and output buffer (y / dx / dy / dbeta / mean /
invstd / argmax / absmax words), whole buffers, so the fill around a channel
slice is pinned with it.

Shapes are the smallest at which each index path exists (the planner side is
checked on the CPU by test_shapes_reach_their_paths):
  s98   m = 2*7*7 = 98, c = 48   fp32 tpr 12 (rpp 21, 4 idle threads), bf16
                                 tpr 6; fewer rows than one block's pass;
                                 folded channel groups 32 + 16
  s578  m = 2*17*17 = 578, c = 192   ragged row tail over several blocks, six
                                 folded channel groups
  seg3  s578 as segments 64 + 48 + 80 in channel slices of 256-wide buffers,
        x itself at channel 32 of a 256-wide buffer
  big   fp32 m = 8209, c = 1024  rpp 1, 514 chunks: the wave-per-channel
                                 finalize with a one-row last chunk
  pools n = 2 (4 grouped), 7x7 (all rows covered) and 8x8 (last row / column
        in no window: +0), c = 48 (blocks of 252 threads in the fused
        backward) and 192, outputs in slices of wider buffers.
Operands come from a seeded numpy generator; beta and mean leave a good share
of pre-activations on each side of 0 (asserted).  Every case runs twice and the
two runs must be byte-equal BEFORE anything is compared with the fixture.  The
JR_FOLD_BN_BWD=1 backward runs in a fresh child process (the knob is read once
per process).

`python tests/test_gpu_bn_bits.py` rewrites the fixture from the code as it
stands -- for a deliberate change of arithmetic order only.  It is never
re-recorded to make a refactor pass.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(GOLDEN, "bn_bits.json")
EPS = 1e-3
S98, S578, BIG = (98, 48), (578, 192), (8209, 1024)
SEG3 = (64, 48, 80)
WIDE, X_OFF = 256, 32            # seg3: every slice lives in a 256-wide buffer; x at channel 32
POOLS = [(2, 7, 7, 48), (2, 8, 8, 192), (2, 7, 7, 192), (2, 8, 8, 48)]
BN_CASES = ["stats", "apply", "apply_multi", "apply_stats", "apply_grouped", "bwd_multi", "bwd_multi_absmax",
            "bwd_frozen", "bwd_batch", "bwd_multi_fold"]
POOL_CASES = ["maxpool", "bn_maxpool_fwd", "bn_maxpool_bwd"]
CASES = [f"{c}-{dt}" for c in BN_CASES + POOL_CASES for dt in ("f32", "bf16")]
_KEEP = []


def _ffi():
    from jr import _ffi
    return _ffi


def _et(dt):
    return torch.bfloat16 if dt else torch.float32


def dev(a, dt=0):
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(_et(dt)).to("cuda")
    _KEEP.append(t)
    return t


def full(n, v, dtype=torch.float32):
    t = torch.full((int(n),), v, dtype=dtype, device="cuda")
    _KEEP.append(t)
    return t


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()).hexdigest()


def in_slice(a, off, stride, fill=3.0):
    """a [..., c] at channels [off, off + c) of a [..., stride] buffer of fill."""
    buf = np.full(a.shape[:-1] + (stride,), fill, np.float32)
    buf[..., off:off + a.shape[-1]] = a
    return buf


class Bn:
    """Operands of one (m, c) BN layer: post-conv-like x, statistics near its
    own, beta around 0 -- pre-activations on both sides of 0."""

    def __init__(self, m, c, dt, seed):
        rng = np.random.default_rng(seed)
        self.m, self.c, self.dt = m, c, dt
        off = rng.standard_normal(c)
        x = rng.standard_normal((m, c)) * 2 + off
        self.x = dev(x, dt).float().cpu().numpy()          # as stored in the path dtype
        self.mean = (off + rng.standard_normal(c) * 0.3).astype(np.float32)
        self.inv = rng.uniform(0.4, 1.5, c).astype(np.float32)
        self.beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
        self.dy = rng.standard_normal((m, c))
        pos = np.mean((self.x - self.mean) * self.inv + self.beta > 0)
        assert 0.25 < pos < 0.75, pos
        self.MEAN, self.INV, self.BETA = dev(self.mean), dev(self.inv), dev(self.beta)


def _bn_layers(dt):
    out = [("s98", Bn(*S98, dt, 1), (S98[1],), False), ("s578", Bn(*S578, dt, 2), (S578[1],), False),
           ("seg3", Bn(*S578, dt, 3), SEG3, True)]
    return out


def _x_of(b, sliced):
    """(X tensor, x_c_off, x_c_stride)"""
    if sliced:
        return dev(in_slice(b.x, X_OFF, WIDE), b.dt), X_OFF, WIDE
    return dev(b.x, b.dt), 0, b.c


def _bwd_segs(ffi, b, segs, sliced, need_dbeta=True):
    """jr_bn_seg array of the layer: segment k's dy in its own buffer (sliced: channels [8k + 8, ...) of a 256-wide
    one), one dbeta vector of fill 7."""
    arr = (ffi.BnSeg * len(segs))()
    DB = full(b.c, 7.0)
    o = 0
    for k, s in enumerate(segs):
        off, stride = (8 * k + 8, WIDE) if sliced else (0, s)
        DY = dev(in_slice(b.dy[:, o:o + s], off, stride, 9.0), b.dt)
        arr[k] = ffi.BnSeg(DY.data_ptr(), off, stride, s, b.BETA.data_ptr() + 4 * o,
                           DB.data_ptr() + 4 * o if need_dbeta else None)
        o += s
    _KEEP.append(arr)
    return arr, DB


def _ws(L, m, c):
    wsb = L.jr_bn_workspace_size(m, c)
    return full(wsb // 4 + 4, 0.0), wsb


def case_stats(ffi, L, dt):
    out = {}
    for name, (m, c), seed in (("s98", S98, 1), ("s578", S578, 2)) + ((("big", BIG, 4),) if dt == 0 else ()):
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((m, c)) * 2 + np.random.default_rng(seed + 50).standard_normal(c)
        X, ST = dev(x, dt), full(2 * c, 7.0)
        ws, wsb = _ws(L, m, c)
        ffi.check("stats", L.jr_bn_stats(dt, X.data_ptr(), m, c, EPS, ST.data_ptr(), ST.data_ptr() + 4 * c,
                                         ws.data_ptr(), wsb, None))
        out[f"{name}/mean_invstd"] = digest(ST)
    return out


def case_apply(ffi, L, dt):
    out = {}
    for name, b, segs, sliced in _bn_layers(dt):
        X, xo, xs = _x_of(b, sliced)
        yo, ys = (64, WIDE) if sliced else (0, b.c)
        Y = full(b.m * ys, 5.0, _et(dt))
        ffi.check("apply", L.jr_bn_relu_apply(dt, X.data_ptr(), xo, xs, b.m, b.c, b.MEAN.data_ptr(), b.INV.data_ptr(),
                                              b.BETA.data_ptr(), Y.data_ptr(), yo, ys, None))
        out[f"{name}/y"] = digest(Y)
    return out


def case_apply_multi(ffi, L, dt):
    out = {}
    for name, b, segs, sliced in _bn_layers(dt):
        X, xo, xs = _x_of(b, sliced)
        arr = (ffi.BnApplySeg * len(segs))()
        ys, o = [], 0
        for k, s in enumerate(segs):
            off, stride = (8 * k + 16, WIDE) if sliced else (0, s)
            ys.append(full(b.m * stride, 5.0, _et(dt)))
            arr[k] = ffi.BnApplySeg(ys[-1].data_ptr(), off, stride, s, b.BETA.data_ptr() + 4 * o)
            o += s
        ffi.check("apply_multi", L.jr_bn_relu_apply_multi(dt, len(segs), ctypes.byref(arr), X.data_ptr(), xo, xs, b.m,
                                                          b.c, b.MEAN.data_ptr(), b.INV.data_ptr(), None))
        for k, y in enumerate(ys):
            out[f"{name}/y{k}"] = digest(y)
    return out


def case_apply_stats(ffi, L, dt):
    """A 1x1 conv 64 -> 192 over 2x17x17 leaves single-stage partials; every member slice of 64 + 48 + 80 channels
    is finalized and applied from them."""
    n, hw, cin, cout = 2, 17, 64, sum(SEG3)
    code = ffi.JR_BF16 if dt else ffi.JR_F32_X8
    d = ffi.ConvDesc(n, hw, hw, cin, cout, 1, 1, 1, 1, 0, 0, hw, hw, 0, cin, 0, cout)
    rng = np.random.default_rng(5)
    M = n * hw * hw
    X, W = dev(rng.standard_normal(M * cin), dt), dev(rng.standard_normal(cin * cout) * 0.1, dt)
    BETA = dev(rng.standard_normal(cout) * 0.5)
    lay = ffi.BnPartials()
    ffi.check("layout", L.jr_conv2d_bn_partials_layout(ctypes.byref(d), code, ctypes.byref(lay)))
    assert lay.single_stage == 1 and lay.M == M and lay.N == cout
    wsb = L.jr_conv2d_workspace_size(ctypes.byref(d), 0, code)
    ws = full(wsb // 4 + 64, 0.0)
    RAW, ST = full(M * cout, 0.0, _et(dt)), full(2 * cout, 7.0)
    ffi.check("partials", L.jr_conv2d_fwd_bn_partials(ctypes.byref(d), code, X.data_ptr(), W.data_ptr(), RAW.data_ptr(),
                                                      ws.data_ptr(), wsb, None))
    out, co = {}, 0
    for k, c in enumerate(SEG3):
        Y = full(M * WIDE, 5.0, _et(dt))
        ffi.check("apply_stats", L.jr_bn_relu_apply_stats(
            dt, RAW.data_ptr(), co, cout, M, c, ws.data_ptr() + lay.ws_offset, lay.P, lay.R, cout, co, EPS,
            ST.data_ptr() + 4 * co, ST.data_ptr() + 4 * (cout + co), BETA.data_ptr() + 4 * co, Y.data_ptr(), 8 * k + 8,
            WIDE, None))
        out[f"conv17/y{k}"] = digest(Y)
        co += c
    out["conv17/mean_invstd"] = digest(ST)
    assert 0.25 < float((Y.view(M, WIDE)[:, 24:24 + 80] > 0).float().mean()) < 0.75
    return out


def case_apply_grouped(ffi, L, dt):
    m, c = S98
    bs = [Bn(m, c, dt, 6), Bn(m, c, dt, 7)]
    X = dev(np.stack([in_slice(b.x, 8, c + 16) for b in bs]), dt)
    ST = dev(np.stack([np.concatenate([b.mean, b.inv]) for b in bs]))
    BE = dev(np.stack([b.beta for b in bs]))
    Y = full(2 * m * (c + 24), 5.0, _et(dt))
    ffi.check("grouped", L.jr_bn_relu_apply_grouped(dt, 2, X.data_ptr(), 8, c + 16, m * (c + 16), m, c, ST.data_ptr(),
                                                    ST.data_ptr() + 4 * c, 2 * c, BE.data_ptr(), c, Y.data_ptr(), 16,
                                                    c + 24, m * (c + 24), None))
    return {"s98x2/y": digest(Y)}


def _bwd(ffi, L, dt, absmax):
    out = {}
    layers = _bn_layers(dt) + ([("big", Bn(*BIG, 0, 4), (BIG[1],), False)] if dt == 0 and not absmax else [])
    for name, b, segs, sliced in layers:
        X, xo, xs = _x_of(b, sliced)
        arr, DB = _bwd_segs(ffi, b, segs, sliced)
        DX = full(b.m * xs, 7.0, _et(dt))
        ws, wsb = _ws(L, b.m, b.c)
        args = (dt, len(segs), ctypes.byref(arr), X.data_ptr(), xo, xs, b.m, b.c, b.MEAN.data_ptr(), b.INV.data_ptr(),
                DX.data_ptr(), ws.data_ptr(), wsb)
        if absmax:
            WORDS = full(64, 0.0)
            ffi.check("bwd absmax", L.jr_bn_relu_bwd_multi_absmax(*args, WORDS.data_ptr(), None))
            out[f"{name}/absmax"] = digest(WORDS)
        else:
            ffi.check("bwd", L.jr_bn_relu_bwd_multi(*args, None))
        out[f"{name}/dx"] = digest(DX)
        out[f"{name}/dbeta"] = digest(DB)
    return out


def case_bwd_multi(ffi, L, dt):
    return _bwd(ffi, L, dt, False)


def case_bwd_multi_absmax(ffi, L, dt):
    return _bwd(ffi, L, dt, True)


def case_bwd_frozen(ffi, L, dt):
    out = {}
    for name, b, segs, sliced in _bn_layers(dt):
        X, xo, xs = _x_of(b, sliced)
        arr, _ = _bwd_segs(ffi, b, segs, sliced, need_dbeta=False)
        DX = full(b.m * xs, 7.0, _et(dt))
        ffi.check("frozen", L.jr_bn_relu_bwd_frozen(dt, len(segs), ctypes.byref(arr), X.data_ptr(), xo, xs, b.m, b.c,
                                                    b.MEAN.data_ptr(), b.INV.data_ptr(), DX.data_ptr(), None))
        out[f"{name}/dx"] = digest(DX)
    return out


def case_bwd_batch(ffi, L, dt):
    specs = _bn_layers(dt)
    layers = (ffi.BnBwdLayer * len(specs))()
    res = []
    for k, (name, b, segs, sliced) in enumerate(specs):
        X, xo, xs = _x_of(b, sliced)
        arr, DB = _bwd_segs(ffi, b, segs, sliced)
        DX = full(b.m * xs, 7.0, _et(dt))
        layers[k].nseg = len(segs)
        for j in range(len(segs)):
            layers[k].segs[j] = arr[j]
        layers[k].x, layers[k].x_c_off, layers[k].x_c_stride, layers[k].m, layers[k].c = X.data_ptr(), xo, xs, b.m, b.c
        layers[k].mean, layers[k].invstd, layers[k].dx = b.MEAN.data_ptr(), b.INV.data_ptr(), DX.data_ptr()
        res.append((name, DX, DB))
    wsb = L.jr_bn_relu_bwd_batch_workspace_size(len(specs), ctypes.byref(layers))
    assert wsb > 0
    ws = full(wsb // 4 + 64, 0.0)
    ffi.check("batch", L.jr_bn_relu_bwd_batch(dt, len(specs), ctypes.byref(layers), ws.data_ptr(), wsb, None))
    out = {}
    for name, DX, DB in res:
        out[f"{name}/dx"], out[f"{name}/dbeta"] = digest(DX), digest(DB)
    return out


class Pool:
    """One pool case: x (post-conv-like) at channel 8 of rows c + 24 wide, y at channel 16 of rows c + 40 wide, the
    fused backward's raw x / dx rows c + 8 wide (the layout of test_gpu_stem_pool)."""

    def __init__(self, ffi, shape, dt, seed, members=1):
        n, h, w, c = self.shape = shape
        self.dt, self.td = dt, _et(dt)
        self.xo, self.xs, self.yo, self.ys, self.xr = 8, c + 24, 16, c + 40, c + 8
        self.ho, self.wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        self.m = n * h * w
        rng = np.random.default_rng(seed)
        off = rng.standard_normal(c)
        self.x = dev(rng.standard_normal(shape) * 2 + off, dt).float().cpu().numpy()
        self.mean = (off + rng.standard_normal((members, c)) * 0.3).astype(np.float32)
        self.inv = rng.uniform(0.4, 1.5, (members, c)).astype(np.float32)
        self.beta = (rng.standard_normal((members, c)) * 0.5).astype(np.float32)
        pos = np.mean((self.x - self.mean[0]) * self.inv[0] + self.beta[0] > 0)
        assert 0.25 < pos < 0.75, pos
        self.pdy = rng.standard_normal((n, self.ho, self.wo, c))
        self.d = ffi.PoolDesc(n, h, w, c, self.ho, self.wo, self.xo, self.xs, self.yo, self.ys)
        self.X = dev(in_slice(self.x, self.xo, self.xs), dt)
        self.ST = dev(np.concatenate([self.mean, self.inv], axis=1))      # [members][mean c | invstd c]
        self.BETA = dev(self.beta)
        self.nout = n * self.ho * self.wo

    def outputs(self):
        return full(self.nout * self.ys, 5.0, self.td), full(self.nout * self.shape[3], 77, torch.uint8)


def case_maxpool(ffi, L, dt):
    out = {}
    for k, shape in enumerate(POOLS):
        p = Pool(ffi, shape, dt, 10 + k)
        name = "x".join(map(str, shape))
        Y, AM = p.outputs()
        ffi.check("mp fwd", L.jr_maxpool3x3s2_fwd(ctypes.byref(p.d), dt, p.X.data_ptr(), Y.data_ptr(), AM.data_ptr(),
                                                  None))
        out[f"{name}/y"], out[f"{name}/argmax"] = digest(Y), digest(AM)
        PDY = dev(in_slice(p.pdy, p.yo, p.ys, 9.0), dt)
        for acc in (0, 1):
            DX = dev(np.random.default_rng(20 + k).standard_normal(p.m * p.xs), dt)
            ffi.check("mp bwd", L.jr_maxpool3x3s2_bwd(ctypes.byref(p.d), dt, AM.data_ptr(), PDY.data_ptr(),
                                                      DX.data_ptr(), acc, None))
            out[f"{name}/dx_acc{acc}"] = digest(DX)
    return out


def case_bn_maxpool_fwd(ffi, L, dt):
    out = {}
    for k, shape in enumerate(POOLS):
        p = Pool(ffi, shape, dt, 10 + k)
        c, name = shape[3], "x".join(map(str, shape))
        Y, AM = p.outputs()
        ffi.check("fused fwd", L.jr_bn_relu_maxpool3x3s2_fwd(ctypes.byref(p.d), dt, p.X.data_ptr(), p.ST.data_ptr(),
                                                             p.ST.data_ptr() + 4 * c, p.BETA.data_ptr(), Y.data_ptr(),
                                                             AM.data_ptr(), None))
        out[f"{name}/y"], out[f"{name}/argmax"] = digest(Y), digest(AM)
        g = Pool(ffi, (4,) + shape[1:], dt, 30 + k, members=2)             # 2 members x 2 images
        Y, AM = g.outputs()
        ffi.check("grouped", L.jr_bn_relu_maxpool3x3s2_fwd_grouped(
            ctypes.byref(g.d), dt, 2, g.X.data_ptr(), g.ST.data_ptr(), g.ST.data_ptr() + 4 * c, 2 * c,
            g.BETA.data_ptr(), c, Y.data_ptr(), AM.data_ptr(), None))
        out[f"{name}/grouped_y"], out[f"{name}/grouped_argmax"] = digest(Y), digest(AM)
    return out


def case_bn_maxpool_bwd(ffi, L, dt):
    out = {}
    for k, shape in enumerate(POOLS):
        p = Pool(ffi, shape, dt, 10 + k)
        c, name = shape[3], "x".join(map(str, shape))
        Y, AM = p.outputs()
        ffi.check("fused fwd", L.jr_bn_relu_maxpool3x3s2_fwd(ctypes.byref(p.d), dt, p.X.data_ptr(), p.ST.data_ptr(),
                                                             p.ST.data_ptr() + 4 * c, p.BETA.data_ptr(), Y.data_ptr(),
                                                             AM.data_ptr(), None))
        PDY = dev(in_slice(p.pdy, p.yo, p.ys, 9.0), dt)
        XR = dev(in_slice(p.x, 0, p.xr), dt)
        wsb = L.jr_bn_relu_bwd_maxpool_workspace_size(ctypes.byref(p.d))
        ws = full(wsb // 4 + 4, 0.0)
        for form in ("plain", "absmax"):
            DY, DX, DB = full(p.m * p.xs, 7.0, p.td), full(p.m * p.xr, 7.0, p.td), full(c, 7.0)
            args = (dt, ctypes.byref(p.d), AM.data_ptr(), PDY.data_ptr(), DY.data_ptr(), XR.data_ptr(), p.xr,
                    p.ST.data_ptr(), p.ST.data_ptr() + 4 * c, p.BETA.data_ptr(), DX.data_ptr(), DB.data_ptr(),
                    ws.data_ptr(), wsb)
            if form == "plain":
                ffi.check("fused bwd", L.jr_bn_relu_bwd_maxpool(*args, None))
            else:
                WORDS = full(64, 0.0)
                ffi.check("fused bwd absmax", L.jr_bn_relu_bwd_maxpool_absmax(*args, WORDS.data_ptr(), None))
                out[f"{name}/{form}/words"] = digest(WORDS)
            for key, t in (("dy", DY), ("dx", DX), ("dbeta", DB)):
                out[f"{name}/{form}/{key}"] = digest(t)
    return out


def run_case(case):
    """{output: sha256} of one case; two runs, byte-equal."""
    ffi = _ffi()
    ffi.init(0)
    L = ffi.load()
    name, dtn = case.rsplit("-", 1)
    fn = globals()["case_" + name]
    runs = []
    for rep in range(2):
        runs.append(fn(ffi, L, 1 if dtn == "bf16" else 0))
        torch.cuda.synchronize()
        _KEEP.clear()
    for k in runs[0]:
        assert runs[0][k] == runs[1][k], f"{case} {k}: two runs of the same call differ"
    return runs[0]


def _fold_child(path):
    """(child process, JR_FOLD_BN_BWD=1) the single-stage backwards through k_bn_relu_bwd_apply_fold"""
    assert os.environ.get("JR_FOLD_BN_BWD") == "1"
    with open(path, "w") as f:
        json.dump({f"bwd_multi_fold-{dtn}": run_case(f"bwd_multi-{dtn}") for dtn in ("f32", "bf16")}, f)


_FOLDED = {}


def measure(case):
    if not case.startswith("bwd_multi_fold"):
        return run_case(case)
    if not _FOLDED:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "fold.json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fold-child", path], capture_output=True,
                               text=True, timeout=120, env=dict(os.environ, JR_FOLD_BN_BWD="1"))
            if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                pytest.exit(f"the folded-backward child died ({r.returncode}): no further GPU work\n"
                            f"{r.stderr[-2000:]}", 1)
            assert r.returncode == 0, r.stderr[-3000:]
            with open(path) as f:
                _FOLDED.update(json.load(f))
    return _FOLDED[case]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)


def test_shapes_reach_their_paths():
    """(CPU) what the docstring says of the shapes, from the planner."""
    ffi = _ffi()
    for dt, vw in ((0, 4), (1, 8)):
        p = ffi.bn_plan(dt, *S98)
        assert p.vec_width == vw and p.apply_grid == (2 if dt == 0 else 1)     # bf16: fewer rows than one block's pass
        assert (p.nchunks, p.single_stage, p.fold_grid_y) == (1, 1, 2) and S98[1] % 32 == 16
        p = ffi.bn_plan(dt, *S578)
        assert p.apply_grid > 2 and S578[0] % (256 // (S578[1] // vw)) != 0 and p.single_stage == 1
        assert p.fold_grid_y == 6 and p.fold_grid_x > 1
    assert 256 % (S98[1] // 4) == 4                              # fp32 tpr 12: 4 idle threads
    p = ffi.bn_plan(0, *BIG)
    assert (p.rows_per_chunk, p.nchunks, p.single_stage) == (16, 514, 0) and BIG[0] % 16 == 1
    assert p.finalize_grid == p.stats_finalize_grid == BIG[1] // 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_bn_bits(case, recorded):
    got, want = measure(case), recorded[case]
    assert sorted(got) == sorted(want)
    moved = [k for k in sorted(got) if got[k] != want[k]]
    assert not moved, f"{case}: {len(moved)} of {len(got)} outputs changed bits: {moved}"


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--fold-child":
        _fold_child(sys.argv[2])
        sys.exit(0)
    fixture = {c: measure(c) for c in CASES}
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes,", sum(len(v) for v in fixture.values()), "digests")
