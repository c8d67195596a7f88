"""Per-block timeline of one conv GEMM launch from the stamps build
(`make -C jama16-retina-replication_amd/csrc stamps` -> jr/libjr_stamps.so;
Stamps in jr_conv_impl.h): where a block's cycles go -- set-up (row / tap /
column decode, then the ring fill up to the first barrier), K loop, of which
vmcnt waits + barriers, stream-K hand-off (publish / count / absorb; the x6h
scale-back of the accumulators is counted here), epilogue -- summed over the
(tile, K range) segments a stream-K block runs, how many blocks share a CU
over the launch, and the clock the chip held.
Diagnostic only (the stamps cost a few % of the loop).
  python tools/conv_stamps.py <dtype 0|1|2|3|4> <op 0|1|2> <layer> <cfg> [reps]
  python tools/conv_stamps.py six [reps]
`six`: the fixed-cost table of six GEMMs of the 299^2 B=64 fp32 x6h training
step at the configs of the committed tile table (jr/tiles_mi355x.json)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "jama16-retina-replication_amd")
os.environ.setdefault("JR_LIB_DIAG", os.path.join(PKG, "jr", "libjr_stamps.so"))
sys.path.insert(0, PKG)
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from jr import _ffi  # noqa: E402

# (n, h, w, c_in, c_out, kh, kw, stride, pad_h, pad_w)
LAYERS = {"c17x7": (64, 17, 17, 192, 192, 1, 7, 1, 0, 3), "c17x1": (64, 17, 17, 768, 192, 1, 1, 1, 0, 0),
          "c35x3": (64, 35, 35, 64, 96, 3, 3, 1, 1, 1), "c8x3": (64, 8, 8, 384, 384, 1, 3, 1, 0, 1),
          "conv5": (64, 73, 73, 80, 192, 3, 3, 1, 0, 0), "conv3": (64, 147, 147, 32, 64, 3, 3, 1, 1, 1),
          "c8x33": (64, 8, 8, 448, 384, 3, 3, 1, 1, 1), "m17": (64, 17, 17, 768, 512, 1, 1, 1, 0, 0),
          "c35x5": (64, 35, 35, 48, 64, 5, 5, 1, 2, 2), "c8x1": (64, 8, 8, 2048, 1152, 1, 1, 1, 0, 0),
          "c17x1f": (64, 17, 17, 768, 576, 1, 1, 1, 0, 0), "c35x3b": (64, 35, 35, 96, 96, 3, 3, 1, 1, 1),
          "conv27": (64, 35, 35, 288, 384, 3, 3, 2, 0, 0)}
# `six`: (title, layer, op, unit of the tile table, DGRAD phase read)
SIX = [("17^2 1x7 192->192 fwd", "c17x7", 0, "conv2d_63", 0), ("17^2 1x7 192->192 dgrad", "c17x7", 1, "conv2d_63", 0),
       ("17^2 1x7 192->192 wgrad", "c17x7", 2, "conv2d_63", 0),
       ("17^2 1x1 fused 768->576 fwd", "c17x1f", 0, "conv2d_61+62+65", 0),
       ("35^2 3x3 96->96 fwd", "c35x3b", 0, "conv2d_11", 0), ("8^2 1x3 384->384 dgrad", "c8x3", 1, "conv2d_79", 0),
       ("conv2d_5 dgrad", "conv5", 1, "conv2d_5", 0), ("conv2d_27 dgrad phase 0", "conv27", 1, "conv2d_27", 0)]
WORDS = 16                 # kStampWords
REGION = WORDS << 16       # words per launch (jr_debug_set_stamps)


def stamp(L, dt, op, layer, cfgs, phase, reps):
    """Stamps [blocks][WORDS] of launch `phase` of one run of the op at config ids cfgs (one per DGRAD phase)."""
    n, h, w, ci, co, kh, kw, s, ph, pw = LAYERS[layer]
    ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    q = 8 if dt in (1, 3) else 4
    cs = (ci + q - 1) // q * q
    d = _ffi.ConvDesc(n, h, w, ci, co, kh, kw, s, s, ph, pw, ho, wo, 0, cs, 0, co)
    d.x_bound = d.w_bound = d.dy_bound = 8.0      # JR_F32_X6H: host magnitude bounds of the test data
    pl = 3 if dt == 3 else 1
    et = torch.bfloat16 if dt in (1, 3) else torch.float32
    x = torch.randn(pl * n * h * w * cs, device="cuda").clamp_(-7, 7).to(et)
    wt = (torch.randn(pl * kh * kw * cs * co, device="cuda") * 0.05).to(et)
    dy = torch.randn(pl * n * ho * wo * co, device="cuda").clamp_(-7, 7).to(et)
    ot = torch.bfloat16 if dt == 1 else torch.float32
    y = torch.zeros(n * ho * wo * co, device="cuda", dtype=ot)
    dx = torch.zeros(n * h * w * cs, device="cuda", dtype=ot)
    dw = torch.zeros(kh * kw * cs * co, device="cuda")
    wsb = 1 << 30
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for p in range(s * s if op == 1 else 1):
        _ffi.check("set", L.jr_conv2d_set_config(ctypes.byref(d), op, dt, p, cfgs[p if p < len(cfgs) else 0]))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def run():
        if op == 0:
            return L.jr_conv2d_fwd(ctypes.byref(d), dt, P(x), P(wt), P(y), P(ws), wsb, None)
        if op == 1:
            return L.jr_conv2d_bwd_data(ctypes.byref(d), dt, P(dy), P(wt), P(dx), 0, P(ws), wsb, None)
        return L.jr_conv2d_bwd_filter(ctypes.byref(d), dt, P(x), P(dy), P(dw), P(ws), wsb, None)

    stamps = torch.zeros(REGION * (s * s if op == 1 else 1), dtype=torch.int64, device="cuda")
    for _ in range(reps):
        _ffi.check("warm", run())
    torch.cuda.synchronize()
    L.jr_debug_set_stamps(P(stamps))
    _ffi.check("stamped", run())
    torch.cuda.synchronize()
    L.jr_debug_set_stamps(None)
    st = stamps[phase * REGION:(phase + 1) * REGION].view(-1, WORDS).cpu().numpy().astype(np.int64)
    return st[st[:, 1] > 0]


def shares(st):
    """(set-up, of which decode, loop, of which waits, hand-off, epilogue) shares of block cycles, segments per block."""
    tot = float((st[:, 2] + st[:, 3] + st[:, 4] + st[:, 8]).sum())
    return [st[:, c].sum() / tot for c in (2, 10, 3, 5, 8, 4)], st[:, 9].mean()


def report(title, st):
    nb = len(st)
    r0, r1 = st[:, 0], st[:, 1]
    wall = (r1.max() - r0.min()) * 10e-3          # 100 MHz ticks -> us
    cyc = st[:, 2] + st[:, 3] + st[:, 4] + st[:, 8]
    dur = (r1 - r0) * 10e-3
    clock = np.median(cyc / np.maximum(r1 - r0, 1)) * 100e6 / 1e9
    hw, xcc = st[:, 6], st[:, 7] & 0xF
    cu = (hw >> 8) & 0xF
    sh = (hw >> 12) & 0x1
    se = (hw >> 13) & 0x7
    cu_key = xcc * 1000 + se * 100 + sh * 16 + cu
    ncu = len(np.unique(cu_key))
    busy = dur.sum() / (wall * ncu)
    print(f"{title}: {nb} blocks on {ncu} CUs, launch {wall:.1f} us, "
          f"clock {clock:.2f} GHz, mean resident blocks per CU {busy:.2f}")
    seg = np.maximum(st[:, 9], 1)
    for name, v in (("block duration us", dur), ("segments per block", st[:, 9]),
                    ("  that handed on", st[:, 11]), ("set-up kcyc / segment", st[:, 2] / seg / 1e3),
                    ("  decode kcyc / segment", st[:, 10] / seg / 1e3), ("K loop kcyc / segment", st[:, 3] / seg / 1e3),
                    ("  waits+barriers kcyc", st[:, 5] / seg / 1e3), ("hand-off kcyc / segment", st[:, 8] / seg / 1e3),
                    ("epilogue kcyc / block", st[:, 4] / 1e3)):
        print(f"  {name:24s} mean {v.mean():8.2f}  p10 {np.percentile(v, 10):8.2f}  p50 {np.median(v):8.2f}  "
              f"p90 {np.percentile(v, 90):8.2f}  max {v.max():8.2f}")
    (su, dc, lp, wt, ho, ep), _ = shares(st)
    print(f"  share of block cycles: set-up {su:.3f} (decode {dc:.3f})  loop {lp:.3f} (waits {wt:.3f})  "
          f"hand-off {ho:.3f}  epilogue {ep:.3f}  | fixed (set-up + hand-off + epilogue) {su + ho + ep:.3f}")
    # start skew: how the blocks enter over the launch
    t = (r0 - r0.min()) * 10e-3
    print(f"  block start times us: p10 {np.percentile(t, 10):.1f} p50 {np.median(t):.1f} p90 {np.percentile(t, 90):.1f}"
          f"  last end {wall:.1f}")
    blocks_per_cu = np.bincount(np.unique(cu_key, return_inverse=True)[1])
    print(f"  blocks per CU: min {blocks_per_cu.min()} mean {blocks_per_cu.mean():.2f} max {blocks_per_cu.max()}")
    return wall


def main():
    _ffi.init(0)
    L = _ffi.load()
    L.jr_debug_set_stamps.restype = ctypes.c_int
    L.jr_debug_set_stamps.argtypes = [ctypes.c_void_p]
    if sys.argv[1] != "six":
        dt, op, layer, cfg = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
        reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
        report(f"{layer} dtype {dt} op {op} cfg {cfg}", stamp(L, dt, op, layer, [cfg], 0, reps))
        return
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    tables = json.load(open(os.path.join(PKG, "jr", "tiles_mi355x.json")))["tables"]
    table = [t for t in tables if (t["conv_math"], t["batch"], t["height"], t["train"]) == ("x6h", 64, 299, True)][0]
    rows = []
    for title, layer, op, unit, phase in SIX:
        f, wg, dg = table["configs"][unit]
        cfgs = [f] if op == 0 else [wg] if op == 2 else list(dg)
        st = stamp(L, 4, op, layer, cfgs, phase, reps)
        wall = report(f"{title} (x6h, config id {cfgs[phase]})", st)
        rows.append((title, cfgs[phase], len(st), wall, shares(st)))
    print("\nshares of block cycles (wave 0 of every block, one launch)")
    print(f"{'GEMM':28s} {'id':>6s} {'blocks':>6s} {'us':>7s} {'seg/blk':>7s} {'set-up':>7s} {'(decode)':>8s} {'loop':>6s} "
          f"{'(waits)':>7s} {'hand-off':>8s} {'epilogue':>8s} {'fixed':>6s}")
    for title, cfg, nb, wall, ((su, dc, lp, wt, ho, ep), seg) in rows:
        print(f"{title:28s} {cfg:6d} {nb:6d} {wall:7.1f} {seg:7.2f} {su:7.3f} {dc:8.3f} {lp:6.3f} {wt:7.3f} {ho:8.3f} "
              f"{ep:8.3f} {su + ho + ep:6.3f}")


if __name__ == "__main__":
    main()
