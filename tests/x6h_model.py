"""A bit-exact numpy model of the JR_F32_X6H operand split (include/jr.h,
csrc/jr_conv_impl.h pow2_scale, csrc/jr_conv.hip SplitFrag16), and the inputs
of test_gpu_x6h_scales.py (shared with test_x6h_model.py, which checks on the
CPU that the model meets the jr.h contract on them and that every GPU case
would notice a lost fp16 subnormal).

The split is deterministic: each operand element is multiplied in fp32 by a
power of two s taken from the operand's stated magnitude, and truncated into
three fp16 terms, x s = h + m + l (+ what falls below fp16's smallest
subnormal, 2^-24).  Six products hh + hm + mh + mm + hl + lh of fp16 terms are
exact in fp32; the kernel adds them in fp32 in an order of its own and scales
back by 1 / (s_a s_b).  The model adds them in fp64, so the kernel may differ
from it by its fp32 additions only: per output at most (6 K + 8) 2^-23 S, S =
sum |a| |b| over the reduction of length K (bar()).
"""
import numpy as np

from oracle import tf_ops as R

F16_MAX = 65504.0
OPS = ("fwd", "dgrad", "wgrad")


# ------------------------------------------------------------------ the split
def pow2_scale(m):
    """The operand scale for a stated magnitude m (fp32): the power of two
    whose biased exponent is min(268 - eb, 227), eb = m's biased exponent, so
    that m s lies in [2^14, 2^15) (s clamped at 2^100); m not greater than 0,
    inf or NaN give 1."""
    m = np.float32(m)
    eb = int((m.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF))
    if not (m > 0) or eb == 255:
        return 1.0
    return float(2.0 ** (min(268 - eb, 227) - 127))


def rtz16(v, flush=False):
    """v (fp64 array of fp32 values) rounded toward zero to fp16, subnormals
    included: a multiple of 2^(max(floor(log2 |v|), -14) - 10).  Magnitudes
    past fp16's range (outside the contract) give the largest finite fp16.
    flush: results below 2^-14 become 0 (sensitivity checks only)."""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    _, e = np.frexp(a)                       # a = f 2^e, f in [0.5, 1): floor(log2 a) = e - 1
    ulp = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)
    r = np.minimum(np.floor(a / ulp) * ulp, F16_MAX)
    if flush:
        r = np.where(r < 2.0 ** -14, 0.0, r)
    return np.copysign(r, v)


def split(x, s, flush=False):
    """(xs, h, m, l) as fp64 arrays: xs = f32(x) * f32(s) rounded to fp32, h =
    rtz16(xs), m = rtz16(xs - h), l = rtz16(xs - h - m) (the remainders are
    exact in fp32, and so in fp64)."""
    with np.errstate(over="ignore", under="ignore"):
        xs = (np.asarray(x, np.float32) * np.float32(s)).astype(np.float64)
    h = rtz16(xs, flush)
    m = rtz16(xs - h, flush)
    l = rtz16(xs - h - m, flush)   # noqa: E741
    return xs, h, m, l


def gemm(A, B, sa, sb, flush=False):
    """A [M, K] x B [K, N] as the kernel forms it: hh + hm + mh + mm + hl + lh
    of the split terms (every product exact), summed in fp64, over s_a s_b."""
    _, ah, am, al = split(A, sa, flush)
    _, bh, bm, bl = split(B, sb, flush)
    acc = ah @ (bh + bm + bl) + am @ (bh + bm) + al @ bh     # (the term sums are exact in fp64)
    return acc / sa / sb


def bar(K, S, splits=1):
    """The kernel's allowance against the model, per output element: 6 K
    exact products added in fp32 in any order (one unit of 2^-23, a truncating
    accumulator's, per addition; + 8 for the pieces of a split reduction,
    forced split-K adding its factor), relative to S = sum |a| |b|."""
    return (6.0 * np.asarray(K, np.float64) + 8.0 + (splits if splits > 1 else 0)) * 2.0 ** -23 * S


# ------------------------------------------------------- convs as one GEMM
def _im2col(x, kh, kw, s, pt, pl, ho, wo):
    """[n*ho*wo, kh*kw*c] patches of x padded by (pt, pl) top/left and by
    whatever the windows need at the bottom/right."""
    n, h, w, c = x.shape
    pb = max(0, (ho - 1) * s + kh - h - pt)
    pr = max(0, (wo - 1) * s + kw - w - pl)
    xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    cols = [xp[:, r:r + s * (ho - 1) + 1:s, c0:c0 + s * (wo - 1) + 1:s, :] for r in range(kh) for c0 in range(kw)]
    return np.stack(cols, axis=3).reshape(n * ho * wo, kh * kw * c)


def geometry(case):
    n, h, w, cin, cout, kh, kw, s, pad = case
    ph, pw = ((kh - 1) // 2, (kw - 1) // 2) if pad == "same" else (0, 0)
    return ph, pw, (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1


def operands(op, case, x, w, dy):
    """(A [M, K], B [K, N], Kred, out_shape) of the op's GEMM, fp32 values.
    fwd: A = x by pixel, B = w by c_out.  dgrad: A = dy by input pixel (the
    stride's zeros between its rows and columns), B = w by c_in.  wgrad: A = x
    by (tap, c_in), B = dy by c_out.  Kred is the reduction length the kernel
    walks per output element (dgrad: its stride phase's taps only), an array
    broadcastable to the output."""
    n, h, wd, cin, cout, kh, kw, s, pad = case
    ph, pw, ho, wo = geometry(case)
    if op == "fwd":
        cp = (cin + 3) // 4 * 4           # the kernel walks c_in padded to 4 (zeros)
        return _im2col(x, kh, kw, s, ph, pw, ho, wo), w.reshape(kh * kw * cin, cout), kh * kw * cp, (n, ho, wo, cout)
    if op == "wgrad":
        return _im2col(x, kh, kw, s, ph, pw, ho, wo).T, dy.reshape(n * ho * wo, cout), n * ho * wo, (kh, kw, cin, cout)
    dil = np.zeros((n, (ho - 1) * s + 1, (wo - 1) * s + 1, cout), dy.dtype)
    dil[:, ::s, ::s, :] = dy
    A = _im2col(dil, kh, kw, 1, kh - 1 - ph, kw - 1 - pw, h, wd)
    B = w[::-1, ::-1].transpose(0, 1, 3, 2).reshape(kh * kw * cout, cin)
    taps_r = np.array([len(range((i + ph) % s, kh, s)) for i in range(h)])
    taps_c = np.array([len(range((j + pw) % s, kw, s)) for j in range(wd)])
    K = (taps_r[:, None] * taps_c[None, :] * cout)[None, :, :, None]
    return A, B, K, (n, h, wd, cin)


def conv(op, case, x, w, dy, sa, sb, flush=False):
    """The op through gemm().  Returns (model, exact, S, K): the model's
    output, the exact fp64 result (oracle.tf_ops), S = sum |a| |b| and the
    reduction length, the first three in the output's shape."""
    n, h, wd, cin, cout, kh, kw, s, pad = case
    A, B, K, shape = operands(op, case, x, w, dy)
    model = gemm(A, B, sa, sb, flush).reshape(shape)
    S = (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)).reshape(shape)
    if op == "fwd":
        exact = R.conv2d(x, w, s, pad)
    elif op == "dgrad":
        exact = R.conv2d_bwd_data(dy, w, (n, h, wd, cin), s, pad)
    else:
        exact = R.conv2d_bwd_filter(x, dy, (kh, kw, cin, cout), s, pad)
    return model, exact, S, K


def scales(op, mags):
    """(s_a, s_b) of the op from the stated magnitudes {x, w, dy}."""
    a, b = {"fwd": ("x", "w"), "dgrad": ("dy", "w"), "wgrad": ("x", "dy")}[op]
    return pow2_scale(mags[a]), pow2_scale(mags[b])


# ---------------------------------------------------------------- the cases
# Ladders: 1x1 stride 1, K = 16.  GEMM row r is on rung RUNGS[r % 42], column c
# on rung RUNGS[c % 42]; rung k holds bound * 2^-k * U[0.5, 1), k = -1 .. 40
# (-1: up to twice the bound, what the engine relies on for a power-of-two
# bound; a bound that is no power of two starts at rung 0).
RUNGS = np.arange(-1, 41)
LADDER_GEOM = {"fwd": (1, 6, 14, 16, 48, 1, 1, 1, "same"),       # M 84 pixels, N 48, K c_in 16
               "dgrad": (1, 6, 14, 48, 16, 1, 1, 1, "same"),     # M 84 pixels, N c_in 48, K c_out 16
               "wgrad": (1, 4, 4, 64, 48, 1, 1, 1, "same")}      # M c_in 64, N 48, K 16 pixels
P2 = lambda e: float(np.float32(2.0) ** e)                       # noqa: E731
BELOW = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))   # noqa: E731
# (how A's magnitude is given, its value, how B's is given, its value): words
# with the max in lane 0 / 31 / 63 ("w0" / "w31" / "w63"), a host bound
# ("bnd"), or bound 0 ("zero": scale 1, the ladder then hangs from 2^14).
# Tiny and huge magnitudes are paired so that every output is a normal fp32.
LADDER_MAGS = [
    ("w0", 4096.0, "bnd", 1.0),
    ("w31", 2048.0, "w63", BELOW(0.25)),
    ("w63", BELOW(8.0), "w0", P2(-20)),
    ("bnd", 4096.0, "w31", 0.0625),
    ("bnd", 1.0, "bnd", 2048.0),
    ("zero", 0.0, "zero", 0.0),
    ("bnd", BELOW(4096.0), "zero", 0.0),
    ("w0", P2(-100), "bnd", P2(100)),
    ("bnd", P2(100), "w63", P2(-100)),
    ("bnd", P2(-100), "w31", P2(100)),
]


def _is_pow2(v):
    return float(np.frexp(np.float32(v))[0]) == 0.5


def ladder_mag(kind, v):
    """The magnitude the ladder hangs from: bound 0 stands for 2^14."""
    return P2(14) if kind == "zero" else v


def _ladder(rng, count, K, mag):
    rung = RUNGS[np.arange(count) % len(RUNGS)]
    if not _is_pow2(mag):
        rung = np.maximum(rung, 0)
    u = rng.uniform(0.5, 1.0, (count, K))
    with np.errstate(under="ignore"):
        return (np.float64(mag) * np.ldexp(u, -rung[:, None])).astype(np.float32), rung


def ladder_case(op, mags, seed=0):
    """Tensors of one ladder launch: ((x, w, dy) fp32 with the unused one
    None, row rungs, column rungs).  All operands positive."""
    ka, va, kb, vb = mags
    case = LADDER_GEOM[op]
    n, h, wd, cin, cout = case[:5]
    rng = np.random.default_rng(1000 + seed)
    M, N = (cin, cout) if op == "wgrad" else (n * h * wd, cin if op == "dgrad" else cout)
    A, ra = _ladder(rng, M, 16, ladder_mag(ka, va))       # [M, K]
    B, rb = _ladder(rng, N, 16, ladder_mag(kb, vb))       # [N, K]
    if op == "fwd":
        t = (A.reshape(n, h, wd, cin), B.T.reshape(1, 1, cin, cout).copy(), None)
    elif op == "dgrad":
        t = (None, B.reshape(1, 1, cin, cout).copy(), A.reshape(n, h, wd, cout))
    else:
        t = (A.T.reshape(n, h, wd, cin).copy(), None, B.T.reshape(n, h, wd, cout).copy())
    return t, ra, rb


def ladder_stated(op, mags):
    """{x, w, dy} magnitudes as stated to the kernel (bound 0 stays 0)."""
    a, b = {"fwd": ("x", "w"), "dgrad": ("dy", "w"), "wgrad": ("x", "dy")}[op]
    return {a: mags[1], b: mags[3]}


# Mixed magnitudes inside one dot product: reduction channel c carries
# 2^-(c % 21) in the A operand and the inverse in the filter, so every channel
# contributes equally to S; signs random.  fwd: x's c_in against w's rows;
# dgrad: dy's c_out against w's columns; wgrad (which reduces over pixels)
# reuses fwd's x, whose GEMM rows then sit at 21 magnitudes, against a plain
# dy.  The A operand is stated through a bound of 4096 (x_bound, dy_bound)
# over values below 1, as the engine states activations; B through its max.
MIXED_GEOM = [(1, 9, 9, 32, 32, 3, 3, 1, "same"), (1, 9, 9, 32, 32, 3, 3, 2, "valid")]
MIXED_BOUND = 4096.0


def mixed_case(op, case, seed=0):
    """((x, w, dy) with the unused one None, {x, w, dy} stated magnitudes)."""
    n, h, wd, cin, cout, kh, kw, s, pad = case
    _, _, ho, wo = geometry(case)
    rng = np.random.default_rng(2000 + seed)
    rnd = lambda *shape: rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape)    # noqa: E731
    ec, eo = np.arange(cin) % 21, np.arange(cout) % 21
    x, w, dy = rnd(n, h, wd, cin), rnd(kh, kw, cin, cout), rnd(n, ho, wo, cout)
    if op == "dgrad":
        dy, w, x = dy * np.ldexp(1.0, -eo), w * np.ldexp(1.0, eo), None
        mags = {"dy": MIXED_BOUND, "w": float(np.abs(w).max())}
    else:
        x = x * np.ldexp(1.0, -ec)
        if op == "fwd":
            w, dy = w * np.ldexp(1.0, ec)[:, None], None
            mags = {"x": MIXED_BOUND, "w": float(np.abs(w).max())}
        else:
            w = None
            mags = {"x": MIXED_BOUND, "dy": float(np.abs(dy).max())}
    f32 = lambda a: None if a is None else a.astype(np.float32)    # noqa: E731
    return (f32(x), f32(w), f32(dy)), mags


# The engine's bounds on ordinary data: cases of test_gpu_x6h.py CASES, inputs
# as its _setup makes them; the image case k / 255 under x_bound = 1.
ORDINARY = [((2, 35, 35, 48, 64, 5, 5, 1, "same"), (4096.0, 2048.0)),
            ((2, 17, 17, 128, 192, 1, 7, 1, "same"), (4096.0, 2048.0)),
            ((3, 17, 17, 192, 320, 3, 3, 2, "valid"), (4096.0, 2048.0)),
            ((2, 37, 37, 3, 32, 3, 3, 2, "valid"), (1.0,))]


def ordinary_case(case, seed=0):
    n, h, wd, cin, cout, kh, kw, s, pad = case
    _, _, ho, wo = geometry(case)
    rng = np.random.default_rng(4000 + seed)
    if cin == 3:
        x = rng.integers(0, 256, (n, h, wd, cin)).astype(np.float32) * np.float32(1 / 255)
    else:
        x = np.maximum(rng.standard_normal((n, h, wd, cin)), 0).astype(np.float32)
    w = (rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * cin)).astype(np.float32)
    dy = rng.standard_normal((n, ho, wo, cout)).astype(np.float32)
    return x, w, dy


# Grouped launch: three members, x magnitudes 2^10 apart and w magnitudes 2^-7
# apart, in the order middle, large, small; both through words at + 64 i.
GROUPED_GEOM = (2, 9, 9, 32, 48, 3, 3, 1, "same")
GROUPED_EXP = (0, 1, -1)


def grouped_case(seed=0):
    """[(x, w, {x, w} stated magnitudes)] per member: mixed_case's fwd pair,
    x times 2^(10 e) and w times 2^(-7 e), x stated as 4096 times its max (an
    upper bound, as the engine's), so that a member run under another
    member's words is far outside the bar."""
    out = []
    for i, e in enumerate(GROUPED_EXP):
        (x, w, _), _ = mixed_case("fwd", GROUPED_GEOM, seed=10 + i)
        x = (x * np.float32(2.0 ** (10 * e))).astype(np.float32)
        w = (w * np.float32(2.0 ** (-7 * e))).astype(np.float32)
        out.append((x, w, {"x": MIXED_BOUND * 2.0 ** (10 * e), "w": float(np.abs(w).max())}))
    return out


# ------------------------------------------------- every GPU case, by name
# What a wrong kernel would look like, as variants of the model; a case lists
# the ones it must tell from the model (test_x6h_model.py checks that it
# does): "flush" = fp16 subnormals lost; "a*2" / "a/2" / "b*2" / "b/2" = one
# operand's scale off by a factor of two.
MUTATIONS = ("flush", "a*2", "a/2", "b*2", "b/2")


class Case:
    def __init__(self, id, op, geom, make, mutations):
        self.id, self.op, self.geom, self.make, self.mutations = id, op, geom, make, mutations

    def __repr__(self):
        return self.id


def ladder_cases():
    return [Case(f"ladder-{op}-{i}", op, LADDER_GEOM[op],
                 lambda op=op, m=m, i=i: (ladder_case(op, m, 16 * i + OPS.index(op))[0], ladder_stated(op, m)),
                 MUTATIONS) for op in OPS for i, m in enumerate(LADDER_MAGS)]


def mixed_cases():
    # (a scale off by a factor of two moves these outputs by ~1e-4 of S, half
    # the bar at K = 288: the ladders are what pins the scales)
    return [Case(f"mixed-{op}-{case[7]}{case[8]}", op, case, lambda op=op, case=case: mixed_case(op, case, case[7]),
                 ("flush",)) for case in MIXED_GEOM for op in OPS]


def grouped_cases():
    return [Case(f"grouped-member{i}", "fwd", GROUPED_GEOM,
                 lambda i=i: ((grouped_case()[i][0], grouped_case()[i][1], None), grouped_case()[i][2]),
                 ("flush",)) for i in range(len(GROUPED_EXP))]


def ordinary_cases():
    """fwd and wgrad of ORDINARY under each x_bound, w and dy through their
    max.  No mutation listed: on Gaussian data under the engine's bounds a
    lost subnormal moves an output by ~2^-22 of S, far inside any fp32 bar
    (these cases pin that the engine's scales meet the fp32 bars, the ladders
    and the mixed cases what the scales and the subnormals do)."""
    out = []
    for case, bounds in ORDINARY:
        for b in bounds:
            for op in ("fwd", "wgrad"):
                def make(case=case, b=b):
                    x, w, dy = ordinary_case(case)
                    return (x, w, dy), {"x": b, "w": float(np.abs(w).max()), "dy": float(np.abs(dy).max())}
                out.append(Case(f"ordinary-{op}-{case[1]}x{case[3]}k{case[5]}x{case[6]}-xb{b:g}", op, case, make, ()))
    return out


def mutated(case_op, geom, tensors, stated, mutation):
    """The model's output with one mutation applied."""
    sa, sb = scales(case_op, stated)
    if mutation == "a*2":
        sa *= 2
    elif mutation == "a/2":
        sa /= 2
    elif mutation == "b*2":
        sb *= 2
    elif mutation == "b/2":
        sb /= 2
    x, w, dy = tensors
    return conv(case_op, geom, x, w, dy, sa, sb, flush=mutation == "flush")[0]
