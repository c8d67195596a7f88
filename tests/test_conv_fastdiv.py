"""The conv kernels' division-free decode, checked on the CPU: the planner
(jr_conv_plan: fastdiv_for, conv_divs) gives every runtime divisor d of a GEMM
launch a reciprocal (mul, add, shift) with

    n // d == ((n * mul + add) >> 32 & 0xffffffff) >> shift      0 <= n <= nmax

or mul = 0 where that form is not exact on [0, nmax]: the kernels carry no
division to fall back to, so the launcher refuses a GEMM with such a divisor
(jr_debug_conv_divs then returns 0).  Through two host-only hooks of libjr
(jr_debug_fastdiv, jr_debug_conv_divs; no HIP call) this asserts quotient and
remainder against // and % for

  divisors   every divisor that the Inception-v3 plans at 299^2 B=64 and
             587^2 B=2 produce -- every conv geometry, op and DGRAD stride
             phase, at the planner's config of x6h / x8 / bf16 and at every
             x6h config id alone and with split field 3 -- plus 1, 2, 3, the
             primes up to 151 and 2^k +- 1;
  dividends  every n up to the largest dividend bound of those plans (at
             least M of conv2d_1 at B=64), and the 4,096 values below 2^31,
             where the planner claims the form for every divisor below 2^31;

that the reciprocals conv_divs hands a launch are the ones checked (one triple
per divisor, claimed valid on the launch's own bound), and that the planner
falls back (mul = 0) on divisor / range pairs built to break the form.
"""
import ctypes

import numpy as np
import pytest

WORKLOADS = ((299, 64), (587, 2))
X6H, X8, BF16 = 4, 2, 1
NDIV = 11          # DV_COUNT of jr_conv_plan.h
DV_IPB = 10


@pytest.fixture(scope="module")
def lib():
    from jr import _ffi
    L = ctypes.CDLL(_ffi.LIB_PATH)
    L.jr_debug_fastdiv.restype = ctypes.c_int
    L.jr_debug_fastdiv.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    L.jr_debug_conv_divs.restype = ctypes.c_int
    L.jr_debug_conv_divs.argtypes = [ctypes.POINTER(_ffi.ConvDesc), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                     ctypes.POINTER(ctypes.c_uint32)]
    L.jr_conv2d_num_configs.restype = ctypes.c_int
    L.jr_conv2d_num_configs.argtypes = [ctypes.c_int]
    return L


_MEMO = {}


def fastdiv(L, d, nmax):
    if (d, nmax) not in _MEMO:
        out = (ctypes.c_uint32 * 3)()
        assert L.jr_debug_fastdiv(d, nmax, out) == 0
        _MEMO[(d, nmax)] = tuple(out)
    return _MEMO[(d, nmax)]


def apply(triple, n):
    """The kernels' fdiv_mul on uint64 numpy values n < 2^32 (n * mul + add < 2^64)."""
    mul, add, shift = (np.uint64(v) for v in triple)
    return (((n * mul + add) >> np.uint64(32)) & np.uint64(0xffffffff)) >> shift


@pytest.fixture(scope="module")
def plans(lib):
    """{divisor: set of triples}, {divisor: largest dividend bound} over the plans of the two workloads."""
    from test_conv_plan import _geometries
    triples, bound = {}, {}
    div, nmax, out = (ctypes.c_uint64 * NDIV)(), (ctypes.c_uint64 * NDIV)(), (ctypes.c_uint32 * (3 * NDIV))()
    ids6 = [-1] + [c | (s << 8) for s in (0, 3) for c in range(lib.jr_conv2d_num_configs(X6H))]
    launches = 0
    for res, batch in WORKLOADS:
        for dt, ids in ((X6H, ids6), (X8, [-1]), (BF16, [-1])):
            for key, has_dgrad in _geometries(res, batch, dt):
                from jr import _ffi
                d = _ffi.ConvDesc(*key)
                stride = key[7]
                for op in range(3):
                    for phase in (range(stride * stride) if has_dgrad else ()) if op == 1 else (0,):
                        for cfg in ids:
                            assert lib.jr_debug_conv_divs(ctypes.byref(d), op, dt, phase, cfg, div, nmax, out) == NDIV
                            launches += 1
                            for i in range(NDIV):
                                t = (out[3 * i], out[3 * i + 1], out[3 * i + 2])
                                if div[i] == 0:
                                    assert t[0] == 0          # a divisor this launch never divides by
                                    continue
                                # the planner claims the form on the launch's own bound, with the
                                # reciprocal it gives that divisor on any bound
                                assert t[0] != 0 and t == fastdiv(lib, div[i], nmax[i]), (key, op, phase, cfg, i)
                                triples.setdefault(div[i], set()).add(t)
                                bound[div[i]] = max(bound.get(div[i], 0), nmax[i])
    assert launches > 10000
    return triples, bound


def _extra_divisors():
    primes = [p for p in range(2, 152) if all(p % q for q in range(2, int(p ** 0.5) + 1))]
    pow2 = [2 ** k + s for k in range(1, 31) for s in (-1, 1)]
    return sorted(set([1, 2, 3] + primes + [v for v in pow2 if 1 <= v < 2 ** 31]))


def test_quotient_and_remainder_exact(lib, plans):
    triples, bound = plans
    top = max(bound.values())
    assert top >= 64 * 149 * 149 - 1                      # M of conv2d_1 at B = 64
    assert all(len(t) == 1 for t in triples.values())     # one reciprocal per divisor
    divisors = sorted(set(triples) | set(_extra_divisors()))
    assert 1 in triples and len(triples) > 60
    low = np.arange(0, top + 1, dtype=np.uint64)
    high = np.arange(2 ** 31 - 4096, 2 ** 31, dtype=np.uint64)
    for d in divisors:
        t = fastdiv(lib, d, 2 ** 31 - 1)
        assert t[0] != 0, d                               # every n < 2^31 is claimed for every d < 2^31
        assert fastdiv(lib, d, top) == t
        if d in triples:
            assert triples[d] == {t}
        for n in (low, high):
            q = apply(t, n)
            assert np.array_equal(q, n // np.uint64(d)), d
            assert np.array_equal(n - q * np.uint64(d), n % np.uint64(d)), d


def test_planner_falls_back_where_the_form_breaks(lib):
    assert fastdiv(lib, 0, 100)[0] == 0                   # no divisor
    assert fastdiv(lib, 7, 2 ** 32)[0] == 0               # a dividend past 32 bits
    assert fastdiv(lib, 2 ** 31, 100)[0] == 0             # a divisor past 31 bits
    assert fastdiv(lib, 1, 2 ** 32 - 1)[0] == 0           # d = 1: (n + 1) wraps at n = 2^32 - 1 ...
    assert fastdiv(lib, 1, 2 ** 32 - 2)[0] != 0           # ... and only there
    # the round-up form of d is exact while n e < 2^(32 + s), e = mul d - 2^(32 + s): for every
    # odd d below build the first n it gets wrong, and ask for the range just short of / reaching it
    broke = 0
    for d in (7, 11, 13, 19, 77, 125, 641, 1000003):
        mul, add, shift = fastdiv(lib, d, 2 ** 31 - 1)
        e = mul * d - 2 ** (32 + shift)
        assert add == 0 and 0 < e < d
        # n mul / 2^(32+s) = q + (r + n e / 2^(32+s)) / d for n = q d + r: the first wrong quotient is at the
        # first n = q d + (d - 1) with n e >= 2^(32+s)
        n_min = -(-2 ** (32 + shift) // e)
        n0 = n_min + (d - 1 - n_min) % d
        assert ((n0 * mul) >> 32) >> shift == n0 // d + 1
        if n0 >= 2 ** 32:
            assert fastdiv(lib, d, 2 ** 32 - 1) == (mul, add, shift)      # exact on all 32 bits
            continue
        broke += 1
        assert all(((n * mul) >> 32) >> shift == n // d for n in range(n0 - 3 * d, n0))
        assert fastdiv(lib, d, n0)[0] == 0, d                              # the breaking range: divide
        assert fastdiv(lib, d, 2 ** 32 - 1)[0] == 0, d
        # (the planner's bound is the sufficient n e < 2^(32+s): it may give up a little early, never late)
        last_claimed = (2 ** (32 + shift) - 1) // e
        assert last_claimed < n0 and fastdiv(lib, d, last_claimed) == (mul, add, shift)
        assert fastdiv(lib, d, last_claimed + 1)[0] == 0
    assert broke >= 3


def test_launcher_refuses_a_walk_past_31_bits(lib):
    """A valid descriptor whose stream-K walk has 2^31 iterations and more (1.07 M tiles of 64 x 64 times
    2,017 K-tiles): the walk's reciprocals are not claimed, so that config is refused; the tile's plain grid is not."""
    from jr import _ffi
    d = _ffi.ConvDesc(1, 8400, 8400, 4, 16, 127, 127, 1, 1, 0, 0, 8274, 8274, 0, 4, 0, 16)
    div, nmax, out = (ctypes.c_uint64 * NDIV)(), (ctypes.c_uint64 * NDIV)(), (ctypes.c_uint32 * (3 * NDIV))()
    assert lib.jr_debug_conv_divs(ctypes.byref(d), 0, X6H, 0, 7, div, nmax, out) == NDIV
    tiles, ktiles = -(-8274 * 8274 // 64), 127 * 127 * 4 // 32 + 1
    assert tiles * ktiles >= 2 ** 31
    assert lib.jr_debug_conv_divs(ctypes.byref(d), 0, X6H, 0, 35, div, nmax, out) == 0       # tile 7's stream-K grid
    assert out[3 * DV_IPB] == 0 and out[3 * (DV_IPB - 1)] == 0


def test_launch_without_stream_k_keeps_no_walk_reciprocal(lib):
    """A split-K / plain grid never walks stream-K iterations: its sk_ipb entry is unused (divisor 0)."""
    from jr import _ffi
    d = _ffi.ConvDesc(64, 17, 17, 192, 192, 1, 7, 1, 1, 0, 3, 17, 17, 0, 192, 0, 192)
    div, nmax, out = (ctypes.c_uint64 * NDIV)(), (ctypes.c_uint64 * NDIV)(), (ctypes.c_uint32 * (3 * NDIV))()
    assert lib.jr_debug_conv_divs(ctypes.byref(d), 0, X6H, 0, 2, div, nmax, out) == NDIV      # tile 2, plain grid
    assert div[DV_IPB] == 0 and out[3 * DV_IPB] == 0
    assert lib.jr_debug_conv_divs(ctypes.byref(d), 0, X6H, 0, 30, div, nmax, out) == NDIV     # its stream-K grid
    assert div[DV_IPB] > 0 and out[3 * DV_IPB] != 0
