"""h2_rowmax and h2_scale (csrc/split_common.hpp) on their own, through mgn_debug_rowmax: one wave takes 32 rows of 128 floats in the
kernels' fragment layout and answers, per row, the maximum the two-piece split scales the row by and the pair of powers of two made from it.

Maxima are exact, so the device must EQUAL numpy: max |x| (abs = 1) and max(x, 0) (abs = 0: what survives the ReLU that follows).  Lane
(c, h) of the wave holds the four-float pieces 2 m + h of row c, i.e. the columns with (column // 4) % 2 == h: a row's two halves are
interleaved, and the half exchange (v_permlane32_swap_b32) brings them together.  The debug kernel writes the maximum from the LOWER half
and the scale pair from the UPPER half's own maximum, so an exchange that serves only one direction fails on one of the two.
No NaN inputs: what a NaN row gives is stated next to h2_rowmax, not promised here."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the library's first HIP call)

import mgn_amd

pytestmark = pytest.mark.gpu

L = 128
H2_EXP_MIN = 87 << 23          # split_common.hpp: rows below 2^-40 are scaled as if their maximum were 2^-40


def upper_half(col):
    return (col // 4) % 2 == 1


def rows():
    rng = np.random.default_rng(20)
    x = np.zeros((32, L), np.float32)
    names = {}
    names[0] = "all zeros"
    x[1] = -0.0
    names[1] = "all -0.0"
    x[2, 5] = np.float32(1e-42)
    names[2] = "one subnormal, lower half"
    x[3, 100] = np.float32(-3e-41)
    assert upper_half(100)
    names[3] = "one negative subnormal, upper half"
    x[4] = -np.abs(rng.standard_normal(L)).astype(np.float32) - np.float32(0.5)
    names[4] = "all negative"
    x[5] = rng.standard_normal(L)
    x[5, 77] = np.inf
    assert upper_half(77)
    names[5] = "a single +inf, upper half"
    x[6] = rng.standard_normal(L)
    x[6, 3] = np.inf
    names[6] = "a single +inf, lower half"
    x[7] = rng.uniform(-1, 1, L)
    x[7, 68] = -7.5                                               # column >= 64 AND in the upper lane half
    assert upper_half(68)
    names[7] = "largest magnitude negative, upper half"
    x[8] = rng.uniform(-1, 1, L)
    x[8, 3] = 9.25
    assert not upper_half(3)
    names[8] = "maximum in the lower half only"
    x[9] = rng.uniform(-1, 1, L)
    x[9, 127] = 11.0
    assert upper_half(127)
    names[9] = "maximum in the upper half only (last column)"
    x[10] = rng.uniform(-1, 1, L)
    x[10, 0] = -13.0
    names[10] = "largest magnitude negative, lower half (first column)"
    scale = 10.0 ** rng.uniform(-6, 6, (21, 1))
    x[11:] = (rng.standard_normal((21, L)) * scale).astype(np.float32)
    for k in range(11, 32):
        names[k] = "random, scale %.1e" % scale[k - 11, 0]
    assert not np.isnan(x).any()
    return x, names


def h2_scale(amax):
    """split_common.hpp, h2_scale, on the bits"""
    eb = amax.astype(np.float32).view(np.uint32) & np.uint32(0x7F800000)
    eb = np.maximum(eb, np.uint32(H2_EXP_MIN)).astype(np.int64)
    s = ((268 << 23) - eb).astype(np.uint32)
    rs = (eb - (14 << 23)).astype(np.uint32)
    return s, rs


@pytest.mark.parametrize("absolute", [1, 0], ids=["abs", "relu"])
def test_row_maxima_and_scales_equal_numpy(absolute):
    lib = mgn_amd.load()
    f = lib.mgn_debug_rowmax
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    x, names = rows()
    amax, s, rs = (np.full(32, np.nan, np.float32) for _ in range(3))
    assert f(x.ctypes.data, 32, absolute, amax.ctypes.data, s.ctypes.data, rs.ctypes.data) == 0
    want = np.abs(x).max(1) if absolute else np.maximum(x.max(1), np.float32(0))
    for k in range(32):
        print(f"row {k:2d} ({names[k]}): device {amax[k]!r}, numpy {want[k]!r}, s {s[k]!r}, rs {rs[k]!r}")
    bad = [k for k in range(32) if not amax[k] == want[k]]
    assert not bad, [(k, names[k], amax[k], want[k]) for k in bad]
    if not absolute:
        assert amax[4] == 0 and amax[1] == 0 and amax[7] < 1 and amax[10] < 1      # negative values never win
    ws, wrs = h2_scale(want)
    bad = [k for k in range(32) if s[k].view(np.uint32) != ws[k] or rs[k].view(np.uint32) != wrs[k]]
    assert not bad, [(k, names[k], s[k], ws[k].view(np.float32), rs[k], wrs[k].view(np.float32)) for k in bad]
    finite = np.isfinite(want)
    assert (s[finite].astype(np.float64) * rs[finite] == 1.0).all()                  # powers of two, exact inverses
    big = finite & (want >= 2.0 ** -40)
    scaled = want[big].astype(np.float64) * s[big]
    assert ((scaled >= 2.0 ** 14) & (scaled < 2.0 ** 15)).all()                      # the row's largest entry lands in [2^14, 2^15)


def test_bad_arguments_are_refused():
    lib = mgn_amd.load()
    f = lib.mgn_debug_rowmax
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    x = np.zeros((32, L), np.float32)
    o = np.zeros(32, np.float32)
    assert f(None, 32, 1, o.ctypes.data, o.ctypes.data, o.ctypes.data) == -1
    assert f(x.ctypes.data, 0, 1, o.ctypes.data, o.ctypes.data, o.ctypes.data) == -1
