"""TESTS ONLY: operand sets, references and checks for the known-answer kernels of freesasa_amd/csrc/kat_kernels.h - the
arithmetic and the lane primitives that are defined one way for the device and another for the CPU emulation, and what is
built on the hardware seeds.  tests/test_device_arith.py runs every case through the emulation, tests/test_device_arith_gpu.py
through the device hooks; both hand a Backend to the functions here.

Exact pieces are computed with integers and fractions; real-valued references in numpy.longdouble (64-bit mantissa: its own
error, 2^-64 relative, is a thousandth of the smallest bound below).  Every bound is derived where it is used or is a figure
the kernels' comments state; none is read off the code under test."""
import functools
import os
import re
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended-precision long double"

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "freesasa_amd", "csrc", "kat_kernels.h")


def _enums():
    """The two op enumerations of kat_kernels.h, read from the header: name without KAT_ -> number."""
    blocks = re.findall(r"enum\s*\{(.*?)\};", open(_HDR).read(), flags=re.S)
    out = []
    for blk in blocks[:2]:
        names = re.findall(r"\bKAT_\w+", re.sub(r"/\*.*?\*/", "", blk, flags=re.S))
        out.append({n[4:]: i for i, n in enumerate(names)})
    return out


EW, WAVE = _enums()
assert EW["RSQ"] == 0 and "EW_OPS" in EW and WAVE["SCAN_ADD"] == 0 and "WAVE_OPS" in WAVE


class Backend:
    """ew(op name, a, b, c, k) -> (out0, out1); wave(op name, uint64 [rows, 64]) -> uint64 [rows, 64]."""

    def __init__(self, ew_fn, wave_fn):
        self._ew, self._wave = ew_fn, wave_fn

    def ew(self, op, a=None, b=None, c=None, k=0.0):
        return self._ew(EW[op], a, b, c, k)

    def wave(self, op, words):
        return self._wave(WAVE[op], words)


def _frozen(a):
    a.setflags(write=False)
    return a


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


# ------------------------------------------------------------------------------------------------ operand sets

@functools.lru_cache(None)
def sqrt_operands():
    """What D = xd^2 + yd^2 and Ri'^2 are: 2^17 uniform values of [1e-12, 1e4], and 1000 log-spaced over 1e-30 .. 1e30."""
    rng = np.random.default_rng(11)
    return _frozen(np.concatenate([rng.uniform(1e-12, 1e4, 1 << 17), np.logspace(-30, 30, 1000)]))


@functools.lru_cache(None)
def acos_operands():
    """test_emulation.py::test_device_math_helpers_accuracy's set: 2e5 uniform values and the edges at +-1, +-0.5 and 0."""
    rng = np.random.default_rng(3)
    edge = np.concatenate([1 - np.logspace(-16, -1, 400), -(1 - np.logspace(-16, -1, 400)),
                           0.5 + np.linspace(-1e-9, 1e-9, 101), -0.5 + np.linspace(-1e-9, 1e-9, 101),
                           np.linspace(-1e-9, 1e-9, 101)])
    x = np.concatenate([rng.uniform(-1, 1, 200_000), edge])
    return _frozen(x[(x > -1) & (x < 1)])


@functools.lru_cache(None)
def acos_lower_operands():
    rng = np.random.default_rng(5)
    return _frozen(np.concatenate([[-1.0, 0.9], rng.uniform(-1.0, 0.9, 200_000 - 2)]))


@functools.lru_cache(None)
def atan2_operands():
    """That test's set too: (y, x, 1/sqrt(x^2 + y^2) from long double, rounded once)."""
    rng = np.random.default_rng(3)
    rng.uniform(-1, 1, 200_000)
    ang = np.concatenate([rng.uniform(-np.pi, np.pi, 200_000), np.pi / 8 * np.arange(-8, 9) + 1e-12,
                          np.pi / 8 * np.arange(-8, 9) - 1e-12, np.array([0.0, 1e-300, -1e-300])])
    rad = rng.uniform(1e-3, 30.0, ang.size)
    y, x = rad * np.sin(ang), rad * np.cos(ang)
    inv = (1 / np.sqrt(_ld(x) * _ld(x) + _ld(y) * _ld(y))).astype(np.float64)
    return _frozen(y), _frozen(x), _frozen(inv)


@functools.lru_cache(None)
def f32_operands():
    rng = np.random.default_rng(13)
    x = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 1 << 16)).astype(np.float32)
    return _frozen(x.astype(np.float64))


@functools.lru_cache(None)
def div_ns_operands():
    """(x, ns, RN(1 / ns)): every slice count 1 .. 1024 under eight heights each, zero among them."""
    rng = np.random.default_rng(17)
    ns = np.tile(np.arange(1, 1025, dtype=np.float64), 8)
    x = rng.uniform(0, 50, ns.size) * rng.choice([1.0, -1.0, 1e-8, 1e6], ns.size)
    x[:1024:97] = 0.0
    return _frozen(x), _frozen(ns), _frozen(1.0 / ns)


FMA_K = (0.5, -float.fromhex("0x1.921fb54442d18p-1"), float.fromhex("0x1.5555555554f05p-3"), 0.0, -1.0)   # (-pi/4 and a coefficient, as the polynomials')


@functools.lru_cache(None)
def fma_operands(k):
    """p, z with p z + k at every distance from cancellation: where a product rounded on its own gives another result."""
    rng = np.random.default_rng(19)
    n = 2048
    p = rng.uniform(-2, 2, n)
    z = rng.uniform(0, 0.5, n)
    near = np.arange(n) % 2 == 0
    with np.errstate(all="ignore"):
        zc = np.where(p != 0, -k / p, 0.0) * (1 + rng.choice([0.0, 1e-16, -1e-16, 1e-12, 1e-8, -1e-4], n))
    z = np.where(near & np.isfinite(zc) & (k != 0), zc, z)
    return _frozen(p), _frozen(z)


def ref_fma(p, z, k):
    return np.array([float(Fraction(a) * Fraction(b) + Fraction(k)) for a, b in zip(p.tolist(), z.tolist())])


def ref_div_ns(x, ns):
    return np.array([float(Fraction(a) / Fraction(b)) for a, b in zip(x.tolist(), ns.tolist())])


@functools.lru_cache(None)
def minmax_operands():
    """Random pairs, equal pairs, +-inf, +-0; no NaN: the macros promise none."""
    rng = np.random.default_rng(23)
    a, b = rng.normal(0, 10, 1000), rng.normal(0, 10, 1000)
    b[:100] = a[:100]
    sp = np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1.7976931348623157e308])
    return _frozen(np.concatenate([a, np.repeat(sp, sp.size)])), _frozen(np.concatenate([b, np.tile(sp, sp.size)]))


SHIFT_LIMS = (1.0, 0.3, 1234.5678, 3.9999999999999929)


@functools.lru_cache(None)
def shift_operands():
    """(w as uint32, v, lim): every word under every comparand at every limit."""
    rng = np.random.default_rng(29)
    ws = np.concatenate([np.array([0, 1, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint64), rng.integers(0, 1 << 32, 11, dtype=np.uint64)])
    W, V, L = [], [], []
    for lim in SHIFT_LIMS:
        vs = [lim, np.nextafter(lim, np.inf), np.nextafter(lim, -np.inf), -lim, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0,
              np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)]
        for w in ws:
            for v in vs:
                W.append(w); V.append(v); L.append(lim)
    return _frozen(np.array(W, dtype=np.uint64)), _frozen(np.array(V)), _frozen(np.array(L))


def words_as_doubles(w):
    """32-bit words in the low half of doubles' bit patterns, as the shift-in op takes and gives them."""
    return np.ascontiguousarray(w, dtype=np.uint64).view(np.float64)


def doubles_as_words(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def ref_shift_in(w, v, lim):
    with np.errstate(invalid="ignore"):
        return ((w << np.uint64(1)) & np.uint64(0xffffffff)) | (v < lim).astype(np.uint64)


# ------------------------------------------------------------------------------------------------ real-valued checks

def within(got, want, tol, what):
    """|got - want| <= tol everywhere (a NaN fails); returns the errors."""
    err = np.abs(_ld(got) - want)
    bad = ~(err <= tol)
    if bad.any():
        i = int(np.argmax(np.where(bad, np.where(np.isnan(err), np.inf, err / np.maximum(tol, LD(5e-324))), 0)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} beyond the bound; operand {i}: got {float(np.asarray(got)[i])!r}, "
                             f"want {float(want[i])!r}, error {float(err[i]):.3e}, bound {float(np.broadcast_to(tol, err.shape)[i]):.3e}")
    return err


E_RSQ_MAX = 2.0 ** -24   # the project's one-off measurement gave 2^-24.2 as a maximum over 4e6 other operands: 15 % for another sample
E_RCP_MAX = 2.0 ** -14   # atan2_fast's two Newton steps take the seed's error e to e^4: below 2^-56 from 2^-14


def seed_errors(x, rsq, rcp):
    """Largest relative errors of the two fp64 seeds; e_rsq <= 2^-24 (the bounds of what is built on the seed use the
    MEASURED figure, so they do not depend on this one)."""
    xl = _ld(x)
    e_rsq = float(np.max(np.abs(_ld(rsq) * np.sqrt(xl) - 1)))
    e_rcp = float(np.max(np.abs(_ld(rcp) * xl - 1)))
    assert e_rsq <= E_RSQ_MAX, f"rsq seed: relative error {e_rsq:.3e} = 2^{np.log2(e_rsq):.2f}"
    assert e_rcp <= E_RCP_MAX, f"rcp seed: relative error {e_rcp:.3e} = 2^{np.log2(e_rcp):.2f}"
    return {"e_rsq": e_rsq, "e_rcp": e_rcp}


def sqrt_g_want_tol(x, e_rsq):
    """One coupled Goldschmidt step on a seed y = (1 + e) / sqrt x: g = RN(x y) = sqrt x (1 + e)(1 + d1), r = 1/2 - h g =
    -(e + d1 / 2) - e^2 / 2 ..., result = g (1 + r)(1 + d3) = sqrt x (1 - 1.5 e^2 + O(d)): relative 1.5 e^2 + 2^-51."""
    want = np.sqrt(_ld(x))
    return want, (LD(1.5) * LD(e_rsq) ** 2 + LD(2.0) ** -51) * want


def h2_want_tol(x, e_rsq):
    """LR2_H2: the same step for h = 1 / (2 sqrt x)."""
    want = LD(0.5) / np.sqrt(_ld(x))
    return want, (LD(1.5) * LD(e_rsq) ** 2 + LD(2.0) ** -51) * want


def sqrt_rh_want_tol(x):
    """g within 1 ulp, h within 2 ulp, as test_device_math_helpers_accuracy asserts with the exact seed."""
    g, h = np.sqrt(_ld(x)), LD(0.5) / np.sqrt(_ld(x))
    return (g, _ld(np.spacing(g.astype(np.float64)))), (h, 2 * _ld(np.spacing(h.astype(np.float64))))


def acos2_want_tol(x, e_rsq):
    """acos_fast2: (6.3e-13 + 1.5 e_rsq^2) 2 asin u + 1e-15, 2 asin u = acos x for x >= 0 and pi - acos x below.  6.3e-13 is
    the header's figure for degree 12; the absolute term: the rounding of t near -pi/4, doubled (1.1e-16), the errors of the
    pi/4 constant, doubled, and of pi/2 (6e-17 each), the rounding of fma(e, q, q) (1.7e-16) and the final rounding: ~6e-16."""
    want = np.arccos(_ld(x))
    two_asin = np.where(np.asarray(x) >= 0, want, LD(np.pi) - want)
    return want, (LD(6.3e-13) + LD(1.5) * LD(e_rsq) ** 2) * np.abs(two_asin) + LD(1e-15)


def acos_want_tol(x, e_rsq):
    """acos_fast: test_device_math_helpers_accuracy's bound with the seed's share added to the relative part."""
    want = np.arccos(_ld(x))
    return want, (LD(2.5e-14) + LD(1.5) * LD(e_rsq) ** 2) * want + LD(4e-16)


ACOS_LOWER_MARGIN = 5e-10   # half the 1e-9 the bound keeps (restated in numpy on 2e6 points: 1.0e-9 at c -> 0)


def check_acos_lower(c, got):
    """A lower bound of acos on [-1, 0.9] that keeps half its margin: the cover filter's soundness rests on it."""
    room = np.arccos(_ld(c)) - _ld(got)
    assert not np.isnan(room).any() and np.all(room >= 0), f"lr2_acos_lower exceeds acos by {float(-room.min()):.3e}"
    assert np.all(room >= ACOS_LOWER_MARGIN), f"lr2_acos_lower keeps only {float(room.min()):.3e} of its margin"
    return {"acos_lower_room": float(room.min())}


def atan2_want_tol(y, x):
    """test_device_math_helpers_accuracy's bounds: 3 ulp of pi absolute, 4 ulp of the result below 1e-3."""
    want = np.arctan2(_ld(y), _ld(x))
    w64 = np.abs(want.astype(np.float64))
    tol = np.where(w64 < 1e-3, 4 * np.spacing(w64 + 1e-300), 3 * np.spacing(np.pi))
    return want, _ld(tol)


F32_TOL = 2.0 ** -23   # "1 ulp": what the margins of sr_caps.h and of the contained-caps test are computed with


def f32_errors(x, rcp, rsq, sqrt):
    xl = _ld(x)
    fig = {"e_rcpf": float(np.max(np.abs(_ld(rcp) * xl - 1))), "e_rsqf": float(np.max(np.abs(_ld(rsq) * np.sqrt(xl) - 1))),
           "e_sqrtf": float(np.max(np.abs(_ld(sqrt) / np.sqrt(xl) - 1)))}
    for name, e in fig.items():
        assert e <= F32_TOL, f"{name} = {e:.3e} = 2^{np.log2(e):.2f}"
    for v in (rcp, rsq, sqrt):
        assert np.array_equal(np.asarray(v, dtype=np.float32).astype(np.float64), v), "not a float"
    return fig


# ------------------------------------------------------------------------------------------------ lr2_arc_limit

def _mant_exp(v):
    """Positive finite doubles as M 2^e, M and e Python integers."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    return (m * 2.0 ** 53).astype(np.int64).tolist(), (e - 53).tolist()


def _product_below(v, h, num, shift):
    """v h < num / 2^shift for every pair, exactly: the comparison of the rationals Fraction(v) * Fraction(h) and num / 2^shift,
    in integers."""
    Mv, ev = _mant_exp(v)
    Mh, eh = _mant_exp(h)
    ok = np.empty(len(Mv), dtype=bool)
    for i in range(len(Mv)):
        s = ev[i] + eh[i] + shift
        p = Mv[i] * Mh[i]
        ok[i] = (p << s) < num if s >= 0 else p < (num << -s)
    return ok


def check_arc_limit(A, h, T):
    """What the screening's limit T = lr2_arc_limit(A, h) guarantees, with no tolerance.  For v the largest double below T:
    v h < 1 - 2^-50 as rationals; the z = RN(1/2 - v hh) that lr2_arc_alpha forms with the hh = h / 2 the screening leaves in
    it_tc (an exact halving) is > 0 - RN of a positive number is positive, so that is v hh < 1/2 as rationals -; and RN(T h)
    lies below 1 (how far: check_arc_limit_reach).  Returns the least room under the first."""
    h, T = np.asarray(h, dtype=np.float64), np.asarray(T, dtype=np.float64)
    assert np.all(np.isfinite(h) & np.isfinite(T) & (h > 0) & (T > 0)), "h or T not a positive number"
    v = np.nextafter(T, -np.inf)
    ok = _product_below(v, h, (1 << 50) - 1, 50)
    assert ok.all(), f"v h >= 1 - 2^-50 for {int((~ok).sum())} operands, the first A = {float(np.asarray(A)[~ok][0])!r}"
    hh = 0.5 * h
    assert np.array_equal(hh * 2.0, h)
    okz = _product_below(v, hh, 1, 1)
    assert okz.all(), f"z <= 0 for {int((~okz).sum())} operands"
    assert np.all(T * h < 1.0), "RN(T h) reaches 1"
    room = (LD(1) - LD(2.0) ** -50) - _ld(v) * _ld(h)
    i = int(np.argmin(room))
    return {"arc_limit_room": float(1 - Fraction(1, 1 << 50) - Fraction(float(v[i])) * Fraction(float(h[i]))), "arc_limit_at": i}


def check_arc_limit_reach(h, T):
    """T is not smaller than it need be: RN(T h) within 2^-49 of 1, from below."""
    p = np.asarray(T, dtype=np.float64) * np.asarray(h, dtype=np.float64)
    far = 1.0 - p
    assert np.all(p < 1.0) and np.all(far <= 2.0 ** -49), \
        (f"1 - RN(T h) spans {float(far.min()) * 2.0 ** 53:.0f} .. {float(far.max()) * 2.0 ** 53:.0f} x 2^-53 (2^-49 is 16); "
         f"{int((far > 2.0 ** -49).sum())} of {far.size} operands beyond 2^-49")
    return {"arc_limit_reach": float(far.max())}


# ------------------------------------------------------------------------------------------------ lanes

def _rows(vals):
    """A flat list of words padded with zeros to whole rows of 64."""
    v = np.asarray(vals, dtype=np.uint64)
    out = np.zeros(((v.size + 63) // 64) * 64, dtype=np.uint64)
    out[:v.size] = v
    return out.reshape(-1, 64)


def pack(lo, hi):
    return (np.asarray(lo).astype(np.int64).astype(np.uint64) & np.uint64(0xffffffff)) | (np.asarray(hi).astype(np.int64).astype(np.uint64) << np.uint64(32))


@functools.lru_cache(None)
def scan_rows():
    """All zeros, all ones, the lane index, the 64 one-hot rows, the 64 rows "1 from lane k on", rows nonzero only at the
    lanes on either side of a row-of-16 boundary, 64 random rows below 2^20: values >= 0, sums < 2^31."""
    rng = np.random.default_rng(31)
    lane = np.arange(64)
    rows = [np.zeros(64), np.ones(64), lane]
    rows += [(lane == k) * 1 for k in range(64)]
    rows += [(lane >= k) * 1 for k in range(64)]
    for a in (15, 31, 47):
        rows += [(lane == a) * 7, (lane == a + 1) * 5, ((lane == a) | (lane == a + 1)) * 3]
    rows += [rng.integers(0, 1 << 20, 64) for _ in range(64)]
    return _frozen(np.array(rows, dtype=np.uint64))


def ref_scan_add(rows):
    return np.cumsum(rows.astype(np.int64), axis=1).astype(np.uint64)


def ref_scan_add16(rows):
    return np.cumsum(rows.astype(np.int64).reshape(-1, 4, 16), axis=2).reshape(-1, 64).astype(np.uint64)


def ref_scan_max16(rows):
    return np.maximum.accumulate(rows.astype(np.int64).reshape(-1, 4, 16), axis=2).reshape(-1, 64).astype(np.uint64)


@functools.lru_cache(None)
def mask_set():
    """0, ~0, the 64 single bits and their complements, 64 random masks."""
    rng = np.random.default_rng(37)
    full = (1 << 64) - 1
    m = [0, full] + [1 << k for k in range(64)] + [full ^ (1 << k) for k in range(64)]
    m += [int(v) for v in rng.integers(0, 1 << 64, 64, dtype=np.uint64)]
    return tuple(m)


def mask_rows():
    """Every lane of a row holds the row's mask."""
    return np.repeat(np.array(mask_set(), dtype=np.uint64)[:, None], 64, axis=1)


def ref_rank(masks):
    """LR2_RANK of the mask itself and of the ballot that reproduces it: bits below the lane, in both halves of the word."""
    out = np.zeros((len(masks), 64), dtype=np.uint64)
    for r, m in enumerate(masks):
        for l in range(64):
            c = bin(m & ((1 << l) - 1)).count("1")
            out[r, l] = c | (c << 32)
    return out


def ref_popc(words):
    return np.array([bin(w).count("1") | (bin(w & 0xffffffff).count("1") << 32) for w in words], dtype=np.uint64)


@functools.lru_cache(None)
def cell_rank_rows():
    """A table word per row (which of 32 cells hold atoms | occupied cells before them << 32), asked at x = lane."""
    rng = np.random.default_rng(41)
    w = [(m & 0xffffffff) | (int(b) << 32) for m, b in zip(mask_set(), rng.integers(0, 1 << 20, len(mask_set())))]
    return _frozen(np.repeat(np.array(w, dtype=np.uint64)[:, None], 64, axis=1))


def ref_cell_rank(rows):
    out = np.zeros(rows.shape, dtype=np.uint64)
    for r in range(rows.shape[0]):
        w = int(rows[r, 0])
        for x in range(64):
            out[r, x] = (w >> 32) + bin(w & 0xffffffff & ((1 << (x & 31)) - 1)).count("1")
    return out


@functools.lru_cache(None)
def lane_rows():
    """128 rows of random 32-bit words (negative ones among them as ints): every source lane of LR2_READLANE twice."""
    rng = np.random.default_rng(43)
    return _frozen(rng.integers(0, 1 << 32, (128, 64), dtype=np.uint64))


def ref_readlane(rows):
    return np.repeat(rows[np.arange(rows.shape[0]), np.arange(rows.shape[0]) % 64][:, None], 64, axis=1)


@functools.lru_cache(None)
def shuffle_sources():
    """Identity, reversal, every lane as the only source, 16 random permutations."""
    rng = np.random.default_rng(47)
    src = [np.arange(64), np.arange(64)[::-1]] + [np.full(64, k) for k in range(64)] + [rng.permutation(64) for _ in range(16)]
    return _frozen(np.array(src, dtype=np.int64))


@functools.lru_cache(None)
def shuffle_payload32():
    rng = np.random.default_rng(53)
    return _frozen(rng.integers(0, 1 << 32, shuffle_sources().shape, dtype=np.uint64))


@functools.lru_cache(None)
def shuffle_payload64():
    """Doubles whose halves differ: -0.0, a NaN with a payload, denormals, among random bit patterns."""
    rng = np.random.default_rng(59)
    p = rng.integers(0, 1 << 64, shuffle_sources().shape, dtype=np.uint64)
    special = np.array([0x8000000000000000, 0x7ff800000badf00d, 0xfff0000000000001, 0x0000000000000001, 0x000fffffffffffff,
                        0x800000007fffffff, 0x3ff0000000000000, 0x00000000ffffffff], dtype=np.uint64)
    p[:, ::8] = special[np.arange(p.shape[0]) % 8][:, None]
    p[0, :8] = special
    return _frozen(p)


def shfl64_rows():
    """Rows in pairs: payloads, then the source lanes."""
    src, p = shuffle_sources(), shuffle_payload64()
    rows = np.empty((2 * src.shape[0], 64), dtype=np.uint64)
    rows[0::2], rows[1::2] = p, src.astype(np.uint64)
    return rows


def ref_shfl64(rows):
    out = np.zeros_like(rows)
    out[0::2] = np.take_along_axis(rows[0::2], rows[1::2].astype(np.int64), axis=1)
    return out


@functools.lru_cache(None)
def mul24_pairs():
    """All pairs of the edge values, the shape of round 5's bug (i 2^17 from 2^31 on), 4096 random pairs below 2^24."""
    rng = np.random.default_rng(61)
    edge = [0, 1, 1 << 12, (1 << 16) - 1, 1 << 16, 1 << 17, 1 << 23, (1 << 24) - 1]
    a = [x for x in edge for _ in edge] + [16383, 16384, 32767]
    b = [y for _ in edge for y in edge] + [1 << 17] * 3
    a = np.concatenate([a, rng.integers(0, 1 << 24, 4096)])
    b = np.concatenate([b, rng.integers(0, 1 << 24, 4096)])
    return _frozen(a.astype(np.int64)), _frozen(b.astype(np.int64))


def ref_mul24(a, b, signed):
    """The product's low 32 bits as an int (sign-extended to the 64-bit word) or as an unsigned number (zero-extended)."""
    out = []
    for x, y in zip(a.tolist(), b.tolist()):
        p = (x * y) & 0xffffffff
        out.append((p - (1 << 32)) & ((1 << 64) - 1) if signed and p >> 31 else p)
    return np.array(out, dtype=np.uint64)


def div_rows():
    """0 .. 68 under lr2_div9 and 0 .. 43 under lr2_div3, exhaustive."""
    i = np.arange(128)
    return pack(i % 69, i % 44).reshape(2, 64)


def ref_div(rows):
    lo, hi = rows & np.uint64(0xffffffff), rows >> np.uint64(32)
    return (lo // np.uint64(9)) | ((hi // np.uint64(3)) << np.uint64(32))


def same_words(got, want, what):
    """Word for word."""
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, want {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, the first at {tuple(bad[0])}: got {int(got[tuple(bad[0])]):#x}, want {int(want[tuple(bad[0])]):#x}"


def same_values(got, want, what):
    """Equal as numbers (+0 and -0 are one value; no NaN is expected)."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(~(got == want))
    assert bad.size == 0, f"{what}: {bad.size} values differ, the first at {int(bad[0])}: got {got[bad[0]]!r}, want {want[bad[0]]!r}"


# ------------------------------------------------------------------------------------------------ the cases, run through a backend

def run_lane_cases(be):
    """Every integer and lane case -> {name: (got, want)}; the caller compares (and the device's with the emulation's)."""
    src = shuffle_sources()
    m24a, m24b = mul24_pairs()
    m24 = _rows(pack(m24a, m24b))
    n24 = m24a.size
    uni = np.repeat(lane_rows()[:, :1], 64, axis=1)
    cases = {
        "scan_add": (be.wave("SCAN_ADD", scan_rows()), ref_scan_add(scan_rows())),
        "scan_add16": (be.wave("SCAN_ADD16", scan_rows()), ref_scan_add16(scan_rows())),
        "scan_max16": (be.wave("SCAN_MAX16", scan_rows()), ref_scan_max16(scan_rows())),
        "rank": (be.wave("RANK", mask_rows()), ref_rank(mask_set())),
        "ballot": (be.wave("BALLOT", mask_rows()), mask_rows()),
        "readlane": (be.wave("READLANE", lane_rows()), ref_readlane(lane_rows())),
        "uniform": (be.wave("UNIFORM", uni), uni),
        "shfl": (be.wave("SHFL", pack(shuffle_payload32(), src)), np.take_along_axis(shuffle_payload32(), src, axis=1)),
        "shfl_f64": (be.wave("SHFL_F64", shfl64_rows()), ref_shfl64(shfl64_rows())),
        "popc": (be.wave("POPC", _rows(mask_set())), _rows(ref_popc(mask_set()))),
        "cell_rank": (be.wave("CELL_RANK", cell_rank_rows()), ref_cell_rank(cell_rank_rows())),
        "mul24": (be.wave("MUL24", m24).reshape(-1)[:n24], ref_mul24(m24a, m24b, True)),
        "umul24": (be.wave("UMUL24", m24).reshape(-1)[:n24], ref_mul24(m24a, m24b, False)),
        "div": (be.wave("DIV", div_rows()), ref_div(div_rows())),
    }
    w, v, lim = shift_operands()
    o0, o1 = be.ew("SHIFT_IN", words_as_doubles(w), v, lim)
    cases["shift_in_lt1"] = (doubles_as_words(o0), ref_shift_in(w, v, 1.0))
    cases["shift_in_lt"] = (doubles_as_words(o1), ref_shift_in(w, v, lim))
    return cases


def run_seeds(be):
    x = sqrt_operands()
    return seed_errors(x, be.ew("RSQ", x)[0], be.ew("RCP", x)[0])


def _rel(err, want):
    return float(np.max(err / np.abs(want)))


def run_sqrt_family(be, e_rsq):
    """sqrt_g, LR2_H2, sqrt_rh and lr2_arc_limit on the sqrt operands -> (figures, (x, h, T))."""
    x = sqrt_operands()
    fig = {}
    want, tol = sqrt_g_want_tol(x, e_rsq)
    fig["sqrt_g"] = _rel(within(be.ew("SQRT_G", x)[0], want, tol, "sqrt_g"), want)
    h, T = be.ew("H2_LIMIT", x)
    want, tol = h2_want_tol(x, e_rsq)
    fig["h2"] = _rel(within(h, want, tol, "LR2_H2"), want)
    g, hh = be.ew("SQRT_RH", x)
    (wg, tg), (wh, th) = sqrt_rh_want_tol(x)
    fig["sqrt_rh_g_ulp"] = float(np.max(within(g, wg, tg, "sqrt_rh g") / tg))
    fig["sqrt_rh_h_ulp"] = float(np.max(within(hh, wh, th, "sqrt_rh h") / (th / 2)))
    fig.update(check_arc_limit(x, h, T))
    return fig, (x, h, T)


def run_acos_family(be, e_rsq):
    x = acos_operands()
    fig = {}
    want, tol = acos2_want_tol(x, e_rsq)
    err = within(be.ew("ACOS2", x)[0], want, tol, "acos_fast2")
    two_asin = np.where(x >= 0, want, LD(np.pi) - want)
    big = two_asin > 0.1
    fig["acos_fast2_rel"] = float(np.max(err[big] / two_asin[big]))   # (as the header's figure is stated: relative to 2 asin u)
    fig["acos_fast2_abs_near_1"] = float(np.max(err[np.abs(x) > 1 - 1e-6]))
    want, tol = acos_want_tol(x, e_rsq)
    err = within(be.ew("ACOS", x)[0], want, tol, "acos_fast")
    fig["acos_fast_rel"] = float(np.max(err / want))
    c = acos_lower_operands()
    fig.update(check_acos_lower(c, be.ew("ACOS_LOWER", c)[0]))
    return fig


def run_atan2_family(be):
    y, x, inv = atan2_operands()
    want, tol = atan2_want_tol(y, x)
    ulp_pi = np.spacing(np.pi)
    return {"atan2_fast_ulp_pi": float(np.max(within(be.ew("ATAN2", y, x)[0], want, tol, "atan2_fast"))) / ulp_pi,
            "atan2_inv_ulp_pi": float(np.max(within(be.ew("ATAN2_INV", y, x, inv)[0], want, tol, "atan2_inv"))) / ulp_pi}


def run_f32(be):
    x = f32_operands()
    rcp, rsq = be.ew("F32", x)
    return f32_errors(x, rcp, rsq, be.ew("F32_SQRT", x)[0])


def run_exact_value_cases(be):
    """fma, the division by the slice count, min / max -> {name: (got, want)}, equal as numbers."""
    cases = {}
    for k in FMA_K:
        p, z = fma_operands(k)
        cases[f"fma_k[{k!r}]"] = (be.ew("FMA_K", p, z, k=k)[0], ref_fma(p, z, k))
    x, ns, inv = div_ns_operands()
    cases["div_ns"] = (be.ew("DIV_NS", x, ns, inv)[0], ref_div_ns(x, ns))
    a, b = minmax_operands()
    mn, mn_into = be.ew("MIN", a, b)
    mx, mx_into = be.ew("MAX", a, b)
    cases.update({"min": (mn, np.minimum(a, b)), "min_into": (mn_into, np.minimum(a, b)), "max": (mx, np.maximum(a, b)),
                  "max_into": (mx_into, np.maximum(a, b))})
    return cases
