"""The known-answer kernels of freesasa_amd/csrc/kat_kernels.h through the CPU emulation (tests/emu: emu_kat_elementwise,
emu_kat_wave) against the references of tests/device_arith_ref.py - the cases tests/test_device_arith_gpu.py runs through the
device hooks, so that what differs there is the device's definitions alone - and the proof that every check can fail.  The
first direct test of acos_fast2 and lr2_acos_lower."""
import numpy as np
import pytest

import device_arith_ref as R
import emu


@pytest.fixture(scope="module")
def be():
    return R.Backend(lambda op, a, b, c, k: emu.kat_elementwise(op, a, b, c, k), emu.kat_wave)


@pytest.fixture(scope="module")
def seeds(be):
    return R.run_seeds(be)


@pytest.fixture(scope="module")
def sqrt_family(be, seeds):
    return R.run_sqrt_family(be, seeds["e_rsq"])


def test_seeds_are_the_exact_quotients_here(seeds):
    """The emulation's SASA_RSQ / SASA_RCP: 1 / sqrt(x) in two roundings, 1 / x in one."""
    print(seeds)
    assert seeds["e_rsq"] <= 2.0 ** -52 and seeds["e_rcp"] <= 2.0 ** -53


def test_sqrt_family_and_the_arc_limits_guarantee(sqrt_family):
    print(sqrt_family[0])


def test_arc_limit_reaches_within_2_49_of_one(sqrt_family):
    """RN(T h) within 2^-49 of 1, from below: the limit is not more cautious than it was meant to be.  This test found that it
    was: with the factor 1 - 2^-49 that lr2_arc_limit first had, 1 - RN(T h) came to 14 .. 18 units of 2^-53 where 2^-49 is 16
    (T1 h = 1 only up to two roundings), 26 476 of the 132 072 operands beyond 16 with the exact seed and 26 596 on the device.
    With 1 - 14 x 2^-53 it is 12 .. 16 by construction (the comment above lr2_arc_limit), and the guarantee on the other side
    keeps five units by the same derivation, 6.0 measured (test_sqrt_family_and_the_arc_limits_guarantee)."""
    _, (x, h, T) = sqrt_family
    print(R.check_arc_limit_reach(h, T))


def test_acos_family(be, seeds):
    fig = R.run_acos_family(be, seeds["e_rsq"])
    print(fig)
    # the figures the header states for acos_fast2, with the exact seed: degree 12, 6.3e-13 of 2 asin u
    assert fig["acos_fast2_rel"] <= 6.3e-13


def test_atan2_family(be):
    print(R.run_atan2_family(be))


def test_fp32_seeds(be):
    print(R.run_f32(be))


def test_exact_values(be):
    for name, (got, want) in R.run_exact_value_cases(be).items():
        R.same_values(got, want, name)


def test_lane_primitives_and_integer_arithmetic(be):
    for name, (got, want) in R.run_lane_cases(be).items():
        R.same_words(got, want, name)


def test_refusals():
    x = np.ones(8)
    for bad in (lambda: emu.kat_elementwise(R.EW["EW_OPS"], x), lambda: emu.kat_elementwise(-1, x), lambda: emu.kat_elementwise(R.EW["ATAN2"], x),
                lambda: emu.kat_elementwise(R.EW["RSQ"], x, outputs=0), lambda: emu.kat_elementwise(R.EW["RSQ"], x, n=0),
                lambda: emu.kat_elementwise(R.EW["RSQ"], np.ones((1 << 20) + 1)),
                lambda: emu.kat_wave(R.WAVE["WAVE_OPS"], np.zeros((1, 64), dtype=np.uint64)), lambda: emu.kat_wave(0, None, rows=1),
                lambda: emu.kat_wave(0, np.zeros((1, 64), dtype=np.uint64), rows=0), lambda: emu.kat_wave(0, np.zeros((4097, 64), dtype=np.uint64)),
                lambda: emu.kat_wave(R.WAVE["SHFL"], R.pack(np.zeros((1, 64)), np.full((1, 64), 64))),
                lambda: emu.kat_wave(R.WAVE["SHFL_F64"], np.zeros((3, 64), dtype=np.uint64)),
                lambda: emu.kat_wave(R.WAVE["DIV"], R.pack(np.full((1, 64), 69), np.zeros((1, 64))))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ every check can fail

def _rejects(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_real_valued_checks_reject_twice_their_bound(seeds):
    """An output at twice the bound from the reference, in one operand, is refused; at half the bound it passes."""
    e = seeds["e_rsq"]
    y, x, _ = R.atan2_operands()
    (wg, tg), (wh, th) = R.sqrt_rh_want_tol(R.sqrt_operands())
    for what, (want, tol) in {"sqrt_g": R.sqrt_g_want_tol(R.sqrt_operands(), e), "h2": R.h2_want_tol(R.sqrt_operands(), e),
                              "sqrt_rh g": (wg, tg), "sqrt_rh h": (wh, th), "acos_fast2": R.acos2_want_tol(R.acos_operands(), e),
                              "acos_fast": R.acos_want_tol(R.acos_operands(), e), "atan2": R.atan2_want_tol(y, x)}.items():
        tol = np.broadcast_to(tol, want.shape)
        for i in (0, want.size // 2, want.size - 1, int(np.argmin(tol)), int(np.argmax(tol))):
            for sign in (1, -1):
                off = want.copy()
                off[i] = want[i] + sign * 2 * tol[i]
                got = off.astype(np.float64)
                if abs(R.LD(got[i]) - want[i]) <= tol[i]:   # (the bound is below the spacing of doubles there: the next double is beyond it)
                    got[i] = np.nextafter(got[i], sign * np.inf)
                    if abs(R.LD(got[i]) - want[i]) <= tol[i]:
                        got[i] = np.nextafter(got[i], sign * np.inf)
                _rejects(R.within, got, want, tol, what)
        R.within((want + tol / 2).astype(R.LD), want, tol, what)
    bad = np.sqrt(R.sqrt_operands())
    bad[7] = np.nan
    _rejects(R.within, bad, *R.sqrt_g_want_tol(R.sqrt_operands(), e), "sqrt_g")


def test_seed_checks_reject_twice_their_bound():
    x = R.sqrt_operands()
    rsq, rcp = 1 / np.sqrt(x), 1 / x
    R.seed_errors(x, rsq, rcp)
    for k in (0, x.size - 1):
        worse = rsq.copy(); worse[k] *= 1 + 2 * R.E_RSQ_MAX
        _rejects(R.seed_errors, x, worse, rcp)
        worse = rcp.copy(); worse[k] *= 1 - 2 * R.E_RCP_MAX
        _rejects(R.seed_errors, x, rsq, worse)
    f = R.f32_operands()
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    rcp, rsq, sq = f32(1 / f), f32(1 / np.sqrt(f)), f32(np.sqrt(f))
    R.f32_errors(f, rcp, rsq, sq)
    for which in range(3):
        outs = [rcp.copy(), rsq.copy(), sq.copy()]
        outs[which][5] = f32(outs[which][5:6] * (1 + 2 * R.F32_TOL))[0]
        _rejects(R.f32_errors, f, *outs)


def test_acos_lower_check_rejects_a_bound_that_loses_its_margin(be):
    c = R.acos_lower_operands()
    got = be.ew("ACOS_LOWER", c)[0]
    room = R.check_acos_lower(c, got)["acos_lower_room"]
    assert room >= 9.9e-10                       # the bound's own margin, 1e-9, at c -> 0
    i = int(np.argmin(np.abs(c)))
    for shift in (2 * R.ACOS_LOWER_MARGIN, 2e-9):   # half the margin gone and a little more; above acos itself
        worse = got.copy(); worse[i] += shift
        _rejects(R.check_acos_lower, c, worse)


def test_arc_limit_check_rejects_a_limit_beyond_the_room(sqrt_family):
    """T replaced by a larger neighbor on the operand with the least room.  The very next double is NOT refused, and must not be:
    the guarantee has 6.0 x 2^-53 to spare at the least (measured here and printed; five by derivation), and one step of T moves v h by 1 to 2 of
    those units - the check has no tolerance to hide in, so it is the first T whose v reaches 1 - 2^-50 that it refuses, and
    every one beyond; a T below the least v that needs the product, by the same, is taken."""
    fig, (x, h, T) = sqrt_family
    print(fig)
    i = fig["arc_limit_at"]
    assert 0 < fig["arc_limit_room"] < 2.0 ** -49
    one = T.copy(); one[i] = np.nextafter(T[i], np.inf)
    R.check_arc_limit(x, h, one)
    steps, bumped = 0, T.copy()
    while True:
        bumped[i] = np.nextafter(bumped[i], np.inf)
        steps += 1
        try:
            R.check_arc_limit(x, h, bumped)
        except AssertionError:
            break
        assert steps < 16
    assert 2 <= steps <= 9                       # room / (h ulp(T)): 6.0 units at 1 to 2 units a step
    bumped[i] = np.nextafter(bumped[i], np.inf)
    _rejects(R.check_arc_limit, x, h, bumped)
    for k in (0, x.size - 1):
        big = T.copy(); big[k] = T[k] * (1 + 2.0 ** -48)
        _rejects(R.check_arc_limit, x, h, big)
    R.check_arc_limit_reach(h, T)                  # the reach: a limit 2^-50 more cautious on one operand, then made-up limits at the edges
    for k in (0, i, x.size - 1):
        low = T.copy(); low[k] = T[k] * (1 - 2.0 ** -50)
        _rejects(R.check_arc_limit_reach, h, low)
    one_h = np.ones(3)
    R.check_arc_limit_reach(one_h, np.array([1 - 2.0 ** -49, 1 - 2.0 ** -50, 1 - 2.0 ** -53]))
    _rejects(R.check_arc_limit_reach, one_h, np.array([1 - 2.0 ** -49, 1 - 2.0 ** -49 - 2.0 ** -53, 1 - 2.0 ** -50]))
    _rejects(R.check_arc_limit_reach, one_h, np.array([1 - 2.0 ** -49, 1.0, 1 - 2.0 ** -50]))


def test_lane_checks_reject_one_in_one_lane_and_one_flipped_mask_bit(be):
    cases = R.run_lane_cases(be)
    rng = np.random.default_rng(1)
    for name, (got, want) in cases.items():
        got = np.array(got, dtype=np.uint64)
        R.same_words(got, want, name)
        flat = got.reshape(-1)
        for j in (0, flat.size - 1, int(rng.integers(flat.size))):
            off = flat.copy(); off[j] += np.uint64(1)                 # one more in one lane
            _rejects(R.same_words, off.reshape(got.shape), want, name)
            off = flat.copy(); off[j] ^= np.uint64(1) << np.uint64(rng.integers(64))   # one flipped bit
            _rejects(R.same_words, off.reshape(got.shape), want, name)
    masks = R.mask_rows()
    for bit in (0, 31, 32, 63):                                       # a ballot with one mask bit flipped, a rank one off from bit 32 on
        off = masks.copy(); off[70, 5] ^= np.uint64(1) << np.uint64(bit)
        _rejects(R.same_words, off, masks, "ballot")
    rank = R.ref_rank(R.mask_set())
    off = rank.copy(); off[1, 33:] += np.uint64(1)
    _rejects(R.same_words, off, rank, "rank")


def test_exact_value_checks_reject_the_neighboring_double(be):
    for name, (got, want) in R.run_exact_value_cases(be).items():
        for j in (0, got.size - 1):
            off = np.array(got); off[j] = (off[j] + 1.0 if abs(off[j]) < 1 else off[j] * 0.5) if np.isfinite(off[j]) else 0.0
            _rejects(R.same_values, off, want, name)
    p, z = R.fma_operands(0.5)
    unfused = p * z + 0.5                                            # what a product rounded on its own gives: the operands tell the two apart
    assert np.any(unfused != R.ref_fma(p, z, 0.5))
