"""The device's own definitions of the arithmetic and the lane primitives - hardware seeds, inline assembly, data-parallel
scans, mbcnt, ballot, readlane, 24-bit products - and what is built on the seeds, through the known-answer kernels of
freesasa_amd/csrc/kat_kernels.h (GpuContext.kat_elementwise / kat_wave) against the references of tests/device_arith_ref.py:
the cases tests/test_device_arith.py runs through the CPU emulation, whose integer and lane results the device's must also
equal word for word.  The measured errors are printed (pytest -s) and kept in profiles/device_arith.md."""
import numpy as np
import pytest

import device_arith_ref as R
import emu
import freesasa_amd as fa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = fa.GpuContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def be(ctx):
    return R.Backend(lambda op, a, b, c, k: ctx.kat_elementwise(op, a, b, c, k), ctx.kat_wave)


@pytest.fixture(scope="module")
def emu_be():
    return R.Backend(lambda op, a, b, c, k: emu.kat_elementwise(op, a, b, c, k), emu.kat_wave)


@pytest.fixture(scope="module")
def seeds(be):
    return R.run_seeds(be)


@pytest.fixture(scope="module")
def sqrt_family(be, seeds):
    return R.run_sqrt_family(be, seeds["e_rsq"])


def test_hardware_seeds(seeds):
    print("device:", seeds, "e_rsq = 2^%.2f, e_rcp = 2^%.2f" % (np.log2(seeds["e_rsq"]), np.log2(seeds["e_rcp"])))


def test_sqrt_family_and_the_arc_limits_guarantee(sqrt_family):
    print("device:", sqrt_family[0])


def test_arc_limit_reaches_within_2_49_of_one(sqrt_family):
    """RN(T h) within 2^-49 of 1, from below: the limit is not more cautious than it was meant to be (the test of this name in
    tests/test_device_arith.py says what it found)."""
    _, (x, h, T) = sqrt_family
    print("device:", R.check_arc_limit_reach(h, T))


def test_acos_family(be, seeds):
    print("device:", R.run_acos_family(be, seeds["e_rsq"]))


def test_atan2_family(be):
    print("device:", R.run_atan2_family(be))


def test_fp32_seeds(be):
    fig = R.run_f32(be)
    print("device:", fig, {k: "2^%.2f" % np.log2(v) for k, v in fig.items()})


def test_exact_values(be):
    for name, (got, want) in R.run_exact_value_cases(be).items():
        R.same_values(got, want, name)


def test_lane_primitives_and_integer_arithmetic(be, emu_be):
    there = R.run_lane_cases(emu_be)
    for name, (got, want) in R.run_lane_cases(be).items():
        R.same_words(got, want, name)
        R.same_words(got, there[name][0], name + " (device against emulation)")


def test_refusals(ctx):
    x = np.ones(8)
    z = np.zeros((1, 64), dtype=np.uint64)
    for bad, why in ((lambda: ctx.kat_elementwise(R.EW["EW_OPS"], x), "unknown op"), (lambda: ctx.kat_elementwise(-1, x), "unknown op"),
                     (lambda: ctx.kat_elementwise(R.EW["ATAN2"], x), "null argument"),
                     (lambda: ctx.kat_elementwise(R.EW["RSQ"], x, outputs=0), "null argument"),
                     (lambda: ctx.kat_elementwise(R.EW["SQRT_RH"], x, outputs=1), "null argument"),
                     (lambda: ctx.kat_elementwise(R.EW["RSQ"], x, n=0), "n must be"),
                     (lambda: ctx.kat_elementwise(R.EW["RSQ"], np.ones((1 << 20) + 1)), "n must be"),
                     (lambda: ctx.kat_wave(R.WAVE["WAVE_OPS"], z), "unknown op"), (lambda: ctx.kat_wave(-1, z), "unknown op"),
                     (lambda: ctx.kat_wave(0, None, rows=1), "null argument"), (lambda: ctx.kat_wave(0, z, rows=0), "rows must be"),
                     (lambda: ctx.kat_wave(0, np.zeros((4097, 64), dtype=np.uint64)), "rows must be"),
                     (lambda: ctx.kat_wave(R.WAVE["SHFL"], R.pack(np.zeros((1, 64)), np.full((1, 64), 64))), "source lane"),
                     (lambda: ctx.kat_wave(R.WAVE["SHFL_F64"], np.zeros((3, 64), dtype=np.uint64)), "in pairs"),
                     (lambda: ctx.kat_wave(R.WAVE["DIV"], R.pack(np.full((1, 64), 69), np.zeros((1, 64)))), "beyond the range")):
        with pytest.raises(ValueError, match=why):
            bad()
    # ... and the context works on: more than one workgroup's worth of operands, the most rows a call takes
    a, b = np.arange(1 << 18, dtype=np.float64), np.full(1 << 18, 1000.0)
    assert np.array_equal(ctx.kat_elementwise(R.EW["MIN"], a, b)[1], np.minimum(a, b))
    rows = np.ones((4096, 64), dtype=np.uint64)
    assert np.array_equal(ctx.kat_wave(R.WAVE["SCAN_ADD"], rows), np.tile(np.arange(1, 65, dtype=np.uint64), (4096, 1)))
