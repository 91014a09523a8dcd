"""The XTC decode kernels (freesasa_amd/csrc/xtc_kernels.h: xtc_scan, xtc_unpack) on the device, on their own, through the test
hook freesasa_gpu_xtc_decode_dev - the launches the file drivers make for a shard - against the pure-Python codec
(tests/xtc_codec.py): the group records are the codec's trace, the fp32 output is the codec's, bit for bit, and every element of
the NaN-prefilled output of a good frame is written.  The CPU emulation of the same phase functions (tests/emu/emu_xtc.cpp) is held
to the same, as a second witness.  Planned frames force every path of the format; long frames make the scan's window move, by
every excess; many frames fill more workgroups than the device has CUs; damaged streams get the emulation's status word."""
import numpy as np
import pytest

import freesasa_amd as fa
import xtc_codec as xc
from emu import xtc_emu
from test_xtc import CASES, case_frame, jittered_ints, mutants, pad_plan, records_as_trace, synth

pytestmark = pytest.mark.gpu

XTC_WIN = 512                      # xtc_kernels.h: 32-bit words of the stream in LDS at a time
ST_BITS, ST_ATOMS, ST_SMALLIDX, ST_VALUE = 1, 2, 4, 8


@pytest.fixture(scope="module")
def ctx():
    c = fa.GpuContext()
    yield c
    c.close()


def assert_decoded(got, frames, who):
    rec, status, xyz = got
    assert len(rec) == len(frames) == len(status) == len(xyz)
    assert not status.any(), (who, status)
    for k, f in enumerate(frames):
        assert xyz[k].shape == f.xyz.shape and xyz[k].dtype == np.float32
        assert records_as_trace(rec[k]) == f.trace, (who, k)
        assert not np.isnan(xyz[k]).any(), (who, k)
        assert xyz[k].tobytes() == f.xyz.tobytes(), (who, k)


def check_shard(ctx, data, n_atoms):
    """the whole frames of `data` as one shard: device and emulation against the codec; returns the codec's frames"""
    frames = xc.decode(data)
    assert all(f.natoms == n_atoms for f in frames)
    assert_decoded(ctx.xtc_decode(data, len(frames), n_atoms), frames, "device")
    assert_decoded(xtc_emu.decode(data, len(frames), n_atoms), frames, "emulation")
    return frames


# ---------------------------------------------------------------- a. every path of the format

@pytest.mark.parametrize("name", list(CASES))
def test_every_format_path_as_a_frame_of_its_own(ctx, name):
    for seed in (7, 8):
        _, _, ints, data = case_frame(name, seed=seed)
        (f,) = check_shard(ctx, data, len(ints))
        assert np.array_equal(f.ints, ints)


def test_every_format_path_as_the_frames_of_one_shard(ctx):
    """twelve frames of 64 atoms, of unequal length, each at its own offset; bitsize == 0 and != 0 frames in one launch"""
    made = [case_frame(name, n=64) for name in CASES]
    frames = check_shard(ctx, b"".join(m[3] for m in made), 64)
    assert len(frames) == len(CASES) and len({f.size for f in frames}) > 6
    zero = [xc.bit_sizes([f.maxint[k] - f.minint[k] + 1 for k in range(3)])[0] == 0 for f in frames]
    assert any(zero) and not all(zero)
    for f, (plan, smallidx, ints, _) in zip(frames, made):
        assert np.array_equal(f.ints, ints) and [t[2] for t in f.trace] == [3 * k for k, _ in plan]


def test_every_remainder_of_the_byte_count(ctx):
    seen = set()
    for n in range(45, 53):
        (f,) = check_shard(ctx, case_frame("runs 0..8", n=n)[3], n)
        seen.add(f.bytecount % 4)
    assert seen == {0, 1, 2, 3}


# ---------------------------------------------------------------- b. the scan's window as it moves

def big_bits(f):
    bitsize, bitsizeint = xc.bit_sizes([f.maxint[k] - f.minint[k] + 1 for k in range(3)])
    return bitsize or sum(bitsizeint)


def window_events(f):
    """xtc_scan_walk's window over the codec's trace: (groups that end on the window's last bit, the excesses end - lim of the
    groups at which it hops, the flags' bits within their words)"""
    bb, total, w0 = big_bits(f), 8 * f.bytecount, 0
    edges, excesses, flag_bits = 0, [], set()
    for bit, _, _, _ in f.trace:
        fpos = bit + bb
        end, lim = min(fpos + 6, total), 32 * (w0 + XTC_WIN)
        if end > lim:
            excesses.append(end - lim)
            w0 = fpos >> 5
            assert end <= 32 * (w0 + XTC_WIN)
        edges += end == lim
        flag_bits.add(fpos & 31)
    return edges, excesses, flag_bits


WINDOW_SPANS = (3000, 10000, 40000, 200000, 1 << 22)   # (10000 is there for the excesses 2 and 4)


def test_the_window_hops_by_every_excess_and_not_at_its_edge(ctx):
    """frames of 901 .. 909 atoms, streams of 4 to 7.5 KiB with big fields of 35 .. 66 bits, a leading run group of 0 .. 8 small
    atoms shifting everything behind it; the frames of one atom count are one shard"""
    edges, excesses, flag_bits, widths, hops = 0, set(), set(), set(), []
    for pre in range(9):
        plan = [(pre, 0)] + [(0, 0)] * 900
        datas = [xc.encode(synth(plan, 20, 100 * pre + 1, span=span), 1000.0, plan=plan, smallidx=20) for span in WINDOW_SPANS]
        for f in check_shard(ctx, b"".join(datas), 901 + pre):
            e, x, fb = window_events(f)
            edges += e
            excesses |= set(x)
            flag_bits |= fb
            widths.add(big_bits(f))
            hops.append(len(x))
            assert 4000 < f.bytecount < 7800
    # what the inputs reach, by the codec alone: the edge itself (no hop), a hop by every excess of 1 .. 6 bits - the flag, or a
    # part of the run field behind it, just outside the window -, flags at both ends of a word, one to three hops per frame
    assert edges >= 1 and excesses >= {1, 2, 3, 4, 5, 6} and {0, 31} <= flag_bits, (edges, sorted(excesses), sorted(flag_bits))
    assert widths == {35, 40, 46, 53, 66} and set(hops) == {1, 2, 3}


def test_runs_and_smallidx_across_the_window(ctx):
    data = b"".join(xc.encode(ints, 1000.0) for ints in jittered_ints(3000, 2, 3000))
    frames = check_shard(ctx, data, 3000)
    assert len(frames) == 2 and min(f.bytecount for f in frames) > 2 * 4 * XTC_WIN and len({f.size for f in frames}) == 2
    assert all(len(window_events(f)[1]) >= 2 and max(t[2] for t in f.trace) > 3 for f in frames)


# ---------------------------------------------------------------- c. many frames

def test_six_hundred_frames_in_one_launch(ctx):
    """more workgroups of the scan than the device has CUs; 37 does not divide the unpack's workgroup: a slot's frame changes
    within a workgroup"""
    data = b"".join(xc.encode(ints, 1000.0) for ints in jittered_ints(37, 600, 37))
    frames = check_shard(ctx, data, 37)
    assert len(frames) == 600 and len({f.size for f in frames}) > 10 and len({len(f.trace) for f in frames}) > 3


# ---------------------------------------------------------------- d. values

PRECISIONS = (100.0, 1000.0, 1234.5, 2e7)


def two_products(ints, precision):
    return (ints.astype(np.float32) * np.float32(1.0 / float(np.float32(precision)))) * np.float32(10.0)


@pytest.mark.parametrize("name", ["bitsize 0", "smallidx held at 72"])
def test_integers_beyond_2_24_at_four_precisions(ctx, name):
    plan, smallidx, kw = CASES[name]
    plan = pad_plan(plan, 40)
    ints = synth(plan, smallidx, 5, span=kw["span"], lo=[-(3 << 24), -(1 << 25), -(1 << 24)])
    assert ints.min() < -(1 << 25) and ints.max() > (1 << 25)
    assert (ints.astype(np.float32).astype(np.int64) != ints).sum() > 20           # (float) rounds
    datas = [xc.encode(ints, p, plan=plan, smallidx=smallidx) for p in PRECISIONS]
    frames = check_shard(ctx, b"".join(datas), 40)
    for f, p in zip(frames, PRECISIONS):
        assert f.precision == np.float32(p) and np.array_equal(f.ints, ints)
        assert f.xyz.tobytes() == two_products(ints, p).tobytes()
    # one product instead of two is another number somewhere
    assert any((f.xyz != ints.astype(np.float32) * (np.float32(1.0 / float(np.float32(p))) * np.float32(10.0))).any() for f, p in zip(frames, PRECISIONS))


def test_the_widest_dimensions_a_header_may_hold(ctx):
    """sizeint = 2^32 - 1 in every dimension: three fields of 32 bits, minint = -2^31; one more is refused by the host, with the
    same reason through the hook and through the emulation"""
    lo, hi = -(1 << 31), (1 << 31) - 2
    plan = [(0, 0)] * 4 + [(3, 0), (8, 0), (1, 0), (0, 0), (2, 0)]
    ints = synth(plan, 72, 9, span=(1 << 32) - (1 << 28), lo=[lo + (1 << 27)] * 3)
    ints[0], ints[1], ints[2] = [lo, hi, lo], [hi, lo, hi], [-1, 0, 1]
    assert ints.min() == lo and ints.max() == hi
    data = xc.encode(ints, 1000.0, plan=plan, smallidx=72, minint=[lo] * 3, maxint=[hi] * 3)
    (f,) = check_shard(ctx, data + data, len(ints))[:1]
    assert np.array_equal(f.ints, ints) and big_bits(f) == 96
    assert f.xyz.tobytes() == two_products(ints, 1000.0).tobytes()
    wider = xc.frame_bytes(f.natoms, 0, 0.0, np.zeros((3, 3)), 1000.0, [lo] * 3, [hi, hi + 1, hi], 72, f.stream)
    reason = "dimension y spans all 2^32 integers"
    with pytest.raises(ValueError) as dev:
        ctx.xtc_decode(data + wider, 2, f.natoms)
    with pytest.raises(ValueError) as emu:
        xtc_emu.decode(data + wider, 2, f.natoms)
    assert str(dev.value) == "freesasa_gpu_xtc_decode_dev: frame 1 of the XTC bytes: " + reason
    assert str(emu.value) == "emu_xtc_shard -2: " + reason
    check_shard(ctx, data, len(ints))                                             # (and the context works on)


# ---------------------------------------------------------------- e. damaged streams

def test_damaged_streams_get_the_emulations_status(ctx):
    """the first 240 of the streams that tests/test_xtc.py has put through the sanitizer-built emulation: one shard per atom count"""
    by_atoms = {}
    for f, s in mutants(2000, seed=11)[:240]:
        by_atoms.setdefault(f.natoms, []).append((f, s))
    n_good = n_damaged = 0
    seen = set()
    for natoms, group in by_atoms.items():
        data = b"".join(xc.frame_bytes(f.natoms, 0, 0.0, np.zeros((3, 3)), float(f.precision), f.minint, f.maxint, f.smallidx, s) for f, s in group)
        rec, status, xyz = ctx.xtc_decode(data, len(group), natoms)
        e_rec, e_status, e_xyz = xtc_emu.decode(data, len(group), natoms)
        # the scan is serial, and XTC_ST_VALUE is the same bit whichever thread of the unpack sets it: the words are equal
        assert status.tobytes() == e_status.tobytes()
        for k, (f, s) in enumerate(group):
            seen.add(int(status[k]))
            if status[k]:
                # Only the status is compared.  Which groups of such a frame wrote their atoms before another thread raised
                # XTC_ST_VALUE is a race by design (a thread tests the status when it starts, not when it writes), and a frame
                # the scan gave a status has records up to where it stopped: what is left of the frame is not a frame.
                n_damaged += 1
                continue
            ints, trace = xc.decode_stream(s, f.natoms, f.minint, f.maxint, f.smallidx)      # (raises if the codec refuses the stream)
            want = xc.to_angstrom(ints, f.precision)
            for who, r, x in (("device", rec[k], xyz[k]), ("emulation", e_rec[k], e_xyz[k])):
                assert records_as_trace(r) == trace, (who, k)
                assert not np.isnan(x).any() and x.tobytes() == want.tobytes(), (who, k)
            n_good += 1
    assert n_good + n_damaged == 240 and n_good >= 20 and n_damaged >= 20
    assert seen >= {0, ST_BITS, ST_ATOMS, ST_SMALLIDX, ST_VALUE}


# ---------------------------------------------------------------- the hook itself

def test_hook_refusals_and_failed_allocations():
    """argument errors through the context's error text; the hook's device and page-locked memory is the context's workspace: the
    n-th allocation fails, the call says so, and the next call works"""
    _, _, ints, data = case_frame("ten atoms")
    (f,) = xc.decode(data)
    c = fa.GpuContext()
    try:
        for nth in (1, 2):                                         # (a new context: the staging first, then the device buffer)
            fa.lib().freesasa_gpu_test_fail_after(nth)
            try:
                with pytest.raises(ValueError, match="page-locked host memory" if nth == 1 else "dev_malloc"):
                    c.xtc_decode(data, 1, 10)
            finally:
                fa.lib().freesasa_gpu_test_fail_after(0)
        assert_decoded(c.xtc_decode(data, 1, 10), [f], "device")
        for args, text in (((data, 0, 10), "xtc_decode: n_frames must be at least 1"), ((data, 1, 0), "xtc_decode: n_atoms must be at least 1"),
                           ((b"", 1, 10), "xtc_decode: len must be at least 1"),
                           ((data, 2, 10), "frame 1 of the XTC bytes: the file ends inside its header"),
                           ((data, 1, 11), "frame 0 of the XTC bytes: it holds 10 atoms, frame 0 holds 11")):
            with pytest.raises(ValueError) as e:
                c.xtc_decode(*args)
            assert str(e.value) == "freesasa_gpu_xtc_decode_dev: " + text
        assert_decoded(c.xtc_decode(data, 1, 10), [f], "device")
    finally:
        c.close()
