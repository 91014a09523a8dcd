"""Run statistics of the trajectory drivers (freesasa_gpu_trajectory_stats and its kin, include/freesasa_gpu.h) without a GPU:
the kernel's phase function (csrc/traj_kernels.h, traj_stats) driven on the CPU against a plain numpy loop in the order of the
definition, the merge of the product library (csrc/trajstats.c) against the same formulas in numpy - both bit for bit -, the
accuracy of the formulation against a long-double reference, and the argument checks, which the library makes before it
touches a device or a file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from emu import stats_emu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")


def partial_ref(a):
    """the definition, per column of a [nf, w]: s = 0; s += a[f]; mean = s / nf; lo, hi; M2 = 0; d = a[f] - mean; M2 += d * d.
    (numpy rounds every elementwise operation on its own: d * d is a product before it is added)"""
    a = np.asarray(a, dtype=np.float64)
    nf, w = a.shape
    s = np.zeros(w)
    for f in range(nf):
        s = s + a[f]
    mean = s / float(nf)
    m2 = np.zeros(w)
    for f in range(nf):
        d = a[f] - mean
        m2 = m2 + d * d
    return np.stack([mean, m2, a.min(0), a.max(0)])


def merge_ref(parts, frames):
    """the merge, left to right from shard 0's partial: [4, W] mean, std, min, max"""
    mean, m2, lo, hi = (np.array(r) for r in parts[0])
    n = int(frames[0])
    for b, nb in zip(parts[1:], frames[1:]):
        nb = int(nb)
        t = n + nb
        d = b[0] - mean
        r = float(nb) / float(t)
        mean = mean + d * r
        m2 = (m2 + b[1]) + (d * d) * (float(n) * r)
        lo, hi = np.minimum(lo, b[2]), np.maximum(hi, b[3])
        n = t
    return np.stack([mean, np.sqrt(m2 / float(n)), lo, hi])


def cut_ref(a, frames):
    """the statistics of a [F, w] cut into shards of `frames` frames, and the partials [K, 4, w]"""
    at = np.concatenate([[0], np.cumsum(frames)])
    parts = np.stack([partial_ref(a[at[k]:at[k + 1]]) for k in range(len(frames))])
    return merge_ref(parts, frames), parts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("nf", [1, 2, 3, 8, 16, 37])      # (8: what a thread loads ahead of its additions)
@pytest.mark.parametrize("w", [1, 3, 602])
def test_emulated_kernel_equals_the_loop_bit_for_bit(nf, w):
    rng = np.random.default_rng(1000 * nf + w)
    a = rng.uniform(0.0, 60.0, (nf, w)) * (rng.random((nf, w)) > 0.3)      # area-like: many exact zeros
    assert same_bits(stats_emu.traj_stats([a]), partial_ref(a))


def test_emulated_kernel_over_a_table_of_segments():
    """several outputs in one launch: every segment's columns land at its first column, with its own width as the stride"""
    rng = np.random.default_rng(5)
    blocks = [rng.uniform(0, 900, (5, 1)), rng.uniform(0, 60, (5, 602)), rng.uniform(0, 300, (5, 3)), rng.uniform(0, 200, (5, 456)),
              rng.uniform(0, 999, (5, 10))]
    got = stats_emu.traj_stats(blocks)
    assert same_bits(got, np.concatenate([partial_ref(b) for b in blocks], axis=1))


def test_constant_and_all_zero_columns():
    """A constant column has std exactly 0 and min == max == mean WHEN ITS RUNNING SUM IS EXACT (42.5: every k * 42.5, k <= 37, is
    a double), and so has an all-zero column.  The definition - s += a[f], mean = s / nf - does not give that for every constant:
    37 additions of 42.7 round, the mean is off 42.7 by a few ulp and M2 is the square of that.  The bound: each addition errs
    by at most eps / 2 of the partial sum, so |mean - c| <= nf eps / 2 c and std <= nf eps / 2 c."""
    a = np.empty((37, 4))
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = 42.5, 0.0, np.random.default_rng(3).uniform(0, 1, 37), 42.7
    p = stats_emu.traj_stats([a])
    assert same_bits(p, partial_ref(a))
    assert p[1, 0] == 0.0 and p[0, 0] == p[2, 0] == p[3, 0] == 42.5
    assert np.all(p[:, 1] == 0.0) and not np.any(np.signbit(p[:, 1]))
    out = fa.traj_stats_merge(np.stack([p, p]), [37, 37])
    assert out[1, 0] == 0.0 and out[0, 0] == out[2, 0] == out[3, 0] == 42.5 and np.all(out[:, 1] == 0.0)
    bound = 37 * np.finfo(np.float64).eps / 2 * 42.7
    assert out[2, 3] == out[3, 3] == 42.7 and abs(out[0, 3] - 42.7) <= bound and out[1, 3] <= bound
    for nf in (1, 2, 3):                                                    # short shards of the same columns
        q = stats_emu.traj_stats([a[:nf, :2]])
        assert np.all(q[1] == 0.0) and same_bits(q[0], q[2]) and same_bits(q[0], q[3])


@pytest.fixture(scope="module")
def seven():
    rng = np.random.default_rng(20261019)
    return rng.uniform(0.0, 60.0, (7, 29)) * (rng.random((7, 29)) > 0.3)


@pytest.mark.parametrize("frames", [[3, 3, 1], [7], [1] * 7], ids=["3-3-1", "one-shard", "one-frame-per-shard"])
def test_merge_of_the_library_equals_the_formulas_bit_for_bit(seven, frames):
    want, parts = cut_ref(seven, frames)
    got = fa.traj_stats_merge(parts, frames)
    assert same_bits(got, want)
    if frames == [1] * 7:
        assert np.all(parts[:, 1] == 0.0)                                   # one frame per shard: every M2 is 0
    if frames == [7]:
        assert same_bits(got[0], parts[0, 0]) and same_bits(got[1], np.sqrt(parts[0, 1] / 7.0))
    whole = partial_ref(seven)                                              # any cut agrees with one shard to rounding
    assert np.allclose(got[0], whole[0], rtol=1e-12, atol=1e-12) and np.allclose(got[1], np.sqrt(whole[1] / 7.0), rtol=1e-12, atol=1e-12)
    assert same_bits(got[2], seven.min(0)) and same_bits(got[3], seven.max(0))


def test_merge_of_a_sub_range_is_the_statistics_of_its_own_partials(seven):
    frames = [2, 3, 1, 1]
    _, parts = cut_ref(seven, frames)
    got = fa.traj_stats_merge(parts, frames, 1, 3)
    assert same_bits(got, merge_ref(parts[1:3], frames[1:3]))
    assert same_bits(got, cut_ref(seven[2:6], [3, 1])[0])


def longdouble_ref(col):
    x = col.astype(np.longdouble)
    mean = x.sum() / np.longdouble(x.size)
    return float(mean), float(np.sqrt(((x - mean) ** 2).sum() / np.longdouble(x.size)))


def rel(got, want):
    return abs(got - want) / max(abs(want), 1e-12) if want != 0 else abs(got) / 1e-12


def test_accuracy_against_long_double():
    rng = np.random.default_rng(11)
    u = rng.uniform(0.0, 1.0, 1000)
    frames37 = [37] * 27 + [1]
    assert sum(frames37) == 1000
    # area-like
    col = (50.0 + u)[:, None]
    out, parts = cut_ref(col, frames37)
    assert same_bits(fa.traj_stats_merge(parts, frames37), out)
    mean, std = longdouble_ref(col[:, 0])
    print("50 + U: mean", rel(out[0, 0], mean), "std", rel(out[1, 0], std))
    assert rel(out[0, 0], mean) <= 1e-12 and rel(out[1, 0], std) <= 1e-12
    # a large offset: the formulation, not just a tolerance
    col = (1e8 + u)[:, None]
    mean, std = longdouble_ref(col[:, 0])
    for frames in (frames37, [1] * 1000):
        _, parts = cut_ref(col, frames)
        got = fa.traj_stats_merge(parts, frames)
        print("1e8 + U, shards of", frames[0], ": std", rel(got[1, 0], std))
        assert rel(got[1, 0], std) <= 1e-6
    x = col[:, 0]
    var = (x * x).sum() / x.size - (x.sum() / x.size) ** 2                  # sum and sum of squares in fp64
    naive = np.sqrt(var) if var >= 0 else np.inf
    print("1e8 + U, sum of squares: std", rel(naive, std))
    assert rel(naive, std) > 1.0


def test_error_returns_of_the_merge():
    L = fa._stats_proto(fa.lib())
    dp, llp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    parts, out = np.zeros((2, 4, 3)), np.full((4, 3), -7.0)
    call = lambda frames, n_parts, width: L.freesasa_gpu_traj_stats_merge(parts.ctypes.data_as(dp), np.asarray(frames, dtype=np.int64).ctypes.data_as(llp),
                                                                          n_parts, width, out.ctypes.data_as(dp), None)
    assert call([3, 3], 0, 3) == -1                                         # zero parts
    assert call([3, 0], 2, 3) == -1                                         # a part without frames
    assert call([3, 3], 2, 0) == -1                                         # width 0
    assert np.all(out == -7.0)
    total = C.c_longlong(0)
    assert L.freesasa_gpu_traj_stats_merge(parts.ctypes.data_as(dp), np.array([3, 4], dtype=np.int64).ctypes.data_as(llp), 2, 3,
                                           out.ctypes.data_as(dp), C.byref(total)) == 0 and total.value == 7
    with pytest.raises(ValueError):
        fa.traj_stats_merge(parts, [3, 3], 1, 1)
    assert fa.traj_stats_width(("atoms", "residues"), 602, 76)[0] == 602 + 456
    W, first = fa.traj_stats_width(tuple(fa.STATS_BITS), 602, 76, 10, 2)
    assert W == 1 + 602 + 602 + 3 + 456 + 10 + 6 and list(first) == [0, 1, 603, 1205, 1208, 1664, 1674]
    with pytest.raises(ValueError):
        fa.stats_word(("medians",))


def test_refusals_come_before_any_device_or_file(tmp_path):
    """statistics of an output the run cannot compute: -1 with a message that names the output, from every entry, with no device
    (this test runs without one: the device list is looked at later) and no file created"""
    L = fa._stats_proto(fa._topology_proto(fa.lib()))
    batch = ingest.load_pdb_files([os.path.join(PDB, "1ubq.pdb")])
    n = batch.n_atoms
    cb = batch._as_c()
    sel = ingest.Selection(["a, resi -10"])
    ids = np.zeros(n, dtype=np.int32)
    devs = np.zeros(1, dtype=np.int32)
    ip, dp, i32p = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    frames = np.zeros((2, n, 3))
    radii = np.ones(n)
    frames_path = tmp_path / "frames.f64"
    frames.tofile(frames_path)
    enc = lambda p: str(p).encode()
    S = fa.STATS_BITS
    plain = [(S["classes"], "class-sums", "a topology"), (S["residues"], "residues", "a topology"), (S["selections"], "selections", "a topology"),
             (S["groups"], "groups", "chain groups"), (S["isolated"], "isolated", "chain groups"), (128, "unknown bit", "")]
    # (selection set, group ids, word) -> the output and what it needs
    topo = [(None, None, S["selections"], "selections", "a selection set"), (sel, None, S["groups"], "groups", "chain groups"),
            (sel, None, S["isolated"] | S["atoms"], "isolated", "chain groups"), (None, ids, S["selections"] | S["groups"], "selections", "a selection set"),
            (sel, ids, 256, "unknown bit", "")]
    outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "cls", "res", "sel", "grp", "iso", "stats", "parts")] + [tmp_path / "done.txt"]
    totals, stats_out = np.zeros(2), np.zeros(4 * (2 * n + 600))
    for word, name, needs in plain:
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_stats(frames.ctypes.data_as(dp), radii.ctypes.data_as(dp), n, 2, fa.LEE_RICHARDS, 1.4, 20, 0,
                                             totals.ctypes.data_as(dp), None, devs.ctypes.data_as(ip), 1, word, stats_out.ctypes.data_as(dp), None, err, 512)
        assert rc == -1 and name in err.value.decode() and needs in err.value.decode(), (word, err.value)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_stats(enc(frames_path), 0, 0, radii.ctypes.data_as(dp), n, 0, fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]),
                                                  None, enc(outs[9]), 0, devs.ctypes.data_as(ip), 1, None, word, enc(outs[7]), enc(outs[8]), err, 512)
        assert rc == -1 and name in err.value.decode() and needs in err.value.decode(), (word, err.value)
        assert not any(p.exists() for p in outs), name
    for s, g, word, name, needs in topo:
        hs, pg, G = (None if s is None else s.handle), (None if g is None else g.ctypes.data_as(i32p)), (0 if g is None else 1)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_groups_stats(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, n, None, hs, pg, G, fa.LEE_RICHARDS, 1.4, 20, 0,
                                                    totals.ctypes.data_as(dp), None, None, None, None, None, None, None, devs.ctypes.data_as(ip), 1,
                                                    word, stats_out.ctypes.data_as(dp), None, err, 512)
        assert rc == -1 and name in err.value.decode() and needs in err.value.decode(), (word, err.value)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_groups_stats(enc(frames_path), 0, 0, 0, C.byref(cb), 0, n, None, hs, pg, G, fa.LEE_RICHARDS, 1.4, 20, 0,
                                                         enc(outs[0]), None, None, None, None, None, None, None, enc(outs[9]), 0,
                                                         devs.ctypes.data_as(ip), 1, None, word, enc(outs[7]), enc(outs[8]), err, 512)
        assert rc == -1 and name in err.value.decode() and needs in err.value.decode(), (word, err.value)
        assert not any(p.exists() for p in outs), name
    # statistics with nowhere to go
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_stats(frames.ctypes.data_as(dp), radii.ctypes.data_as(dp), n, 2, fa.LEE_RICHARDS, 1.4, 20, 0,
                                         totals.ctypes.data_as(dp), None, devs.ctypes.data_as(ip), 1, S["atoms"], None, None, err, 512)
    assert rc == -1 and "stats_out" in err.value.decode()
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_file_stats(enc(frames_path), 0, 0, radii.ctypes.data_as(dp), n, 0, fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]),
                                              None, enc(outs[9]), 0, devs.ctypes.data_as(ip), 1, None, S["atoms"], enc(outs[7]), None, err, 512)
    assert rc == -1 and "partials path" in err.value.decode() and not any(p.exists() for p in outs)
    # ... and through the Python front-end
    with pytest.raises(RuntimeError, match="residues output need a topology"):
        fa.trajectory(frames, radii, stats=("residues",), devices=[0])
    with pytest.raises(RuntimeError, match="selections output need a selection set"):
        fa.trajectory_topology(frames, batch, stats=("selections",), devices=[0])
    with pytest.raises(RuntimeError, match="groups output need chain groups"):
        fa.trajectory_file_topology(frames_path, batch, outs[0], stats=("groups",), stats_path=outs[7], partials_path=outs[8], devices=[0])
    assert not any(p.exists() for p in outs)
    sel.close()


def test_stand_alone_sanitizer_program():
    """the merge and the widths under AddressSanitizer + UBSan, in a program of their own (nothing is preloaded anywhere)"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/stats_check"], check=True, stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "stats_check")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    for case in ("shards-3-3-1", "one-shard", "one-frame-per-shard", "sub-range-1-3", "constant-column", "error-returns", "widths"):
        assert f"{case} ok" in lines, res.stdout
