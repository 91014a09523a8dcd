"""Exposure masks and surface dots (include/freesasa_gpu.h: freesasa_gpu_calc_masks, freesasa_gpu_dots_from_masks,
freesasa_gpu_trajectory_masks) without a GPU: the kernels' phase functions (the store phase of csrc/sr_caps.h in mask mode, the
scan and the expansion of csrc/dots_kernels.h) driven on the CPU against the numpy restatement of the definitions
(tests/dots_ref.py, tests/volume_ref.py's exposed_mask), bit for bit; the same phases in a stand-alone program under
sanitizers; the argument checks that come before a device is touched or an output file opened; and the record format of
tools/dots_pdb.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
import dots_ref as dr
import volume_ref as vr
from emu import dots_emu

PROBE = 1.4
ENTRIES = ("freesasa_gpu_sr_masks_dev", "freesasa_gpu_dots_count_dev", "freesasa_gpu_dots_expand_dev", "freesasa_gpu_calc_masks",
           "freesasa_gpu_dots_from_masks", "freesasa_gpu_masks_count", "freesasa_gpu_trajectory_masks", "freesasa_gpu_trajectory_file_masks")


@pytest.fixture(scope="module")
def batch():
    return vr.batch()


_REF = {}


def reference_masks(batch, n_points):
    """vr.exposed_mask on every structure of the batch as masks [n, 4], once per point count"""
    if n_points not in _REF:
        xyz, radii, offsets = batch
        unit = fa.test_points(n_points)
        rows = [vr.exposed_mask(xyz[b:e], radii[b:e] + PROBE, unit) for b, e in zip(offsets[:-1], offsets[1:]) if e > b]
        _REF[n_points] = dr.masks_of(np.concatenate(rows))
    return _REF[n_points]


# ---------------------------------------------------------------- the restatement itself

def test_the_restatement_packs_and_unpacks_bits():
    rng = np.random.default_rng(1)
    for N in (1, 31, 32, 33, 100, 128):
        e = rng.random((9, N)) < 0.5
        m = dr.masks_of(e)
        assert m.dtype == np.uint32 and m.shape == (9, 4)
        assert np.array_equal(dr.bits_of(m, N), e)
        assert not np.any(m & ~dr.full_words(N))
        assert np.array_equal(dr.popcounts(m, N), e.sum(1))
    assert list(dr.full_words(33)) == [0xffffffff, 1, 0, 0] and list(dr.full_words(128)) == [0xffffffff] * 4
    m = np.array([[0b101, 0, 0, 0], [0, 0, 0, 0], [0xffffffff, 1, 0, 0]], dtype=np.uint32)
    assert list(dr.dot_first(m, 33)) == [0, 2, 2, 35]
    d, a, p = dr.dots(np.array([[1.0, 2, 3], [0, 0, 0], [4, 5, 6]]), [1.0, 1.0, 2.0], 0.5, fa.test_points(33), m)
    assert list(a[:3]) == [0, 0, 2] and list(p[:3]) == [0, 2, 0] and len(d) == 35
    u = fa.test_points(33)
    assert np.array_equal(d[1], u[2] * 1.5 + np.array([1.0, 2, 3]))


# ---------------------------------------------------------------- the store phase in mask mode, on the CPU

@pytest.mark.parametrize("n_points", vr.POINT_COUNTS)
def test_emulated_store_phase_keeps_the_exposure_masks_bit_for_bit(batch, n_points):
    """the tile kernel's phases as tests/test_sr_caps.py drives them, with the masks asked for: sr_caps_store<SR_STORE_MASK>"""
    xyz, radii, offsets = batch
    want = reference_masks(batch, n_points)
    unit = fa.test_points(n_points)
    sasa, counts, totals, st, masks = dots_emu.sr_batch_with_masks(xyz, radii, offsets, unit, PROBE)
    plain = __import__("emu").run_batch(False, xyz, radii, offsets, probe=PROBE, resolution=n_points, unit_pts=unit)
    assert sasa.tobytes() == plain[0].tobytes() and counts.tobytes() == plain[1].tobytes() and totals.tobytes() == plain[2].tobytes()
    assert st["slab_tiles"] == 0                     # (no tile in the last launch: that one runs the second arrangement)
    assert masks.tobytes() == want.tobytes()
    assert np.array_equal(dr.popcounts(masks, n_points), counts)
    assert not np.any(masks & ~dr.full_words(n_points))
    pop_all = np.array([bin(int(w)).count("1") for w in masks.reshape(-1)]).reshape(-1, 4).sum(1)
    assert np.array_equal(pop_all, counts)           # ... counted over all 128 bits too


def test_a_redone_tile_writes_its_masks_exactly_once(batch):
    """segments of 8 records per atom in the main launch: the dense tiles overflow, store nothing there and are redone by the
    second launch - the same masks"""
    xyz, radii, offsets = batch
    sasa, counts, totals, st, masks = dots_emu.sr_batch_with_masks(xyz, radii, offsets, fa.test_points(100), PROBE, cap_idx=8)
    assert st["fallback_tiles"] > 0 and st["slab_tiles"] == 0
    assert masks.tobytes() == reference_masks(batch, 100).tobytes()


# ---------------------------------------------------------------- the scan and the expansion, on the CPU

def scan_sizes():
    B, T = dots_emu.shape()
    return [1, B - 1, B, B + 1, 2 * B + 3, B * T + 1]


@pytest.mark.parametrize("k", range(6))
def test_emulated_scan_equals_cumsum(k):
    n = scan_sizes()[k]
    rng = np.random.default_rng(100 + k)
    masks = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    masks[rng.random(n) < 0.2] = 0
    for N in (100, 128):
        got = dots_emu.count(masks, N)
        pop = np.zeros(n, dtype=np.int64)
        for w, full in enumerate(dr.full_words(N)):
            v = masks[:, w] & full
            for s in (1, 2, 4, 8, 16):       # (popcount by folding, a way of its own)
                m = np.uint32([0x55555555, 0x33333333, 0x0f0f0f0f, 0x00ff00ff, 0x0000ffff][(1, 2, 4, 8, 16).index(s)])
                v = (v & m) + ((v >> np.uint32(s)) & m)
            pop += v
        want = np.concatenate([[0], np.cumsum(pop)]).astype(np.int64)
        assert got.dtype == np.int64 and np.array_equal(got, want)


def test_emulated_scan_of_an_all_zero_array():
    B, _ = dots_emu.shape()
    got = dots_emu.count(np.zeros((2 * B + 3, 4), dtype=np.uint32), 100)
    assert np.array_equal(got, np.zeros(2 * B + 4, dtype=np.int64))


def synthetic(seed, n, N, stray=False):
    rng = np.random.default_rng(seed)
    return rng.uniform(-50, 50, (n, 3)), rng.uniform(1.0, 2.0, n), dr.random_masks(rng, n, N, stray)


@pytest.mark.parametrize("n_points", [1, 33, 100, 128])
def test_emulated_expansion_equals_the_definition_bit_for_bit(n_points):
    xyz, radii, masks = synthetic(7 + n_points, 900, n_points)
    assert (dr.popcounts(masks, n_points) == 0).any() and (dr.popcounts(masks, n_points) == n_points).any()
    unit = fa.test_points(n_points)
    first = dots_emu.count(masks, n_points)
    assert np.array_equal(first, dr.dot_first(masks, n_points))
    want_xyz, want_atom, want_point = dr.dots(xyz, radii, PROBE, unit, masks)
    D = int(first[-1])
    assert D == len(want_xyz) > 0
    dx, da, dp = dots_emu.expand(xyz, radii, PROBE, unit, masks, first, D)
    assert dx[:D].tobytes() == want_xyz.tobytes() and np.array_equal(da[:D], want_atom) and np.array_equal(dp[:D], want_point)
    assert np.all(np.isnan(dx[D:])) and np.all(da[D:] == -7) and np.all(dp[D:] == -7)


def test_the_expansions_pair_index_is_the_integer_division_up_to_two_to_the_30_atoms():
    """no GPU test can hold 2^30 atoms' dots: the arithmetic that replaces the 64-bit division is walked on the CPU"""
    assert dots_emu.pair_misses() == 0


def test_emulated_expansion_ignores_stray_bits():
    xyz, radii, masks = synthetic(3, 500, 33, stray=True)
    assert np.any(masks & ~dr.full_words(33))
    unit = fa.test_points(33)
    first = dots_emu.count(masks, 33)
    assert np.array_equal(first, dr.dot_first(masks, 33))
    want_xyz, want_atom, want_point = dr.dots(xyz, radii, PROBE, unit, masks)
    D = int(first[-1])
    dx, da, dp = dots_emu.expand(xyz, radii, PROBE, unit, masks, first, D)
    assert dx[:D].tobytes() == want_xyz.tobytes() and np.array_equal(da[:D], want_atom) and np.array_equal(dp[:D], want_point)
    assert np.all(np.isnan(dx[D:])) and np.all(da[D:] == -7)


def test_emulated_expansion_writes_nothing_past_the_capacity():
    xyz, radii, masks = synthetic(5, 600, 100)
    unit = fa.test_points(100)
    first = dots_emu.count(masks, 100)
    want_xyz, want_atom, want_point = dr.dots(xyz, radii, PROBE, unit, masks)
    D = int(first[-1])
    dx, da, dp = dots_emu.expand(xyz, radii, PROBE, unit, masks, first, D - 3)
    assert dx[:D - 3].tobytes() == want_xyz[:D - 3].tobytes() and np.array_equal(da[:D - 3], want_atom[:D - 3])
    assert np.array_equal(dp[:D - 3], want_point[:D - 3])
    assert np.all(np.isnan(dx[D - 3:])) and np.all(da[D - 3:] == -7) and np.all(dp[D - 3:] == -7)      # the guard region
    # ... and a dot_first that lies (every atom claims its neighbour's slots too) still writes inside the arrays
    lying = first.copy()
    lying[1:-1] -= 1
    dx, da, dp = dots_emu.expand(xyz, radii, PROBE, unit, masks, np.maximum(lying, 0), D - 3)
    assert np.all(np.isnan(dx[D - 3:])) and np.all(da[D - 3:] == -7)


def test_stand_alone_sanitizer_program():
    """scan and expansion under AddressSanitizer + UBSan, in a program of their own (nothing is preloaded anywhere)"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/dots_check"], check=True, stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "dots_check")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")
    B, T = dots_emu.shape()
    for case in ["pair-index"] + [f"scan-{n}" for n in (1, B - 1, B, B + 1, 2 * B + 3, B * T + 1)] + ["scan-all-zero", "scan-stray-bits", "expand-1", "expand-33",
                                                                                    "expand-100", "expand-128", "expand-all-zero",
                                                                                    "expand-stray-bits", "expand-capacity-short-by-3"]:
        assert f"{case} ok" in lines, res.stdout


# ---------------------------------------------------------------- the C boundary without a device

def test_the_entries_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", fa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert f" T {name}\n" in syms, name
    assert "masks_resident" not in syms and "kl_dots_expand" not in syms


def test_calc_masks_refuses_bad_arguments_before_a_device_is_touched():
    L = fa.lib()
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    xyz, radii = np.zeros(6), np.ones(2)
    sasa, masks = np.full(2, -7.0), np.full((2, 4), 7, dtype=np.uint32)
    err = C.create_string_buffer(256)

    def call(x=xyz, r=radii, off=(0, 2), ns=1, n_points=100, s=sasa, m=masks):
        off = np.array(off, dtype=np.int64)
        p = lambda a: None if a is None else a.ctypes.data_as(dp)
        rc = L.freesasa_gpu_calc_masks(p(x), p(r), off.ctypes.data_as(lp), ns, PROBE, n_points, p(s), None, None,
                                       None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint32)), -1, err, 256)
        return rc, err.value.decode()

    assert call(x=None) == (-1, "null argument") and call(r=None) == (-1, "null argument")
    assert call(s=None) == (-1, "null argument") and call(m=None) == (-1, "null argument")
    assert call(n_points=0) == (-1, "n_points must be > 0") and call(n_points=-3) == (-1, "n_points must be > 0")
    assert call(ns=0) == (-1, "n_structs must be > 0")
    assert call(off=(1, 2)) == (-1, "offsets[0] must be 0")
    assert call(off=(0, 2, 1), ns=2) == (-1, "offsets must be non-decreasing")
    assert call(off=(0, 0)) == (-1, "empty batch")
    assert call(off=(0, (1 << 30) + 1)) == (-1, "batch too large (max 2^30 atoms per call)")
    assert np.all(sasa == -7.0) and np.all(masks == 7)
    # the device-pointer entries without a context
    assert L.freesasa_gpu_sr_masks_dev(None, None, None, None, 1, PROBE, 100, None, None, None, None) == -1
    assert L.freesasa_gpu_dots_count_dev(None, None, 1, 100, None, None) == -1
    assert L.freesasa_gpu_dots_expand_dev(None, None, None, 1, PROBE, 100, None, None, 0, None, None, None) == -1
    with pytest.raises(RuntimeError, match="freesasa_gpu_calc_masks: n_points must be > 0"):
        fa.calc_masks(xyz, radii, [0, 2], n_points=0)


def test_masks_count_counts_on_the_host_and_refuses_stray_bits():
    rng = np.random.default_rng(17)
    for N in (1, 33, 100, 128):
        masks = dr.random_masks(rng, 257, N)
        assert fa.masks_count(masks, N) == int(dr.popcounts(masks, N).sum())
    masks = np.array([[0b1011, 0, 0, 0], [0, 0, 0, 0], [0xffffffff, 1, 0, 0]], dtype=np.uint32)
    assert fa.masks_count(masks, 33) == 36 and fa.masks_count(masks, 128) == 36 and fa.masks_count(masks[:2], 4) == 3
    with pytest.raises(RuntimeError, match="atom 2: a mask bit at or above n_points .32. is set"):
        fa.masks_count(masks, 32)
    with pytest.raises(RuntimeError, match="n_points must be > 0"):
        fa.masks_count(masks, 0)
    with pytest.raises(RuntimeError, match="hold up to 128 test points"):
        fa.masks_count(masks, 129)
    with pytest.raises(RuntimeError, match="n_atoms must be > 0"):
        fa.masks_count(masks[:0], 100)
    err = C.create_string_buffer(64)
    assert fa.lib().freesasa_gpu_masks_count(None, 3, 100, C.byref(C.c_longlong(0)), err, 64) == -1 and err.value == b"null argument"
    assert fa.lib().freesasa_gpu_masks_count(masks.ctypes.data_as(C.POINTER(C.c_uint32)), 3, 100, None, err, 64) == -1


def test_dots_from_masks_checks_the_masks_before_a_device_is_touched():
    xyz, radii = np.zeros((3, 3)), np.ones(3)
    masks = np.array([[0b1011, 0, 0, 0], [0, 0, 0, 0], [0xffffffff, 1, 0, 0]], dtype=np.uint32)        # 3 + 0 + 33 bits
    with pytest.raises(RuntimeError, match="the masks hold 36 exposed points, n_dots says 35"):
        fa.dots_from_masks(xyz, radii, masks, 35, n_points=33)
    with pytest.raises(RuntimeError, match="the masks hold 36 exposed points, n_dots says 37"):
        fa.dots_from_masks(xyz, radii, masks, 37, n_points=100)
    with pytest.raises(RuntimeError, match="atom 2: a mask bit at or above n_points .32. is set"):
        fa.dots_from_masks(xyz, radii, masks, 36, n_points=32)
    with pytest.raises(RuntimeError, match="n_points must be > 0"):
        fa.dots_from_masks(xyz, radii, masks, 36, n_points=0)
    with pytest.raises(RuntimeError, match="hold up to 128 test points"):
        fa.dots_from_masks(xyz, radii, masks, 36, n_points=129)
    with pytest.raises(RuntimeError, match="n_dots must be >= 0"):
        fa.dots_from_masks(xyz, radii, masks, -1, n_points=100)
    with pytest.raises(ValueError, match="must agree"):
        fa.dots_from_masks(xyz, radii, masks[:2], 3, n_points=100)
    L = fa.lib()
    err = C.create_string_buffer(256)
    dp = C.POINTER(C.c_double)
    out = np.full(3 * 36, -7.0)
    args = lambda x, r, m, o: (None if x is None else x.ctypes.data_as(dp), None if r is None else r.ctypes.data_as(dp), 3, PROBE, 100,
                               None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint32)), 36, None,
                               None if o is None else o.ctypes.data_as(dp), None, None, -1, err, 256)
    for a in (args(None, radii, masks, out), args(xyz.reshape(-1), None, masks, out), args(xyz.reshape(-1), radii, None, out),
              args(xyz.reshape(-1), radii, masks, None)):
        assert L.freesasa_gpu_dots_from_masks(*a) == -1 and err.value.decode() == "null argument"
    assert np.all(out == -7.0)


@pytest.fixture(scope="module")
def topology(tmp_path_factory):
    """the first 70 atoms of 1UBQ as a loaded batch of one structure"""
    src = os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb")
    lines = [l for l in open(src) if l.startswith("ATOM")][:70]
    path = tmp_path_factory.mktemp("dots") / "ubq70.pdb"
    path.write_text("".join(lines) + "END\n")
    one = ingest.load_pdb_files([str(path)])
    assert one.n_atoms == 70
    return one


def test_trajectory_entries_refuse_before_a_device_is_touched_or_a_file_opened(topology, tmp_path):
    one = topology
    frames = np.zeros((2, 70, 3))
    with pytest.raises(RuntimeError, match="exposure masks .* Lee-Richards is not offered"):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.LEE_RICHARDS)
    with pytest.raises(RuntimeError, match="exposure masks are offered up to 128 test points .129 asked for"):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=129)
    with pytest.raises(RuntimeError, match="resolution must be > 0"):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=0)
    with pytest.raises(ValueError, match="masks=True is not offered with chain groups"):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=100, separate_chains=True)
    with pytest.raises(ValueError, match="masks=True is not offered with .*stats="):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=100, stats=("totals",))
    with pytest.raises(ValueError, match="masks=True is not offered with .*volumes=True"):
        fa.trajectory_topology(frames, one, masks=True, volumes=True, alg=fa.SHRAKE_RUPLEY, resolution=100)
    # the C entries with nowhere to put the masks
    L = fa._topology_proto(fa.lib())
    err = C.create_string_buffer(256)
    cb = one._as_c()
    dp = C.POINTER(C.c_double)
    totals = np.zeros(2)
    dev = np.zeros(1, dtype=np.int32)
    rc = L.freesasa_gpu_trajectory_masks(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, 70, None, None, fa.SHRAKE_RUPLEY, PROBE, 100, 0,
                                         totals.ctypes.data_as(dp), None, None, None, None, None, None, dev.ctypes.data_as(C.POINTER(C.c_int)), 1, err, 256)
    assert rc == -1 and "null argument" in err.value.decode()
    # the file form: nothing is opened
    frames.astype(np.float32).tofile(tmp_path / "frames.f32")
    out = {k: str(tmp_path / f"o.{k}") for k in ("totals", "masks", "vol", "done")}
    kw = dict(masks_path=out["masks"], done_path=out["done"], f32=True, resolution=100)
    with pytest.raises(RuntimeError, match="Lee-Richards is not offered"):
        fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.LEE_RICHARDS, **kw)
    for bits in (dict(dcd=True, pbc=True), dict(dcd=True, pbc=True, triclinic=True)):
        with pytest.raises(RuntimeError, match="periodic images. are not offered with the exposure masks"):
            fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.SHRAKE_RUPLEY, frame_atoms=70, **bits, **dict(kw, f32=False))
    with pytest.raises(RuntimeError, match="up to 128 test points"):
        fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.SHRAKE_RUPLEY, **dict(kw, resolution=200))
    with pytest.raises(ValueError, match="masks_path is not offered with .*volumes_path"):
        fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.SHRAKE_RUPLEY, volumes_path=out["vol"], **kw)
    with pytest.raises(ValueError, match="masks_path is not offered with chain groups"):
        fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.SHRAKE_RUPLEY, separate_chains=True, **kw)
    with pytest.raises(ValueError, match="masks_path is not offered with .*stats="):
        fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.SHRAKE_RUPLEY, stats=("totals",), **kw)
    rc = L.freesasa_gpu_trajectory_file_masks(str(tmp_path / "frames.f32").encode(), 1, 0, 0, C.byref(cb), 0, 70, None, None, fa.SHRAKE_RUPLEY, PROBE,
                                              100, 0, out["totals"].encode(), None, None, None, None, None, None, None, 0,
                                              dev.ctypes.data_as(C.POINTER(C.c_int)), 1, None, err, 256)
    assert rc == -1 and "null argument" in err.value.decode()
    assert not any(os.path.exists(p) for p in out.values()), "an output file was opened"


# ---------------------------------------------------------------- the tool's records

def test_dots_pdb_formats_its_records():
    from tools import dots_pdb
    dots = np.array([[1.0, -2.5, 3.25], [-123.4567, 0.0005, 9999.999], [0.0, 0.0, 0.0]])
    lines = dots_pdb.format_dots(dots, np.array([0, 10010, 99998], dtype=np.int32))
    assert lines[0] == "HETATM    1  DOT DOT     1       1.000  -2.500   3.250  1.00  0.00"
    assert lines[1] == "HETATM    2  DOT DOT    11    -123.457   0.001" + "9999.999  1.00  0.00"       # serial 10011 modulo 10000
    assert lines[2] == "HETATM    3  DOT DOT  9999       0.000   0.000   0.000  1.00  0.00"
    for l in lines:
        assert len(l) == 66 and l[17:20] == "DOT" and l[12:16] == " DOT" and float(l[30:38]) == round(float(l[30:38]), 3)
    assert [int(l[22:26]) for l in lines] == [1, 11, 9999]
    assert dots_pdb.format_dots(np.zeros((0, 3)), np.zeros(0, dtype=np.int32)) == []
