"""Molecular volume (include/freesasa_gpu.h: freesasa_gpu_calc_volume, freesasa_gpu_trajectory_volume) without a GPU: the numpy
restatement of the definition (tests/volume_ref.py) against analytic volumes; the kernels' phase functions (csrc/vol_kernels.h,
the store phase of csrc/sr_caps.h) driven on the CPU against that restatement, bit for bit; the condition the GPU tests rest on
(the restatement's counts are the oracle's on the seeded batch); and the argument checks that come before a device is touched
or an output file opened."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
import volume_ref as vr
from emu import volume_emu

PROBE = 1.4
ENTRIES = ("freesasa_gpu_sr_volume_dev", "freesasa_gpu_calc_volume", "freesasa_gpu_trajectory_volume", "freesasa_gpu_trajectory_file_volume")


@pytest.fixture(scope="module")
def batch():
    return vr.batch()


_REF = {}


def reference(batch, n_points):
    """the restatement on the batch, once per point count"""
    if n_points not in _REF:
        _REF[n_points] = vr.volume_batch(*batch, PROBE, fa.test_points(n_points))
    return _REF[n_points]


# ---------------------------------------------------------------- the restatement against analytic volumes

@pytest.mark.parametrize("n_points", [1, 24, 100, 128])
def test_a_lone_sphere_is_exact_anywhere_in_space(n_points):
    """d = x - o is exactly 0, so E drops out: V = (4 pi R^2 / N)(R N) / 3, a handful of roundings from 4/3 pi R^3"""
    rng = np.random.default_rng(5)
    unit = fa.test_points(n_points)
    for scale in (1e-3, 1.0, 100.0, 1e6):
        x, r = rng.uniform(-1e3, 1e3, 3) * scale, rng.uniform(0.5, 3.0)
        R = r + PROBE
        want = 4.0 / 3.0 * math.pi * R ** 3
        assert abs(vr.volume_one([x], [r], PROBE, unit) - want) <= 4 * np.spacing(want)


def test_two_overlapping_spheres_converge_to_the_lens_formula():
    """R = 3 A (1.6 + the probe), the centres 3 A apart along x.  Measured with this restatement on the CPU: -0.893 % at 100
    points, -0.222 % at 1000, +0.0090 % at 5000; the bounds are twice that."""
    err = {}
    for n_points in (100, 1000, 5000):
        got = vr.volume_one([[0, 0, 0], [3, 0, 0]], [1.6, 1.6], PROBE, fa.test_points(n_points))
        want = vr.two_sphere_union(3.0, 3.0)
        err[n_points] = (got - want) / want
        print(n_points, got, want, err[n_points])
    assert abs(err[100]) < 1.8e-2        # 2 x 0.893 %
    assert abs(err[1000]) < 4.5e-3       # 2 x 0.222 %
    assert abs(err[5000]) < 1.8e-4       # 2 x 0.0090 %
    assert abs(err[5000]) <= abs(err[100])


def test_the_lens_formula_itself():
    assert vr.two_sphere_union(3.0, 6.0) == pytest.approx(2 * 4 / 3 * math.pi * 27)      # tangent: two spheres
    assert vr.two_sphere_union(3.0, 0.0) == pytest.approx(4 / 3 * math.pi * 27)          # coincident: one


# ---------------------------------------------------------------- the batch, and the condition the bit-for-bit tests rest on

def test_the_batch_is_what_the_kernels_can_go_wrong_on(batch, oracle_lib):
    xyz, radii, offsets = batch
    assert list(np.diff(offsets)) == [1, 2, 2, 3, 0, 70, 400]
    ref = reference(batch, 100)
    c = ref["counts"]
    assert c[0] == 100 and list(c[1:3]) == [100, 100]                            # alone; no neighbours
    assert 0 < c[3] < 100 and 0 < c[4] < 100                                     # overlapping
    assert c[6] == 0 and np.all(ref["evec"][6] == 0) and ref["vol"][6] == 0      # wholly inside another atom
    assert ref["volumes"][4] == 0 and np.all(ref["origin"][4] == 0)              # no atoms
    assert np.all(ref["volumes"][[0, 1, 2, 3, 5, 6]] > 0)
    R = radii[0] + PROBE
    assert abs(ref["volumes"][0] - 4.0 / 3.0 * math.pi * R ** 3) <= 4 * np.spacing(ref["volumes"][0])
    assert np.array_equal(ref["origin"][0], xyz[0])                              # one atom: o = x exactly
    # buried atoms in the two large structures, and atoms whose exposure spans more than one mask word
    for s in (5, 6):
        cs = c[offsets[s]:offsets[s + 1]]
        assert (cs == 0).any() and (cs > 32).any()


@pytest.mark.parametrize("n_points", vr.POINT_COUNTS)
def test_the_restatements_counts_are_the_oracles_on_every_atom(batch, oracle_lib, n_points):
    """a condition on the INPUTS, with zero exceptions: the GPU tests compare bit for bit under it (the engine's counts are the
    oracle's: tests/test_gpu_parity.py)"""
    xyz, radii, offsets = batch
    ref = reference(batch, n_points)
    for s in range(7):
        b, e = int(offsets[s]), int(offsets[s + 1])
        if e > b:
            _, counts = oracle_lib.shrake_rupley(xyz[b:e], radii[b:e], PROBE, n_points)
            assert np.array_equal(counts, ref["counts"][b:e]), s
    # ... and on the 400 atoms far from the origin, where they are what they are near it
    b, e = int(offsets[6]), int(offsets[7])
    _, moved = oracle_lib.shrake_rupley(xyz[b:e] + vr.SHIFT, radii[b:e], PROBE, n_points)
    assert np.array_equal(moved, ref["counts"][b:e])
    assert np.array_equal(vr.exposed_mask(xyz[b:e] + vr.SHIFT, radii[b:e] + PROBE, fa.test_points(n_points)).sum(1), moved)


# ---------------------------------------------------------------- the kernels' phase functions on the CPU

@pytest.mark.parametrize("n_points", vr.POINT_COUNTS)
def test_emulated_origin_terms_and_totals_equal_the_definition_bit_for_bit(batch, n_points):
    xyz, radii, offsets = batch
    ref = reference(batch, n_points)
    origin, vol, volumes = volume_emu.volume(xyz, radii, offsets, ref["counts"], ref["evec"], PROBE, n_points)
    assert origin.tobytes() == ref["origin"].tobytes()
    assert vol.tobytes() == ref["vol"].tobytes()
    assert volumes.tobytes() == ref["volumes"].tobytes()


def test_emulated_kernels_on_frames_that_share_their_radii(batch):
    """the trajectory lanes' form: structures of n atoms, one set of radii"""
    xyz, radii, offsets = batch
    b, e = int(offsets[5]), int(offsets[6])
    rng = np.random.default_rng(3)
    frames = xyz[b:e][None] + rng.uniform(-0.2, 0.2, (3, e - b, 3))
    off = np.arange(4, dtype=np.int64) * (e - b)
    unit = fa.test_points(100)
    ref = vr.volume_batch(frames.reshape(-1, 3), radii[b:e], off, PROBE, unit, shared_radii=True)
    tiled = vr.volume_batch(frames.reshape(-1, 3), np.tile(radii[b:e], 3), off, PROBE, unit)
    assert ref["volumes"].tobytes() == tiled["volumes"].tobytes()
    origin, vol, volumes = volume_emu.volume(frames, radii[b:e], off, ref["counts"], ref["evec"], PROBE, 100, shared_radii=True)
    assert vol.tobytes() == ref["vol"].tobytes() and volumes.tobytes() == ref["volumes"].tobytes()


def test_totals_of_more_than_one_chunk():
    """a structure above SASA_BOUNDS_CHUNK atoms: the totals kernels add its chunks in order"""
    rng = np.random.default_rng(11)
    n = vr.BOUNDS_CHUNK + 300
    xyz, radii = rng.uniform(-50, 50, (n, 3)), rng.uniform(1.0, 2.0, n)
    counts, evec = rng.integers(0, 100, n).astype(np.int32), rng.uniform(-5, 5, (n, 3))
    off = np.array([0, n], dtype=np.int64)
    origin, vol, volumes = volume_emu.volume(xyz, radii, off, counts, evec, PROBE, 100)
    o = vr.origin_of(xyz)
    want = vr.atom_terms(xyz, radii + PROBE, counts, evec, o, 100)
    assert origin[0].tobytes() == o.tobytes() and vol.tobytes() == want.tobytes()
    assert volumes[0] == vr.totals_of(want) and volumes[0] != float(np.sum(want[::-1]))


@pytest.mark.parametrize("n_points", vr.POINT_COUNTS)
def test_emulated_store_phase_makes_the_exposed_vectors_bit_for_bit(batch, n_points):
    """the tile kernel's phases as tests/test_sr_caps.py drives them, with the vectors asked for: sr_caps_store<true>"""
    xyz, radii, offsets = batch
    ref = reference(batch, n_points)
    unit = fa.test_points(n_points)
    sasa, counts, totals, st, evec = volume_emu.sr_batch_with_evec(xyz, radii, offsets, unit, PROBE)
    plain = __import__("emu").run_batch(False, xyz, radii, offsets, probe=PROBE, resolution=n_points, unit_pts=unit)
    assert sasa.tobytes() == plain[0].tobytes() and counts.tobytes() == plain[1].tobytes() and totals.tobytes() == plain[2].tobytes()
    assert np.array_equal(counts, ref["counts"])
    assert st["slab_tiles"] == 0                     # (no tile in the last launch: that one runs the second arrangement)
    assert evec.tobytes() == ref["evec"].tobytes()


def test_a_redone_tile_writes_its_vectors_exactly_once(batch):
    """segments of 8 records per atom in the main launch: the dense tiles overflow, store nothing there and are redone by the
    second launch - the same vectors"""
    xyz, radii, offsets = batch
    ref = reference(batch, 100)
    unit = fa.test_points(100)
    sasa, counts, totals, st, evec = volume_emu.sr_batch_with_evec(xyz, radii, offsets, unit, PROBE, cap_idx=8)
    assert st["fallback_tiles"] > 0 and st["slab_tiles"] == 0
    assert np.array_equal(counts, ref["counts"]) and evec.tobytes() == ref["evec"].tobytes()


# ---------------------------------------------------------------- the C boundary without a device

def test_the_four_entries_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", fa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert f" T {name}\n" in syms, name
    assert "volume_resident" not in syms and "kl_vol_atom" not in syms


def test_calc_volume_refuses_bad_arguments_before_a_device_is_touched():
    L = fa.lib()
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int)
    xyz, radii = np.zeros(6), np.ones(2)
    sasa, vols = np.full(2, -7.0), np.full(1, -7.0)
    err = C.create_string_buffer(256)

    def call(x=xyz, r=radii, off=(0, 2), ns=1, n_points=100, s=sasa, v=vols):
        off = np.array(off, dtype=np.int64)
        p = lambda a: None if a is None else a.ctypes.data_as(dp)
        rc = L.freesasa_gpu_calc_volume(p(x), p(r), off.ctypes.data_as(lp), ns, PROBE, n_points, p(s), None, None, None, None, p(v), -1, err, 256)
        return rc, err.value.decode()

    assert call(x=None) == (-1, "null argument") and call(r=None) == (-1, "null argument")
    assert call(s=None) == (-1, "null argument") and call(v=None) == (-1, "null argument")
    assert call(n_points=0) == (-1, "n_points must be > 0") and call(n_points=-3) == (-1, "n_points must be > 0")
    assert call(ns=0) == (-1, "n_structs must be > 0")
    assert call(off=(1, 2)) == (-1, "offsets[0] must be 0")
    assert call(off=(0, 2, 1), ns=2) == (-1, "offsets must be non-decreasing")
    assert call(off=(0, 0)) == (-1, "empty batch")
    assert call(off=(0, (1 << 30) + 1)) == (-1, "batch too large (max 2^30 atoms per call)")
    assert np.all(sasa == -7.0) and np.all(vols == -7.0)
    # the device-pointer entry without a context
    assert L.freesasa_gpu_sr_volume_dev(None, None, None, None, 1, PROBE, 100, None, None, None, None, None, None) == -1
    with pytest.raises(RuntimeError, match="freesasa_gpu_calc_volume: n_points must be > 0"):
        fa.calc_volume(xyz, radii, [0, 2], n_points=0)


@pytest.fixture(scope="module")
def topology(tmp_path_factory):
    """the first 70 atoms of 1UBQ as a loaded batch of one structure"""
    src = os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb")
    lines = [l for l in open(src) if l.startswith("ATOM")][:70]
    path = tmp_path_factory.mktemp("vol") / "ubq70.pdb"
    path.write_text("".join(lines) + "END\n")
    one = ingest.load_pdb_files([str(path)])
    assert one.n_atoms == 70
    return one


def test_trajectory_entries_refuse_before_a_device_is_touched_or_a_file_opened(topology, tmp_path):
    one = topology
    frames = np.zeros((2, 70, 3))
    with pytest.raises(RuntimeError, match="Lee-Richards is not offered"):
        fa.trajectory_topology(frames, one, volumes=True, alg=fa.LEE_RICHARDS)
    with pytest.raises(RuntimeError, match="up to 128 test points .129 asked for"):
        fa.trajectory_topology(frames, one, volumes=True, alg=fa.SHRAKE_RUPLEY, resolution=129)
    with pytest.raises(RuntimeError, match="resolution must be > 0"):
        fa.trajectory_topology(frames, one, volumes=True, alg=fa.SHRAKE_RUPLEY, resolution=0)
    with pytest.raises(ValueError, match="not offered with chain groups"):
        fa.trajectory_topology(frames, one, volumes=True, alg=fa.SHRAKE_RUPLEY, resolution=100, separate_chains=True)
    # the C entries with nowhere to put the volumes
    L = fa._topology_proto(fa.lib())
    err = C.create_string_buffer(256)
    cb = one._as_c()
    dp = C.POINTER(C.c_double)
    totals = np.zeros(2)
    dev = np.zeros(1, dtype=np.int32)
    rc = L.freesasa_gpu_trajectory_volume(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, 70, None, None, fa.SHRAKE_RUPLEY, PROBE, 100, 0,
                                          totals.ctypes.data_as(dp), None, None, None, None, None, None, dev.ctypes.data_as(C.POINTER(C.c_int)), 1, err, 256)
    assert rc == -1 and "null argument" in err.value.decode()
    # the file form: nothing is opened
    frames.astype(np.float32).tofile(tmp_path / "frames.f32")
    out = {k: str(tmp_path / f"o.{k}") for k in ("totals", "vol", "done")}
    kw = dict(volumes_path=out["vol"], done_path=out["done"], f32=True, resolution=100)
    with pytest.raises(RuntimeError, match="Lee-Richards is not offered"):
        fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.LEE_RICHARDS, **kw)
    for bits in (dict(dcd=True, pbc=True), dict(dcd=True, pbc=True, triclinic=True)):
        with pytest.raises(RuntimeError, match="periodic images. are not offered with the volume"):
            fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.SHRAKE_RUPLEY, frame_atoms=70, **bits, **dict(kw, f32=False))
    with pytest.raises(RuntimeError, match="up to 128 test points"):
        fa.trajectory_file_topology(tmp_path / "frames.f32", one, out["totals"], alg=fa.SHRAKE_RUPLEY, **dict(kw, resolution=200))
    rc = L.freesasa_gpu_trajectory_file_volume(str(tmp_path / "frames.f32").encode(), 1, 0, 0, C.byref(cb), 0, 70, None, None, fa.SHRAKE_RUPLEY, PROBE,
                                               100, 0, out["totals"].encode(), None, None, None, None, None, None, None, 0,
                                               dev.ctypes.data_as(C.POINTER(C.c_int)), 1, None, err, 256)
    assert rc == -1 and "null argument" in err.value.decode()
    assert not any(os.path.exists(p) for p in out.values()), "an output file was opened"
