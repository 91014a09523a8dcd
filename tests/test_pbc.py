"""Periodic images (include/freesasa_gpu.h: freesasa_gpu_calc_periodic, FREESASA_GPU_FRAMES_PBC) without a GPU: the kernels'
phase functions (csrc/pbc_kernels.h) driven on the CPU against the numpy restatement of the definition (tests/pbc_ref.py), bit
for bit; that restatement itself against the explicit 27-replica system through the oracle; and the argument checks that come
before a device is touched or an output file opened."""
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
import pbc_ref
from emu import pbc_emu
from test_dcd import write_dcd

PROBE = 1.4


@pytest.fixture(scope="module")
def batch():
    return pbc_ref.batch()


@pytest.fixture(scope="module")
def expanded(batch):
    return pbc_ref.expand_batch(*batch, probe=PROBE)


def test_the_batch_is_what_the_kernels_can_go_wrong_on(batch, expanded):
    xyz, radii, offsets, cells = batch
    _, _, eoff, images = expanded
    assert list(np.diff(offsets)) == [0, 1, 2, 60, 516]
    a, b = int(offsets[3]), int(offsets[4])
    c = pbc_ref.cutoff(radii[a:b], PROBE)
    assert c == 2.0 * (2.0 + 1.4) and cells[3][0] < 2 * c                     # (12, 14, 16): both shifts on one axis
    w = pbc_ref.wrap(xyz[a:b], cells[3])
    both = (w < c) & (w > cells[3] - c)
    assert both[:, 0].any() and not both[:, 1:].any()
    assert images[1] == 26                                                     # the one atom: both shifts on every axis
    # atoms up to 1.5 box lengths outside the cell, on both sides
    for s in (3, 4):
        q = xyz[offsets[s]:offsets[s + 1]] / cells[s]
        assert q.min() < -0.5 and q.max() > 1.5 and q.min() > -1.5 and q.max() < 2.5
    assert images[0] == 0 and images[1] > 0 and np.all(images[1:] > 0)
    assert images[3] > 4 * 60                                                  # the periodic answer is another system


def test_emulated_kernels_equal_the_definition_bit_for_bit(batch, expanded):
    xyz, radii, offsets, cells = batch
    want_xyz, want_r, want_eoff, want_images = expanded
    got_xyz, got_r, eoff, images, rmax, ibase = pbc_emu.expand(xyz, radii, offsets, cells, PROBE)
    assert np.array_equal(images, want_images) and np.array_equal(eoff, want_eoff)
    assert got_xyz.shape == want_xyz.shape
    assert got_xyz.tobytes() == want_xyz.tobytes() and got_r.tobytes() == want_r.tobytes()      # coordinates, radii, order
    for s in range(5):
        a, b = int(offsets[s]), int(offsets[s + 1])
        assert rmax[s] == (radii[a:b].max() if b > a else 0.0)
        if b > a:                                                               # the bases: an exclusive scan in atom order
            assert ibase[a] == 0 and np.all(np.diff(ibase[a:b]) >= 0) and np.all(np.diff(ibase[a:b]) <= 26)
    # collect: the first n areas of every expanded structure
    fake = np.arange(eoff[-1], dtype=np.float64) + 0.5
    got = pbc_emu.collect(offsets, eoff, fake)
    want = np.concatenate([fake[eoff[s]:eoff[s] + offsets[s + 1] - offsets[s]] for s in range(5)])
    assert np.array_equal(got, want)


def test_emulated_kernels_on_frames_that_share_their_radii():
    """the trajectory lanes' form: no offsets, n atoms per structure, one set of radii"""
    n, nf = 60, 3
    xyz0, radii = pbc_ref.structure(n, (12.0, 14.0, 16.0), 5)
    radii[7] = 2.0
    rng = np.random.default_rng(6)
    frames = np.stack([xyz0 + rng.uniform(-0.3, 0.3, xyz0.shape) for _ in range(nf)])
    cells = np.array([(12.0 + 0.3 * f, 14.0, 16.0 - 0.2 * f) for f in range(nf)])
    got_xyz, got_r, eoff, images, _, _ = pbc_emu.expand(frames, radii, None, cells, PROBE, n_fixed=n)
    for f in range(nf):
        x, r, k = pbc_ref.expand(frames[f], radii, cells[f], PROBE)
        assert images[f] == k and eoff[f + 1] - eoff[f] == n + k
        assert got_xyz[eoff[f]:eoff[f + 1]].tobytes() == x.tobytes() and got_r[eoff[f]:eoff[f + 1]].tobytes() == r.tobytes()


def test_in_box_coordinates_are_not_touched():
    """every coordinate in [0, L) and further than c from every face: w == x bit for bit and no image"""
    rng = np.random.default_rng(9)
    xyz, radii = rng.uniform(100.0, 900.0, (300, 3)), rng.uniform(1.2, 2.0, 300)
    got_xyz, got_r, eoff, images, _, _ = pbc_emu.expand(xyz, radii, [0, 300], [(1000.0, 1000.0, 1000.0)], PROBE)
    assert images[0] == 0 and got_xyz.tobytes() == xyz.tobytes() and got_r.tobytes() == radii.tobytes()


def sixty(batch, case):
    xyz, radii, offsets, cells = batch
    if case == "12x14x16":
        return xyz[offsets[3]:offsets[4]], radii[offsets[3]:offsets[4]], cells[3]
    x, r = pbc_ref.structure(60, (30.0, 9.0, 50.0), 77)
    return x, r, np.array((30.0, 9.0, 50.0))


@pytest.mark.parametrize("case", ["12x14x16", "30x9x50"])
def test_the_yardstick_equals_the_explicit_27_replica_system(oracle_lib, batch, case):
    """tests/pbc_ref.py's expansion through the oracle against the central cell of the 27 replicas: S&R-100 exactly, L&R-20 within
    1e-8 A^2 per atom (the project's asserted L&R bound on ordinary inputs)"""
    x, r, cell = sixty(batch, case)
    n = r.size
    ex, er, k = pbc_ref.expand(x, r, cell, PROBE)
    rx, rr = pbc_ref.replicas(x, r, cell)
    assert 0 < k < 26 * n
    sr_e, _ = oracle_lib.shrake_rupley(ex, er, PROBE, 100)
    sr_r, _ = oracle_lib.shrake_rupley(rx, rr, PROBE, 100)
    assert np.array_equal(sr_e[:n], sr_r[:n])
    lr_e = oracle_lib.lee_richards(ex, er, PROBE, 20)
    lr_r = oracle_lib.lee_richards(rx, rr, PROBE, 20)
    print(f"{case}: images {k}, L&R max |expansion - replicas| = {np.max(np.abs(lr_e[:n] - lr_r[:n])):.3e} A^2")
    assert np.max(np.abs(lr_e[:n] - lr_r[:n])) <= 1e-8
    # ... and it is another number than the non-periodic one
    lr_0 = oracle_lib.lee_richards(pbc_ref.wrap(x, cell), r, PROBE, 20)
    assert np.max(np.abs(lr_0 - lr_e[:n])) > 10.0 and lr_0.sum() > lr_e[:n].sum() + 100.0


def test_the_yardstick_through_the_reference_library(reference_lib, batch):
    """the same through the reference library itself, where it is built: the (12, 14, 16) case only - on the expansion of the
    (30, 9, 50) case the reference library ends in a segmentation fault of its own (311 finite atoms, none closer than 1 A to
    another), which would take the test session with it"""
    x, r, cell = sixty(batch, "12x14x16")
    n = r.size
    ex, er, _ = pbc_ref.expand(x, r, cell, PROBE)
    rx, rr = pbc_ref.replicas(x, r, cell)
    a = reference_lib.calc_coord(ex, er, alg=fa.SHRAKE_RUPLEY, probe=PROBE, n_points=100)[0]
    b = reference_lib.calc_coord(rx, rr, alg=fa.SHRAKE_RUPLEY, probe=PROBE, n_points=100)[0]
    assert np.array_equal(a[:n], b[:n])
    a = reference_lib.calc_coord(ex, er, alg=fa.LEE_RICHARDS, probe=PROBE, n_slices=20)[0]
    b = reference_lib.calc_coord(rx, rr, alg=fa.LEE_RICHARDS, probe=PROBE, n_slices=20)[0]
    assert np.max(np.abs(a[:n] - b[:n])) <= 1e-8


# ---------------------------------------------------------------- refusals that need no device

def paths(tmp, tag):
    return {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "done")}


def test_file_driver_refusals_before_a_device_is_touched(tmp_path):
    rng = np.random.default_rng(1)
    frames = rng.uniform(100.0, 900.0, (3, 7, 3)).astype(np.float32)
    radii = np.full(7, 1.7)
    # bit 3 without bit 2
    frames.tofile(tmp_path / "frames.f32")
    p = paths(tmp_path, "raw")
    with pytest.raises(RuntimeError, match="bit 3 of frames_f32 .* needs bit 2"):
        fa.trajectory_file(tmp_path / "frames.f32", radii, p["totals"], p["sasa"], done_path=p["done"], f32=True, pbc=True)
    # a DCD file without a cell record
    write_dcd(tmp_path / "nocell.dcd", frames)
    p = paths(tmp_path, "nocell")
    with pytest.raises(RuntimeError, match="unit-cell record"):
        fa.trajectory_file(tmp_path / "nocell.dcd", radii, p["totals"], p["sasa"], done_path=p["done"], dcd=True, pbc=True)
    assert not any(os.path.exists(q) for q in list(paths(tmp_path, "raw").values()) + list(p.values())), "an output file was opened"


def test_chain_groups_refuse_periodic_images(tmp_path):
    b = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    n = int(b.n_atoms)
    write_dcd(tmp_path / "f.dcd", np.asarray(b.xyz, dtype=np.float32)[None] + 500.0, cell=True)
    with pytest.raises(RuntimeError, match="not offered with chain groups"):
        fa.trajectory_file_topology(tmp_path / "f.dcd", b, str(tmp_path / "t"), group=np.zeros(n, dtype=np.int32), n_groups=1,
                                    group_areas_path=str(tmp_path / "g"), dcd=True, pbc=True)
    assert not os.path.exists(tmp_path / "t") and not os.path.exists(tmp_path / "g")


def test_calc_periodic_refusals_before_a_device_is_touched(batch):
    xyz, radii, offsets, cells = batch
    bad = cells.copy()
    c = pbc_ref.cutoff(radii[offsets[2]:offsets[3]], PROBE)
    bad[2][1] = c - 0.01
    with pytest.raises(RuntimeError, match=r"structure 2: edge y .* shorter than c"):
        fa.calc_periodic(xyz, radii, offsets, bad, probe=PROBE)
    bad = cells.copy()
    bad[3][2] = np.inf
    with pytest.raises(RuntimeError, match=r"structure 3: edge z .* not finite"):
        fa.calc_periodic(xyz, radii, offsets, bad, probe=PROBE)
    bad = cells.copy()
    bad[4][0] = np.nan
    with pytest.raises(RuntimeError, match=r"structure 4: edge x .* not finite"):
        fa.calc_periodic(xyz, radii, offsets, bad, probe=PROBE)
    # a structure without atoms has no cell to check
    odd = cells.copy()
    odd[0] = np.nan
    odd[1][0] = 1.0
    with pytest.raises(RuntimeError, match=r"structure 1: edge x"):
        fa.calc_periodic(xyz, radii, offsets, odd, probe=PROBE)
    # the engine's 2^30 limit, from the offsets alone: no array is read (these hold one atom)
    with pytest.raises(RuntimeError, match="expanded batch is too large"):
        fa.calc_periodic(np.zeros(3), np.ones(1), [0, (1 << 30) + 1], [(100.0, 100.0, 100.0)], probe=PROBE)
