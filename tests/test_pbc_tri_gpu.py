"""Periodic images in a triclinic cell on the device (include/freesasa_gpu.h: freesasa_gpu_calc_periodic_triclinic,
FREESASA_GPU_FRAMES_TRICLINIC).  The yardstick of the batch entry is the engine itself on the explicit expansion
tests/pbc_tri_ref.py makes (checked against the 5 x 5 x 5 replica system in tests/test_pbc_tri.py): the real atoms' areas must be
the same bits; on right-angled cells it is the orthorhombic entry.  The yardstick of the trajectory drivers is the batch entry,
frame by frame with the cell fa.cell_from_dcd makes of each frame's record, byte for byte between result files.  Small seeded
systems; frames_per_batch = 2 over 5 frames gives shards of 2, 2 and 1 frames."""
import math
import os
import struct

import numpy as np
import pytest

import freesasa_amd as fa
import tools
import pbc_ref
import pbc_tri_ref as tri
from test_dcd import write_dcd
from test_dcd_gpu import jittered, solvated  # noqa: F401  (solvated: a fixture)

pytestmark = pytest.mark.gpu

PROBE = 1.4
N, F, FPB = 37, 5, 2
ALGS = {"lr20": (fa.LEE_RICHARDS, 20), "sr100": (fa.SHRAKE_RUPLEY, 100)}


@pytest.fixture(scope="module")
def batch():
    return tri.batch()


@pytest.fixture(scope="module")
def expanded(batch):
    return tri.expand_batch(*batch, probe=PROBE)


# ---------------------------------------------------------------- 1. against the engine on the explicit expansion

@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_calc_periodic_triclinic_equals_the_engine_on_the_explicit_expansion(batch, expanded, alg):
    import torch
    xyz, radii, offsets, cells6 = batch
    ex, er, eoff, want_images = expanded
    a, res = ALGS[alg]
    sasa, totals, images = fa.calc_periodic_triclinic(xyz, radii, offsets, cells6, alg=a, probe=PROBE, resolution=res)
    want, _, _ = fa.calc_batch(ex, er, eoff, a, probe=PROBE, resolution=res)
    assert np.array_equal(images, want_images)
    for s in range(len(offsets) - 1):
        n = int(offsets[s + 1] - offsets[s])
        got = sasa[offsets[s]:offsets[s + 1]]
        assert got.tobytes() == want[eoff[s]:eoff[s] + n].tobytes(), s
        # totals over the real atoms only: n * 2^-53 for n <= 1e4, with a decade of room
        exact = math.fsum(got)
        print(f"{alg} structure {s}: n {n} images {images[s]} total {totals[s]!r} fsum {exact!r}")
        assert abs(totals[s] - exact) <= 1e-11 * abs(exact), s
    assert totals[0] == 0.0 and np.all(totals[1:] > 0)
    # the device entry: the same arrays
    dev = torch.device("cuda:0")
    d_xyz, d_r = torch.from_numpy(xyz).to(dev), torch.from_numpy(radii).to(dev)
    d_out = torch.empty(len(radii), dtype=torch.float64, device=dev)
    d_tot = torch.empty(5, dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0)
    try:
        k = ctx.periodic_triclinic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, cells6, d_out.data_ptr(), d_tot.data_ptr(), alg=a, probe=PROBE,
                                   resolution=res)
        assert np.array_equal(k, images) and d_out.cpu().numpy().tobytes() == sasa.tobytes() and d_tot.cpu().numpy().tobytes() == totals.tobytes()
    finally:
        ctx.close()


def test_the_device_entry_checks_the_widths_against_the_device_s_max_radius(batch):
    import torch
    xyz, radii, offsets, cells6 = batch
    c = tri.cutoff(radii[offsets[3]:offsets[4]], PROBE)
    bad = cells6.copy()
    bad[3] *= (c - 0.01) / tri.widths(cells6[3])[0]
    dev = torch.device("cuda:0")
    d_xyz, d_r = torch.from_numpy(xyz).to(dev), torch.from_numpy(radii).to(dev)
    d_out = torch.empty(len(radii), dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0)
    try:
        with pytest.raises(RuntimeError, match=r"structure 3: width a of its cell is .* smaller than c"):
            ctx.periodic_triclinic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, bad, d_out.data_ptr(), probe=PROBE)
        bad[3] = cells6[3]
        bad[3][5] = -15.0
        with pytest.raises(RuntimeError, match=r"structure 3: entry cz of its cell is -15"):
            ctx.periodic_triclinic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, bad, d_out.data_ptr(), probe=PROBE)
        with pytest.raises(ValueError, match="six numbers per structure"):
            ctx.periodic_triclinic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, cells6[:, :3], d_out.data_ptr(), probe=PROBE)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. against the orthorhombic entry

@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_right_angled_cells_equal_the_orthorhombic_entry(alg):
    xyz, radii, offsets, cells = pbc_ref.batch()
    cells6 = np.zeros((5, 6))
    cells6[:, 0], cells6[:, 2], cells6[:, 5] = cells[:, 0], cells[:, 1], cells[:, 2]
    a, res = ALGS[alg]
    want = fa.calc_periodic(xyz, radii, offsets, cells, alg=a, probe=PROBE, resolution=res)
    got = fa.calc_periodic_triclinic(xyz, radii, offsets, cells6, alg=a, probe=PROBE, resolution=res)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2])
    assert want[2][1] == 26 and np.all(want[2][1:] > 0)


# ---------------------------------------------------------------- 3. analytic

def test_one_atom_in_a_small_hexagonal_cell_is_a_free_sphere(batch):
    """radius 2.0 in the hexagonal cell with widths 6.84, 6.84, 7.0: its 26 images lie at >= 6.84 >= c = 6.8 and the neighbour
    predicate is strict"""
    xyz, radii, offsets, cells6 = batch
    x, r, h = xyz[0:1], radii[0:1], cells6[1:2]
    sasa, totals, images = fa.calc_periodic_triclinic(x, r, [0, 1], h, alg=fa.LEE_RICHARDS, probe=PROBE, resolution=20)
    want = 4.0 * math.pi * 3.4 ** 2
    assert images[0] == 26
    assert abs(sasa[0] - want) <= 1e-4 * want and totals[0] == sasa[0]
    sr, _, _ = fa.calc_periodic_triclinic(x, r, [0, 1], h, alg=fa.SHRAKE_RUPLEY, probe=PROBE, resolution=100)
    free, _, _ = fa.calc_batch(x, r, [0, 1], fa.SHRAKE_RUPLEY, probe=PROBE, resolution=100)
    assert sr[0] == free[0]


def test_two_atoms_across_the_b_face_are_two_spheres():
    """fractional (0.5, 0.03, 0.5) and (0.5, 0.97, 0.5) of the hexagonal cell, |b| = 14: each sees the other's image 0.84 A away
    through the b face, which is not perpendicular to an axis.  Fails on any implementation that wraps or shifts along y alone."""
    h = tri.HEXAGONAL
    H = tri.matrix(h)
    xyz = np.array([[0.5, 0.03, 0.5], [0.5, 0.97, 0.5]]) @ H
    r = np.array([1.5, 1.8])
    pair = np.vstack([xyz[0], xyz[1] - H[1]])
    assert abs(np.linalg.norm(pair[0] - pair[1]) - 0.84) < 1e-12
    for alg, (a, res) in ALGS.items():
        sasa, totals, images = fa.calc_periodic_triclinic(xyz, r, [0, 2], [h], alg=a, probe=PROBE, resolution=res)
        want, _, _ = fa.calc_batch(pair, r, [0, 2], a, probe=PROBE, resolution=res)
        alone, _, _ = fa.calc_batch(xyz, r, [0, 2], a, probe=PROBE, resolution=res)
        print(f"{alg}: periodic {sasa!r} two spheres {want!r} non-periodic {alone!r}")
        assert np.max(np.abs(sasa - want)) <= 1e-8
        assert np.min(np.abs(sasa - alone)) > 1.0, "the face was not crossed"
        assert images[0] > 0


# ---------------------------------------------------------------- 4. invariance

def test_invariance_under_lattice_vectors_translations_and_a_change_of_basis():
    """The 60 atoms (seed 20261018 + 3) in the hexagonal cell, and the same system three more ways: moved by the lattice vector
    2a - b + c; moved by (5.3, -17.1, 40.2); described in the basis a, b' = b + a, c' = c - a (widths 9.66, 12.12, 16: still >= c).
    L&R-20: per-atom areas within 1e-8 A^2.  S&R-100: at most 1 of the 60 atoms may differ at all - a condition, not a
    measurement: another wrap changes last bits of coordinates, which can flip a test point that lies on a neighbour's sphere;
    the oracle on the CPU gives 0 of 60 for seeds +3 .. +7, so the cap holds with room."""
    h = np.array(tri.HEXAGONAL)
    a, b, c = tri.matrix(h)
    x, r = tri.sixty(h)
    h2 = np.array([h[0], h[1] + h[0], h[2], h[3] - h[0], h[4], h[5]])
    assert np.all(tri.widths(h2) >= tri.cutoff(r, PROBE)) and np.allclose(tri.widths(h2), [9.66, 12.12, 16.0], atol=0.01)
    ways = np.vstack([x, x + (2 * a - b + c), x + np.array([5.3, -17.1, 40.2]), x])
    cells6, offsets = [h, h, h, h2], [0, 60, 120, 180, 240]
    lr, _, images = fa.calc_periodic_triclinic(ways, np.tile(r, 4), offsets, cells6, alg=fa.LEE_RICHARDS, probe=PROBE, resolution=20)
    sr, _, _ = fa.calc_periodic_triclinic(ways, np.tile(r, 4), offsets, cells6, alg=fa.SHRAKE_RUPLEY, probe=PROBE, resolution=100)
    assert images[0] > 4 * 60
    for k, way in enumerate(("lattice vector", "translation", "basis"), 1):
        d = np.max(np.abs(lr[:60] - lr[60 * k:60 * k + 60]))
        differ = int(np.sum(sr[:60] != sr[60 * k:60 * k + 60]))
        print(f"{way}: images {images[k]}, L&R-20 max |difference| = {d:.3e} A^2, S&R-100 atoms that differ: {differ} of 60")
        assert d <= 1e-8, way
        assert differ <= 1, way


# ---------------------------------------------------------------- 5. the DCD drivers

def frame_records(degrees):
    """CHARMM's A, gamma, B, beta, alpha, C per frame: cells that change from frame to frame, every angle at work.  The coil's
    extent is (10.9, 9.5, 9.1) and c = 2 (1.88 + 1.4) = 6.56; the smallest width of these cells is above 11."""
    ang = lambda v: float(v) if degrees else float(np.cos(np.float64(v) * np.pi / 180.0))
    return [(14.0 + 0.3 * f, ang(75.0 + f), 13.0, ang(100.0 - f), ang(95.0), 12.5 - 0.2 * f) for f in range(F)]


def patch_records(path, records):
    """the cell records of the DCD file at `path` (tests/test_dcd.py's writer puts 50 + f into all six fields)"""
    info = fa.dcd_info(path)
    assert info.has_cell
    data = bytearray(open(path, "rb").read())
    for f, rec in enumerate(records):
        struct.pack_into((">" if info.big_endian else "<") + "6d", data, info.first_frame + f * info.frame_bytes + 4, *rec)
    open(path, "wb").write(bytes(data))
    return info


def run(tmp, tag, path, radii, alg="lr20", **kw):
    a, res = ALGS[alg]
    p = {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "done")}
    done, n_frames = fa.trajectory_file(path, radii, p["totals"], p["sasa"], done_path=p["done"], alg=a, probe=PROBE, resolution=res,
                                        frames_per_batch=FPB, dcd=True, **kw)
    return {k: open(p[k], "rb").read() for k in ("totals", "sasa")}, p, done, n_frames


@pytest.fixture(scope="module")
def coil():
    """tests/test_dcd_gpu.py's coil: x in [-10.4, 0.5], y in [-2.5, 7.0], z in [-8.6, 0.6] - astride the faces at 0 of every axis"""
    xyz, radii = tools.coil(N, 20261018)
    return jittered(xyz, F, 1), radii


_WANT = {}


def periodic_frames(coil, alg, degrees):
    """calc_periodic_triclinic frame by frame - the frames' fp32 values widened, each frame's cell out of its record by
    fa.cell_from_dcd - once per algorithm and form of the angles"""
    if (alg, degrees) not in _WANT:
        frames, radii = coil
        a, res = ALGS[alg]
        sasa, totals, images = [], [], []
        for f, rec in enumerate(frame_records(degrees)):
            h = fa.cell_from_dcd(rec)
            assert np.all(tri.widths(h) > 11.0) and all(h[k] != 0.0 for k in (1, 3, 4))
            s, t, k = fa.calc_periodic_triclinic(frames[f].astype(np.float64), radii, [0, N], [h], alg=a, probe=PROBE, resolution=res)
            sasa.append(s); totals.append(t[0]); images.append(int(k[0]))
        assert min(images) > 0, "the coil does not reach the faces"
        _WANT[(alg, degrees)] = (np.array(sasa), np.array(totals))
    return _WANT[(alg, degrees)]


@pytest.mark.parametrize("kind, alg, out_f32, degrees", [("little", "lr20", False, True), ("big", "lr20", False, False),
                                                          ("little-4d", "sr100", False, False), ("big-4d", "lr20", True, True)])
def test_triclinic_dcd_run_equals_calc_periodic_triclinic_frame_by_frame(coil, tmp_path, kind, alg, out_f32, degrees):
    frames, radii = coil
    sasa, totals = periodic_frames(coil, alg, degrees)
    dcd = tmp_path / "frames.dcd"
    write_dcd(dcd, frames, endian=">" if kind.startswith("big") else "<", cell=True, dim4=kind.endswith("4d"), nset_header=0)
    patch_records(dcd, frame_records(degrees))
    got, p, done, n_frames = run(tmp_path, kind, dcd, radii, alg, pbc=True, triclinic=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == totals.tobytes()
    assert got["sasa"] == (sasa.astype(np.float32) if out_f32 else sasa).tobytes()
    assert f" f32={4 + 8 + 16 + (2 if out_f32 else 0)} " in open(p["done"]).readline()
    # without bit 4 the run is refused at its first frame, as ever
    q = {k: str(tmp_path / f"ortho.{k}") for k in ("totals", "sasa", "done")}
    with pytest.raises(RuntimeError, match="frame [0-4] of the DCD file: its cell is not orthorhombic"):
        fa.trajectory_file(dcd, radii, q["totals"], q["sasa"], done_path=q["done"], frames_per_batch=FPB, dcd=True, pbc=True, probe=PROBE)
    if kind != "little":
        return
    # it is not the non-periodic run's answer
    plain, _, _, _ = run(tmp_path, kind + "-plain", dcd, radii, alg, out_f32=out_f32)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"]))
    # stopped after one shard and resumed: the files of the uninterrupted run
    a, res = ALGS[alg]
    q = {k: str(tmp_path / f"part.{k}") for k in ("totals", "sasa", "done")}
    kw = dict(done_path=q["done"], alg=a, probe=PROBE, resolution=res, frames_per_batch=FPB, dcd=True, pbc=True, triclinic=True)
    done, _ = fa.trajectory_file(dcd, radii, q["totals"], q["sasa"], max_new_shards=1, **kw)
    assert not done and open(q["done"]).read().count("shard ") == 1
    done, _ = fa.trajectory_file(dcd, radii, q["totals"], q["sasa"], **kw)
    assert done and open(q["done"]).read().count("shard ") == 3
    assert open(q["totals"], "rb").read() == got["totals"] and open(q["sasa"], "rb").read() == got["sasa"]


def test_triclinic_dcd_run_with_a_topology(solvated, tmp_path):
    """2jo4 scattered among 41 solvent atoms (a shuffled index), two frames in skewed cells around the solute's extent: totals and
    per-atom areas are calc_periodic_triclinic's on the gathered frames, byte for byte"""
    b, full, index = solvated
    n, nf = int(b.n_atoms), 2
    full = full[:nf]
    solute = full[:, index].astype(np.float64)
    ext = solute.reshape(-1, 3).max(0) - solute.reshape(-1, 3).min(0) + 6.0
    records = [(float(ext[0]) + 0.25 * f, 80.0 + f, float(ext[1]), 97.0, 85.0 - f, float(ext[2])) for f in range(nf)]
    cells6 = np.array([fa.cell_from_dcd(rec) for rec in records])
    dcd = tmp_path / "solvated.dcd"
    write_dcd(dcd, full, cell=True)
    patch_records(dcd, records)
    p = {k: str(tmp_path / f"tri.{k}") for k in ("totals", "sasa", "done")}
    done, n_frames, _ = fa.trajectory_file_topology(dcd, b, p["totals"], atom_index=index, sasa_path=p["sasa"], done_path=p["done"],
                                                    frames_per_batch=FPB, devices=[0, 0], dcd=True, pbc=True, triclinic=True, probe=PROBE)
    assert done and n_frames == nf
    radii = np.tile(np.asarray(b.radii, dtype=np.float64), nf)
    sasa, totals, images = fa.calc_periodic_triclinic(solute.reshape(-1, 3), radii, [0, n, 2 * n], cells6, probe=PROBE)
    assert np.all(images > 0)
    assert open(p["sasa"], "rb").read() == sasa.tobytes() and open(p["totals"], "rb").read() == totals.tobytes()
    assert " f32=28 " in open(p["done"]).readline()


def test_a_right_angled_file_gives_the_files_of_the_orthorhombic_run(coil, tmp_path):
    frames, radii = coil
    dcd = tmp_path / "right.dcd"
    write_dcd(dcd, frames, cell=True)
    patch_records(dcd, [(14.0 + 0.3 * f, 90.0, 13.0, 0.0, 90.0, 12.5 - 0.2 * f) for f in range(F)])
    old, p0, done0, _ = run(tmp_path, "pbc", dcd, radii, pbc=True)
    new, p1, done1, _ = run(tmp_path, "tri", dcd, radii, pbc=True, triclinic=True)
    assert done0 and done1
    assert new["totals"] == old["totals"] and new["sasa"] == old["sasa"]
    plain, _, _, _ = run(tmp_path, "plain", dcd, radii)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(old["totals"]))
    assert " f32=12 " in open(p0["done"]).readline() and " f32=28 " in open(p1["done"]).readline()
    # each run refuses the other's done-list
    a, res = ALGS["lr20"]
    kw = dict(alg=a, probe=PROBE, resolution=res, frames_per_batch=FPB, dcd=True, pbc=True)
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
        fa.trajectory_file(dcd, radii, p0["totals"], p0["sasa"], done_path=p0["done"], triclinic=True, **kw)
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
        fa.trajectory_file(dcd, radii, p1["totals"], p1["sasa"], done_path=p1["done"], **kw)
    assert open(p0["totals"], "rb").read() == old["totals"] and open(p1["sasa"], "rb").read() == new["sasa"]


@pytest.mark.parametrize("what, text", [("width", r"width b of its cell is .* smaller than c"), ("angles", "span no cell")])
def test_a_frame_with_a_bad_cell_ends_the_run_and_is_not_listed(coil, tmp_path, what, text):
    """frame 3 (of shard 1: frames 2 and 3) has a width of c - 0.01, or angles that span no cell: a host check on the staged bytes,
    nothing of the shard reaches the device.  With one lane the shards go in order: shard 0 is listed, shard 1 is not, shard 2 is
    never begun."""
    frames, radii = coil
    c = tri.cutoff(radii, PROBE)
    records = frame_records(True)
    if what == "width":
        # gamma = 60 degrees as a cosine: by = B sqrt(0.75) is the width b (beta = alpha = 90 degrees); every edge is above c
        A, B, C = records[3][0], (c - 0.01) / math.sqrt(0.75), records[3][5]
        records[3] = (A, 0.5, B, 0.0, 0.0, C)
        assert tri.widths(fa.cell_from_dcd(records[3]))[1] < c < B
    else:
        records[3] = (records[3][0], 20.0, records[3][2], 30.0, 160.0, records[3][5])
    dcd = tmp_path / "bad.dcd"
    write_dcd(dcd, frames, cell=True)
    patch_records(dcd, records)
    os.environ["FREESASA_AMD_TRAJ_LANES"] = "1"
    try:
        p = {k: str(tmp_path / f"bad.{k}") for k in ("totals", "sasa", "done")}
        with pytest.raises(RuntimeError, match=r"frame 3 of the DCD file: .*" + text):
            fa.trajectory_file(dcd, radii, p["totals"], p["sasa"], done_path=p["done"], frames_per_batch=FPB, dcd=True, pbc=True,
                               triclinic=True, probe=PROBE, device=0)
    finally:
        os.environ.pop("FREESASA_AMD_TRAJ_LANES", None)
    assert [int(line.split()[1]) for line in open(p["done"]).read().splitlines()[1:]] == [0]
