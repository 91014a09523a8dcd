"""Periodic images on the device (include/freesasa_gpu.h: freesasa_gpu_calc_periodic, FREESASA_GPU_FRAMES_PBC).  The yardstick
of the batch entry is the engine itself on the explicit expansion tests/pbc_ref.py makes (checked against the 27-replica system
in tests/test_pbc.py): the real atoms' areas must be the same bits.  The yardstick of the trajectory drivers is the batch entry,
frame by frame with each frame's own cell, byte for byte between result files.  Small seeded systems; frames_per_batch = 2 over
5 frames gives shards of 2, 2 and 1 frames."""
import math
import os
import struct

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import tools
from freesasa_amd import ingest
import pbc_ref
from test_dcd import write_dcd
from test_dcd_gpu import COMMANDS, jittered, solvated  # noqa: F401  (solvated: a fixture)

pytestmark = pytest.mark.gpu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
PROBE = 1.4
N, F, FPB = 37, 5, 2
ALGS = {"lr20": (fa.LEE_RICHARDS, 20), "sr100": (fa.SHRAKE_RUPLEY, 100)}


@pytest.fixture(scope="module")
def batch():
    return pbc_ref.batch()


@pytest.fixture(scope="module")
def expanded(batch):
    return pbc_ref.expand_batch(*batch, probe=PROBE)


# ---------------------------------------------------------------- 1. against the engine on the explicit expansion

@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_calc_periodic_equals_the_engine_on_the_explicit_expansion(batch, expanded, alg):
    xyz, radii, offsets, cells = batch
    ex, er, eoff, want_images = expanded
    a, res = ALGS[alg]
    sasa, totals, images = fa.calc_periodic(xyz, radii, offsets, cells, alg=a, probe=PROBE, resolution=res)
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


# ---------------------------------------------------------------- 2. analytic

def test_one_atom_in_a_small_cube_is_a_free_sphere():
    """radius 2.0 in a 7 A cube: its 26 images lie at >= 7 >= c = 6.8 and the neighbour predicate is strict"""
    xyz, r, cell = np.array([[1.0, 2.0, 3.0]]), np.array([2.0]), [(7.0, 7.0, 7.0)]
    sasa, totals, images = fa.calc_periodic(xyz, r, [0, 1], cell, alg=fa.LEE_RICHARDS, probe=PROBE, resolution=20)
    want = 4.0 * math.pi * 3.4 ** 2
    assert images[0] == 26
    assert abs(sasa[0] - want) <= 1e-4 * want and totals[0] == sasa[0]
    sr, _, _ = fa.calc_periodic(xyz, r, [0, 1], cell, alg=fa.SHRAKE_RUPLEY, probe=PROBE, resolution=100)
    free, _, _ = fa.calc_batch(xyz, r, [0, 1], fa.SHRAKE_RUPLEY, probe=PROBE, resolution=100)
    assert sr[0] == free[0]


def test_two_atoms_across_a_face_are_two_spheres_one_angstrom_apart():
    """x = 0.5 and x = Lx - 0.5 in (8, 9, 10): each sees the other's image 1.0 A away through the face and nothing else (the atom
    itself is 7 A away, further than the 6.1 A at which these two can touch).  Fails on any implementation that forgets the wrap
    or a face."""
    cell = (8.0, 9.0, 10.0)
    xyz = np.array([[0.5, 4.5, 5.0], [cell[0] - 0.5, 4.5, 5.0]])
    r = np.array([1.5, 1.8])
    pair = np.array([[4.0, 4.5, 5.0], [3.0, 4.5, 5.0]])          # atom 1 on the -x side of atom 0, 1.0 A away
    for alg, (a, res) in ALGS.items():
        sasa, totals, images = fa.calc_periodic(xyz, r, [0, 2], [cell], alg=a, probe=PROBE, resolution=res)
        want, _, _ = fa.calc_batch(pair, r, [0, 2], a, probe=PROBE, resolution=res)
        alone, _, _ = fa.calc_batch(xyz, r, [0, 2], a, probe=PROBE, resolution=res)
        print(f"{alg}: periodic {sasa!r} two spheres {want!r}")
        assert np.max(np.abs(sasa - want)) <= 1e-8
        assert np.min(np.abs(sasa - alone)) > 1.0, "the face was not crossed"
        assert images[0] > 0


# ---------------------------------------------------------------- 3. translation invariance

def test_translation_invariance(batch):
    """The 60 atoms in (12, 14, 16) moved by (+5.3, -17.1, +40.2).  L&R-20: per-atom areas within 1e-8 A^2.  S&R-100: at most 1
    of the 60 atoms may differ at all - a condition, not a measurement: the shifted wrap changes last bits of coordinates, which
    can flip a test point that lies on a neighbour's sphere.  The structure is the batch's (tests/pbc_ref.py, seed 20261018 + 3):
    chosen because the oracle, run on the CPU over the two expansions, gives 0 differing atoms of 60 for S&R-100 (and
    1.5e-13 A^2 for L&R-20), so the cap of 1 holds with room; seeds 1 .. 7 of the same generator give 0 as well."""
    xyz, radii, offsets, cells = batch
    x, r, cell = xyz[offsets[3]:offsets[4]], radii[offsets[3]:offsets[4]], cells[3]
    moved = x + np.array([5.3, -17.1, 40.2])
    both = np.vstack([x, moved])
    lr, _, images = fa.calc_periodic(both, np.tile(r, 2), [0, 60, 120], [cell, cell], alg=fa.LEE_RICHARDS, probe=PROBE, resolution=20)
    print(f"L&R-20 max |moved - unmoved| = {np.max(np.abs(lr[:60] - lr[60:])):.3e} A^2, images {images}")
    assert np.max(np.abs(lr[:60] - lr[60:])) <= 1e-8
    sr, _, _ = fa.calc_periodic(both, np.tile(r, 2), [0, 60, 120], [cell, cell], alg=fa.SHRAKE_RUPLEY, probe=PROBE, resolution=100)
    print(f"S&R-100 atoms that differ: {int(np.sum(sr[:60] != sr[60:]))} of 60")
    assert int(np.sum(sr[:60] != sr[60:])) <= 1


# ---------------------------------------------------------------- the DCD drivers

def patch_cells(path, cells, degrees=True):
    """the cell records of the DCD file at `path` (tests/test_dcd.py's writer puts 50 + f into all six fields): CHARMM's A,
    gamma, B, beta, alpha, C with the edges of cells[f] and right angles - as degrees, or as cosines"""
    info = fa.dcd_info(path)
    assert info.has_cell
    data = bytearray(open(path, "rb").read())
    ang = 90.0 if degrees else 0.0
    for f, (lx, ly, lz) in enumerate(cells):
        struct.pack_into((">" if info.big_endian else "<") + "6d", data, info.first_frame + f * info.frame_bytes + 4, lx, ang, ly, ang, ang, lz)
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


def test_a_cell_that_touches_nothing_changes_nothing(coil, tmp_path):
    frames, radii = coil
    far = (frames + (500.0 - frames.reshape(-1, 3).mean(0))).astype(np.float32)
    assert far.min() >= 100.0 and far.max() <= 900.0
    dcd = tmp_path / "far.dcd"
    write_dcd(dcd, far, cell=True)
    patch_cells(dcd, [(1000.0, 1000.0, 1000.0)] * F)
    plain, p0, done0, _ = run(tmp_path, "plain", dcd, radii)
    pbc, p1, done1, _ = run(tmp_path, "pbc", dcd, radii, pbc=True)
    assert done0 and done1
    assert pbc["totals"] == plain["totals"] and pbc["sasa"] == plain["sasa"]
    assert len(plain["totals"]) == 8 * F and np.all(np.frombuffer(plain["totals"]) > 0)
    assert " f32=12 " in open(p1["done"]).readline() and " f32=4 " in open(p0["done"]).readline()
    # each run refuses the other's done-list
    a, res = ALGS["lr20"]
    kw = dict(alg=a, probe=PROBE, resolution=res, frames_per_batch=FPB, dcd=True)
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
        fa.trajectory_file(dcd, radii, p0["totals"], p0["sasa"], done_path=p0["done"], pbc=True, **kw)
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
        fa.trajectory_file(dcd, radii, p1["totals"], p1["sasa"], done_path=p1["done"], **kw)
    assert open(p0["totals"], "rb").read() == plain["totals"] and open(p1["sasa"], "rb").read() == pbc["sasa"]


CELL0 = (14.0, 13.0, 12.5)         # the coil's extent is (10.9, 9.5, 9.1); c = 2 (1.88 + 1.4) = 6.56
_WANT = {}


def frame_cells():
    return [(CELL0[0] + 0.3 * f, CELL0[1], CELL0[2] - 0.2 * f) for f in range(F)]


def periodic_frames(coil, alg):
    """calc_periodic frame by frame - the frames' fp32 values widened, each frame's own cell - once per algorithm"""
    if alg not in _WANT:
        frames, radii = coil
        a, res = ALGS[alg]
        sasa, totals, images = [], [], []
        for f, cell in enumerate(frame_cells()):
            s, t, k = fa.calc_periodic(frames[f].astype(np.float64), radii, [0, N], [cell], alg=a, probe=PROBE, resolution=res)
            sasa.append(s); totals.append(t[0]); images.append(int(k[0]))
        assert min(images) > 0, "the coil does not reach the faces"
        _WANT[alg] = (np.array(sasa), np.array(totals))
    return _WANT[alg]


@pytest.mark.parametrize("kind, alg, out_f32", [("little", "lr20", False), ("big", "lr20", False), ("little-4d", "sr100", False),
                                                 ("big-4d", "lr20", True)])
def test_periodic_dcd_run_equals_calc_periodic_frame_by_frame(coil, tmp_path, kind, alg, out_f32):
    frames, radii = coil
    sasa, totals = periodic_frames(coil, alg)
    dcd = tmp_path / "frames.dcd"
    write_dcd(dcd, frames, endian=">" if kind.startswith("big") else "<", cell=True, dim4=kind.endswith("4d"), nset_header=0)
    patch_cells(dcd, frame_cells(), degrees=not kind.endswith("4d"))
    got, p, done, n_frames = run(tmp_path, kind, dcd, radii, alg, pbc=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == totals.tobytes()
    assert got["sasa"] == (sasa.astype(np.float32) if out_f32 else sasa).tobytes()
    # it is not the non-periodic run's answer
    plain, _, _, _ = run(tmp_path, kind + "-plain", dcd, radii, alg, out_f32=out_f32)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"]))
    if kind != "little":
        return
    # stopped after one shard and resumed: the files of the uninterrupted run
    a, res = ALGS[alg]
    q = {k: str(tmp_path / f"part.{k}") for k in ("totals", "sasa", "done")}
    kw = dict(done_path=q["done"], alg=a, probe=PROBE, resolution=res, frames_per_batch=FPB, dcd=True, pbc=True)
    done, _ = fa.trajectory_file(dcd, radii, q["totals"], q["sasa"], max_new_shards=1, **kw)
    assert not done and open(q["done"]).read().count("shard ") == 1
    done, _ = fa.trajectory_file(dcd, radii, q["totals"], q["sasa"], **kw)
    assert done and open(q["done"]).read().count("shard ") == 3
    assert open(q["totals"], "rb").read() == got["totals"] and open(q["sasa"], "rb").read() == got["sasa"]


def test_periodic_dcd_run_with_a_topology(solvated, tmp_path):
    """2jo4 scattered among 41 solvent atoms; the cell is the solute's extent plus 4 A per axis, two frames.  Every output file
    is, byte for byte, what the memory-form sums give on calc_periodic's per-atom areas of the gathered frames."""
    import torch
    b, full, index = solvated
    n, R, nf = int(b.n_atoms), int(b.n_residues), 2
    full = full[:nf]
    solute = full[:, index].astype(np.float64)
    cell = tuple(float(v) for v in solute.reshape(-1, 3).max(0) - solute.reshape(-1, 3).min(0) + 4.0)
    cells = [cell, (cell[0] + 0.25, cell[1], cell[2])]
    dcd = tmp_path / "solvated.dcd"
    write_dcd(dcd, full, cell=True)
    patch_cells(dcd, cells)
    sel = ingest.Selection(COMMANDS)
    try:
        p = {k: str(tmp_path / f"pbc.{k}") for k in ("totals", "sasa", "cls", "res", "sel", "done")}
        done, n_frames, atoms = fa.trajectory_file_topology(dcd, b, p["totals"], atom_index=index, selection=sel, sasa_path=p["sasa"],
                                                            class_sums_path=p["cls"], residues_path=p["res"], selections_path=p["sel"],
                                                            done_path=p["done"], frames_per_batch=FPB, devices=[0, 0], dcd=True, pbc=True,
                                                            probe=PROBE)
        assert done and n_frames == nf
        b2 = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")] * nf)
        sasa, totals, images = fa.calc_periodic(solute.reshape(-1, 3), b2.radii, b2.offsets, cells, probe=PROBE)
        assert np.all(images > 0)
        dev = torch.device("cuda:0")
        d_sasa = torch.from_numpy(sasa).to(dev)
        d_cls, d_bb = torch.from_numpy(b2.atom_class).to(dev), torch.from_numpy(b2.atom_backbone).to(dev)
        d_cs = torch.empty(3 * nf, dtype=torch.float64, device=dev)
        d_abs = torch.empty(6 * R * nf, dtype=torch.float64, device=dev)
        ctx = fa.GpuContext(0)
        ctx.class_sums(d_sasa.data_ptr(), d_cls.data_ptr(), b2.offsets, d_cs.data_ptr())
        ctx.residue_areas(d_sasa.data_ptr(), d_cls.data_ptr(), d_bb.data_ptr(), b2.res_first, d_abs.data_ptr())
        ctx.close()
        areas, counts = fa.select_batch(b2, sel, sasa)
    finally:
        sel.close()
    read = lambda k: open(p[k], "rb").read()
    assert read("sasa") == sasa.tobytes() and read("totals") == totals.tobytes()
    assert read("cls") == d_cs.cpu().numpy().tobytes() and read("res") == d_abs.cpu().numpy().tobytes()
    assert read("sel") == np.ascontiguousarray(areas).tobytes() and np.array_equal(atoms, counts[0])
    assert " f32=12 " in open(p["done"]).readline()
    # the per-residue sums are sums of those per-atom areas
    assert np.allclose(np.frombuffer(read("res")).reshape(nf * R, 6)[:, 0], b2.residue_sums(sasa), rtol=1e-13, atol=1e-12)


# ---------------------------------------------------------------- 7. refusals on the device path

def test_a_frame_with_a_short_edge_ends_the_run_and_is_not_listed(coil, tmp_path):
    """frame 3 (of shard 1: frames 2 and 3) has an edge of c - 0.01: a host check on the staged bytes, nothing of the shard
    reaches the device.  With one lane the shards go in order: shard 0 is listed, shard 1 is not, shard 2 is never begun."""
    frames, radii = coil
    c = pbc_ref.cutoff(radii, PROBE)
    cells = frame_cells()
    cells[3] = (cells[3][0], c - 0.01, cells[3][2])
    dcd = tmp_path / "short.dcd"
    write_dcd(dcd, frames, cell=True)
    patch_cells(dcd, cells)
    listed = {}
    for tag, lanes in (("lanes", None), ("one", "1")):
        if lanes:
            os.environ["FREESASA_AMD_TRAJ_LANES"] = lanes
        try:
            p = {k: str(tmp_path / f"{tag}.{k}") for k in ("totals", "sasa", "done")}
            with pytest.raises(RuntimeError, match=r"frame 3 of the DCD file: edge y .* shorter than c"):
                fa.trajectory_file(dcd, radii, p["totals"], p["sasa"], done_path=p["done"], frames_per_batch=FPB, dcd=True, pbc=True,
                                   probe=PROBE, device=0)
        finally:
            os.environ.pop("FREESASA_AMD_TRAJ_LANES", None)
        listed[tag] = [int(line.split()[1]) for line in open(p["done"]).read().splitlines()[1:]]
    assert 1 not in listed["lanes"] and listed["one"] == [0]


@pytest.mark.parametrize("what, text", [("angle", "not orthorhombic"), ("edge", "not finite")])
def test_a_frame_with_an_odd_cell_ends_the_run(coil, tmp_path, what, text):
    """an angle of 60 degrees, a non-finite edge: host checks on the staged bytes, behind an open device"""
    frames, radii = coil
    dcd = tmp_path / "odd.dcd"
    write_dcd(dcd, frames, cell=True)
    info = patch_cells(dcd, frame_cells())
    data = bytearray(open(dcd, "rb").read())
    at = info.first_frame + 1 * info.frame_bytes + 4
    struct.pack_into("<d", data, at + (8 * 3 if what == "angle" else 8 * 5), 60.0 if what == "angle" else float("inf"))
    open(dcd, "wb").write(bytes(data))
    p = {k: str(tmp_path / f"odd.{k}") for k in ("totals", "sasa", "done")}
    with pytest.raises(RuntimeError, match="frame 1 of the DCD file: .*" + text):
        fa.trajectory_file(dcd, radii, p["totals"], p["sasa"], done_path=p["done"], frames_per_batch=FPB, dcd=True, pbc=True, probe=PROBE,
                           device=0)
    assert "shard 0 " not in open(p["done"]).read()


def test_calc_periodic_refuses_a_short_edge_and_an_oversized_batch(batch):
    xyz, radii, offsets, cells = batch
    bad = cells.copy()
    bad[2][0] = pbc_ref.cutoff(radii[offsets[2]:offsets[3]], PROBE) - 0.01
    with pytest.raises(RuntimeError, match=r"structure 2: edge x .* shorter than c"):
        fa.calc_periodic(xyz, radii, offsets, bad, probe=PROBE)
    # the device entry makes the check with the device's own max radius, behind the count and in front of the engine
    import torch
    dev = torch.device("cuda:0")
    d_xyz, d_r = torch.from_numpy(xyz).to(dev), torch.from_numpy(radii).to(dev)
    d_out = torch.empty(len(radii), dtype=torch.float64, device=dev)
    d_tot = torch.empty(5, dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0)
    try:
        with pytest.raises(RuntimeError, match=r"structure 2: edge x .* shorter than c"):
            ctx.periodic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, bad, d_out.data_ptr(), probe=PROBE)
        images = ctx.periodic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, cells, d_out.data_ptr(), d_tot.data_ptr(), probe=PROBE)
        want, want_totals, want_images = fa.calc_periodic(xyz, radii, offsets, cells, probe=PROBE)
        assert np.array_equal(d_out.cpu().numpy(), want) and np.array_equal(images, want_images)
        assert np.array_equal(d_tot.cpu().numpy(), want_totals)
    finally:
        ctx.close()
    # 2^30: from the offsets alone, before an array is read (these hold one atom)
    with pytest.raises(RuntimeError, match="expanded batch is too large"):
        fa.calc_periodic(np.zeros(3), np.ones(1), [0, (1 << 30) + 1], [(100.0, 100.0, 100.0)], probe=PROBE)
