"""AMBER NetCDF input of the trajectory file drivers (FREESASA_GPU_FRAMES_NETCDF, include/freesasa_gpu.h) on the device.  Every
comparison is byte for byte between result files: one run reads an AMBER NetCDF file written by tests/netcdf_writer.py (or the
committed file scipy wrote), the other a raw fp32 frame file of the same values - a path the existing tests pin to the
per-structure entries - or, for periodic images, a DCD file of the same frames and cells.  Small seeded systems;
frames_per_batch = 2 over 5 frames gives shards of 2, 2 and 1 frames: non-zero frame offsets and a short last shard."""
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from netcdf_writer import write_amber
from test_dcd import write_dcd
from test_dcd_gpu import ALGS, COMMANDS, OUTS, coil, plain_run, raw_plain, solvated, topo_run  # noqa: F401  (coil, raw_plain, solvated: fixtures)
from test_pbc_gpu import frame_cells, patch_cells
from test_pbc_tri_gpu import frame_records, patch_records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "netcdf")
N, F, FPB = 37, 5, 2
PROBE = 1.4
KINDS = {"coordinates": dict(time=False), "time": dict(), "cells+velocities": dict(cells=True, velocities=True)}
STRIDE = {"coordinates": 444, "time": 448, "cells+velocities": 940}


def far_cells(nf=F):
    return np.tile([1000.0, 1000.0, 1000.0, 90.0, 90.0, 90.0], (nf, 1))


def write(path, frames, kind, version=2, **kw):
    k = dict(KINDS[kind], **kw)
    return write_amber(path, frames, far_cells(len(frames)) if k.pop("cells", False) else None, version=version, **k)


@pytest.mark.parametrize("kind, version, alg, out_f32", [("coordinates", 2, "lr20", False), ("coordinates", 1, "lr20", False), ("time", 1, "lr20", False),
                                                          ("cells+velocities", 2, "lr20", False), ("cells+velocities", 1, "sr100", False),
                                                          ("time", 2, "lr20", True)])
def test_plain_driver_equals_the_raw_run(coil, raw_plain, tmp_path, kind, version, alg, out_f32):
    frames, radii = coil
    want = raw_plain(alg, out_f32)
    write(tmp_path / "frames.nc", frames, kind, version, numrecs=-1 if kind == "time" else None)
    info = fa.nc_info(tmp_path / "frames.nc")
    assert info.record_bytes == STRIDE[kind] and info.version == version and info.n_frames == F
    got, done_path, done, n_frames = plain_run(tmp_path, kind, tmp_path / "frames.nc", radii, alg, netcdf=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    head = open(done_path).readline()
    assert f" f32={32 | (2 if out_f32 else 0)} " in head and f" header_bytes={info.first_record} " in head and f" n_frames={F} " in head


def test_the_committed_scipy_written_file_equals_its_raw_run(coil, tmp_path):
    _, radii = coil
    frames = np.load(os.path.join(GOLDEN, "amber_37x5_cell.npz"))["frames"]
    assert frames.shape == (F, N, 3) and frames.dtype == np.float32
    frames.tofile(tmp_path / "frames.f32")
    want, _, done, n_frames = plain_run(tmp_path, "raw", tmp_path / "frames.f32", radii, f32=True)
    assert done and n_frames == F and np.all(np.frombuffer(want["totals"]) > 0)
    got, _, done, n_frames = plain_run(tmp_path, "nc", os.path.join(GOLDEN, "amber_37x5_cell.nc"), radii, netcdf=True)
    assert done and n_frames == F
    assert got == want


@pytest.mark.parametrize("groups", [False, True], ids=["topology", "chain-groups"])
def test_topology_and_chain_groups_equal_the_raw_run(solvated, tmp_path, groups):
    """2jo4 (516 atoms) scattered among 41 solvent atoms, a shuffled index, two lanes of one device, selections, residues, class sums"""
    b, full, index = solvated
    n, R = int(b.n_atoms), int(b.n_residues)
    full.tofile(tmp_path / "frames.f32")
    sel = ingest.Selection(COMMANDS)
    try:
        want, want_atoms = topo_run(tmp_path, "raw", tmp_path / "frames.f32", solvated, sel, groups, frame_atoms=n + 41, f32=True)
        for kind, version in (("cells+velocities", 2), ("coordinates", 1)):
            write(tmp_path / "frames.nc", full, kind, version)
            got, atoms = topo_run(tmp_path, kind, tmp_path / "frames.nc", solvated, sel, groups, netcdf=True)    # (frame_atoms: the file's)
            assert sorted(got) == sorted(want) == sorted(OUTS if groups else OUTS[:5])
            for k in got:
                assert got[k] == want[k], (kind, k)
            assert np.array_equal(atoms, want_atoms) and atoms.min() > 0
    finally:
        sel.close()
    assert len(want["totals"]) == 8 * F and len(want["sasa"]) == 8 * F * n and len(want["res"]) == 8 * 6 * R * F
    if groups:
        assert len(want["grp"]) == 8 * 3 * 4 * F and len(want["iso"]) == 8 * F * n


def run(tmp, tag, path, radii, alg="lr20", **kw):
    a, res = ALGS[alg]
    p = {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "done")}
    done, n_frames = fa.trajectory_file(path, radii, p["totals"], p["sasa"], done_path=p["done"], alg=a, probe=PROBE, resolution=res,
                                        frames_per_batch=FPB, **kw)
    return {k: open(p[k], "rb").read() for k in ("totals", "sasa")}, p, done, n_frames


@pytest.mark.parametrize("alg, out_f32, version", [("lr20", False, 2), ("sr100", True, 1)])
def test_periodic_orthorhombic_run_equals_the_dcd_run(coil, tmp_path, alg, out_f32, version):
    frames, radii = coil
    dcd, nc = tmp_path / "frames.dcd", tmp_path / "frames.nc"
    write_dcd(dcd, frames, cell=True)
    patch_cells(dcd, frame_cells())
    want, _, done, _ = run(tmp_path, "dcd", dcd, radii, alg, dcd=True, pbc=True, out_f32=out_f32)
    assert done
    cells = np.array([list(c) + [90.0, 90.00005, 89.99995] for c in frame_cells()])      # (|v - 90| <= 1e-4: right angles)
    write_amber(nc, frames, cells, version=version, velocities=True)
    got, p, done, n_frames = run(tmp_path, "nc", nc, radii, alg, netcdf=True, pbc=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    assert f" f32={40 | (2 if out_f32 else 0)} " in open(p["done"]).readline()
    # it is not the non-periodic run's answer
    plain, _, _, _ = run(tmp_path, "plain", nc, radii, alg, netcdf=True, out_f32=out_f32)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"]))


def test_a_cell_that_touches_nothing_changes_nothing(coil, tmp_path):
    frames, radii = coil
    far = (frames + (500.0 - frames.reshape(-1, 3).mean(0))).astype(np.float32)
    nc = tmp_path / "far.nc"
    write_amber(nc, far, far_cells())
    plain, p0, done0, _ = run(tmp_path, "plain", nc, radii, netcdf=True)
    pbc, p1, done1, _ = run(tmp_path, "pbc", nc, radii, netcdf=True, pbc=True)
    tri, p2, done2, _ = run(tmp_path, "tri", nc, radii, netcdf=True, pbc=True, triclinic=True)
    assert done0 and done1 and done2
    assert pbc == plain and tri == plain
    assert len(plain["totals"]) == 8 * F and np.all(np.frombuffer(plain["totals"]) > 0)
    assert [open(p["done"]).readline().split(" f32=")[1].split()[0] for p in (p0, p1, p2)] == ["32", "40", "56"]


@pytest.mark.parametrize("alg, out_f32, version", [("lr20", False, 2), ("sr100", True, 1)])
def test_periodic_triclinic_run_equals_the_dcd_run_in_degrees(coil, tmp_path, alg, out_f32, version):
    frames, radii = coil
    dcd, nc = tmp_path / "frames.dcd", tmp_path / "frames.nc"
    records = frame_records(True)                      # CHARMM's A, gamma, B, beta, alpha, C
    write_dcd(dcd, frames, cell=True)
    patch_records(dcd, records)
    want, _, done, _ = run(tmp_path, "dcd", dcd, radii, alg, dcd=True, pbc=True, triclinic=True, out_f32=out_f32)
    assert done
    cells = np.array([[r[0], r[2], r[5], r[4], r[3], r[1]] for r in records])
    write_amber(nc, frames, cells, version=version)
    got, p, done, n_frames = run(tmp_path, "nc", nc, radii, alg, netcdf=True, pbc=True, triclinic=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    assert f" f32={56 | (2 if out_f32 else 0)} " in open(p["done"]).readline()
    # without bit 4 such a file is refused at its first frame
    with pytest.raises(RuntimeError, match="frame 0 of the NetCDF file: its cell is not orthorhombic"):
        run(tmp_path, "ortho", nc, radii, alg, netcdf=True, pbc=True)


def test_a_right_angled_file_gives_the_files_of_the_orthorhombic_run(coil, tmp_path):
    frames, radii = coil
    nc = tmp_path / "right.nc"
    write_amber(nc, frames, np.array([list(c) + [90.0, 90.0, 90.0] for c in frame_cells()]))
    old, _, done0, _ = run(tmp_path, "pbc", nc, radii, netcdf=True, pbc=True)
    new, _, done1, _ = run(tmp_path, "tri", nc, radii, netcdf=True, pbc=True, triclinic=True)
    assert done0 and done1 and new == old


def test_periodic_run_with_a_topology_equals_the_dcd_run(solvated, tmp_path):
    b, full, index = solvated
    full = full[:2]
    solute = full[:, index].astype(np.float64)
    cell = tuple(float(v) for v in solute.reshape(-1, 3).max(0) - solute.reshape(-1, 3).min(0) + 4.0)
    cells = [cell, (cell[0] + 0.25, cell[1], cell[2])]
    dcd, nc = tmp_path / "solvated.dcd", tmp_path / "solvated.nc"
    write_dcd(dcd, full, cell=True)
    patch_cells(dcd, cells)
    write_amber(nc, full, np.array([list(c) + [90.0] * 3 for c in cells]), velocities=True)
    sel = ingest.Selection(COMMANDS)
    try:
        out = {}
        for tag, path, kw in (("dcd", dcd, dict(dcd=True)), ("nc", nc, dict(netcdf=True)), ("nc-tri", nc, dict(netcdf=True, triclinic=True))):
            p = {k: str(tmp_path / f"{tag}.{k}") for k in OUTS[:5] + ("done",)}
            done, n_frames, atoms = fa.trajectory_file_topology(path, b, p["totals"], atom_index=index, selection=sel, sasa_path=p["sasa"],
                                                                class_sums_path=p["cls"], residues_path=p["res"], selections_path=p["sel"],
                                                                done_path=p["done"], frames_per_batch=FPB, devices=[0, 0], pbc=True, probe=PROBE, **kw)
            assert done and n_frames == 2
            out[tag] = {k: open(p[k], "rb").read() for k in OUTS[:5]}
    finally:
        sel.close()
    assert out["nc"] == out["dcd"] and np.all(np.frombuffer(out["nc"]["totals"]) > 0)
    assert out["nc-tri"] == out["nc"]          # (an atom index and triclinic cells: the right-angled cells through the general geometry)


def test_a_bad_frame_ends_the_run_and_a_repaired_file_completes_it(coil, tmp_path):
    """frame 3 (of shard 1: frames 2 and 3) has an edge below c: a host check on the staged bytes, nothing of the shard reaches the
    device and it is not listed.  The done-list names the frame file by size and modification time: a repair in place that keeps
    both resumes the run, which ends with the files of an uninterrupted one."""
    frames, radii = coil
    good = np.array([list(c) + [90.0] * 3 for c in frame_cells()])
    bad = good.copy()
    bad[3, 1] = 2 * (radii.max() + PROBE) - 0.01
    nc, ref = tmp_path / "frames.nc", tmp_path / "ref.nc"
    write_amber(ref, frames, good)
    want, _, done, _ = run(tmp_path, "ref", ref, radii, netcdf=True, pbc=True)
    assert done
    write_amber(nc, frames, bad)
    st = os.stat(nc)
    os.environ["FREESASA_AMD_TRAJ_LANES"] = "1"
    try:
        with pytest.raises(RuntimeError, match=r"frame 3 of the NetCDF file: edge y of its cell is .* shorter than c"):
            run(tmp_path, "bad", nc, radii, netcdf=True, pbc=True, device=0)
    finally:
        os.environ.pop("FREESASA_AMD_TRAJ_LANES", None)
    done_path = str(tmp_path / "bad.done")
    assert [int(line.split()[1]) for line in open(done_path).read().splitlines()[1:]] == [0]     # (one lane: the shards go in order)
    write_amber(nc, frames, good)
    os.utime(nc, ns=(st.st_atime_ns, st.st_mtime_ns))
    got, p, done, n_frames = run(tmp_path, "bad", nc, radii, netcdf=True, pbc=True)
    assert done and n_frames == F and got == want
    assert sorted(int(line.split()[1]) for line in open(done_path).read().splitlines()[1:]) == [0, 1, 2]


def test_resume_and_done_lists_of_other_formats(coil, raw_plain, tmp_path):
    frames, radii = coil
    want = raw_plain("lr20", False)
    nc, dcd, raw = tmp_path / "frames.nc", tmp_path / "frames.dcd", tmp_path / "frames.f32"
    write(nc, frames, "cells+velocities")
    write_dcd(dcd, frames, cell=True)
    frames.tofile(raw)
    a, res = ALGS["lr20"]
    p = {k: str(tmp_path / f"part.{k}") for k in ("totals", "sasa", "done")}
    kw = dict(done_path=p["done"], alg=a, resolution=res, frames_per_batch=FPB)
    done, n_frames = fa.trajectory_file(nc, radii, p["totals"], p["sasa"], netcdf=True, max_new_shards=1, **kw)
    assert not done and n_frames == F and open(p["done"]).read().count("shard ") == 1
    done, _ = fa.trajectory_file(nc, radii, p["totals"], p["sasa"], netcdf=True, **kw)
    assert done and open(p["done"]).read().count("shard ") == 3
    assert open(p["totals"], "rb").read() == want["totals"] and open(p["sasa"], "rb").read() == want["sasa"]
    # a NetCDF run's list is not a DCD run's nor a raw run's, and the other way round: refused, files untouched
    before = open(p["done"]).read()
    for path, other in ((dcd, dict(dcd=True)), (raw, dict(f32=True))):
        with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
            fa.trajectory_file(path, radii, p["totals"], p["sasa"], **other, **kw)
        tag = "dcdlist" if "dcd" in other else "rawlist"
        got, other_done, done, _ = plain_run(tmp_path, tag, path, radii, **other)
        assert done and got == want
        other_list = open(other_done).read()
        with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
            fa.trajectory_file(nc, radii, str(tmp_path / f"{tag}.totals"), str(tmp_path / f"{tag}.sasa"), netcdf=True, **dict(kw, done_path=other_done))
        assert open(other_done).read() == other_list and open(tmp_path / f"{tag}.totals", "rb").read() == want["totals"]
    assert open(p["done"]).read() == before and open(p["totals"], "rb").read() == want["totals"]
