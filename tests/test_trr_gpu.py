"""GROMACS TRR input of the trajectory file drivers (FREESASA_GPU_FRAMES_TRR, include/freesasa_gpu.h) on the device.  Every
comparison is byte for byte between result files: one run reads a TRR file written by tests/trr_codec.py, in single or double
precision, the other the raw fp64 frame file that holds float64(x_nm) * 10.0 - a path the existing tests pin to the per-structure
entries - or, for periodic images, a DCD file of the same frames and cells.  Small seeded systems; frames_per_batch = 2 over 5
frames gives shards of 2, 2 and 1 frames, of records of unequal length, some of them without coordinates."""
import os
import stat
import struct
import threading

import numpy as np
import pytest

import freesasa_amd as fa
import tools
import trr_codec as tc
from freesasa_amd import ingest
from test_dcd import write_dcd
from test_dcd_gpu import ALGS, COMMANDS, F, FPB, OUTS, jittered, plain_run, solvated, topo_run  # noqa: F401  (solvated: a fixture)
from test_pbc_gpu import patch_cells
from test_pbc_tri_gpu import patch_records
from test_xtc_gpu import boxes_nm, exact_triclinic, indexed_periodic_runs_equal_the_dcd_run, solute_cells

pytestmark = pytest.mark.gpu

N = 37
BOX = np.array([[3.0, 0, 0], [0.5, 3.5, 0], [-0.25, 0.75, 4.0]])
PRECISIONS = pytest.mark.parametrize("double", [False, True], ids=["single", "double"])


def records_of(frames_nm, double, boxes=None, extras=True):
    """the five frames as TRR records of unequal length: with and without box, virial, pressure, velocities and forces, and - with
    extras - velocity-only records in front of frame 0, between frames 0 and 1 (inside shard 0), between frames 1 and 2 (the last
    record of shard 0's bytes: at a shard boundary) and behind frame 4"""
    n = frames_nm.shape[1]
    rng = np.random.default_rng(17)
    k = dict(natoms=n, double=double)
    other = lambda: rng.uniform(-1, 1, (n, 3))
    box = (lambda f: boxes[f]) if boxes is not None else (lambda f: BOX if f in (0, 2, 4) else None)
    x = frames_nm
    recs = [dict(k, box=box(0), x=x[0], v=other(), f=other(), step=0), dict(k, box=box(1), x=x[1], step=10),
            dict(k, box=box(2), vir=BOX, pres=BOX, x=x[2], v=other(), step=20, t=1.0), dict(k, box=box(3), x=x[3], f=other(), step=30),
            dict(k, box=box(4), x=x[4], step=40)]
    if extras:
        vel = lambda step: dict(k, v=other(), step=step)
        recs = [vel(-5), recs[0], vel(5), recs[1], vel(15), recs[2], recs[3], recs[4], vel(45)]
    return recs


def trr_and_raw(tmp, frames_angstrom, double, boxes=None, extras=True, name="frames"):
    """the frames (float32, Angstrom) as a TRR file of that precision and as the raw fp64 file of what the TRR file holds:
    -> (float64(x_nm) * 10.0 [F, n, 3], the codec's records)"""
    data = tc.write_trr(tmp / f"{name}.trr", records_of(frames_angstrom.astype(np.float64) / 10.0, double, boxes, extras))
    recs = tc.decode(data)
    decoded = tc.frames_angstrom(recs)
    assert decoded.dtype == np.float64 and decoded.shape == frames_angstrom.shape and np.abs(decoded - frames_angstrom).max() < 1e-5
    decoded.tofile(tmp / f"{name}.f64")
    return decoded, recs


_COIL = []


def coil():
    if not _COIL:
        xyz, radii = tools.coil(N, 20261018)
        _COIL.append((jittered(xyz, F, 1), radii))
    return _COIL[0]


@pytest.mark.parametrize("out_f32", [False, True], ids=["f64-out", "f32-out"])
@pytest.mark.parametrize("alg", ["lr20", "sr100"])
@PRECISIONS
def test_plain_driver_equals_the_raw_fp64_run(tmp_path, double, alg, out_f32):
    frames, radii = coil()
    _, recs = trr_and_raw(tmp_path, frames, double)
    kinds = [r.x is not None for r in recs]
    assert kinds == [False, True, False, True, False, True, True, True, False]           # coordinate-less records inside shard 0 and at its end
    assert len({r.size for r in recs if r.x is not None}) == F and {r.box is not None for r in recs if r.x is not None} == {False, True}
    info = fa.trr_info(tmp_path / "frames.trr")
    assert (info.n_frames, info.n_records, info.real_bytes) == (F, 9, 8 if double else 4)
    want, _, done, n_frames = plain_run(tmp_path, "raw", tmp_path / "frames.f64", radii, alg, out_f32=out_f32)
    assert done and n_frames == F and len(want["totals"]) == 8 * F and len(want["sasa"]) == (4 if out_f32 else 8) * F * N
    assert np.all(np.frombuffer(want["totals"]) > 0)
    got, done_path, done, n_frames = plain_run(tmp_path, "trr", tmp_path / "frames.trr", radii, alg, trr=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    head = open(done_path).readline()
    assert f" f32={128 | (2 if out_f32 else 0)} " in head and " header_bytes=0 " in head and f" n_frames={F} " in head
    assert open(done_path).read().count("shard ") == 3


@pytest.mark.parametrize("groups", [False, True], ids=["topology", "chain-groups"])
@PRECISIONS
def test_topology_and_chain_groups_equal_the_raw_fp64_run(solvated, tmp_path, double, groups):
    """2jo4 (516 atoms) scattered among 41 solvent atoms, a shuffled index, two lanes of one device, selections, residues, class sums"""
    b, full, index = solvated
    n, R = int(b.n_atoms), int(b.n_residues)
    decoded, _ = trr_and_raw(tmp_path, full, double)
    system = (b, decoded, index)
    sel = ingest.Selection(COMMANDS)
    try:
        want, want_atoms = topo_run(tmp_path, "raw", tmp_path / "frames.f64", system, sel, groups, frame_atoms=n + 41)
        got, atoms = topo_run(tmp_path, "trr", tmp_path / "frames.trr", system, sel, groups, trr=True)    # (frame_atoms: the file's)
        assert sorted(got) == sorted(want) == sorted(OUTS if groups else OUTS[:5])
        for k in got:
            assert got[k] == want[k], k
        assert np.array_equal(atoms, want_atoms) and atoms.min() > 0
    finally:
        sel.close()
    assert len(want["totals"]) == 8 * F and len(want["sasa"]) == 8 * F * n and len(want["res"]) == 8 * 6 * R * F
    assert np.all(np.frombuffer(want["totals"]) > 0)
    if groups:
        assert len(want["grp"]) == 8 * 3 * 4 * F and len(want["iso"]) == 8 * F * n


def on_the_grid(frames_angstrom):
    """the frames moved onto the grid on which nm * 10 is exact in fp32: nm a multiple of 2^-12 below 256 -> (nm float64, Angstrom
    float32): the DCD file's fp32 values and the TRR file's reals times 10.0 are then the very same numbers, in both precisions"""
    grid = np.round(frames_angstrom.astype(np.float64) / 10.0 * 4096.0) / 4096.0
    angstrom = (grid * 10.0).astype(np.float32)
    assert np.abs(grid).max() < 256 and np.array_equal(angstrom.astype(np.float64), grid * 10.0)
    assert np.array_equal(grid.astype(np.float32).astype(np.float64), grid)
    return grid, angstrom


def periodic_files(tmp, frames_angstrom, double, boxes):
    """(the TRR file of the grid frames with a box per frame, the DCD file of the same frames with a cell record per frame)"""
    grid, angstrom = on_the_grid(frames_angstrom)
    data = tc.write_trr(tmp / "frames.trr", records_of(grid, double, [np.asarray(b, dtype=np.float64) for b in boxes]))
    assert np.array_equal(tc.frames_angstrom(tc.decode(data)), angstrom.astype(np.float64))
    write_dcd(tmp / "frames.dcd", angstrom, cell=True)
    return tmp / "frames.trr", tmp / "frames.dcd"


def ortho_cells():
    """the coil's extent is (10.9, 9.5, 9.1) and c = 2 (1.88 + 1.4) = 6.56: its atoms see their images through every face"""
    return [(14.0 + 0.3 * f, 13.0, 12.5 - 0.1 * f) for f in range(F)]


@pytest.mark.parametrize("alg, out_f32, indexed", [("lr20", False, False), ("sr100", True, False), ("lr20", False, True)],
                         ids=["lr20-False", "sr100-True", "atom-index"])
@PRECISIONS
def test_periodic_orthorhombic_run_equals_the_dcd_run(request, tmp_path, double, alg, out_f32, indexed):
    if indexed:
        b, full, index = request.getfixturevalue("solvated")
        boxes, cells = boxes_nm(solute_cells(full, index))
        trr, dcd = periodic_files(tmp_path, full, double, boxes)
        patch_cells(dcd, cells)
        return indexed_periodic_runs_equal_the_dcd_run(tmp_path, (b, full, index), dcd, trr, trr=True)
    frames, radii = coil()
    boxes, cells = boxes_nm(ortho_cells())
    trr, dcd = periodic_files(tmp_path, frames, double, boxes)
    patch_cells(dcd, cells)
    want, _, done, _ = plain_run(tmp_path, "dcd", dcd, radii, alg, dcd=True, pbc=True, out_f32=out_f32)
    got, done_path, done2, n_frames = plain_run(tmp_path, "trr", trr, radii, alg, trr=True, pbc=True, out_f32=out_f32)
    assert done and done2 and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    assert f" f32={136 | (2 if out_f32 else 0)} " in open(done_path).readline()
    # it is not the non-periodic run's answer
    plain, _, _, _ = plain_run(tmp_path, "plain", trr, radii, alg, trr=True, out_f32=out_f32)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"]))
    # a right-angled box with triclinic=True: the orthorhombic files
    tri, done_path, done, _ = plain_run(tmp_path, "tri", trr, radii, alg, trr=True, pbc=True, triclinic=True, out_f32=out_f32)
    assert done and tri == got and f" f32={152 | (2 if out_f32 else 0)} " in open(done_path).readline()


@pytest.mark.parametrize("alg, out_f32", [("lr20", False), ("sr100", True)])
@PRECISIONS
def test_periodic_triclinic_run_equals_the_dcd_run(tmp_path, double, alg, out_f32):
    frames, radii = coil()
    boxes, records = exact_triclinic(F)
    assert len({tuple(b.reshape(-1)) for b in boxes}) == F and all(b[2, 0] != 0 and b[2, 1] != 0 for b in boxes)
    trr, dcd = periodic_files(tmp_path, frames, double, boxes)
    patch_records(dcd, records)
    want, _, done, _ = plain_run(tmp_path, "dcd", dcd, radii, alg, dcd=True, pbc=True, triclinic=True, out_f32=out_f32)
    got, done_path, done2, n_frames = plain_run(tmp_path, "trr", trr, radii, alg, trr=True, pbc=True, triclinic=True, out_f32=out_f32)
    assert done and done2 and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    assert f" f32={152 | (2 if out_f32 else 0)} " in open(done_path).readline()
    plain, _, _, _ = plain_run(tmp_path, "plain", trr, radii, alg, trr=True, out_f32=out_f32)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"]))
    # without bit 4 such a file is refused at its first frame; an upper element is refused with it
    with pytest.raises(RuntimeError, match="frame 0 of the TRR file: its cell is not orthorhombic"):
        plain_run(tmp_path, "ortho", trr, radii, alg, trr=True, pbc=True)
    upper = [np.array(b, dtype=np.float64) for b in boxes]
    upper[3][0, 2] = 0.25
    grid, _ = on_the_grid(frames)
    tc.write_trr(tmp_path / "upper.trr", records_of(grid, double, upper))
    with pytest.raises(RuntimeError, match=r"frame 3 of the TRR file: element \[0\]\[2\] of its box is 0.25"):
        plain_run(tmp_path, "upper", tmp_path / "upper.trr", radii, alg, trr=True, pbc=True, triclinic=True)


@PRECISIONS
def test_a_box_that_touches_nothing_changes_nothing(tmp_path, double):
    frames, radii = coil()
    far = (frames + (500.0 - frames.reshape(-1, 3).mean(0))).astype(np.float32)
    boxes = [np.diag([100.0, 100.0, 100.0])] * F
    tc.write_trr(tmp_path / "far.trr", records_of(far.astype(np.float64) / 10.0, double, boxes))
    plain, p0, done0, _ = plain_run(tmp_path, "plain", tmp_path / "far.trr", radii, trr=True)
    pbc, p1, done1, _ = plain_run(tmp_path, "pbc", tmp_path / "far.trr", radii, trr=True, pbc=True)
    tri, p2, done2, _ = plain_run(tmp_path, "tri", tmp_path / "far.trr", radii, trr=True, pbc=True, triclinic=True)
    assert done0 and done1 and done2
    assert pbc == plain and tri == plain
    assert len(plain["totals"]) == 8 * F and np.all(np.frombuffer(plain["totals"]) > 0)
    assert [open(p).readline().split(" f32=")[1].split()[0] for p in (p0, p1, p2)] == ["128", "136", "152"]
    # a frame without a box in a periodic run, one whose box is all zero, and an edge below c: host checks on the staged bytes
    for tag, box, text in (("nobox", None, "frame 3 of the TRR file: it has no box"), ("zero", np.zeros((3, 3)), "frame 3 of the TRR file: its box is all zero"),
                           ("small", np.diag([100.0, 0.65, 100.0]), r"frame 3 of the TRR file: edge y of its cell is .* shorter than c")):
        odd = list(boxes)
        odd[3] = box
        tc.write_trr(tmp_path / f"{tag}.trr", records_of(far.astype(np.float64) / 10.0, double, odd))
        with pytest.raises(RuntimeError, match=text):
            plain_run(tmp_path, tag, tmp_path / f"{tag}.trr", radii, trr=True, pbc=True)


@PRECISIONS
def test_run_statistics_equal_those_of_the_raw_fp64_run(tmp_path, double):
    frames, radii = coil()
    trr_and_raw(tmp_path, frames, double)
    a, res = ALGS["lr20"]
    files = {}
    for tag, path, kw in (("raw", tmp_path / "frames.f64", {}), ("trr", tmp_path / "frames.trr", dict(trr=True))):
        p = {k: str(tmp_path / f"{tag}.{k}") for k in ("totals", "sasa", "done", "stats", "parts")}
        done, n_frames = fa.trajectory_file(path, radii, p["totals"], p["sasa"], done_path=p["done"], alg=a, resolution=res, frames_per_batch=FPB,
                                            stats=("totals", "atoms"), stats_path=p["stats"], partials_path=p["parts"], **kw)
        assert done and n_frames == F
        files[tag] = {k: open(p[k], "rb").read() for k in ("totals", "sasa", "stats", "parts")}
        assert open(p["done"]).readline().endswith(" stats=%d\n" % fa.stats_word(("totals", "atoms")))
    assert files["trr"] == files["raw"]
    assert len(files["raw"]["stats"]) == 8 * 4 * (1 + N) and len(files["raw"]["parts"]) == 8 * 4 * (1 + N) * 3
    st = np.frombuffer(files["raw"]["stats"]).reshape(4, 1 + N)
    assert np.all(st[0, 0] > 0) and np.all(st[2] <= st[0]) and np.all(st[0] <= st[3]) and st[1].max() > 0


def test_a_damaged_header_ends_the_run_and_a_repaired_file_completes_it(tmp_path):
    """The pass over the headers sees every header before a device is touched: a file damaged at rest is refused there ("record K
    of the TRR file"), whatever its done-list holds.  The check of the staged bytes is for a file that changes under a running
    call, which is what this test arranges without waiting for anything: the done-list's path is a FIFO, on which the call - its
    index made, the frame file open - blocks until a helper thread, itself blocked until then, has overwritten the magic number of
    frame 3 (of shard 1: frames 2 and 3), removed the FIFO and let go; the call then starts a done-list as a regular file.  With
    one lane the shards go in order: shard 0 is computed and listed, shard 1 ends the run on the host, nothing of it is written.
    The done-list names the frame file by size and modification time: a repair in place that keeps both resumes the run, which
    ends with the files of an uninterrupted one."""
    frames, radii = coil()
    _, recs = trr_and_raw(tmp_path, frames, True, name="good")
    good = tmp_path / "good.trr"
    want, _, done, _ = plain_run(tmp_path, "good", good, radii, trr=True)
    assert done
    data = good.read_bytes()
    frame3 = [r for r in recs if r.x is not None][3]
    assert struct.unpack_from(">i", data, frame3.offset)[0] == tc.MAGIC
    damaged = data[:frame3.offset] + struct.pack(">i", 1995) + data[frame3.offset + 4:]
    bad = tmp_path / "frames.trr"
    bad.write_bytes(data)
    st = os.stat(bad)
    paths = {k: str(tmp_path / f"bad.{k}") for k in ("totals", "sasa", "done")}
    os.mkfifo(paths["done"])

    def damage():
        fd = os.open(paths["done"], os.O_WRONLY)                   # (returns when the call reads its done-list)
        try:
            bad.write_bytes(damaged)
            os.unlink(paths["done"])
        finally:
            os.close(fd)

    helper = threading.Thread(target=damage)
    helper.start()
    os.environ["FREESASA_AMD_TRAJ_LANES"] = "1"
    a, res = ALGS["lr20"]
    kw = dict(done_path=paths["done"], alg=a, resolution=res, frames_per_batch=FPB, trr=True)
    try:
        with pytest.raises(RuntimeError, match="frame 3 of the TRR file is damaged: its magic number is 1995, not 1993"):
            fa.trajectory_file(bad, radii, paths["totals"], paths["sasa"], device=0, **kw)
    finally:
        os.environ.pop("FREESASA_AMD_TRAJ_LANES", None)
        if os.path.exists(paths["done"]) and helper.is_alive():     # (the call ended before its done-list: let the helper go)
            os.close(os.open(paths["done"], os.O_RDONLY | os.O_NONBLOCK))
        helper.join()
    assert bad.read_bytes() == damaged and stat.S_ISREG(os.stat(paths["done"]).st_mode)
    assert [int(line.split()[1]) for line in open(paths["done"]).read().splitlines()[1:]] == [0]     # (one lane: the shards go in order)
    assert open(paths["totals"], "rb").read()[:8 * FPB] == want["totals"][:8 * FPB]
    assert open(paths["sasa"], "rb").read()[:8 * N * FPB] == want["sasa"][:8 * N * FPB]
    # at rest the damaged file is refused by the pass over the headers, before the done-list is looked at: shard 0 stays listed
    listed = open(paths["done"]).read()
    with pytest.raises(RuntimeError, match="record 6 of the TRR file: its magic number is 1995, not 1993"):
        fa.trajectory_file(bad, radii, paths["totals"], paths["sasa"], **kw)
    assert open(paths["done"]).read() == listed
    bad.write_bytes(data)
    os.utime(bad, ns=(st.st_atime_ns, st.st_mtime_ns))
    done, n_frames = fa.trajectory_file(bad, radii, paths["totals"], paths["sasa"], **kw)
    assert done and n_frames == F
    assert open(paths["totals"], "rb").read() == want["totals"] and open(paths["sasa"], "rb").read() == want["sasa"]
    assert sorted(int(line.split()[1]) for line in open(paths["done"]).read().splitlines()[1:]) == [0, 1, 2]


def test_resume_and_done_lists_of_other_formats(tmp_path):
    from netcdf_writer import write_amber
    import xtc_codec as xc
    frames, radii = coil()
    grid, angstrom = on_the_grid(frames)                           # (fp32 holds these: every format's run gives the same files)
    trr, raw, raw32, dcd, nc, xtc = (tmp_path / f"frames.{e}" for e in ("trr", "f64", "f32", "dcd", "nc", "xtc"))
    tc.write_trr(trr, records_of(grid, False))
    angstrom.astype(np.float64).tofile(raw)
    angstrom.tofile(raw32)
    write_dcd(dcd, angstrom, cell=True)
    write_amber(nc, angstrom)
    want, _, done, _ = plain_run(tmp_path, "want", raw, radii)
    assert done
    a, res = ALGS["lr20"]
    p = {k: str(tmp_path / f"part.{k}") for k in ("totals", "sasa", "done")}
    kw = dict(done_path=p["done"], alg=a, resolution=res, frames_per_batch=FPB)
    done, n_frames = fa.trajectory_file(trr, radii, p["totals"], p["sasa"], trr=True, max_new_shards=1, **kw)
    assert not done and n_frames == F and open(p["done"]).read().count("shard ") == 1
    done, _ = fa.trajectory_file(trr, radii, p["totals"], p["sasa"], trr=True, devices=[0, 0], **kw)
    assert done and open(p["done"]).read().count("shard ") == 3
    assert open(p["totals"], "rb").read() == want["totals"] and open(p["sasa"], "rb").read() == want["sasa"]
    # a TRR run's list is not a raw, a DCD, a NetCDF or an XTC run's, and the other way round: refused, files untouched
    xc.write_xtc(xtc, angstrom, 1000.0, None)
    before = open(p["done"]).read()
    for tag, path, other, same in (("rawlist", raw, {}, True), ("raw32list", raw32, dict(f32=True), True), ("dcdlist", dcd, dict(dcd=True), True),
                                   ("nclist", nc, dict(netcdf=True), True), ("xtclist", xtc, dict(xtc=True), False)):
        with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
            fa.trajectory_file(path, radii, p["totals"], p["sasa"], **other, **kw)
        got, q, done, _ = plain_run(tmp_path, tag, path, radii, **other)
        assert done and (got == want or not same)                  # (an XTC file holds three decimals: other numbers, its own list)
        other_list = open(q).read()
        qt = str(tmp_path / f"{tag}.totals")
        with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
            fa.trajectory_file(trr, radii, qt, str(tmp_path / f"{tag}.sasa"), trr=True, **dict(kw, done_path=q))
        assert open(q).read() == other_list and open(qt, "rb").read() == got["totals"]
    assert open(p["done"]).read() == before and open(p["totals"], "rb").read() == want["totals"]
