"""GROMACS XTC input of the trajectory file drivers (FREESASA_GPU_FRAMES_XTC, include/freesasa_gpu.h) on the device.  Every
comparison is byte for byte between result files: one run reads an XTC file written by tests/xtc_codec.py, the other the raw fp32
frame file of the values the codec decodes that file to - a path the existing tests pin to the per-structure entries - or, for
periodic images, a DCD file of the same decoded frames and cells.  Small seeded systems; frames_per_batch = 4 over 11 frames gives
shards of 4, 4 and 3 frames, each of frames of unequal length."""
import os

import numpy as np
import pytest

import freesasa_amd as fa
import tools
import xtc_codec as xc
from emu import xtc_emu
from freesasa_amd import ingest
from test_dcd import write_dcd
from test_dcd_gpu import ALGS, COMMANDS, OUTS, jittered, solvated, topo_run  # noqa: F401  (solvated: a fixture)
from test_pbc_gpu import patch_cells
from test_pbc_tri_gpu import patch_records

pytestmark = pytest.mark.gpu

F, FPB = 11, 4
PROBE = 1.4


def xtc_of(path, frames_angstrom, precision=1000.0, boxes=None):
    """the frames as an XTC file -> (what the file decodes to: [F, n, 3] float32 in Angstrom, the codec's frames)"""
    data = xc.write_xtc(path, frames_angstrom, precision, boxes)
    frames = xc.decode(data)
    return np.array([f.xyz for f in frames]), frames


_COILS = {}


def coil(n):
    """a coil of n atoms, 11 jittered frames, as an XTC file's bytes would hold them: (decoded frames, radii, input frames)"""
    if n not in _COILS:
        xyz, radii = tools.coil(n, 20261018)
        _COILS[n] = (jittered(xyz, F, 1), radii)
    return _COILS[n]


def run(tmp, tag, path, radii, alg="lr20", fpb=FPB, **kw):
    """trajectory_file into files of their own: ({output: bytes}, the paths, complete, frames)"""
    a, res = ALGS[alg]
    p = {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "done")}
    done, n_frames = fa.trajectory_file(path, radii, p["totals"], p["sasa"], done_path=p["done"], alg=a, probe=PROBE, resolution=res,
                                        frames_per_batch=fpb, **kw)
    return {k: open(p[k], "rb").read() for k in ("totals", "sasa")}, p, done, n_frames


def raw_and_xtc(tmp, n, precision=1000.0, boxes=None):
    frames, radii = coil(n)
    decoded, coded = xtc_of(tmp / "frames.xtc", frames, precision, boxes)
    assert decoded.shape == (F, n, 3) and np.abs(decoded - frames).max() < 10.0 / precision + 1e-5
    decoded.tofile(tmp / "frames.f32")
    return radii, decoded, coded


@pytest.mark.parametrize("out_f32", [False, True], ids=["f64-out", "f32-out"])
@pytest.mark.parametrize("alg", ["lr20", "sr100"])
@pytest.mark.parametrize("n", [37, 516])
def test_plain_driver_equals_the_raw_run(tmp_path, n, alg, out_f32):
    radii, _, coded = raw_and_xtc(tmp_path, n)
    assert all(len({f.size for f in coded[k:k + FPB]}) > 1 for k in range(0, F, FPB))          # frames of unequal length within every shard
    want, _, done, n_frames = run(tmp_path, "raw", tmp_path / "frames.f32", radii, alg, f32=True, out_f32=out_f32)
    assert done and n_frames == F and len(want["totals"]) == 8 * F and len(want["sasa"]) == (4 if out_f32 else 8) * F * n
    assert np.all(np.frombuffer(want["totals"]) > 0)
    got, p, done, n_frames = run(tmp_path, "xtc", tmp_path / "frames.xtc", radii, alg, xtc=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    head = open(p["done"]).readline()
    assert f" f32={64 | (2 if out_f32 else 0)} " in head and " header_bytes=0 " in head and f" n_frames={F} " in head
    assert open(p["done"]).read().count("shard ") == 3


def test_bitsize_zero_and_ten_atoms(tmp_path):
    """a precision at which the coil spans more than 0xffffff integers in a dimension: one field per dimension; and the smallest
    system XTC compresses"""
    radii, _, coded = raw_and_xtc(tmp_path, 37, precision=2.0e7)
    assert all(xc.bit_sizes([f.maxint[k] - f.minint[k] + 1 for k in range(3)])[0] == 0 for f in coded)
    want, _, done, _ = run(tmp_path, "raw", tmp_path / "frames.f32", radii, f32=True)
    got, _, done2, n_frames = run(tmp_path, "xtc", tmp_path / "frames.xtc", radii, xtc=True)
    assert done and done2 and n_frames == F and got == want and np.all(np.frombuffer(want["totals"]) > 0)
    sub = tmp_path / "ten"
    sub.mkdir()
    radii, _, _ = raw_and_xtc(sub, 10)
    want, _, done, _ = run(sub, "raw", sub / "frames.f32", radii, "sr100", f32=True)
    got, _, done2, n_frames = run(sub, "xtc", sub / "frames.xtc", radii, "sr100", xtc=True)
    assert done and done2 and n_frames == F and got == want and np.all(np.frombuffer(want["totals"]) > 0)


@pytest.mark.parametrize("groups", [False, True], ids=["topology", "chain-groups"])
def test_topology_and_chain_groups_equal_the_raw_run(solvated, tmp_path, groups):
    """2jo4 (516 atoms) scattered among 41 solvent atoms, a shuffled index, two lanes of one device, selections, residues, class sums"""
    b, full, index = solvated
    n, R = int(b.n_atoms), int(b.n_residues)
    decoded, _ = xtc_of(tmp_path / "frames.xtc", full)
    decoded.tofile(tmp_path / "frames.f32")
    system = (b, decoded, index)
    sel = ingest.Selection(COMMANDS)
    try:
        want, want_atoms = topo_run(tmp_path, "raw", tmp_path / "frames.f32", system, sel, groups, frame_atoms=n + 41, f32=True)
        got, atoms = topo_run(tmp_path, "xtc", tmp_path / "frames.xtc", system, sel, groups, xtc=True)    # (frame_atoms: the file's)
        assert sorted(got) == sorted(want) == sorted(OUTS if groups else OUTS[:5])
        for k in got:
            assert got[k] == want[k], k
        assert np.array_equal(atoms, want_atoms) and atoms.min() > 0
    finally:
        sel.close()
    nf = len(full)
    assert len(want["totals"]) == 8 * nf and len(want["sasa"]) == 8 * nf * n and len(want["res"]) == 8 * 6 * R * nf
    assert np.all(np.frombuffer(want["totals"]) > 0)
    if groups:
        assert len(want["grp"]) == 8 * 3 * 4 * nf and len(want["iso"]) == 8 * nf * n


def boxes_nm(cells_angstrom):
    """per frame the float32 box in nm and the cell it stands for: each element (double) float * 10.0"""
    boxes = [np.diag(np.asarray(c, dtype=np.float64) / 10.0).astype(np.float32) for c in cells_angstrom]
    return boxes, [tuple(float(b[k, k]) * 10.0 for k in range(3)) for b in boxes]


def ortho_cells():
    """the coil's extent is (10.9, 9.5, 9.1) and c = 2 (1.88 + 1.4) = 6.56: its atoms see their images through every face"""
    return [(14.0 + 0.3 * f, 13.0, 12.5 - 0.1 * f) for f in range(F)]


def solute_cells(full, index):
    """right-angled cells for the solvated system's frames, another in every frame: 2 A short of the solute's extent (about 30 A, far
    above c), so that the images of its outermost atoms lie among the atoms of the opposite face - with 4 A more than the extent
    no image of 2jo4 reaches an atom (the solvent, which the index drops, may lie anywhere)"""
    s = full[:, index].astype(np.float64).reshape(-1, 3)
    ext = s.max(0) - s.min(0) - 2.0
    return [(float(ext[0]) + 0.25 * f, float(ext[1]), float(ext[2]) + 0.125 * f) for f in range(len(full))]


def indexed_periodic_runs_equal_the_dcd_run(tmp, system, dcd, path, **how):
    """A periodic run WITH an atom index (the solvated system: a short last shard, two lanes) on a container file against the
    DCD run of the same frames and cells: totals, areas, class sums, residues and selections byte for byte; the container's
    run once more with its right-angled cells read as triclinic ones: the same files; and not the non-periodic run's"""
    sel = ingest.Selection(COMMANDS)
    try:
        want, want_atoms = topo_run(tmp, "dcd-index", dcd, system, sel, False, dcd=True, pbc=True)
        got, atoms = topo_run(tmp, "index", path, system, sel, False, pbc=True, **how)
        tri, _ = topo_run(tmp, "index-tri", path, system, sel, False, pbc=True, triclinic=True, **how)
        plain, _ = topo_run(tmp, "index-plain", path, system, sel, False, **how)
    finally:
        sel.close()
    assert sorted(got) == sorted(OUTS[:5]) and got == want and tri == got and np.array_equal(atoms, want_atoms)
    # images bury area and never add any; in cells this tight they bury some in every frame
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"])) and np.all(np.frombuffer(got["totals"]) > 0)


@pytest.mark.parametrize("alg, out_f32, indexed", [("lr20", False, False), ("sr100", True, False), ("lr20", False, True)],
                         ids=["lr20-False", "sr100-True", "atom-index"])
def test_periodic_orthorhombic_run_equals_the_dcd_run(request, tmp_path, alg, out_f32, indexed):
    if indexed:             # the only kind whose decoded fp32 frames lie inside c->g_xyz, behind the cells and the group records
        b, full, index = request.getfixturevalue("solvated")
        boxes, cells = boxes_nm(solute_cells(full, index))
        decoded, _ = xtc_of(tmp_path / "frames.xtc", full, boxes=boxes)
        write_dcd(tmp_path / "frames.dcd", decoded, cell=True)
        patch_cells(tmp_path / "frames.dcd", cells)
        return indexed_periodic_runs_equal_the_dcd_run(tmp_path, (b, decoded, index), tmp_path / "frames.dcd", tmp_path / "frames.xtc", xtc=True)
    frames, radii = coil(37)
    boxes, cells = boxes_nm(ortho_cells())
    decoded, _ = xtc_of(tmp_path / "frames.xtc", frames, boxes=boxes)
    dcd = tmp_path / "frames.dcd"
    write_dcd(dcd, decoded, cell=True)
    patch_cells(dcd, cells)
    want, _, done, _ = run(tmp_path, "dcd", dcd, radii, alg, dcd=True, pbc=True, out_f32=out_f32)
    got, p, done2, n_frames = run(tmp_path, "xtc", tmp_path / "frames.xtc", radii, alg, xtc=True, pbc=True, out_f32=out_f32)
    assert done and done2 and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    assert f" f32={72 | (2 if out_f32 else 0)} " in open(p["done"]).readline()
    # it is not the non-periodic run's answer
    plain, _, _, _ = run(tmp_path, "plain", tmp_path / "frames.xtc", radii, alg, xtc=True, out_f32=out_f32)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"]))
    # a right-angled box with triclinic=True: the orthorhombic files
    tri, p, done, _ = run(tmp_path, "tri", tmp_path / "frames.xtc", radii, alg, xtc=True, pbc=True, triclinic=True, out_f32=out_f32)
    assert done and tri == got and f" f32={88 | (2 if out_f32 else 0)} " in open(p["done"]).readline()


def exact_triclinic(count, seed=0):
    """float32 boxes in nm, rows a = (ax, 0, 0), b = (0, by, 0), c = (cx, cy, cz), and for each a DCD cell record (the angles as
    cosines) that freesasa_gpu_cell_from_dcd decodes to EXACTLY the box's elements times 10.0: found by trying (a few dozen
    candidates give `count` of them), so that a DCD run and an XTC run see the same cells to the last bit"""
    rng = np.random.default_rng(seed)
    boxes, records = [], []
    for _ in range(100000):
        ax, by, cz = (np.float32(round(rng.uniform(lo, hi), 3)) for lo, hi in ((1.3, 1.6), (1.25, 1.4), (1.15, 1.3)))
        cx, cy = (np.float32(round(rng.uniform(-0.4, 0.4), 3)) for _ in range(2))
        h = np.array([float(ax) * 10.0, 0.0, float(by) * 10.0, float(cx) * 10.0, float(cy) * 10.0, float(cz) * 10.0])
        c0 = float(np.sqrt(h[3] * h[3] + h[4] * h[4] + h[5] * h[5]))
        for c in (c0, float(np.nextafter(c0, 0.0)), float(np.nextafter(c0, 100.0))):
            rec = (h[0], 0.0, h[2], h[3] / c, h[4] / c, c)             # CHARMM's A, gamma, B, beta, alpha, C
            if min(abs(rec[3]), abs(rec[4])) > 1e-6 and np.array_equal(fa.cell_from_dcd(rec), h):
                boxes.append(np.array([[ax, 0, 0], [0, by, 0], [cx, cy, cz]], dtype=np.float32))
                records.append(rec)
                break
        if len(boxes) == count:
            return boxes, records
    raise AssertionError("no exact triclinic cells found")


@pytest.mark.parametrize("alg, out_f32", [("lr20", False), ("sr100", True)])
def test_periodic_triclinic_run_equals_the_dcd_run(tmp_path, alg, out_f32):
    frames, radii = coil(37)
    boxes, records = exact_triclinic(F)
    assert len({tuple(b.reshape(-1)) for b in boxes}) == F and all(b[2, 0] != 0 and b[2, 1] != 0 for b in boxes)
    decoded, _ = xtc_of(tmp_path / "frames.xtc", frames, boxes=boxes)
    dcd = tmp_path / "frames.dcd"
    write_dcd(dcd, decoded, cell=True)
    patch_records(dcd, records)
    want, _, done, _ = run(tmp_path, "dcd", dcd, radii, alg, dcd=True, pbc=True, triclinic=True, out_f32=out_f32)
    got, p, done2, n_frames = run(tmp_path, "xtc", tmp_path / "frames.xtc", radii, alg, xtc=True, pbc=True, triclinic=True, out_f32=out_f32)
    assert done and done2 and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    assert f" f32={88 | (2 if out_f32 else 0)} " in open(p["done"]).readline()
    plain, _, _, _ = run(tmp_path, "plain", tmp_path / "frames.xtc", radii, alg, xtc=True, out_f32=out_f32)
    assert np.all(np.frombuffer(plain["totals"]) > np.frombuffer(got["totals"]))
    # without bit 4 such a file is refused at its first frame; an upper element is refused with it
    with pytest.raises(RuntimeError, match="frame 0 of the XTC file: its cell is not orthorhombic"):
        run(tmp_path, "ortho", tmp_path / "frames.xtc", radii, alg, xtc=True, pbc=True)
    upper = [b.copy() for b in boxes]
    upper[6][0, 2] = 0.25
    xtc_of(tmp_path / "upper.xtc", frames, boxes=upper)
    with pytest.raises(RuntimeError, match=r"frame 6 of the XTC file: element \[0\]\[2\] of its box is 0.25"):
        run(tmp_path, "upper", tmp_path / "upper.xtc", radii, alg, xtc=True, pbc=True, triclinic=True)


def test_a_box_that_touches_nothing_changes_nothing(tmp_path):
    frames, radii = coil(37)
    far = (frames + (500.0 - frames.reshape(-1, 3).mean(0))).astype(np.float32)
    boxes, _ = boxes_nm([(1000.0, 1000.0, 1000.0)] * F)
    xtc_of(tmp_path / "far.xtc", far, boxes=boxes)
    plain, p0, done0, _ = run(tmp_path, "plain", tmp_path / "far.xtc", radii, xtc=True)
    pbc, p1, done1, _ = run(tmp_path, "pbc", tmp_path / "far.xtc", radii, xtc=True, pbc=True)
    tri, p2, done2, _ = run(tmp_path, "tri", tmp_path / "far.xtc", radii, xtc=True, pbc=True, triclinic=True)
    assert done0 and done1 and done2
    assert pbc == plain and tri == plain
    assert len(plain["totals"]) == 8 * F and np.all(np.frombuffer(plain["totals"]) > 0)
    assert [open(p["done"]).readline().split(" f32=")[1].split()[0] for p in (p0, p1, p2)] == ["64", "72", "88"]
    # a frame without a box in a periodic run, and an edge below c: host checks on the staged bytes
    boxes[9] = np.zeros((3, 3), dtype=np.float32)
    xtc_of(tmp_path / "nobox.xtc", far, boxes=boxes)
    with pytest.raises(RuntimeError, match="frame 9 of the XTC file: its box is all zero"):
        run(tmp_path, "nobox", tmp_path / "nobox.xtc", radii, xtc=True, pbc=True)
    boxes[9] = np.diag([100.0, 0.65, 100.0]).astype(np.float32)
    xtc_of(tmp_path / "small.xtc", far, boxes=boxes)
    with pytest.raises(RuntimeError, match=r"frame 9 of the XTC file: edge y of its cell is .* shorter than c"):
        run(tmp_path, "small", tmp_path / "small.xtc", radii, xtc=True, pbc=True)


def test_a_damaged_stream_ends_the_run_and_a_repaired_file_completes_it(tmp_path):
    """frame 5 (of shard 1: frames 4 .. 7) keeps its header and gets a stream with one bit flipped that the CPU emulation of the
    kernels refuses: the device's status ends the run, nothing of the shard is written and it is not listed.  The done-list names
    the frame file by size and modification time: a repair in place that keeps both resumes the run, which ends with the files of
    an uninterrupted one."""
    frames, radii = coil(37)
    good = tmp_path / "good.xtc"
    _, coded = xtc_of(good, frames)
    want, _, done, _ = run(tmp_path, "good", good, radii, xtc=True)
    assert done
    data = good.read_bytes()
    f5 = coded[5]
    for bit in range(8, 8 * f5.bytecount):                     # the first flip whose frame the emulation gives a status
        s = bytearray(f5.stream)
        s[bit >> 3] ^= 0x80 >> (bit & 7)
        mutant = data[f5.offset:f5.offset + xc.HEADER] + bytes(s) + data[f5.offset + xc.HEADER + f5.bytecount:f5.offset + f5.size]
        _, status, _ = xtc_emu.decode(mutant, 1, 37)
        if status[0]:
            break
    assert status[0] and len(mutant) == f5.size
    bad = tmp_path / "frames.xtc"
    bad.write_bytes(data[:f5.offset] + mutant + data[f5.offset + f5.size:])
    assert fa.xtc_info(bad).n_frames == F                       # the headers are whole: only the stream is not
    st = os.stat(bad)
    os.environ["FREESASA_AMD_TRAJ_LANES"] = "1"
    try:
        with pytest.raises(RuntimeError, match="frame 5 of the XTC file is damaged: "):
            run(tmp_path, "bad", bad, radii, xtc=True, device=0)
    finally:
        os.environ.pop("FREESASA_AMD_TRAJ_LANES", None)
    done_path = str(tmp_path / "bad.done")
    assert [int(line.split()[1]) for line in open(done_path).read().splitlines()[1:]] == [0]     # (one lane: the shards go in order)
    assert open(tmp_path / "bad.totals", "rb").read()[:8 * FPB] == want["totals"][:8 * FPB]
    bad.write_bytes(data)
    os.utime(bad, ns=(st.st_atime_ns, st.st_mtime_ns))
    got, p, done, n_frames = run(tmp_path, "bad", bad, radii, xtc=True)
    assert done and n_frames == F and got == want
    assert sorted(int(line.split()[1]) for line in open(done_path).read().splitlines()[1:]) == [0, 1, 2]


def test_resume_and_done_lists_of_other_formats(tmp_path):
    from netcdf_writer import write_amber
    radii, decoded, _ = raw_and_xtc(tmp_path, 37)
    xtc, raw, dcd, nc = tmp_path / "frames.xtc", tmp_path / "frames.f32", tmp_path / "frames.dcd", tmp_path / "frames.nc"
    write_dcd(dcd, decoded, cell=True)
    write_amber(nc, decoded)
    want, _, done, _ = run(tmp_path, "want", raw, radii, f32=True)
    assert done
    a, res = ALGS["lr20"]
    p = {k: str(tmp_path / f"part.{k}") for k in ("totals", "sasa", "done")}
    kw = dict(done_path=p["done"], alg=a, probe=PROBE, resolution=res, frames_per_batch=FPB)
    done, n_frames = fa.trajectory_file(xtc, radii, p["totals"], p["sasa"], xtc=True, max_new_shards=1, **kw)
    assert not done and n_frames == F and open(p["done"]).read().count("shard ") == 1
    done, _ = fa.trajectory_file(xtc, radii, p["totals"], p["sasa"], xtc=True, devices=[0, 0], **kw)
    assert done and open(p["done"]).read().count("shard ") == 3
    assert open(p["totals"], "rb").read() == want["totals"] and open(p["sasa"], "rb").read() == want["sasa"]
    # an XTC run's list is not a raw, a DCD or a NetCDF run's, and the other way round: refused, files untouched
    before = open(p["done"]).read()
    for tag, path, other in (("rawlist", raw, dict(f32=True)), ("dcdlist", dcd, dict(dcd=True)), ("nclist", nc, dict(netcdf=True))):
        with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
            fa.trajectory_file(path, radii, p["totals"], p["sasa"], **other, **kw)
        got, q, done, _ = run(tmp_path, tag, path, radii, **other)
        assert done and got == want
        other_list = open(q["done"]).read()
        with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
            fa.trajectory_file(xtc, radii, q["totals"], q["sasa"], xtc=True, **dict(kw, done_path=q["done"]))
        assert open(q["done"]).read() == other_list and open(q["totals"], "rb").read() == want["totals"]
    assert open(p["done"]).read() == before and open(p["totals"], "rb").read() == want["totals"]
