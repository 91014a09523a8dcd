"""Interfaces between chain groups among periodic images over a trajectory (include/freesasa_gpu.h:
freesasa_gpu_trajectory_file_interfaces_periodic / _interface_residues_periodic; Python: trajectory_file_groups_periodic with
interface_pairs=) on the device, against the features the run composes: the groups' periodic run for every shared output, the
periodic batch entry (calc_periodic / calc_periodic_triclinic) on the pair structures cut on the host for every row and every
residue segment, the run without cells where no cell makes an image - and the split complex, whose buried area the run without
cells loses.

The system is tests/test_groups_pbc_gpu.py's: 2jo4, its four chains a group each, 5 jittered fp32 frames astride the faces at 0,
each frame's own cell, frames_per_batch = 2 (a short last shard).  All six pairs."""
import os

import numpy as np
import pytest

import freesasa_amd as fa
import groups_pbc_ref as gr
import traj_interface_residues_ref as tq
import traj_interfaces_ref as tr
from freesasa_amd import ingest
from test_dcd import write_dcd
from test_pbc_gpu import patch_cells
from test_pbc_tri_gpu import patch_records
from test_traj_groups_gpu import COMMANDS
from test_traj_stats import partial_ref, same_bits
from test_xtc_gpu import boxes_nm, xtc_of

pytestmark = pytest.mark.gpu

PROBE = gr.PROBE
ALGS = {"lr20": (fa.LEE_RICHARDS, 20), "sr100": (fa.SHRAKE_RUPLEY, 100)}
F, FPB, G, N = 5, 2, 4, 516
PAIRS = tr.all_pairs(G)
K = len(PAIRS)
SHARED = ("totals", "sasa", "iso", "groups", "cls", "res", "sel")
MIN_BURIED = 5.0                                 # A^2: the positive threshold of the in_interface column
_SYS, _RUNS = {}, {}


def kw(alg):
    a, res = ALGS[alg]
    return dict(alg=a, probe=PROBE, resolution=res)


@pytest.fixture(scope="module")
def sel():
    s = ingest.Selection(COMMANDS)
    yield s
    s.close()


def system():
    """2jo4, its four chains a group each, 5 jittered fp32 frames astride the faces at 0, each frame's own cell"""
    if not _SYS:
        b = ingest.load_pdb_files([os.path.join(gr.PDB, "2jo4.pdb")])
        ids = np.asarray(b.chain_groups(separate_chains=True)[0], dtype=np.int32)
        assert b.n_atoms == N and np.array_equal(ids, np.repeat(np.arange(G, dtype=np.int32), 129))
        rng = np.random.default_rng(20261019)
        x0 = np.asarray(b.xyz, dtype=np.float64).reshape(-1, 3)
        frames = (x0[None] + rng.uniform(-0.3, 0.3, (F,) + x0.shape)).astype(np.float32)
        ext = np.ceil(x0.max(0) - x0.min(0)) + 3.0
        cells = [(float(ext[0]) + 0.5 * f, float(ext[1]), float(ext[2]) - 0.25 * f) for f in range(F)]
        first, seg_res, seg_side, pside, psrc = tq.segments(ids, G, PAIRS, np.asarray(b.res_first[:b.res_offsets[1] + 1], np.int64))
        pfirst, psrc2 = tr.cut(ids, PAIRS)
        assert np.array_equal(psrc, psrc2) and psrc.size == 2 * 129 * K
        _SYS.update(b=b, ids=ids, frames=frames, cells=cells, seg_first=first, psrc=psrc, pfirst=pfirst, S=seg_res.size)
    return _SYS


def container(tmp, kind):
    """the system's frames as a file -> (path, what the file's frames decode to [F, n, 3] float32, the cells the run reads - three
    edges, or with "tri" six numbers of a skewed cell -, the container's keywords)"""
    s = system()
    if kind == "xtc":
        path = tmp / "frames.xtc"
        boxes, cells = boxes_nm(s["cells"])
        frames, _ = xtc_of(path, s["frames"], boxes=boxes)
        return path, frames, cells, dict(xtc=True)
    path = tmp / f"frames.{kind}.dcd"
    write_dcd(path, s["frames"], cell=True)
    if kind == "tri":
        recs = [(lx, 80.0 + f, ly, 95.0, 92.0 - f, lz) for f, (lx, ly, lz) in enumerate(s["cells"])]
        patch_records(path, recs)
        return path, s["frames"], [fa.cell_from_dcd(r) for r in recs], dict(dcd=True, triclinic=True)
    patch_cells(path, s["cells"])
    return path, s["frames"], s["cells"], dict(dcd=True)


def file_run(tmp, tag, path, alg, how, sel=None, pairs="all", residues=True, min_buried=0.0, **more):
    """the run with every output into a file of its own -> ({output: path}, complete)"""
    s = system()
    p = {k: str(tmp / f"{tag}.{k}") for k in SHARED + ("pairs", "pres", "done")}
    extra = {} if pairs is None else dict(interface_pairs=pairs, pair_areas_path=p["pairs"])
    if pairs is not None and residues:
        extra.update(pair_residues_path=p["pres"], min_buried=min_buried)
    done, n_frames, _ = fa.trajectory_file_groups_periodic(path, s["b"], p["totals"], sasa_path=p["sasa"], group=s["ids"], n_groups=G,
                                                           group_areas_path=p["groups"], isolated_path=p["iso"], class_sums_path=p["cls"],
                                                           residues_path=p["res"], selection=sel, selections_path=p["sel"] if sel else None,
                                                           frames_per_batch=FPB, **kw(alg), **how, **dict(extra, **more))
    assert n_frames == F
    return p, done


def read(p, k, shape=(F, -1)):
    return np.fromfile(p[k], dtype=np.float64).reshape(shape)


def pair_part_areas(frames, cells, alg, tri=False):
    """[F, n_pair]: per frame the K pair structures cut on the host, as a batch through the periodic entry with the frame's cell
    repeated - and the image counts [F, K]"""
    s = system()
    psrc, pfirst, radii = s["psrc"], s["pfirst"], np.asarray(s["b"].radii, np.float64)
    call = fa.calc_periodic_triclinic if tri else fa.calc_periodic
    out, images = [], []
    for f in range(F):
        a, _, k = call(frames[f].astype(np.float64)[psrc], radii[psrc], pfirst, [cells[f]] * K, **kw(alg))
        out.append(a); images.append(k)
    return np.array(out), np.array(images)


def run_and_reference(tmp_factory, sel, kind, alg):
    """once per (container, algorithm): the groups' periodic run without pairs, the run with all pairs and their residues at
    min_buried = 0, and the periodic entry on the pair structures"""
    if (kind, alg) not in _RUNS:
        tmp = tmp_factory.mktemp(f"{kind}_{alg}")
        path, frames, cells, how = container(tmp, kind)
        without, done0 = file_run(tmp, "groups", path, alg, how, sel, pairs=None)
        got, done1 = file_run(tmp, "pairs", path, alg, how, sel)
        assert done0 and done1
        areas, images = pair_part_areas(frames, cells, alg, tri=kind == "tri")
        assert np.all(images > 0), "the pair structures do not reach the faces"
        _RUNS[(kind, alg)] = dict(without=without, got=got, areas=areas, path=path, how=how, frames=frames, cells=cells)
    return _RUNS[(kind, alg)]


# 1
@pytest.mark.parametrize("kind, alg", [("dcd", "lr20"), ("xtc", "sr100")])
def test_the_shared_outputs_are_the_groups_periodic_runs(tmp_path_factory, sel, kind, alg):
    r = run_and_reference(tmp_path_factory, sel, kind, alg)
    for k in SHARED:
        a, b = open(r["got"][k], "rb").read(), open(r["without"][k], "rb").read()
        assert len(a) > 0 and a == b, k
    assert os.path.getsize(r["got"]["pairs"]) == 8 * F * K * 6 and os.path.getsize(r["got"]["pres"]) == 8 * F * system()["S"] * 4
    assert not os.path.exists(r["without"]["pairs"])


# 2
@pytest.mark.parametrize("kind, alg", [("dcd", "lr20"), ("xtc", "sr100"), ("tri", "lr20")])
def test_every_row_is_the_periodic_entry_on_the_pair_structure(tmp_path_factory, sel, kind, alg):
    s = system()
    r = run_and_reference(tmp_path_factory, sel, kind, alg)
    groups, pairs = read(r["got"], "groups", (F, G, 3)), read(r["got"], "pairs", (F, K, 6))
    want = np.stack([tr.frame_rows(s["ids"], PAIRS, groups[f, :, 0], r["areas"][f]) for f in range(F)])
    for c, name in enumerate(("iso_g", "iso_h", "in_pair_g", "in_pair_h", "buried_g", "buried_h")):
        assert np.all(pairs[:, :, c] == want[:, :, c]), (name, np.argwhere(pairs[:, :, c] != want[:, :, c])[:5])
    assert np.array_equal(pairs, want)
    # not vacuous: chains of a thousand A^2 and more that bury area in their pairs
    assert np.all(pairs[:, :, 0] > 1000.0) and pairs[:, :, 4:].max() > 100.0


# 3
@pytest.mark.parametrize("kind, alg", [("dcd", "lr20"), ("xtc", "sr100")])
def test_the_pair_residues_are_the_restatement(tmp_path_factory, tmp_path, sel, kind, alg):
    s = system()
    r = run_and_reference(tmp_path_factory, sel, kind, alg)
    iso = read(r["got"], "iso", (F, N))

    def table(mb):
        return np.stack([tq.frame_table(iso[f], r["areas"][f], s["seg_first"], s["psrc"], mb) for f in range(F)])

    got, want = read(r["got"], "pres", (F, s["S"], 4)), table(0.0)
    for c, name in enumerate(("iso_res", "in_pair_res", "buried_res", "in_interface")):
        assert np.all(got[:, :, c] == want[:, :, c]), (name, np.argwhere(got[:, :, c] != want[:, :, c])[:5])
    assert np.array_equal(got[:, :, 3], (got[:, :, 2] > 0.0).astype(np.float64))                  # strict >
    assert 0 < got[:, :, 3].sum() < got[:, :, 3].size
    if kind != "dcd":
        return
    # ... and at a positive threshold: the three areas the same, the flags by the same strict >
    p, done = file_run(tmp_path, "mb", r["path"], alg, r["how"], min_buried=MIN_BURIED)
    pos = read(p, "pres", (F, s["S"], 4))
    assert done and np.array_equal(pos, table(MIN_BURIED)) and np.array_equal(pos[:, :, :3], got[:, :, :3])
    assert np.array_equal(pos[:, :, 3], (pos[:, :, 2] > MIN_BURIED).astype(np.float64))
    assert 0 < pos[:, :, 3].sum() < got[:, :, 3].sum()
    assert open(p["pairs"], "rb").read() == open(r["got"]["pairs"], "rb").read()


# 4
@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_a_cell_that_touches_nothing_gives_the_files_of_the_run_without_cells(tmp_path, alg):
    s = system()
    b, ids = s["b"], s["ids"]
    far = (s["frames"].astype(np.float64) + (500.0 - np.round(s["frames"].astype(np.float64).mean((0, 1))))).astype(np.float32)
    assert far.min() > 100.0 and far.max() < 900.0
    cells = [(1000.0, 1000.0, 1000.0)] * F
    path = tmp_path / "far.dcd"
    write_dcd(path, far, cell=True)
    patch_cells(path, cells)
    _, _, images = fa.calc_periodic(far.astype(np.float64).reshape(-1, 3), np.tile(b.radii, F), np.arange(F + 1) * N, cells, **kw(alg))
    _, k_images = pair_part_areas(far, cells, alg)
    assert not images.any() and not k_images.any()
    p, done = file_run(tmp_path, "pbc", path, alg, dict(dcd=True))
    q = {k: str(tmp_path / f"plain.{k}") for k in ("totals", "groups", "pairs", "pres")}
    done2, n_frames, _ = fa.trajectory_file_topology(path, b, q["totals"], group=ids, n_groups=G, group_areas_path=q["groups"], dcd=True,
                                                     frames_per_batch=FPB, interface_pairs="all", pair_areas_path=q["pairs"],
                                                     pair_residues_path=q["pres"], **kw(alg))
    assert done and done2 and n_frames == F
    for k in ("pairs", "pres", "groups", "totals"):
        a = open(p[k], "rb").read()
        assert len(a) > 0 and a == open(q[k], "rb").read(), k


# 5
def test_the_split_complex(tmp_path):
    """chains A and B of 2jo4 on a grid of 2^-10 A in a cube of 128 A, two frames of a DCD: whole and mid-cell - and with chain B one
    cell vector further along x, an exact shift.  Among periodic images the two frames are the same system; the run without cells
    finds no interface in the second."""
    xyz, radii, ids = gr.dimer()
    keep = []                                             # the topology: chains A and B of the file's first model as a file of their own
    for ln in open(os.path.join(gr.PDB, "2jo4.pdb")):
        if ln.startswith("ENDMDL"):
            break
        if ln[:6] in ("ATOM  ", "HETATM") and ln[21] in "AB":
            keep.append(ln)
    (tmp_path / "dimer.pdb").write_text("".join(keep) + "END\n")
    b = ingest.load_pdb_files([str(tmp_path / "dimer.pdb")])
    assert b.n_atoms == 258 and np.array_equal(np.asarray(b.radii), radii) and np.array_equal(ids, np.repeat([0, 1], 129))
    L = 128.0
    whole = (np.round((xyz + 64.0) * 1024.0) / 1024.0).astype(np.float32)
    moved = whole.copy()
    moved[ids == 1, 0] += np.float32(L)
    assert np.array_equal(whole.astype(np.float64), np.round((xyz + 64.0) * 1024.0) / 1024.0)          # fp32 holds the grid
    assert np.array_equal(moved[ids == 1, 0] - np.float32(L), whole[ids == 1, 0])
    path = tmp_path / "split.dcd"
    write_dcd(path, np.stack([whole, moved]), cell=True)
    patch_cells(path, [(L, L, L)] * 2)
    p = {k: str(tmp_path / k) for k in ("totals", "groups", "pairs", "t0", "g0", "p0")}
    ids32 = ids.astype(np.int32)
    done, n_frames, _ = fa.trajectory_file_groups_periodic(path, b, p["totals"], group=ids32, n_groups=2, group_areas_path=p["groups"], dcd=True,
                                                           interface_pairs=[(0, 1)], pair_areas_path=p["pairs"], probe=PROBE)
    assert done and n_frames == 2
    rows = np.fromfile(p["pairs"]).reshape(2, 6)
    print("rows among periodic images:", rows, "max |whole - moved| = %.3e A^2" % np.max(np.abs(rows[0] - rows[1])))
    assert np.max(np.abs(rows[0] - rows[1])) <= 2e-8
    assert np.all(rows[:, 4:] > 100.0)
    # the failure the feature removes: the same frames without cells
    done, _, _ = fa.trajectory_file_topology(path, b, p["t0"], group=ids32, n_groups=2, group_areas_path=p["g0"], dcd=True,
                                             interface_pairs=[(0, 1)], pair_areas_path=p["p0"], probe=PROBE)
    plain = np.fromfile(p["p0"]).reshape(2, 6)
    print("rows without cells:", plain)
    assert done and np.all(plain[0, 4:] > 100.0)
    assert abs(plain[1, 4]) <= 129 * 2.0 ** -53 * plain[1, 0] and abs(plain[1, 5]) <= 129 * 2.0 ** -53 * plain[1, 1]


# 6
def test_driver_properties(tmp_path_factory, tmp_path, sel):
    s = system()
    b, ids = s["b"], s["ids"]
    r = run_and_reference(tmp_path_factory, sel, "dcd", "lr20")
    path, how, want = r["path"], r["how"], r["got"]
    kinds = SHARED[:4] + ("cls", "res", "pairs", "pres")
    same = lambda p: all(open(p[k], "rb").read() == open(want[k], "rb").read() for k in kinds)
    # in two calls - one shard, then the rest
    q, done = file_run(tmp_path, "part", path, "lr20", how, done_path=str(tmp_path / "part.done"), max_new_shards=1)
    assert not done and open(q["done"]).read().count("shard ") == 1
    q, done = file_run(tmp_path, "part", path, "lr20", how, done_path=str(tmp_path / "part.done"))
    assert done and open(q["done"]).read().count("shard ") == 3 and same(q)
    head = open(q["done"]).readline()
    assert " pairs=" in head and " minburied=" in head and " f32=%d " % (fa.FRAMES_DCD | fa.FRAMES_PBC) in head
    # a right-angled cell read as a triclinic one; one device named twice
    t, done = file_run(tmp_path, "tri", path, "lr20", dict(how, triclinic=True))
    assert done and same(t)
    d, done = file_run(tmp_path, "dev", path, "lr20", how, devices=[0, 0])
    assert done and same(d)
    # the done-list of the run without cells, and this run's for other pairs: refused, nothing written
    before = {k: open(q[k], "rb").read() for k in kinds + ("done",)}
    plain = {k: str(tmp_path / f"plain.{k}") for k in ("totals", "groups", "pairs", "pres", "done")}
    done, _, _ = fa.trajectory_file_topology(path, b, plain["totals"], group=ids, n_groups=G, group_areas_path=plain["groups"], frames_per_batch=FPB,
                                             interface_pairs="all", pair_areas_path=plain["pairs"], pair_residues_path=plain["pres"], min_buried=0.0,
                                             done_path=plain["done"], **kw("lr20"), **how)
    assert done
    kept = {k: open(plain[k], "rb").read() for k in plain}
    with pytest.raises(RuntimeError, match="done-list belongs"):
        fa.trajectory_file_groups_periodic(path, b, plain["totals"], group=ids, n_groups=G, group_areas_path=plain["groups"], frames_per_batch=FPB,
                                           interface_pairs="all", pair_areas_path=plain["pairs"], pair_residues_path=plain["pres"], min_buried=0.0,
                                           done_path=plain["done"], **kw("lr20"), **how)
    assert kept == {k: open(plain[k], "rb").read() for k in plain}
    for other in (dict(pairs=PAIRS[:5]), dict(min_buried=MIN_BURIED), dict(residues=False)):
        with pytest.raises(RuntimeError, match="done-list belongs"):
            file_run(tmp_path, "part", path, "lr20", how, done_path=str(tmp_path / "part.done"), **other)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        file_run(tmp_path, "part", path, "lr20", dict(how, triclinic=True), done_path=str(tmp_path / "part.done"))
    assert before == {k: open(q[k], "rb").read() for k in before}
    # the statistics of both pair outputs: the shards' partials by the definition on the delivered tables, merged by the library
    st, done = file_run(tmp_path, "stats", path, "lr20", how, stats=("pairs", "pair_residues"), stats_path=str(tmp_path / "stats.stats"),
                        partials_path=str(tmp_path / "stats.parts"))
    assert done and same(st)
    cols = np.concatenate([read(want, "pairs"), read(want, "pres")], axis=1)
    parts = np.stack([partial_ref(cols[0:2]), partial_ref(cols[2:4]), partial_ref(cols[4:5])])
    got = fa.traj_stats_read(str(tmp_path / "stats.stats"), ("pairs", "pair_residues"), N, n_groups=G, partials_path=str(tmp_path / "stats.parts"),
                             frames=[2, 2, 1], n_pairs=K, n_segments=s["S"])
    assert same_bits(got.partials, parts) and same_bits(got.raw, fa.traj_stats_merge(parts, [2, 2, 1]))
    assert got["pairs"].shape == (4, K, 6) and got["pair_residues"].shape == (4, s["S"], 4)
