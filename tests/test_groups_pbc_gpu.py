"""Chain groups among periodic images on the device (include/freesasa_gpu.h: freesasa_gpu_calc_groups_periodic and its kin,
freesasa_gpu_trajectory_file_groups_periodic) against the two features they compose: the periodic entries on the same batch and
on the groups cut out on the host, the chain-group entry where no image is made, and per frame of a trajectory the batch entry."""
import os

import numpy as np
import pytest

import freesasa_amd as fa
import groups_pbc_ref as gr
from freesasa_amd import ingest
from test_dcd import write_dcd
from test_pbc_gpu import patch_cells
from test_traj_stats import partial_ref, same_bits
from test_xtc_gpu import boxes_nm, xtc_of

pytestmark = pytest.mark.gpu

PROBE = gr.PROBE
ALGS = {"lr20": (fa.LEE_RICHARDS, 20), "sr100": (fa.SHRAKE_RUPLEY, 100)}
_GOT = {}


@pytest.fixture(scope="module")
def gb():
    return gr.gpu_batch()


def kw(alg):
    a, res = ALGS[alg]
    return dict(alg=a, probe=PROBE, resolution=res)


def periodic_groups(gb, alg):
    """calc_groups_periodic on the batch, once per algorithm"""
    if alg not in _GOT:
        xyz, radii, offsets, group, n_groups, cells = gb
        _GOT[alg] = fa.calc_groups_periodic(xyz, radii, offsets, group, n_groups, cells, **kw(alg))
    return _GOT[alg]


def totals_ref(areas, offsets):
    """the totals kernels restated (csrc/sasa_kernels.h, totals_chunk_phase0 / _phase1, totals_struct): per chunk of 4096 atoms of
    a structure 256 threads add every 256th area, thread 0 adds the 256 sums in order; a structure adds its chunks in order"""
    out = np.zeros(len(offsets) - 1)
    for s in range(len(offsets) - 1):
        t = 0.0
        for b in range(int(offsets[s]), int(offsets[s + 1]), 4096):
            chunk = areas[b:min(b + 4096, int(offsets[s + 1]))]
            part = np.zeros(256)
            for i0 in range(0, chunk.size, 256):
                row = chunk[i0:i0 + 256]
                part[:row.size] = part[:row.size] + row
            c = 0.0
            for p in part:
                c = c + p
            t = t + c
        out[s] = t
    return out


def test_the_batch_is_the_issues(gb):
    xyz, radii, offsets, group, n_groups, cells = gb
    assert list(np.diff(offsets)) == [516, 400, 0, 300, 600, 5] and list(n_groups) == [4, 0, 1, 4, 3, 2]
    comb, src, gbase, cplx = gr.cut(offsets, group, n_groups)
    assert list(np.diff(comb)[6:]) == [129, 129, 129, 129, 0, 257, 0, 1, 30, 200, 200, 200, 1, 4]
    c = 6.8
    assert c <= cells[3][0] < 2 * c and all(c <= e < 2 * c for e in cells[5])
    assert (group[offsets[3]:offsets[4]] == -1).sum() == 12 and np.all(group[offsets[1]:offsets[2]] == -1)


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_complex_areas_are_the_periodic_entrys(gb, alg):
    xyz, radii, offsets, group, n_groups, cells = gb
    sasa, iso, totals, gt, images = periodic_groups(gb, alg)
    w_sasa, w_totals, w_images = fa.calc_periodic(xyz, radii, offsets, cells, **kw(alg))
    assert sasa.tobytes() == w_sasa.tobytes() and totals.tobytes() == w_totals.tobytes() and np.array_equal(images, w_images)
    assert np.all(images[[0, 1, 3, 4]] > 0) and images[2] == 0 and images[5] >= 26
    # ... and not the chain-group entry's: the images bury area
    plain = fa.calc_groups(xyz, radii, offsets, group, n_groups, **kw(alg))
    print("totals without images", plain[2], "among images", totals)
    assert np.all(plain[2][[0, 1, 3, 4, 5]] > totals[[0, 1, 3, 4, 5]]) and np.all(totals[[0, 1, 3, 4]] > 1000.0)
    assert np.all(plain[2][[1, 3, 4]] > totals[[1, 3, 4]] + 100.0)


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_isolated_areas_are_the_periodic_entrys_on_the_groups_cut_out(gb, alg):
    xyz, radii, offsets, group, n_groups, cells = gb
    sasa, iso, totals, gt, _ = periodic_groups(gb, alg)
    gx, gradii, goff, gcells, src = gr.group_structures(xyz, radii, offsets, group, n_groups, cells)
    w_sasa, w_totals, w_images = fa.calc_periodic(gx, gradii, goff, gcells, **kw(alg))
    assert iso[src].tobytes() == w_sasa.tobytes() and gt[:, 0].tobytes() == w_totals.tobytes()
    free = group < 0
    assert free.sum() == 412 and iso[free].tobytes() == sasa[free].tobytes()
    assert w_images[12] == 26                                        # the group of one atom mid-cell: all 26 images on its own
    # complex totals and buried areas: the group entry's reduction - the totals kernels over the gathered complex areas -
    # applied to the periodic areas; the restatement of that reduction is first held to the existing path's own bytes
    plain = fa.calc_groups(xyz, radii, offsets, group, n_groups, **kw(alg))
    assert totals_ref(plain[0][src], goff).tobytes() == plain[3][:, 1].tobytes()
    assert totals_ref(plain[0], offsets).tobytes() == plain[2].tobytes()
    assert totals_ref(sasa[src], goff).tobytes() == gt[:, 1].tobytes()
    assert (gt[:, 0] - gt[:, 1]).tobytes() == gt[:, 2].tobytes()
    print("group totals (isolated, complex, buried)", gt)
    assert np.all(gt[[4, 6]] == 0.0) and np.all(gt[[0, 1, 2, 3, 5, 8, 9, 10, 11], 2] > 1.0)      # empty groups; groups that bury area


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_a_cell_that_touches_nothing_gives_the_group_entrys_bytes(gb, alg):
    """every structure moved into a cell so large and so placed that no atom comes within c of a face"""
    xyz, radii, offsets, group, n_groups, _ = gb
    far = xyz.copy()
    for s in range(6):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if b > a:
            far[a:b] += 500.0 - np.round(far[a:b].mean(0))
    cells = np.full((6, 3), 1000.0)
    assert far.min() > 100.0 and far.max() < 900.0
    got = fa.calc_groups_periodic(far, radii, offsets, group, n_groups, cells, **kw(alg))
    want = fa.calc_groups(far, radii, offsets, group, n_groups, **kw(alg))
    assert not got[4].any()
    for g, w, name in zip(got, want, ("sasa", "iso", "totals", "group totals")):
        assert g.tobytes() == w.tobytes(), name


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_triclinic_entries(gb, alg):
    xyz, radii, offsets, group, n_groups, cells = gb
    want = periodic_groups(gb, alg)
    right = np.zeros((6, 6))
    right[:, 0], right[:, 2], right[:, 5] = cells[:, 0], cells[:, 1], cells[:, 2]
    got = fa.calc_groups_periodic_triclinic(xyz, radii, offsets, group, n_groups, right, **kw(alg))
    for g, w, name in zip(got, want, ("sasa", "iso", "totals", "group totals", "images")):
        assert g.tobytes() == w.tobytes(), name                        # right-angled cells: the orthorhombic entry's bytes
    # a skewed cell for the 600 atoms (widths 37.5, 29.9, 33): the triclinic periodic entry on the batch and on the groups cut out
    skew = right.copy()
    skew[4] = (38.0, 5.0, 30.0, -3.0, 2.0, 33.0)
    sasa, iso, totals, gt, images = fa.calc_groups_periodic_triclinic(xyz, radii, offsets, group, n_groups, skew, **kw(alg))
    w_sasa, w_totals, w_images = fa.calc_periodic_triclinic(xyz, radii, offsets, skew, **kw(alg))
    assert sasa.tobytes() == w_sasa.tobytes() and totals.tobytes() == w_totals.tobytes() and np.array_equal(images, w_images)
    assert not np.array_equal(sasa[offsets[4]:], want[0][offsets[4]:])
    gx, gradii, goff, gcells, src = gr.group_structures(xyz, radii, offsets, group, n_groups, skew)
    w_sasa, w_totals, _ = fa.calc_periodic_triclinic(gx, gradii, goff, gcells, **kw(alg))
    assert iso[src].tobytes() == w_sasa.tobytes() and gt[:, 0].tobytes() == w_totals.tobytes()
    assert gt[:, 1].tobytes() == totals_ref(sasa[src], goff).tobytes()


def test_device_pointer_entries(gb):
    import torch
    xyz, radii, offsets, group, n_groups, cells = gb
    want = periodic_groups(gb, "lr20")
    dev = torch.device("cuda:0")
    n, G = len(radii), int(n_groups.sum())
    d_xyz, d_r, d_g = torch.from_numpy(xyz).to(dev), torch.from_numpy(radii).to(dev), torch.from_numpy(group).to(dev)
    d_sasa, d_iso = (torch.full((n,), np.nan, dtype=torch.float64, device=dev) for _ in range(2))
    d_tot, d_gt = torch.empty(6, dtype=torch.float64, device=dev), torch.empty(3 * G, dtype=torch.float64, device=dev)
    right = np.zeros((6, 6))
    right[:, 0], right[:, 2], right[:, 5] = cells[:, 0], cells[:, 1], cells[:, 2]
    ctx = fa.GpuContext(0)
    try:
        for call, c in ((ctx.groups_periodic, cells), (ctx.groups_periodic_triclinic, right)):
            images = call(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_g.data_ptr(), n_groups, c, d_sasa.data_ptr(), d_iso.data_ptr(),
                          d_tot.data_ptr(), d_gt.data_ptr(), probe=PROBE)
            got = (d_sasa.cpu().numpy(), d_iso.cpu().numpy(), d_tot.cpu().numpy(), d_gt.cpu().numpy().reshape(-1, 3), images)
            for g, w, name in zip(got, want, ("sasa", "iso", "totals", "group totals", "images")):
                assert g.tobytes() == w.tobytes(), name
        # the device's own checks: a bad id with the group entry's message, a short edge naming the complex; the context stays usable
        bad = group.copy()
        bad[700] = 7
        with pytest.raises(RuntimeError, match=r"atom 700 \(structure 1\) has group id 7: ids are -1 .. n_groups\[s\] - 1 = -1"):
            ctx.groups_periodic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, torch.from_numpy(bad).to(dev).data_ptr(), n_groups, cells,
                                d_sasa.data_ptr(), d_iso.data_ptr(), probe=PROBE)
        short = cells.copy()
        short[3][0] = 6.8 - 0.01
        with pytest.raises(RuntimeError, match=r"structure 3: edge x .* shorter than c"):
            ctx.groups_periodic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_g.data_ptr(), n_groups, short, d_sasa.data_ptr(),
                                d_iso.data_ptr(), probe=PROBE)
        ctx.groups_periodic(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_g.data_ptr(), n_groups, cells, d_sasa.data_ptr(), d_iso.data_ptr(),
                            probe=PROBE)
        assert d_iso.cpu().numpy().tobytes() == want[1].tobytes()
    finally:
        ctx.close()


def test_the_split_complex():
    """chains A and B of 2jo4 on a grid of 2^-10 A in a cube of 128 A: whole, mid-cell - and with chain B one cell vector further
    along x, an exact shift.  Among periodic images the two are the same system; without them the moved copy buries nothing."""
    xyz, radii, ids = gr.dimer()
    L = 128.0
    whole = np.round((xyz + 64.0) * 1024.0) / 1024.0
    moved = whole.copy()
    moved[ids == 1, 0] += L
    assert np.array_equal(moved[ids == 1, 0] - L, whole[ids == 1, 0])
    args = ([0, len(radii)], ids, [2])
    a = fa.calc_groups_periodic(whole, radii, *args, [(L, L, L)], probe=PROBE)
    b = fa.calc_groups_periodic(moved, radii, *args, [(L, L, L)], probe=PROBE)
    for x, y, name in zip(a[:4], b[:4], ("sasa", "iso", "totals", "group totals")):
        print(f"{name}: max |whole - moved| = {np.max(np.abs(x - y)):.3e} A^2")
        assert np.max(np.abs(x - y)) <= 2e-8, name
    assert np.all(a[3][:, 2] > 100.0) and a[4][0] == 0 and b[4][0] == 0
    # the failure the feature removes
    plain = fa.calc_groups(moved, radii, *args, probe=PROBE)
    assert np.all(plain[3][:, 2] == 0.0)
    assert np.max(np.abs(fa.calc_groups(whole, radii, *args, probe=PROBE)[3] - a[3])) <= 2e-8


def test_results_do_not_depend_on_the_tile_shape_or_on_the_batch(gb, monkeypatch):
    xyz, radii, offsets, group, n_groups, cells = gb
    want = periodic_groups(gb, "lr20")
    monkeypatch.setenv("FREESASA_AMD_LR2", "3,0,-1,0")
    fa.lib().freesasa_gpu_release_pool()
    got = fa.calc_groups_periodic(xyz, radii, offsets, group, n_groups, cells, **kw("lr20"))
    monkeypatch.delenv("FREESASA_AMD_LR2")
    fa.lib().freesasa_gpu_release_pool()
    for g, w, name in zip(got, want, ("sasa", "iso", "totals", "group totals", "images")):
        assert g.tobytes() == w.tobytes(), name
    gbase = np.concatenate([[0], np.cumsum(n_groups)])
    for alg in ("lr20", "sr100"):
        want = periodic_groups(gb, alg)
        for s in (0, 3, 4, 5):
            a, b = int(offsets[s]), int(offsets[s + 1])
            one = fa.calc_groups_periodic(xyz[a:b], radii[a:b], [0, b - a], group[a:b], n_groups[s:s + 1], cells[s:s + 1], **kw(alg))
            assert one[0].tobytes() == want[0][a:b].tobytes() and one[1].tobytes() == want[1][a:b].tobytes()
            assert one[2][0] == want[2][s] and one[3].tobytes() == want[3][gbase[s]:gbase[s + 1]].tobytes() and one[4][0] == want[4][s]


# ---------------------------------------------------------------- the trajectory run

F, FPB = 5, 2
KINDS = ("totals", "sasa", "iso", "groups")
_SYS = {}


def system():
    """2jo4, its four chains a group each, 5 jittered fp32 frames astride the faces at 0, each frame's own cell"""
    if not _SYS:
        b = ingest.load_pdb_files([os.path.join(gr.PDB, "2jo4.pdb")])
        ids = np.asarray(b.chain_groups(separate_chains=True)[0], dtype=np.int32)
        rng = np.random.default_rng(20261019)
        x0 = np.asarray(b.xyz, dtype=np.float64).reshape(-1, 3)
        frames = (x0[None] + rng.uniform(-0.3, 0.3, (F,) + x0.shape)).astype(np.float32)
        ext = np.ceil(x0.max(0) - x0.min(0)) + 3.0
        cells = [(float(ext[0]) + 0.5 * f, float(ext[1]), float(ext[2]) - 0.25 * f) for f in range(F)]
        _SYS.update(b=b, ids=ids, frames=frames, cells=cells)
    return _SYS


def per_frame(frames, cells, b, ids, alg):
    """calc_groups_periodic frame by frame -> {output: bytes of the run's file}"""
    n = int(b.n_atoms)
    rows = [fa.calc_groups_periodic(frames[f].astype(np.float64), b.radii, [0, n], ids, [4], [cells[f]], **kw(alg)) for f in range(F)]
    assert all(r[4][0] > 0 for r in rows), "the frames do not reach the faces"
    return dict(totals=np.array([r[2][0] for r in rows]), sasa=np.array([r[0] for r in rows]), iso=np.array([r[1] for r in rows]),
                groups=np.array([r[3] for r in rows]))


def file_run(tmp, tag, path, b, ids, alg="lr20", **more):
    p = {k: str(tmp / f"{tag}.{k}") for k in KINDS + ("done", "stats", "parts")}
    done, n_frames, _ = fa.trajectory_file_groups_periodic(path, b, p["totals"], sasa_path=p["sasa"], group=ids, n_groups=4,
                                                           group_areas_path=p["groups"], isolated_path=p["iso"], done_path=p["done"],
                                                           frames_per_batch=FPB, **kw(alg), **more)
    return p, done, n_frames


@pytest.mark.parametrize("kind, alg", [("dcd", "lr20"), ("xtc", "sr100"), ("xtc", "lr20")])
def test_every_frame_of_a_run_is_the_batch_entrys(tmp_path, kind, alg):
    s = system()
    b, ids = s["b"], s["ids"]
    if kind == "dcd":
        path, frames, cells, how = tmp_path / "frames.dcd", s["frames"], s["cells"], dict(dcd=True)
        write_dcd(path, frames, cell=True)
        patch_cells(path, cells)
    else:
        path, how = tmp_path / "frames.xtc", dict(xtc=True)
        boxes, cells = boxes_nm(s["cells"])
        frames, _ = xtc_of(path, s["frames"], boxes=boxes)
    want = per_frame(frames, cells, b, ids, alg)
    p, done, n_frames = file_run(tmp_path, "all", path, b, ids, alg, **how)
    assert done and n_frames == F and open(p["done"]).read().count("shard ") == 3          # 2 + 2 + 1 frames
    for k in KINDS:
        assert open(p[k], "rb").read() == np.ascontiguousarray(want[k]).tobytes(), k
    if (kind, alg) != ("dcd", "lr20"):
        return
    # a right-angled cell read as a triclinic one: the same files
    tri, done, _ = file_run(tmp_path, "tri", path, b, ids, alg, triclinic=True, **how)
    assert done and all(open(tri[k], "rb").read() == open(p[k], "rb").read() for k in KINDS)
    # in two calls - one shard, then the rest: the files of the single run, byte for byte
    q, done, _ = file_run(tmp_path, "part", path, b, ids, alg, max_new_shards=1, **how)
    assert not done and open(q["done"]).read().count("shard ") == 1
    q, done, _ = file_run(tmp_path, "part", path, b, ids, alg, **how)
    assert done and open(q["done"]).read().count("shard ") == 3
    for k in KINDS:
        assert open(q[k], "rb").read() == open(p[k], "rb").read(), k
    # fp32 per-atom files: the fp64 values narrowed
    n32, done, _ = file_run(tmp_path, "f32", path, b, ids, alg, out_f32=True, **how)
    assert done and open(n32["sasa"], "rb").read() == want["sasa"].astype(np.float32).tobytes()
    assert open(n32["iso"], "rb").read() == want["iso"].astype(np.float32).tobytes() and open(n32["groups"], "rb").read() == open(p["groups"], "rb").read()
    # the statistics of the group column: the shards' partials by the definition, merged by the library
    st, done, _ = file_run(tmp_path, "stats", path, b, ids, alg, stats=("groups",), stats_path=str(tmp_path / "stats.stats"),
                           partials_path=str(tmp_path / "stats.parts"), **how)
    assert done and open(st["groups"], "rb").read() == open(p["groups"], "rb").read()
    cols = want["groups"].reshape(F, -1)
    parts = np.stack([partial_ref(cols[0:2]), partial_ref(cols[2:4]), partial_ref(cols[4:5])])
    got = fa.traj_stats_read(st["stats"], ("groups",), int(b.n_atoms), n_groups=4, partials_path=st["parts"], frames=[2, 2, 1])
    assert same_bits(got.partials, parts) and same_bits(got.raw, fa.traj_stats_merge(parts, [2, 2, 1]))
    assert got["groups"].shape == (4, 4, 3)
    # the done-lists of this run, of the plain periodic run and of the non-periodic groups run refuse each other
    before = {k: open(p[k], "rb").read() for k in p if os.path.exists(p[k])}
    topo = lambda tag, **m: fa.trajectory_file_topology(path, b, str(tmp_path / f"{tag}.totals"), sasa_path=str(tmp_path / f"{tag}.sasa"),
                                                        frames_per_batch=FPB, **kw(alg), **how, **m)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        topo("x", done_path=p["done"], pbc=True)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        topo("x", done_path=p["done"], group=ids, n_groups=4, group_areas_path=str(tmp_path / "x.groups"))
    assert topo("pbc", done_path=str(tmp_path / "pbc.done"), pbc=True)[0]
    assert topo("grp", done_path=str(tmp_path / "grp.done"), group=ids, n_groups=4, group_areas_path=str(tmp_path / "grp.groups"),
                isolated_path=str(tmp_path / "grp.iso"))[0]
    for tag in ("pbc", "grp"):
        with pytest.raises(RuntimeError, match="done-list belongs"):
            fa.trajectory_file_groups_periodic(path, b, str(tmp_path / f"{tag}.totals"), sasa_path=str(tmp_path / f"{tag}.sasa"), group=ids,
                                               n_groups=4, group_areas_path=str(tmp_path / f"{tag}.groups"),
                                               isolated_path=str(tmp_path / f"{tag}.iso") if tag == "grp" else None,
                                               done_path=str(tmp_path / f"{tag}.done"), frames_per_batch=FPB, **kw(alg), **how)
    assert before == {k: open(p[k], "rb").read() for k in before}
    # the plain periodic run's per-atom areas and totals are this run's; the non-periodic groups run buries less
    assert open(tmp_path / "pbc.totals", "rb").read() == open(p["totals"], "rb").read()
    assert open(tmp_path / "pbc.sasa", "rb").read() == open(p["sasa"], "rb").read()
    assert open(tmp_path / "grp.groups", "rb").read() != open(p["groups"], "rb").read()
