"""Chain groups among periodic images (include/freesasa_gpu.h: freesasa_gpu_groups_periodic_dev and its kin,
freesasa_gpu_trajectory_file_groups_periodic) without a GPU: the two phase functions of their own (csrc/pbc_kernels.h,
GpbcArgs) and the periodic kernels over the combined batch, driven on the CPU against the numpy restatement
(tests/groups_pbc_ref.py), bit for bit; that restatement's isolated structures against the explicit replica system through the
oracle and the reference library; and the refusals that come before a device is touched or an output file opened."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
import groups_pbc_ref as gr
import pbc_ref
import pbc_tri_ref
from emu import groups_pbc_emu as ge
from test_dcd import write_dcd

PROBE = gr.PROBE


@pytest.fixture(scope="module")
def batch():
    return gr.batch()


def test_the_batch_is_what_the_kernels_can_go_wrong_on(batch):
    xyz, radii, offsets, group, n_groups, cells = batch
    exyz, eradii, eoff, images, comb, src, gbase, cplx = gr.expanded(xyz, radii, offsets, group, n_groups, cells, PROBE)
    assert list(np.diff(offsets)) == [20, 300, 0, 5, 40] and list(n_groups) == [0, 4, 1, 2, 2]      # 0 groups; an empty structure between full ones
    sizes = list(np.diff(comb)[5:])
    assert sizes == [257, 0, 1, 30, 0, 1, 4, 20, 20]                                                   # 257 = PBC_B + 1; 0 atoms; 1 atom
    assert (group[offsets[1]:offsets[2]] == -1).sum() == 12 and np.all(group[:20] == -1)
    assert np.any(np.diff(src[:257]) > 1)                                                              # the cut is no copy
    c = pbc_ref.cutoff(radii[offsets[3]:offsets[4]], PROBE)
    assert c == 6.8 and all(c <= e < 2 * c for e in gr.SMALL_CELL)
    assert images[3] >= 26 and images[5 + 5] == 26                         # the atom mid-cell: all 26 in the complex and on its own
    # a group's cutoff is its own: the four other atoms of structure 3 admit fewer images alone than in the complex
    own = pbc_ref.cutoff(radii[offsets[3] + 1:offsets[4]], PROBE)
    assert own < c and images[5 + 6] < images[3] - 26
    assert list(cplx) == [0, 1, 2, 3, 4, 1, 1, 1, 1, 2, 3, 3, 4, 4] and list(gbase) == [0, 0, 4, 5, 7, 9]


def emulate(batch, cells_dev):
    """the pipeline of the device on the CPU: cells, count and emit over the combined batch -> (expanded batch, eoff, images, ...)"""
    xyz, radii, offsets, group, n_groups, _ = batch
    cxyz, cradii, comb, src, gbase, cplx = gr.combined(xyz, radii, offsets, group, n_groups)
    ccells = ge.cells(cells_dev, comb.size - 1, gbase=gbase)
    return ge.expand(cxyz, cradii, comb, ccells, PROBE) + (ccells, comb, src, gbase, cplx)


@pytest.mark.parametrize("tri", [False, True])
def test_emulated_kernels_equal_the_restatement_bit_for_bit(batch, tri):
    xyz, radii, offsets, group, n_groups, cells = batch
    cells_def = gr.triclinic_cells(cells) if tri else cells
    cells_dev = pbc_tri_ref.cell9(cells_def) if tri else cells
    want_xyz, want_r, want_eoff, want_images, comb, src, gbase, cplx = gr.expanded(xyz, radii, offsets, group, n_groups, cells_def, PROBE)
    got_xyz, got_r, eoff, images, ccells, *_ = emulate(batch, cells_dev)
    # the per-structure cells: every combined structure has its complex's row, bit for bit (NaN rows included)
    assert ccells.tobytes() == np.ascontiguousarray(cells_dev)[cplx].tobytes()
    # the expanded batch: every group among its own images, with its own cutoff
    assert np.array_equal(images, want_images) and np.array_equal(eoff, want_eoff)
    assert got_xyz.tobytes() == want_xyz.tobytes() and got_r.tobytes() == want_r.tobytes()
    if tri:
        assert images[1] != gr.expanded(xyz, radii, offsets, group, n_groups, cells, PROBE)[3][1]      # the skewed cell is another system
    # which expanded slot each real atom's two areas come from: areas that name their slot
    fake = np.arange(eoff[-1], dtype=np.float64) + 0.25
    sasa, iso, carea, cgath = ge.finish(5, comb, eoff, fake, src, group, gbase=gbase)
    slot_sasa, slot_iso = gr.slots(offsets, group, comb, eoff, src)
    assert np.array_equal(sasa, slot_sasa + 0.25) and np.array_equal(iso, slot_iso + 0.25)
    w_sasa, w_iso, w_carea, w_cgath = gr.finish(fake, offsets, group, comb, eoff, src)
    assert np.array_equal(sasa, w_sasa) and np.array_equal(iso, w_iso) and np.array_equal(carea, w_carea) and np.array_equal(cgath, w_cgath)
    assert not np.isnan(carea).any() and not np.isnan(cgath).any() and not np.isnan(iso).any()           # every thread's share is written
    # no area comes from an image
    real = np.concatenate([np.arange(eoff[k], eoff[k] + comb[k + 1] - comb[k]) for k in range(comb.size - 1)])
    assert np.all(np.isin(slot_sasa, real)) and np.all(np.isin(slot_iso, real))


def test_emulated_kernels_on_a_shards_frames():
    """the trajectory lanes' form: nf frames of n atoms, G groups each, the topology's src and ids - against the batch form on the
    frames given as a batch with the ids repeated"""
    n, nf = 37, 3
    rng = np.random.default_rng(4)
    xyz0, radii = pbc_ref.structure(n, (12.0, 14.0, 16.0), 5)
    radii[3] = 2.0
    frames = np.stack([xyz0 + rng.uniform(-0.3, 0.3, xyz0.shape) for _ in range(nf)])
    ids = gr._ids(rng, n, (20, 0, 9), 8)
    cells = np.array([(12.0 + 0.3 * f, 14.0, 16.0 - 0.2 * f) for f in range(nf)])
    G, offsets = 3, np.arange(nf + 1, dtype=np.int64) * n
    # the batch form: the reference
    group, n_groups = np.tile(ids, nf), np.full(nf, G, dtype=np.int32)
    want_xyz, want_r, want_eoff, _, comb_b, src_b, gbase, cplx = gr.expanded(frames.reshape(-1, 3), np.tile(radii, nf), offsets, group, n_groups, cells, PROBE)
    # the shard's combined batch (csrc/traj_kernels.h): frames, then frame-major every group
    _, src_t, _, _ = gr.cut([0, n], ids, [G])
    n_iso = src_t.size
    cxyz = np.vstack([frames.reshape(-1, 3)] + [frames[f][src_t] for f in range(nf)])
    cradii = np.concatenate([np.tile(radii, nf)] + [radii[src_t]] * nf)
    assert np.array_equal(cxyz, np.vstack([frames.reshape(-1, 3), frames.reshape(-1, 3)[src_b]]))        # the same combined batch
    ccells = ge.cells(cells, nf * (1 + G), g_fixed=G)
    assert ccells.tobytes() == cells[cplx].tobytes()
    got_xyz, got_r, eoff, _ = ge.expand(cxyz, cradii, comb_b, ccells, PROBE)
    assert np.array_equal(eoff, want_eoff) and got_xyz.tobytes() == want_xyz.tobytes() and got_r.tobytes() == want_r.tobytes()
    fake = np.arange(eoff[-1], dtype=np.float64) + 0.5
    got = ge.finish(nf, comb_b, eoff, fake, src_t, ids, g_fixed=G, n_fixed=n, n_iso_fixed=n_iso)
    want = ge.finish(nf, comb_b, eoff, fake, src_b, group, gbase=gbase)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert np.array_equal(got[0], gr.finish(fake, offsets, group, comb_b, eoff, src_b)[0])


def test_a_cell_that_touches_nothing_expands_to_the_groups_batch(batch):
    """every coordinate in [0, L) and further than c from every face: the expanded batch IS the chain-group entry's combined batch"""
    xyz, radii, offsets, group, n_groups, _ = batch
    rng = np.random.default_rng(9)
    xyz = rng.uniform(100.0, 900.0, xyz.shape)
    cells = np.full((5, 3), 1000.0)
    cxyz, cradii, comb, *_ = gr.combined(xyz, radii, offsets, group, n_groups)
    got_xyz, got_r, eoff, images, *_ = emulate((xyz, radii, offsets, group, n_groups, None), cells)
    assert not images.any() and np.array_equal(eoff, comb) and got_xyz.tobytes() == cxyz.tobytes() and got_r.tobytes() == cradii.tobytes()


# ---------------------------------------------------------------- the restatement's isolated structures against replicas

def isolated_cases(batch, which=(3, 5, 6, 7, 8)):
    """(tag, xyz, radii, cell) of the group structures with atoms of structures 3 and 4, and of the 30 atoms of structure 1"""
    xyz, radii, offsets, group, n_groups, cells = batch
    gx, gradii, goff, gcells, _ = gr.group_structures(xyz, radii, offsets, group, n_groups, cells)
    return [(f"group {k}", gx[goff[k]:goff[k + 1]], gradii[goff[k]:goff[k + 1]], gcells[k]) for k in which]


def test_isolated_groups_of_the_restatement_equal_the_explicit_27_replica_system(oracle_lib, batch):
    """an isolated group among ITS images in its complex's cell, with ITS cutoff: the restatement's expanded group structures
    through the oracle against the central cell of the group's 27 replicas - S&R-100 exactly, L&R-20 within 1e-8 A^2 per atom
    (the project's asserted L&R bound)"""
    for tag, x, r, cell in isolated_cases(batch):
        n = r.size
        ex, er, k = pbc_ref.expand(x, r, cell, PROBE)
        rx, rr = pbc_ref.replicas(x, r, cell)
        sr_e, _ = oracle_lib.shrake_rupley(ex, er, PROBE, 100)
        sr_r, _ = oracle_lib.shrake_rupley(rx, rr, PROBE, 100)
        assert np.array_equal(sr_e[:n], sr_r[:n]), tag
        lr_e = oracle_lib.lee_richards(ex, er, PROBE, 20)
        lr_r = oracle_lib.lee_richards(rx, rr, PROBE, 20)
        print(f"{tag}: {n} atoms, {k} images, L&R max |expansion - replicas| = {np.max(np.abs(lr_e[:n] - lr_r[:n])):.3e} A^2")
        assert np.max(np.abs(lr_e[:n] - lr_r[:n])) <= 1e-8, tag


def test_isolated_groups_through_the_reference_library(reference_lib, batch):
    """the same through the reference library itself, where it is built: Shrake-Rupley areas of the real atoms bit for bit,
    Lee-Richards within 1e-8 - the 30 atoms in the (12, 14, 16) cell only: on the expansions or the replicas of the other groups
    (1, 4 and 20 atoms in the (7, 7.5, 8) and (30, 9, 50) cells) the reference library ends in a segmentation fault of its own
    (tests/test_pbc.py met it first), which would take the test session with it"""
    for tag, x, r, cell in isolated_cases(batch, (3,)):
        n = r.size
        ex, er, _ = pbc_ref.expand(x, r, cell, PROBE)
        rx, rr = pbc_ref.replicas(x, r, cell)
        a = reference_lib.calc_coord(ex, er, alg=fa.SHRAKE_RUPLEY, probe=PROBE, n_points=100)[0]
        b = reference_lib.calc_coord(rx, rr, alg=fa.SHRAKE_RUPLEY, probe=PROBE, n_points=100)[0]
        assert np.array_equal(a[:n], b[:n]), tag
        a = reference_lib.calc_coord(ex, er, alg=fa.LEE_RICHARDS, probe=PROBE, n_slices=20)[0]
        b = reference_lib.calc_coord(rx, rr, alg=fa.LEE_RICHARDS, probe=PROBE, n_slices=20)[0]
        assert np.max(np.abs(a[:n] - b[:n])) <= 1e-8, tag


# ---------------------------------------------------------------- refusals that need no device

def test_batch_entries_refuse_before_a_device_is_touched(batch):
    xyz, radii, offsets, group, n_groups, cells = batch
    ok = np.nan_to_num(cells, nan=50.0)
    # a bad cell names the COMPLEX, with the periodic entries' messages
    bad = ok.copy()
    bad[3][1] = 6.8 - 0.01
    with pytest.raises(RuntimeError, match=r"structure 3: edge y .* shorter than c = 2 \(max radius \+ probe\)"):
        fa.calc_groups_periodic(xyz, radii, offsets, group, n_groups, bad, probe=PROBE)
    bad = ok.copy()
    bad[4][2] = np.inf
    with pytest.raises(RuntimeError, match=r"structure 4: edge z .* not finite"):
        fa.calc_groups_periodic(xyz, radii, offsets, group, n_groups, bad, probe=PROBE)
    # a structure without atoms has no cell to check (structure 2's is NaN)
    bad = cells.copy()
    bad[1][0] = 1.0
    with pytest.raises(RuntimeError, match=r"structure 1: edge x"):
        fa.calc_groups_periodic(xyz, radii, offsets, group, n_groups, bad, probe=PROBE)
    tri = gr.triclinic_cells(ok)
    tri[1][2] = -1.0
    with pytest.raises(RuntimeError, match=r"structure 1: entry by .* must be > 0"):
        fa.calc_groups_periodic_triclinic(xyz, radii, offsets, group, n_groups, tri, probe=PROBE)
    tri = gr.triclinic_cells(ok)
    tri[3][0] = 6.0
    with pytest.raises(RuntimeError, match=r"structure 3: width a .* smaller than c"):
        fa.calc_groups_periodic_triclinic(xyz, radii, offsets, group, n_groups, tri, probe=PROBE)
    # the engine's 2^30 limit, from the offsets alone: no array is read (these hold one atom)
    # (through the C entry: the wrapper checks that group holds one id per atom)
    with pytest.raises(RuntimeError, match="expanded batch is too large"):
        _c_entry_refuses_2_30()
    with pytest.raises(ValueError, match="three edges per structure"):
        fa.calc_groups_periodic(xyz, radii, offsets, group, n_groups, ok[:4], probe=PROBE)


def _c_entry_refuses_2_30():
    L = fa.lib()
    one, r, cell = np.zeros(3), np.ones(1), np.full(3, 100.0)
    off = np.array([0, (1 << 30) + 1], dtype=np.int64)
    g, ng = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32)
    err = C.create_string_buffer(512)
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    rc = L.freesasa_gpu_calc_groups_periodic(one.ctypes.data_as(dp), r.ctypes.data_as(dp), off.ctypes.data_as(lp), 1, g.ctypes.data_as(ip),
                                             ng.ctypes.data_as(ip), cell.ctypes.data_as(dp), 0, PROBE, 20, one.ctypes.data_as(dp),
                                             one.ctypes.data_as(dp), None, None, None, -1, err, 512)
    assert rc == -1
    raise RuntimeError(err.value.decode())


def test_null_arguments_are_refused():
    L = fa.lib()
    x = np.zeros(3)
    off = np.array([0, 1], dtype=np.int64)
    g, ng = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32)
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    full = [x.ctypes.data_as(dp), x.ctypes.data_as(dp), off.ctypes.data_as(lp), 1, g.ctypes.data_as(ip), ng.ctypes.data_as(ip),
            x.ctypes.data_as(dp), 0, PROBE, 20, x.ctypes.data_as(dp), x.ctypes.data_as(dp), None, None, None, -1]
    for fn in (L.freesasa_gpu_calc_groups_periodic, L.freesasa_gpu_calc_groups_periodic_triclinic):
        for k in (0, 1, 2, 4, 5, 6, 10, 11):                   # xyz, radii, offsets, group, n_groups, cells, sasa_out, iso_out
            args = list(full)
            args[k] = None
            err = C.create_string_buffer(512)
            assert fn(*args, err, 512) == -1 and err.value == b"null argument", (fn, k)
    # the device-pointer entries: a NULL context
    for fn in (L.freesasa_gpu_groups_periodic_dev, L.freesasa_gpu_groups_periodic_triclinic_dev):
        assert fn(None, 0, None, None, off.ctypes.data_as(lp), 1, None, ng.ctypes.data_as(ip), x.ctypes.data_as(dp), PROBE, 20, None, None,
                  None, None, None) == -1


def dimer_dcd(tmp_path):
    b = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    write_dcd(tmp_path / "f.dcd", np.asarray(b.xyz, dtype=np.float32)[None] + 500.0, cell=True)
    return b, int(b.n_atoms)


def test_the_file_entry_refuses_before_a_file_is_opened(tmp_path):
    b, n = dimer_dcd(tmp_path)
    ids = np.zeros(n, dtype=np.int32)
    t, g = str(tmp_path / "t"), str(tmp_path / "g")
    L = fa._stats_proto(fa._topology_proto(fa.lib()))
    cb = b._as_c()
    err = C.create_string_buffer(512)

    def call(bits, group):
        return L.freesasa_gpu_trajectory_file_groups_periodic(str(tmp_path / "f.dcd").encode(), bits, 0, 0, C.byref(cb), 0, n, None, None,
                                                              None if group is None else group.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                                              0, PROBE, 20, 0, t.encode(), None, None, None, None, None, g.encode(), None,
                                                              None, 0, None, 0, None, 0, None, None, err, 512)
    # bit 3 is required; bit 4 needs it
    assert call(fa.FRAMES_DCD, ids) == -1 and b"need bit 3 of frames_f32" in err.value
    assert call(fa.FRAMES_DCD | fa.FRAMES_TRICLINIC, ids) == -1 and b"need bit 3 of frames_f32" in err.value
    # group == NULL
    assert call(fa.FRAMES_DCD | fa.FRAMES_PBC, None) == -1 and b"need group ids (group is NULL)" in err.value
    # raw frames carry no cell
    assert call(fa.FRAMES_PBC, ids) == -1 and b"raw frame files carry no cell" in err.value
    # an id out of range, group ids without group areas: the groups run's own checks
    with pytest.raises(RuntimeError, match=r"atom 0 has group id 5"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, t, group=ids + 5, n_groups=1, group_areas_path=g, dcd=True)
    with pytest.raises(RuntimeError, match="group areas have nowhere to go"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, t, group=ids, n_groups=1, dcd=True)
    # a DCD file without a cell record
    write_dcd(tmp_path / "nocell.dcd", np.asarray(b.xyz, dtype=np.float32)[None])
    with pytest.raises(RuntimeError, match="unit-cell record"):
        fa.trajectory_file_groups_periodic(tmp_path / "nocell.dcd", b, t, group=ids, n_groups=1, group_areas_path=g, dcd=True)
    assert not os.path.exists(t) and not os.path.exists(g), "an output file was opened"


def test_the_other_entries_keep_refusing_and_name_the_new_one(tmp_path):
    b, n = dimer_dcd(tmp_path)
    for tri in (False, True):
        with pytest.raises(RuntimeError, match="not offered with chain groups by this entry: freesasa_gpu_trajectory_file_groups_periodic"):
            fa.trajectory_file_topology(tmp_path / "f.dcd", b, str(tmp_path / "t"), group=np.zeros(n, dtype=np.int32), n_groups=1,
                                        group_areas_path=str(tmp_path / "g"), dcd=True, pbc=True, triclinic=tri)
        with pytest.raises(RuntimeError, match="not offered with chain groups by this entry"):
            fa.trajectory_file_topology(tmp_path / "f.dcd", b, str(tmp_path / "t"), group=np.zeros(n, dtype=np.int32), n_groups=1,
                                        group_areas_path=str(tmp_path / "g"), dcd=True, pbc=True, triclinic=tri, stats=("groups",),
                                        stats_path=str(tmp_path / "s"), partials_path=str(tmp_path / "p"))
    assert not os.path.exists(tmp_path / "t") and not os.path.exists(tmp_path / "g")


def test_phase_functions_under_sanitizers_stand_alone():
    """tests/emu/emu_groups_pbc.cpp with its main under AddressSanitizer + UBSan, every array of exactly its size: one line per stage"""
    import subprocess
    subprocess.run(["make", "-C", ROOT, "tests/emu/groups_pbc_check"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "tests", "emu", "groups_pbc_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [line.split(":")[0] for line in r.stdout.splitlines()] == ["cells ok", "expand ok", "finish ok"]
