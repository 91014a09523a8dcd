"""The trajectory drivers with a topology (freesasa_gpu_trajectory_topology / _trajectory_file_topology) on the device.
The yardsticks are the per-structure entries: the frames of a small trajectory tiled into ONE batch of as many structures
and sent through calc_batch, GpuContext.class_sums / residue_areas and select_batch - every per-frame output of the
trajectory drivers must equal those bit for bit; frame 0 (the file's own coordinates) is anchored to the reference's RSA
output with the comparison tests/test_ingest.py makes."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from test_ingest import read_rsa

pytestmark = pytest.mark.gpu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
UBQ = os.path.join(PDB, "1ubq.pdb")
F, N, R, FPB, DEVS = 7, 602, 76, 3, [0, 0]
# ten selections: more than SEL_G = 8, so the sums make a second pass; an open range, a chain, a "resn ... and not name ..."
COMMANDS = ["a, resi -10", "b, chain A", "c, resn LYS and not name CA+N", "d, symbol O", "e, resi 70-", "f, name CB",
            "g, resn ILE+LEU+VAL", "h, resi 20-40 and symbol N", "i, not symbol C", "j, resi 1+76"]
ALGS = {"lr20": (fa.LEE_RICHARDS, 20), "sr100": (fa.SHRAKE_RUPLEY, 100)}


@pytest.fixture(scope="module")
def sel():
    s = ingest.Selection(COMMANDS)
    yield s
    s.close()


@pytest.fixture(scope="module")
def system():
    """1UBQ, 7 frames (frame 0: the file's coordinates, 1-6: a seeded +-0.3 A jitter), and the same frames with 150 decoy
    atoms spliced in: in place (order kept) and with the real atoms scattered (a non-monotonic index)"""
    one = ingest.load_pdb_files([UBQ])
    assert (one.n_atoms, one.n_residues) == (N, R)
    rng = np.random.default_rng(20261017)
    frames = np.repeat(one.xyz[None], F, 0)
    frames[1:] += rng.uniform(-0.3, 0.3, (F - 1, N, 3))
    big = {}
    for kind in ("spliced", "scattered"):
        slots = rng.permutation(N + 150)[:N]
        index = (np.sort(slots) if kind == "spliced" else slots).astype(np.int32)
        full = rng.uniform(one.xyz.min(0), one.xyz.max(0), (F, N + 150, 3))       # decoys inside the protein's box
        full[:, index] = frames                                                      # frame atom index[i] IS topology atom i
        big[kind] = (full, index)
    assert np.any(np.diff(big["scattered"][1]) < 0) and np.all(np.diff(big["spliced"][1]) > 0)
    return one, frames, big


_REF = {}


def reference(system, sel, alg):
    """the 7 frames as one 7-structure batch through the per-structure entries (computed once per algorithm)"""
    if alg in _REF:
        return _REF[alg]
    import torch
    one, frames, _ = system
    b7 = ingest.load_pdb_files([UBQ] * F)
    b7.xyz = frames.reshape(-1, 3).copy()
    a, res = ALGS[alg]
    sasa, _, totals = fa.calc_batch(b7.xyz, b7.radii, b7.offsets, a, resolution=res)
    dev = torch.device("cuda:0")
    d_sasa = torch.from_numpy(sasa).to(dev)
    d_cls, d_bb = torch.from_numpy(b7.atom_class).to(dev), torch.from_numpy(b7.atom_backbone).to(dev)
    d_cs = torch.empty(3 * F, dtype=torch.float64, device=dev)
    d_abs = torch.empty(6 * R * F, dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0)
    ctx.class_sums(d_sasa.data_ptr(), d_cls.data_ptr(), b7.offsets, d_cs.data_ptr())
    ctx.residue_areas(d_sasa.data_ptr(), d_cls.data_ptr(), d_bb.data_ptr(), b7.res_first, d_abs.data_ptr())
    ctx.close()
    areas, counts = fa.select_batch(b7, sel, sasa)
    assert np.all(counts == counts[0])
    _REF[alg] = dict(totals=totals, sasa=sasa.reshape(F, N), cls=d_cs.cpu().numpy().reshape(F, 3),
                     res=d_abs.cpu().numpy().reshape(F, R, 6), sel=areas, atoms=counts[0])
    return _REF[alg]


def same(got, want):
    assert np.array_equal(got.totals, want["totals"])
    if got.sasa is not None:
        assert np.array_equal(got.sasa, want["sasa"])
    assert np.array_equal(got.class_sums, want["cls"])
    assert np.array_equal(got.residues, want["res"])
    assert np.array_equal(got.selection_areas, want["sel"])
    assert np.array_equal(got.selection_atoms, want["atoms"])


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_every_output_equals_the_per_structure_path_bit_for_bit(system, sel, alg):
    one, frames, _ = system
    want = reference(system, sel, alg)
    a, res = ALGS[alg]
    got = fa.trajectory_topology(frames, one, selection=sel, per_atom=True, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS)
    same(got, want)
    assert got.residues.shape == (F, R, 6) and got.selection_areas.shape == (F, len(COMMANDS))
    assert want["atoms"].min() > 0 and np.array_equal(got.res_ref, one.res_ref)
    # without the per-atom output the other numbers are the same
    same(fa.trajectory_topology(frames, one, selection=sel, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS), want)


def test_frame_0_agrees_with_the_references_rsa_file(system, sel):
    """tests/test_ingest.py test_relative_sasa_matches_the_references_rsa_output's comparison (its parser, its column map, its
    tolerances: the file prints %.2f absolute and %.1f relative values), on frame 0 of the trajectory"""
    one, frames, _ = system
    got = fa.trajectory_topology(frames, one, frames_per_batch=FPB, devices=DEVS)
    A = got.residues[0]
    table = ingest.residue_reference_table().reshape(-1, 5)
    rows, total = read_rsa("1ubq.lr20.rsa")
    assert len(rows) == R
    cols = [0, 2, 1, 4, 3]
    for r, (res, chain, number, vals) in enumerate(rows):
        assert (one.res_name[r], one.res_chain[r], one.res_number[r].strip()) == (res.strip(), chain, number)
        for k, (a, rel) in enumerate(vals):
            assert abs(A[r, cols[k]] - a) <= 0.005 + 1e-9, (r, k)
            with np.errstate(divide="ignore", invalid="ignore"):      # (N/A: no reference row, or a reference area of 0)
                mine = np.nan if got.res_ref[r] < 0 else 100.0 * A[r, cols[k]] / table[got.res_ref[r], cols[k]]
            if rel is None:
                assert not np.isfinite(mine), (r, k)
            else:
                assert abs(mine - rel) <= 0.05 + 1e-9, (r, k)
    sums = A.sum(0)
    for k, w in enumerate(total):
        assert abs(sums[cols[k]] - w) <= 0.05 + 1e-6
    assert abs(sums[0] - got.totals[0]) < 1e-9 * got.totals[0] and np.all(A[:, 5] == 0)


@pytest.mark.parametrize("kind", ["spliced", "scattered"])
def test_solute_subset_of_larger_frames(system, sel, kind):
    """150 decoy atoms in every frame, dropped by the gather.  In both cases frame atom index[i] holds topology atom i's
    coordinates - the scattered index undoes the scatter - so every output is identical to the plain test's, on the
    UNSHUFFLED topology."""
    one, _, big = system
    full, index = big[kind]
    assert full.shape[1] == 752
    want = reference(system, sel, "lr20")
    got = fa.trajectory_topology(full, one, atom_index=index, selection=sel, per_atom=True, frames_per_batch=FPB, devices=DEVS)
    same(got, want)


def read_files(paths, S):
    g = lambda k, shape: np.fromfile(paths[k]).reshape(shape)
    return dict(totals=g("totals", (F,)), sasa=g("sasa", (F, N)), cls=g("cls", (F, 3)), res=g("res", (F, R, 6)), sel=g("sel", (F, S)))


def file_run(tmp, tag, frames_path, one, sel, **kw):
    paths = {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "cls", "res", "sel", "done")}
    kw.setdefault("devices", DEVS)
    done, n_frames, atoms = fa.trajectory_file_topology(frames_path, one, paths["totals"], selection=sel, sasa_path=paths["sasa"],
                                                        class_sums_path=paths["cls"], residues_path=paths["res"],
                                                        selections_path=paths["sel"], done_path=paths["done"],
                                                        frames_per_batch=FPB, **kw)
    return paths, done, n_frames, atoms


def test_fp32_frames_equal_the_frames_widened_on_the_host(system, sel, tmp_path):
    one, _, big = system
    full, index = big["scattered"]
    full32 = full.astype(np.float32)
    path = tmp_path / "frames.f32"
    full32.tofile(path)
    want = fa.trajectory_topology(full32.astype(np.float64), one, atom_index=index, selection=sel, per_atom=True,
                                  frames_per_batch=FPB, devices=DEVS)
    paths, done, n_frames, atoms = file_run(tmp_path, "f32", path, one, sel, atom_index=index, frame_atoms=752, f32=True)
    assert done and n_frames == F and np.array_equal(atoms, want.selection_atoms)
    got = read_files(paths, len(COMMANDS))
    for k, w in (("totals", want.totals), ("sasa", want.sasa), ("cls", want.class_sums), ("res", want.residues), ("sel", want.selection_areas)):
        assert np.array_equal(got[k], w), k


def test_files_resume_and_done_list(system, sel, tmp_path):
    one, frames, big = system
    full, index = big["spliced"]
    want = reference(system, sel, "lr20")
    path = tmp_path / "frames.f64"
    full.tofile(path)
    kw = dict(atom_index=index, frame_atoms=752)
    paths, done, n_frames, atoms = file_run(tmp_path, "all", path, one, sel, **kw)
    assert done and n_frames == F and np.array_equal(atoms, want["atoms"])
    got = read_files(paths, len(COMMANDS))
    for k in ("totals", "sasa", "cls", "res", "sel"):
        assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    # stopped after one shard, finished on another device list: the same files byte for byte
    part, done, _, _ = file_run(tmp_path, "part", path, one, sel, max_new_shards=1, **kw)
    assert not done and open(part["done"]).read().count("shard ") == 1
    head = open(part["done"]).readline()
    for word in (" topology ", " frame_atoms=752 ", " index=", " residues=", " selection=", " outputs=15"):
        assert word in head, word
    part, done, _, atoms = file_run(tmp_path, "part", path, one, sel, devices=[0], **kw)
    assert done and np.array_equal(atoms, want["atoms"]) and open(part["done"]).read().count("shard ") == 3
    for k in ("totals", "sasa", "cls", "res", "sel"):
        assert open(part[k], "rb").read() == open(paths[k], "rb").read(), k
    # a done-list of a run with another selection set, another index or other outputs belongs to another run
    before = {k: open(paths[k], "rb").read() for k in paths}
    other_sel = ingest.Selection(COMMANDS[:9] + ["j, resi 2+76"])
    other_index = index.copy()
    other_index[[0, 1]] = other_index[[1, 0]]
    with pytest.raises(RuntimeError, match="done-list belongs"):
        file_run(tmp_path, "all", path, one, other_sel, **kw)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        file_run(tmp_path, "all", path, one, sel, atom_index=other_index, frame_atoms=752)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        fa.trajectory_file_topology(path, one, paths["totals"], selection=sel, class_sums_path=paths["cls"], done_path=paths["done"],
                                    frames_per_batch=FPB, devices=DEVS, **kw)
    other_sel.close()
    assert before == {k: open(paths[k], "rb").read() for k in paths}          # (a refused call touches nothing)


def test_plain_done_lists_are_the_plain_drivers_own(system, sel, tmp_path):
    """The done-list of trajectory_file without a topology keeps its first line: the plain entry resumes from it and ends with
    the files of an uninterrupted run; neither entry takes the other's list."""
    one, frames, _ = system
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    p = lambda k: str(tmp_path / k)
    args = dict(frames_per_batch=FPB, devices=DEVS)
    assert fa.trajectory_file(path, one.radii, p("t0"), p("s0"), p("d0"), **args) == (True, F)
    assert " topology" not in open(p("d0")).readline()
    assert fa.trajectory_file(path, one.radii, p("t1"), p("s1"), p("d1"), max_new_shards=1, **args) == (False, F)
    assert fa.trajectory_file(path, one.radii, p("t1"), p("s1"), p("d1"), **args) == (True, F)
    assert open(p("t1"), "rb").read() == open(p("t0"), "rb").read() and open(p("s1"), "rb").read() == open(p("s0"), "rb").read()
    want = reference(system, sel, "lr20")
    assert np.array_equal(np.fromfile(p("t0")), want["totals"]) and np.array_equal(np.fromfile(p("s0")).reshape(F, N), want["sasa"])
    with pytest.raises(RuntimeError, match="done-list belongs"):
        fa.trajectory_file_topology(path, one, p("t0"), sasa_path=p("s0"), done_path=p("d0"), **args)
    fa.trajectory_file_topology(path, one, p("t2"), sasa_path=p("s2"), done_path=p("d2"), **args)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        fa.trajectory_file(path, one.radii, p("t2"), p("s2"), p("d2"), **args)
    assert open(p("t2"), "rb").read() == open(p("t0"), "rb").read() and open(p("s2"), "rb").read() == open(p("s0"), "rb").read()


def test_topology_from_the_second_structure_of_a_batch(system, sel):
    one, frames, big = system
    two = ingest.load_pdb_files([os.path.join(PDB, "3bkr.pdb"), UBQ])
    assert two.offsets[1] > 0 and two.res_offsets[1] > 0
    want = reference(system, sel, "lr20")
    same(fa.trajectory_topology(frames, two, structure=1, selection=sel, per_atom=True, frames_per_batch=FPB, devices=DEVS), want)
    full, index = big["scattered"]
    same(fa.trajectory_topology(full, two, structure=1, atom_index=index, selection=sel, frames_per_batch=FPB, devices=DEVS), want)


@pytest.mark.parametrize("hook", ["gpu", "host"])
def test_every_allocation_failure_is_an_error_and_the_next_call_works(system, sel, hook):
    """The n-th device / page-locked allocation (freesasa_gpu_test_fail_after) or host allocation / thread start
    (freesasa_host_test_fail_after) fails, n = 1, 2, ... up to the first n at which the call goes through: every failing
    call returns -1 with a message and the call after it gives the right numbers."""
    one, _, big = system
    full, index = big["scattered"]
    want = reference(system, sel, "lr20")
    L = fa.lib()

    def call():
        try:
            return fa.trajectory_topology(full[:3], one, atom_index=index, selection=sel, per_atom=True, frames_per_batch=2, devices=[0])
        except RuntimeError as e:
            assert len(str(e)) > len("freesasa_gpu_trajectory_topology: ")
            return None

    def right(got):
        assert got is not None
        for k, w in (("totals", got.totals), ("sasa", got.sasa), ("cls", got.class_sums), ("res", got.residues), ("sel", got.selection_areas)):
            assert np.array_equal(w, want[k][:3]), k
        assert np.array_equal(got.selection_atoms, want["atoms"])

    right(call())
    failures = 0
    try:
        for k in range(1, 2000):
            if hook == "gpu":
                L.freesasa_gpu_release_pool()            # fresh contexts: every buffer is allocated in this call
                L.freesasa_gpu_test_fail_after(k)
                got = call()
                L.freesasa_gpu_test_fail_after(0)
            else:
                fa.host_test_fail_after(k)
                try:
                    got = call()
                finally:
                    fa.host_test_fail_after(0)
            if got is not None:
                right(got)
                break
            failures += 1
            right(call())
        else:
            raise AssertionError("the walk did not end")
    finally:
        L.freesasa_gpu_test_fail_after(0)
        fa.host_test_fail_after(0)
    assert failures >= 5, (hook, failures)
    L.freesasa_gpu_release_pool()


# ------------------------------------------------------------------------------------------------ the table of outputs

KINDS = ("totals", "sasa", "cls", "res", "sel")
PATH_ARG = dict(sasa="sasa_path", cls="class_sums_path", res="residues_path", sel="selections_path")


@pytest.fixture(scope="module")
def all_outputs(system, sel, tmp_path_factory):
    """the spliced 752-atom frames in a file and the run that writes every output: (frame file, its result files)"""
    one, _, big = system
    tmp = tmp_path_factory.mktemp("outputs")
    full, index = big["spliced"]
    path = tmp / "frames.f64"
    full.tofile(path)
    paths, done, n_frames, _ = file_run(tmp, "all", path, one, sel, atom_index=index, frame_atoms=752)
    assert done and n_frames == F
    return path, paths


@pytest.mark.parametrize("asked, with_sel, word", [(("cls",), True, 2), (("res",), False, 4), (("sel",), True, 8), (("res", "sel"), True, 12),
                                                   (("sasa", "cls"), False, 3), ((), False, 0)])
def test_every_subset_of_outputs_lays_its_block_out_correctly(system, sel, all_outputs, tmp_path, asked, with_sel, word):
    """The sums of a shard lie one behind the other in one block - classes | residues | selection areas | atom counts - so where
    an output begins depends on which of the others are computed: every subset's files equal the all-outputs run's, nothing
    else is written, and the done-list names the outputs."""
    one, _, big = system
    path, ref = all_outputs
    mine = {k: str(tmp_path / k) for k in KINDS + ("done",)}
    kw = {PATH_ARG[k]: mine[k] for k in asked}
    done, n_frames, atoms = fa.trajectory_file_topology(path, one, mine["totals"], atom_index=big["spliced"][1], frame_atoms=752,
                                                        selection=sel if with_sel else None, done_path=mine["done"],
                                                        frames_per_batch=FPB, devices=DEVS, **kw)
    assert done and n_frames == F
    for k in KINDS:
        if k == "totals" or k in asked:
            assert open(mine[k], "rb").read() == open(ref[k], "rb").read(), k
        else:
            assert not os.path.exists(mine[k]), k
    if with_sel:
        assert np.array_equal(atoms, reference(system, sel, "lr20")["atoms"])
    else:
        assert atoms is None
    assert open(mine["done"]).readline().endswith(" outputs=%d\n" % word)


def test_fp32_per_atom_file_with_a_topology_and_a_gather(system, sel, tmp_path):
    one, _, big = system
    full, index = big["scattered"]
    want = reference(system, sel, "lr20")
    path = tmp_path / "frames.f64"
    full.tofile(path)
    kw = dict(atom_index=index, frame_atoms=752)
    p64, done, _, _ = file_run(tmp_path, "f64", path, one, sel, **kw)
    assert done
    p32, done, _, atoms = file_run(tmp_path, "f32", path, one, sel, out_f32=True, **kw)
    assert done and np.array_equal(atoms, want["atoms"])
    got = np.fromfile(p32["sasa"], dtype=np.float32)
    assert got.tobytes() == want["sasa"].astype(np.float32).tobytes()
    for k in ("totals", "cls", "res", "sel"):
        assert open(p32[k], "rb").read() == open(p64[k], "rb").read(), k
    before = {k: open(p32[k], "rb").read() for k in p32}
    with pytest.raises(RuntimeError, match="other parameters"):
        file_run(tmp_path, "f32", path, one, sel, **kw)
    assert before == {k: open(p32[k], "rb").read() for k in p32}


def test_page_locked_caller_arrays(system, sel):
    """Frames in page-locked memory are uploaded from where they are, and page-locked result arrays are written by the device:
    the paths without staging give the bytes of the staged ones."""
    import torch
    one, frames, _ = system
    want = reference(system, sel, "lr20")
    radii = np.ascontiguousarray(one.radii, dtype=np.float64)
    totals, sasa = fa.trajectory(frames, radii, frames_per_batch=FPB, device=0)
    assert totals.tobytes() == want["totals"].tobytes() and sasa.tobytes() == np.ascontiguousarray(want["sasa"]).tobytes()
    pinned = torch.from_numpy(frames).pin_memory()
    view = pinned.numpy()
    assert pinned.is_pinned() and np.ascontiguousarray(view, dtype=np.float64) is view
    t2, s2 = fa.trajectory(view, radii, frames_per_batch=FPB, device=0)
    assert t2.tobytes() == totals.tobytes() and s2.tobytes() == sasa.tobytes()
    # the output arrays page-locked too: the entry itself
    L = fa.lib()
    dp = C.POINTER(C.c_double)
    devs = (C.c_int * len(DEVS))(*DEVS)
    for per_atom in (True, False):
        t_out = torch.zeros(F, dtype=torch.float64).pin_memory()
        s_out = torch.zeros(F, N, dtype=torch.float64).pin_memory()
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_devices(C.cast(pinned.data_ptr(), dp), radii.ctypes.data_as(dp), N, F, fa.LEE_RICHARDS, 1.4, 20, FPB,
                                               C.cast(t_out.data_ptr(), dp), C.cast(s_out.data_ptr(), dp) if per_atom else None,
                                               devs, len(DEVS), err, 512)
        assert rc == 0, err.value
        assert t_out.numpy().tobytes() == totals.tobytes()
        assert s_out.numpy().tobytes() == (sasa.tobytes() if per_atom else bytes(8 * F * N))


def fnv1a(data, h=1469598103934665603):
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def plain_head(path, radii, n_frames, fpb, alg=0, resolution=20, probe=1.4, flags=0, header_bytes=0):
    """the first line of a trajectory done-list as freesasa_amd/csrc/gpu_drivers.hip documents it"""
    st = os.stat(path)
    return ("freesasa_amd trajectory done-list v2 n_atoms=%d n_frames=%d frames_per_batch=%d alg=%d resolution=%d probe=%s f32=%d "
            "header_bytes=%d frames_size=%d frames_mtime=%d.%09d radii=%016x\n"
            % (radii.size, n_frames, fpb, alg, resolution, "%.17g" % probe, flags, header_bytes, st.st_size,
               st.st_mtime_ns // 10**9, st.st_mtime_ns % 10**9, fnv1a(np.ascontiguousarray(radii, dtype=np.float64).tobytes())))


def test_the_done_lists_first_line_is_the_documented_one(system, sel, all_outputs, tmp_path):
    """The first line names the run, and a list written by one build must be resumed by the next: the whole line of a plain
    run, and of a run with a topology everything but the digest of the selection set's program (its words are the library's)."""
    import re
    one, frames, big = system
    path = tmp_path / "frames.f32"
    frames.astype(np.float32).tofile(path)
    p = lambda k: str(tmp_path / k)
    assert fa.trajectory_file(path, one.radii, p("t"), p("s"), p("d"), f32=True, out_f32=True, frames_per_batch=FPB, devices=DEVS) == (True, F)
    assert open(p("d")).readline() == plain_head(path, one.radii, F, FPB, flags=3)
    full_path, ref = all_outputs
    index = big["spliced"][1]
    res_first = np.ascontiguousarray(one.res_first[:R + 1] - one.offsets[0], dtype=np.int64)
    h_res = fnv1a(one.atom_backbone[:N].tobytes(), fnv1a(one.atom_class[:N].tobytes(), fnv1a(res_first.tobytes())))
    head = open(ref["done"]).readline()
    lead = plain_head(full_path, one.radii, F, FPB)[:-1] + " topology frame_atoms=752 index=%016x residues=%016x " % (fnv1a(index.tobytes()), h_res)
    assert head.startswith(lead)
    assert re.fullmatch(r"selection=[0-9a-f]{16} outputs=15\n", head[len(lead):])
