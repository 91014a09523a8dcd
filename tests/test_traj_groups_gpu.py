"""Chain groups in the trajectory drivers (freesasa_gpu_trajectory_groups / _trajectory_file_groups) on the device.  The
yardstick is the batch entry: the frames of a small trajectory tiled into ONE batch of as many structures, the group ids tiled
as often, through calc_groups - the per-frame group areas and isolated areas must equal its group totals and isolated areas bit
for bit, and every other output the run without groups; frame 0 (the file's own coordinates) is anchored to the reference's
committed chain-group totals with the tolerance of tests/test_groups_gpu.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import freesasa_amd as fa
from freesasa_amd import ingest

pytestmark = pytest.mark.gpu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
F, N, FPB, DEVS = 7, 516, 3, [0, 0]
COMMANDS = ["a, resi -10", "b, chain A", "c, resn LYS and not name CA+N", "d, symbol O", "e, resi 20-", "f, name CB",
            "g, resn ILE+LEU+VAL", "h, resi 5-15 and symbol N", "i, not symbol C", "j, chain B+D"]
ALGS = {"lr20": (fa.LEE_RICHARDS, 20), "sr100": (fa.SHRAKE_RUPLEY, 100)}


def jitter(xyz, n_frames, seed):
    """frame 0: the file's coordinates, the others a seeded +-0.3 A jitter"""
    rng = np.random.default_rng(seed)
    frames = np.repeat(xyz[None], n_frames, 0)
    frames[1:] += rng.uniform(-0.3, 0.3, (n_frames - 1,) + xyz.shape)
    return frames


@pytest.fixture(scope="module")
def sel():
    s = ingest.Selection(COMMANDS)
    yield s
    s.close()


@pytest.fixture(scope="module")
def system():
    """2jo4 (chains A, B, C, D of 129 atoms) cut by "AC+B": group 0 in two runs of atoms, group 1 between them, D in no group;
    7 frames, and the same frames with 150 decoy atoms and the real ones scattered among them (a non-monotonic index)"""
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    assert b.n_atoms == N
    ids, ng, st = b.chain_groups("AC+B")
    assert ng[0] == 2 and st[0] == 0 and np.array_equal(ids, np.repeat(np.array([0, 1, 0, -1], np.int32), 129))
    frames = jitter(b.xyz, F, 20261018)
    rng = np.random.default_rng(5)
    index = rng.permutation(N + 150)[:N].astype(np.int32)
    full = rng.uniform(b.xyz.min(0), b.xyz.max(0), (F, N + 150, 3))
    full[:, index] = frames
    assert np.any(np.diff(index) < 0)
    return b, ids, frames, full, index


def yardstick(b, frames, ids, G, alg):
    """the frames as one batch of len(frames) structures through calc_groups: (sasa [F, n], iso [F, n], totals [F], areas [F, G, 3])"""
    nf, n = frames.shape[:2]
    a, res = ALGS[alg]
    offs = np.arange(nf + 1, dtype=np.int64) * n
    sasa, iso, totals, gt = fa.calc_groups(frames.reshape(-1, 3), np.tile(b.radii, nf), offs, np.tile(ids, nf), np.full(nf, G, np.int32),
                                           alg=a, resolution=res, device=0)
    return sasa.reshape(nf, n), iso.reshape(nf, n), totals, gt.reshape(nf, G, 3)


_REF = {}


def reference(system, sel, alg):
    """the yardstick and the run WITHOUT groups of the 2jo4 frames (once per algorithm)"""
    if alg not in _REF:
        b, ids, frames, _, _ = system
        a, res = ALGS[alg]
        plain = fa.trajectory_topology(frames, b, selection=sel, per_atom=True, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS)
        assert plain.group_areas is None and plain.isolated is None and plain.group_atoms is None
        _REF[alg] = (yardstick(b, frames, ids, 2, alg), plain)
    return _REF[alg]


def same(got, ref, per_atom=True):
    (sasa, iso, totals, areas), plain = ref
    assert np.array_equal(got.group_areas, areas)
    assert np.array_equal(got.totals, totals) and np.array_equal(got.totals, plain.totals)
    if per_atom:
        assert np.array_equal(got.isolated, iso)
        assert np.array_equal(got.sasa, sasa) and np.array_equal(got.sasa, plain.sasa)
    else:
        assert got.isolated is None and got.sasa is None
    assert np.array_equal(got.class_sums, plain.class_sums)
    assert np.array_equal(got.residues, plain.residues)
    assert np.array_equal(got.selection_areas, plain.selection_areas)
    assert np.array_equal(got.selection_atoms, plain.selection_atoms)


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_every_output_equals_the_batch_entry_or_the_run_without_groups(system, sel, alg):
    """F = 7 in shards of 3: the last shard is short, so the combined batch's offsets change once"""
    b, ids, frames, _, _ = system
    ref = reference(system, sel, alg)
    a, res = ALGS[alg]
    kw = dict(selection=sel, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS, chain_groups="AC+B")
    got = fa.trajectory_topology(frames, b, per_atom=True, **kw)
    same(got, ref)
    assert got.group_areas.shape == (F, 2, 3) and np.array_equal(got.group_atoms, [258, 129])
    assert np.all(got.group_areas[:, :, 2] > 0) and np.all(got.isolated >= got.sasa - 1e-9)
    assert np.array_equal(got.isolated[:, ids < 0], got.sasa[:, ids < 0])
    same(fa.trajectory_topology(frames, b, **kw), ref, per_atom=False)


@pytest.mark.parametrize("name, spec, n_frames, fpb", [("1a0q.pdb", "H+L", 3, 2), ("2jo4.pdb", "AB+CD", 3, 2)])
def test_frame_0_agrees_with_the_references_chain_group_totals(name, spec, n_frames, fpb):
    """1a0q: the file has chain L before chain H, so group 0's atoms come after group 1's"""
    with open(os.path.join(GOLDEN, "chain_groups.json")) as fh:
        case = [c for c in json.load(fh) if c["file"] == name and c["spec"] == spec][0]
    b = ingest.load_pdb_files([os.path.join(PDB, name)])
    ids, ng, st = b.chain_groups(spec)
    G = int(ng[0])
    assert st[0] == 0 and G == len(case["groups"]) and b.n_atoms == case["complex"]["atoms"]
    if name == "1a0q.pdb":
        assert np.nonzero(ids == 0)[0].min() > np.nonzero(ids == 1)[0].max()
    frames = jitter(b.xyz, n_frames, 11)
    for alg, (a, res) in ALGS.items():
        got = fa.trajectory_topology(frames, b, per_atom=True, alg=a, resolution=res, frames_per_batch=fpb, devices=DEVS, chain_groups=spec)
        want = case["complex"][alg]
        assert abs(got.totals[0] - want) <= 1e-8 * b.n_atoms + 1e-12 * want, (name, alg, got.totals[0], want)
        for k, wg in enumerate(case["groups"]):
            assert got.group_atoms[k] == wg["atoms"]
            assert abs(got.group_areas[0, k, 0] - wg[alg]) <= 1e-8 * wg["atoms"] + 1e-12 * wg[alg], (name, alg, k, got.group_areas[0, k, 0], wg[alg])
        sasa, iso, totals, areas = yardstick(b, frames, ids, G, alg)
        assert np.array_equal(got.group_areas, areas) and np.array_equal(got.isolated, iso)
        assert np.array_equal(got.totals, totals) and np.array_equal(got.sasa, sasa)


def test_solute_scattered_among_decoys_and_fp32_frames(system, sel, tmp_path):
    b, ids, frames, full, index = system
    ref = reference(system, sel, "lr20")
    kw = dict(atom_index=index, selection=sel, per_atom=True, frames_per_batch=FPB, devices=DEVS, group=ids, n_groups=2)
    same(fa.trajectory_topology(full, b, **kw), ref)
    # fp32 frames (a file: the memory form takes fp64) equal the frames widened on the host
    full32 = full.astype(np.float32)
    want = fa.trajectory_topology(full32.astype(np.float64), b, **kw)
    path = tmp_path / "frames.f32"
    full32.tofile(path)
    p = {k: str(tmp_path / k) for k in ("totals", "sasa", "groups", "iso")}
    done, n_frames, _ = fa.trajectory_file_topology(path, b, p["totals"], atom_index=index, frame_atoms=N + 150, sasa_path=p["sasa"], f32=True,
                                                    frames_per_batch=FPB, devices=DEVS, group=ids, n_groups=2,
                                                    group_areas_path=p["groups"], isolated_path=p["iso"])
    assert done and n_frames == F
    for k, w in (("totals", want.totals), ("sasa", want.sasa), ("groups", want.group_areas), ("iso", want.isolated)):
        assert np.fromfile(p[k]).tobytes() == np.ascontiguousarray(w).tobytes(), k
    assert not np.array_equal(want.group_areas, ref[0][3])          # (rounding the coordinates does change the numbers)


def test_separate_chains_equal_explicit_ids(system):
    b, _, frames, _, _ = system
    explicit = np.repeat(np.arange(4, dtype=np.int32), 129)
    kw = dict(per_atom=True, frames_per_batch=FPB, devices=DEVS)
    got = fa.trajectory_topology(frames, b, separate_chains=True, **kw)
    want = fa.trajectory_topology(frames, b, group=explicit, n_groups=4, **kw)
    assert got.group_areas.shape == (F, 4, 3) and np.array_equal(got.group_atoms, [129] * 4)
    for k in ("group_areas", "isolated", "totals", "sasa", "class_sums", "residues"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    sasa, iso, totals, areas = yardstick(b, frames, explicit, 4, "lr20")
    assert np.array_equal(got.group_areas, areas) and np.array_equal(got.isolated, iso)


# ------------------------------------------------------------------------------------------------ the file form

KINDS = ("totals", "sasa", "cls", "res", "sel", "groups", "iso")


def file_run(tmp, tag, frames_path, b, sel, ids, **kw):
    paths = {k: str(tmp / f"{tag}.{k}") for k in KINDS + ("done",)}
    kw.setdefault("devices", DEVS)
    if ids is not None:
        kw.update(group=ids, n_groups=2, group_areas_path=paths["groups"], isolated_path=paths["iso"])
    done, n_frames, atoms = fa.trajectory_file_topology(frames_path, b, paths["totals"], selection=sel, sasa_path=paths["sasa"],
                                                        class_sums_path=paths["cls"], residues_path=paths["res"],
                                                        selections_path=paths["sel"], done_path=paths["done"], frames_per_batch=FPB, **kw)
    return paths, done, n_frames, atoms


def test_files_equal_the_arrays_resume_and_refuse_other_lists(system, sel, tmp_path):
    b, ids, frames, _, _ = system
    (sasa, iso, totals, areas), plain = reference(system, sel, "lr20")
    want = dict(totals=totals, sasa=sasa, cls=plain.class_sums, res=plain.residues, sel=plain.selection_areas, groups=areas, iso=iso)
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    paths, done, n_frames, atoms = file_run(tmp_path, "all", path, b, sel, ids)
    assert done and n_frames == F and np.array_equal(atoms, plain.selection_atoms)
    for k in KINDS:
        assert open(paths[k], "rb").read() == np.ascontiguousarray(want[k]).tobytes(), k
    # the per-atom files as fp32: the fp64 values narrowed, every other file the same
    p32, done, _, _ = file_run(tmp_path, "f32", path, b, sel, ids, out_f32=True)
    assert done
    assert open(p32["iso"], "rb").read() == iso.astype(np.float32).tobytes()
    assert open(p32["sasa"], "rb").read() == sasa.astype(np.float32).tobytes()
    for k in ("totals", "cls", "res", "sel", "groups"):
        assert open(p32[k], "rb").read() == open(paths[k], "rb").read(), k
    # stopped after one shard, finished on another device list: the same files byte for byte
    part, done, _, _ = file_run(tmp_path, "part", path, b, sel, ids, max_new_shards=1)
    assert not done and open(part["done"]).read().count("shard ") == 1
    part, done, _, _ = file_run(tmp_path, "part", path, b, sel, ids, devices=[0])
    assert done and open(part["done"]).read().count("shard ") == 3
    for k in KINDS:
        assert open(part[k], "rb").read() == open(paths[k], "rb").read(), k
    # a done-list written without groups, or with other ids, belongs to another run
    before = {k: open(paths[k], "rb").read() for k in paths}
    other = ids.copy()
    other[0] = 1
    with pytest.raises(RuntimeError, match="done-list belongs"):
        file_run(tmp_path, "all", path, b, sel, other)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        file_run(tmp_path, "all", path, b, sel, None)
    assert before == {k: open(paths[k], "rb").read() for k in paths}
    nog, done, _, _ = file_run(tmp_path, "nog", path, b, sel, None)
    assert done and not os.path.exists(nog["groups"]) and not os.path.exists(nog["iso"])
    head = open(nog["done"]).readline()
    assert head.endswith(" outputs=15\n") and "groups=" not in head
    with pytest.raises(RuntimeError, match="done-list belongs"):
        file_run(tmp_path, "nog", path, b, sel, ids)
    for k in ("totals", "sasa", "cls", "res", "sel"):
        assert open(nog[k], "rb").read() == open(paths[k], "rb").read(), k


def fnv1a(data, h=1469598103934665603):
    for x in bytes(data):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_done_lists_first_line_is_the_documented_one(system, sel, tmp_path):
    """include/freesasa_gpu.h and gpu_drivers.hip (traj_done_head): the plain line, the topology's words, outputs= with the bits
    of the groups (16) and the isolated areas (32), and at the end groups=<fnv1a of n_groups (int32), then of the ids>"""
    b, ids, frames, _, _ = system
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    paths, done, _, _ = file_run(tmp_path, "all", path, b, sel, ids)
    assert done
    head = open(paths["done"]).readline()
    st = os.stat(path)
    lead = ("freesasa_amd trajectory done-list v2 n_atoms=%d n_frames=%d frames_per_batch=%d alg=0 resolution=20 probe=%s f32=0 "
            "header_bytes=0 frames_size=%d frames_mtime=%d.%09d radii=%016x topology frame_atoms=%d index=%016x "
            % (N, F, FPB, "%.17g" % 1.4, st.st_size, st.st_mtime_ns // 10**9, st.st_mtime_ns % 10**9,
               fnv1a(np.ascontiguousarray(b.radii, dtype=np.float64).tobytes()), N, 0))
    assert head.startswith(lead)
    digest = fnv1a(ids.tobytes(), fnv1a(np.int32(2).tobytes()))
    assert re.fullmatch(r"residues=[0-9a-f]{16} selection=[0-9a-f]{16} outputs=63 groups=%016x\n" % digest, head[len(lead):])
    # the group areas alone: bit 16
    p = lambda k: str(tmp_path / k)
    done, _, _ = fa.trajectory_file_topology(path, b, p("t"), done_path=p("d"), frames_per_batch=FPB, devices=DEVS, group=ids, n_groups=2,
                                             group_areas_path=p("g"))
    assert done and open(p("d")).readline().endswith(" outputs=16 groups=%016x\n" % digest)
    assert open(p("g"), "rb").read() == open(paths["groups"], "rb").read() and not os.path.exists(p("iso"))


@pytest.mark.parametrize("hook", ["gpu", "host"])
def test_every_allocation_failure_is_an_error_and_the_next_call_works(system, sel, hook):
    """The n-th device / page-locked allocation (freesasa_gpu_test_fail_after) or host allocation / thread start
    (freesasa_host_test_fail_after) fails, n = 1, 2, ... up to the first n at which the call goes through: every failing call
    returns -1 with a message and the call after it gives the right numbers."""
    b, ids, frames, full, index = system
    ref = reference(system, sel, "lr20")
    (sasa, iso, totals, areas), plain = ref
    L = fa.lib()

    def call():
        try:
            return fa.trajectory_topology(full[:3], b, atom_index=index, selection=sel, per_atom=True, frames_per_batch=2, devices=[0],
                                          group=ids, n_groups=2)
        except RuntimeError as e:
            assert len(str(e)) > len("freesasa_gpu_trajectory_groups: ")
            return None

    def right(got):
        assert got is not None
        for w, r in ((got.totals, totals), (got.sasa, sasa), (got.isolated, iso), (got.group_areas, areas), (got.class_sums, plain.class_sums),
                     (got.residues, plain.residues), (got.selection_areas, plain.selection_areas)):
            assert np.array_equal(w, r[:3])
        assert np.array_equal(got.selection_atoms, plain.selection_atoms)

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
