"""Run statistics of the trajectory drivers on the device (freesasa_gpu_trajectory_stats, _groups_stats, _file_stats,
_file_groups_stats).  The yardstick is never the code under test: the drivers WITHOUT statistics deliver every per-frame output
once, and from those arrays the expected partials and statistics are the numpy loop and merge of tests/test_traj_stats.py, in the
order include/freesasa_gpu.h fixes - the device is held to them bit for bit.  The system is tests/test_traj_topology_gpu.py's:
1UBQ, 7 frames, shards of 3, 3 and 1 frames, the device list [0, 0], ten selections."""
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import tools
from freesasa_amd import ingest
from test_dcd import write_dcd
from test_dcd_gpu import jittered, solvated  # noqa: F401  (solvated: a fixture)
from test_pbc_gpu import patch_cells
from test_traj_stats import cut_ref, partial_ref, same_bits
from test_traj_topology_gpu import ALGS, COMMANDS, DEVS, F, FPB, N, R, sel, system  # noqa: F401  (sel, system: fixtures)

pytestmark = pytest.mark.gpu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
SHARDS = [3, 3, 1]
ALL5 = ("totals", "atoms", "classes", "residues", "selections")
_BASE = {}


def columns(totals=None, atoms=None, isolated=None, classes=None, residues=None, selections=None, groups=None):
    """per-frame arrays -> [F, W] in the order of a partial's columns"""
    given = [a for a in (totals, atoms, isolated, classes, residues, selections, groups) if a is not None]
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(len(a), -1) for a in given], axis=1)


def base(system, sel, alg):
    """the drivers WITHOUT statistics, every output delivered, once per algorithm: (the result, expected statistics [4, W],
    expected partials [3, 4, W]) of ALL5"""
    if alg not in _BASE:
        one, frames, _ = system
        a, res = ALGS[alg]
        got = fa.trajectory_topology(frames, one, selection=sel, per_atom=True, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS)
        assert got.stats is None
        cols = columns(got.totals, got.sasa, None, got.class_sums, got.residues, got.selection_areas)
        assert cols.shape == (F, 1 + N + 3 + 6 * R + len(COMMANDS))
        _BASE[alg] = (got, cols) + cut_ref(cols, SHARDS)
    return _BASE[alg]


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_statistics_of_every_output_bit_for_bit_with_and_without_the_per_frame_outputs(system, sel, alg):
    one, frames, _ = system
    want, cols, stats, parts = base(system, sel, alg)
    a, res = ALGS[alg]
    kw = dict(selection=sel, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS, stats=ALL5)
    got = fa.trajectory_topology(frames, one, per_atom=True, **kw)
    assert same_bits(got.stats.raw, stats) and same_bits(got.stats.partials, parts) and list(got.stats.frames) == SHARDS
    # asking for statistics changes no bit of a per-frame output
    for k in ("totals", "sasa", "class_sums", "residues", "selection_areas", "selection_atoms"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    # the dict of named arrays is a reshaping of the same numbers
    s = got.stats
    assert s["totals"].shape == (4,) and s["atoms"].shape == (4, N) and s["classes"].shape == (4, 3) and s["residues"].shape == (4, R, 6)
    assert s["selections"].shape == (4, len(COMMANDS)) and set(s) == set(ALL5)
    assert same_bits(columns(s["totals"][:, None], s["atoms"], None, s["classes"], s["residues"], s["selections"]), stats)
    assert np.all(s["atoms"][1] >= 0) and np.all(s["atoms"][2] <= s["atoms"][0] + 1e-9) and np.all(s["atoms"][0] <= s["atoms"][3] + 1e-9)
    assert np.array_equal(s["atoms"][2], want.sasa.min(0)) and np.array_equal(s["residues"][3], want.residues.max(0))
    # without the per-frame outputs: the per-atom areas never downloaded, residues, class sums and selections computed but not delivered
    bare = fa.trajectory_topology(frames, one, per_atom=False, per_frame=False, **kw)
    assert bare.sasa is None and bare.residues is None and bare.class_sums is None and bare.selection_areas is None
    assert same_bits(bare.stats.raw, stats) and same_bits(bare.stats.partials, parts) and np.array_equal(bare.totals, want.totals)
    assert np.array_equal(bare.selection_atoms, want.selection_atoms)
    # a subset: where an output begins depends on which others are computed
    sub = fa.trajectory_topology(frames, one, per_frame=False, selection=sel, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS,
                                 stats=("residues", "atoms"))
    assert same_bits(sub.stats["atoms"], s["atoms"]) and same_bits(sub.stats["residues"], s["residues"]) and set(sub.stats) == {"atoms", "residues"}
    # the entry without a topology
    totals, sasa, plain = fa.trajectory(frames, one.radii, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS, per_atom=False,
                                        stats=("totals", "atoms"))
    assert sasa is None and np.array_equal(totals, want.totals)
    assert same_bits(plain["totals"], s["totals"]) and same_bits(plain["atoms"], s["atoms"]) and same_bits(plain.partials, parts[:, :, :1 + N])


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_isolated_and_group_statistics_with_separate_chains(alg):
    """2jo4, its four chains a group each (tests/test_traj_groups_gpu.py's fixture and jitter)"""
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    rng = np.random.default_rng(20261018)
    frames = np.repeat(b.xyz[None], F, 0)
    frames[1:] += rng.uniform(-0.3, 0.3, (F - 1,) + b.xyz.shape)
    a, res = ALGS[alg]
    kw = dict(separate_chains=True, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS)
    want = fa.trajectory_topology(frames, b, per_atom=True, **kw)
    assert want.group_areas.shape == (F, 4, 3) and np.any(want.isolated != want.sasa)
    stats, parts = cut_ref(columns(want.totals, want.sasa, want.isolated, None, None, None, want.group_areas), SHARDS)
    names = ("totals", "atoms", "isolated", "groups")
    got = fa.trajectory_topology(frames, b, per_atom=True, stats=names, **kw)
    assert same_bits(got.stats.raw, stats) and same_bits(got.stats.partials, parts)
    assert got.stats["isolated"].shape == (4, b.n_atoms) and got.stats["groups"].shape == (4, 4, 3)
    for k in ("totals", "sasa", "isolated", "group_areas", "class_sums", "residues"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    bare = fa.trajectory_topology(frames, b, per_frame=False, stats=("isolated", "groups"), **kw)
    assert bare.isolated is None and bare.group_areas is None
    assert same_bits(bare.stats["isolated"], got.stats["isolated"]) and same_bits(bare.stats["groups"], got.stats["groups"])


def test_one_shard_is_the_plain_two_pass_loop(system, sel):
    one, frames, _ = system
    want, cols, stats331, _ = base(system, sel, "lr20")
    got = fa.trajectory_topology(frames, one, selection=sel, per_frame=False, frames_per_batch=F, devices=DEVS, stats=ALL5)
    whole = partial_ref(cols)
    assert same_bits(got.stats.partials[0], whole) and got.stats.partials.shape[0] == 1
    assert same_bits(got.stats.raw, np.stack([whole[0], np.sqrt(whole[1] / float(F)), whole[2], whole[3]]))
    # another frames_per_batch agrees to rounding, not to the bit
    assert np.allclose(got.stats.raw, stats331, rtol=1e-12, atol=1e-12)
    assert same_bits(got.stats.raw[2:], stats331[2:]) and not same_bits(got.stats.raw[:2], stats331[:2])


def test_device_lists_give_identical_bytes(system, sel):
    one, frames, _ = system
    _, _, stats, parts = base(system, sel, "lr20")
    for devices in ([0], [0, 0, 0]):
        got = fa.trajectory_topology(frames, one, selection=sel, per_frame=False, frames_per_batch=FPB, devices=devices, stats=ALL5)
        assert got.stats.raw.tobytes() == stats.tobytes() and got.stats.partials.tobytes() == parts.tobytes(), devices


def test_file_form_resume_and_done_list(system, sel, tmp_path):
    one, frames, _ = system
    _, _, stats, parts = base(system, sel, "lr20")
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    word = fa.stats_word(ALL5)

    def run(tag, names=ALL5, **kw):
        p = {k: str(tmp_path / f"{tag}.{k}") for k in ("totals", "done", "stats", "parts")}
        kw.setdefault("devices", DEVS)
        extra = dict(stats=names, stats_path=p["stats"], partials_path=p["parts"]) if names else {}
        done, n_frames, _ = fa.trajectory_file_topology(path, one, p["totals"], selection=sel, done_path=p["done"], frames_per_batch=FPB, **extra, **kw)
        assert n_frames == F
        return p, done

    read = lambda name: open(name, "rb").read()
    # uninterrupted: the files are the memory form's bytes; no per-frame file but the totals
    p, done = run("all")
    assert done and read(p["stats"]) == stats.tobytes() and read(p["parts"]) == parts.tobytes()
    assert open(p["done"]).readline().endswith(" stats=%d\n" % word) and word == 1 + 2 + 8 + 16 + 32
    got = fa.traj_stats_read(p["stats"], ALL5, N, R, len(COMMANDS), partials_path=p["parts"], frames=SHARDS)
    assert same_bits(got.raw, stats) and got["residues"].shape == (4, R, 6)
    # block averages: any run of consecutive shards of the partials file
    assert same_bits(fa.traj_stats_merge(got.partials, got.frames, 1, 3), cut_ref(base(system, sel, "lr20")[1][3:], [3, 1])[0])
    # a repeated call on the complete run merges again: the same bytes
    os.remove(p["stats"])
    assert run("all")[1] and read(p["stats"]) == stats.tobytes()
    # stopped after one shard: not complete, no statistics file - a stale one is removed at the start of a run that is not resumed
    q = {k: str(tmp_path / f"part.{k}") for k in ("stats",)}
    open(q["stats"], "wb").write(b"stale")
    q, done = run("part", max_new_shards=1)
    assert not done and not os.path.exists(q["stats"]) and open(q["done"]).read().count("shard ") == 1
    # resumed on another device list: complete, byte for byte the uninterrupted run's files
    q, done = run("part", devices=[0])
    assert done and open(q["done"]).read().count("shard ") == 3
    assert read(q["stats"]) == stats.tobytes() and read(q["parts"]) == parts.tobytes() and read(q["totals"]) == read(p["totals"])
    # a done-list of a run with another statistics word is refused, and nothing is touched
    before = {k: read(v) for k, v in p.items()}
    with pytest.raises(RuntimeError, match="done-list belongs"):
        run("all", names=("atoms",))
    with pytest.raises(RuntimeError, match="done-list belongs"):
        run("all", names=None)
    assert before == {k: read(v) for k, v in p.items()}
    # a run without statistics keeps its first line and its list: stopped and resumed as before, refused with statistics
    r, done = run("none", names=None, max_new_shards=1)
    assert not done and " stats=" not in open(r["done"]).readline() and not os.path.exists(r["stats"]) and not os.path.exists(r["parts"])
    with pytest.raises(RuntimeError, match="done-list belongs"):
        run("none")
    r, done = run("none", names=None, devices=[0])
    assert done and read(r["totals"]) == read(p["totals"]) and not os.path.exists(r["stats"])


def test_dcd_with_periodic_images_and_a_gather(solvated, tmp_path):  # noqa: F811
    """The statistics of a periodic DCD run are those of the run's own per-frame files: the real atoms' areas, collected from
    among their images, are what the statistics read.  Plain entry: test_pbc_gpu.py's coil and cells; with a topology: 2jo4
    gathered from among 41 solvent atoms."""
    xyz, radii = tools.coil(37, 20261018)
    frames = jittered(xyz, 5, 1)
    dcd = tmp_path / "coil.dcd"
    write_dcd(dcd, frames, cell=True)
    patch_cells(dcd, [(14.0 + 0.3 * f, 13.0, 12.5 - 0.2 * f) for f in range(5)])
    p = {k: str(tmp_path / f"coil.{k}") for k in ("totals", "sasa", "done", "stats", "parts")}
    kw = dict(done_path=p["done"], frames_per_batch=2, dcd=True, devices=DEVS)
    done, n_frames = fa.trajectory_file(dcd, radii, p["totals"], p["sasa"], pbc=True, stats=("totals", "atoms"), stats_path=p["stats"],
                                        partials_path=p["parts"], **kw)
    assert done and n_frames == 5
    cols = columns(np.fromfile(p["totals"]), np.fromfile(p["sasa"]).reshape(5, 37))
    want, parts = cut_ref(cols, [2, 2, 1])
    assert open(p["stats"], "rb").read() == want.tobytes() and open(p["parts"], "rb").read() == parts.tobytes()
    plain = {k: str(tmp_path / f"plain.{k}") for k in ("totals", "sasa", "done")}
    fa.trajectory_file(dcd, radii, plain["totals"], plain["sasa"], done_path=plain["done"], frames_per_batch=2, dcd=True, devices=DEVS)
    assert np.all(np.fromfile(plain["totals"]) > cols[:, 0])                  # (the images bury area: it is the periodic run's numbers)
    # with a topology and an index
    b, full, index = solvated
    nf, n = 2, int(b.n_atoms)
    solute = full[:nf, index].astype(np.float64)
    cell = tuple(float(v) for v in solute.reshape(-1, 3).max(0) - solute.reshape(-1, 3).min(0) + 4.0)
    dcd = tmp_path / "solvated.dcd"
    write_dcd(dcd, full[:nf], cell=True)
    patch_cells(dcd, [cell, (cell[0] + 0.25, cell[1], cell[2])])
    q = {k: str(tmp_path / f"solv.{k}") for k in ("totals", "sasa", "done", "stats", "parts")}
    done, n_frames, _ = fa.trajectory_file_topology(dcd, b, q["totals"], atom_index=index, sasa_path=q["sasa"], done_path=q["done"],
                                                    frames_per_batch=1, devices=DEVS, dcd=True, pbc=True, stats=("totals", "atoms"),
                                                    stats_path=q["stats"], partials_path=q["parts"])
    assert done and n_frames == nf
    want, parts = cut_ref(columns(np.fromfile(q["totals"]), np.fromfile(q["sasa"]).reshape(nf, n)), [1, 1])
    assert open(q["stats"], "rb").read() == want.tobytes() and open(q["parts"], "rb").read() == parts.tobytes()
    assert np.all(parts[:, 1] == 0.0)


def test_narrowed_output_keeps_fp64_statistics(system, sel, tmp_path):
    one, frames, _ = system
    want, cols, stats, _ = base(system, sel, "lr20")
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    p = {k: str(tmp_path / f"f32.{k}") for k in ("totals", "sasa", "done", "stats", "parts")}
    done, _ = fa.trajectory_file(path, one.radii, p["totals"], p["sasa"], done_path=p["done"], frames_per_batch=FPB, devices=DEVS, out_f32=True,
                                 stats=("atoms",), stats_path=p["stats"], partials_path=p["parts"])
    assert done
    narrowed = np.fromfile(p["sasa"], dtype=np.float32).reshape(F, N)
    assert narrowed.tobytes() == want.sasa.astype(np.float32).tobytes()
    got = fa.traj_stats_read(p["stats"], ("atoms",), N)
    assert same_bits(got["atoms"], stats[:, 1:1 + N])                          # the statistics of the fp64 areas ...
    assert not same_bits(got["atoms"], cut_ref(narrowed.astype(np.float64), SHARDS)[0])   # ... not of the narrowed file
