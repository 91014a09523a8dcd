"""Interfaces between chain groups in the trajectory drivers (freesasa_gpu_trajectory_interfaces / _trajectory_file_interfaces) on
the device.  The system is 2jo4 with its four chains a group each and all six pairs; in two frames chain D is moved away, so its
three pairs do not touch there and still have their rows.  A row's in-pair columns are held to the plain entry (calc_batch) on
the pair structures cut on the host, summed in the restated order of the totals kernel (tests/traj_interfaces_ref.py), with ==;
the batch entry (calc_interfaces) on the frames tiled into one batch is the yardstick for the rows it lists; every output the run
shares with the groups' run must be that run's byte for byte.

A pair that does not touch: its in_pair is the sum of the terms of its iso in another order.  The bound |buried| <= N * 2^-53 *
iso, N = 129 the side's atoms, is the one tests/test_interfaces_gpu.py derives at its head for a sum of N areas."""
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import interfaces_ref as ir
import traj_interfaces_ref as tr
from freesasa_amd import ingest
from test_traj_groups_gpu import ALGS, COMMANDS, fnv1a, jitter

pytestmark = pytest.mark.gpu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
F, N, FPB, DEVS, G = 7, 516, 3, [0, 0], 4
AWAY = (2, 5)                       # the frames in which chain D is translated by (200, 0, 0)
PAIRS = tr.all_pairs(G)
K = len(PAIRS)
D_PAIRS = [k for k, (g, h) in enumerate(PAIRS) if h == 3]


@pytest.fixture(scope="module")
def sel():
    s = ingest.Selection(COMMANDS)
    yield s
    s.close()


@pytest.fixture(scope="module")
def system():
    """(batch, ids [516], frames [7, 516, 3], touch [7, 6] bool: do the pair's groups touch in the frame - decided on the CPU)"""
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    assert b.n_atoms == N
    ids = np.repeat(np.arange(G, dtype=np.int32), 129)
    got, ng, st = b.chain_groups(separate_chains=True)
    assert ng[0] == G and st[0] == 0 and np.array_equal(got, ids)
    frames = jitter(b.xyz, F, 20261018)
    for f in AWAY:
        frames[f, ids == 3] += (200.0, 0.0, 0.0)
    offsets = np.array([0, N])
    mem = [ir.members(offsets, ids, 0, g) for g in range(G)]
    touch = np.array([[bool(ir.contact_matrix(frames[f], b.radii, mem[g], mem[h]).any()) for g, h in PAIRS] for f in range(F)])
    for f in range(F):
        if f in AWAY:
            assert not touch[f, D_PAIRS].any()
        else:
            assert touch[f].sum() >= 2, f
    assert touch[:, D_PAIRS].any()                      # (chain D does touch the others where it was not moved)
    return b, ids, frames, touch


_RUNS = {}


def runs(system, sel, alg):
    """the groups' run without pairs and the run with all pairs, every output asked for (once per algorithm)"""
    if alg not in _RUNS:
        b, ids, frames, _ = system
        a, res = ALGS[alg]
        kw = dict(selection=sel, per_atom=True, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS, separate_chains=True)
        without = fa.trajectory_topology(frames, b, **kw)
        assert without.pair_areas is None and without.pair_groups is None
        _RUNS[alg] = (without, fa.trajectory_topology(frames, b, interface_pairs="all", **kw))
    return _RUNS[alg]


SHARED = ("totals", "sasa", "isolated", "group_areas", "group_atoms", "class_sums", "residues", "selection_areas", "selection_atoms")


def same_shared(got, want):
    for k in SHARED:
        assert np.ascontiguousarray(getattr(got, k)).tobytes() == np.ascontiguousarray(getattr(want, k)).tobytes(), k


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_the_shared_outputs_are_the_groups_runs(system, sel, alg):
    without, got = runs(system, sel, alg)
    same_shared(got, without)
    assert got.pair_areas.shape == (F, K, 6) and np.array_equal(got.pair_groups, PAIRS)


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_every_row_is_the_plain_entry_on_the_pair_structure_summed_in_the_totals_order(system, sel, alg):
    b, ids, frames, touch = system
    _, got = runs(system, sel, alg)
    a, res = ALGS[alg]
    pfirst, psrc = tr.cut(ids, PAIRS)
    n_pair = psrc.size
    assert n_pair == 2 * 129 * K
    # the pair structures of every frame cut on the host: one batch of F K structures through the plain entry
    offs = np.concatenate([f * n_pair + pfirst[:-1] for f in range(F)] + [[F * n_pair]]).astype(np.int64)
    areas, _, _ = fa.calc_batch(frames[:, psrc].reshape(-1, 3), np.tile(b.radii[psrc], F), offs, alg=a, resolution=res, device=0)
    for f in range(F):
        iso = got.group_areas[f, :, 0]
        want = tr.frame_rows(ids, PAIRS, iso, areas[f * n_pair:(f + 1) * n_pair])
        for k, (g, h) in enumerate(PAIRS):
            row = got.pair_areas[f, k]
            assert row[0] == iso[g] and row[1] == iso[h], (f, k)
            assert row[2] == want[k, 2] and row[3] == want[k, 3], (f, k, row, want[k])
            assert row[4] == row[0] - row[2] and row[5] == row[1] - row[3], (f, k)
    assert np.array_equal(got.pair_areas, np.stack([tr.frame_rows(ids, PAIRS, got.group_areas[f, :, 0], areas[f * n_pair:(f + 1) * n_pair])
                                                    for f in range(F)]))
    # what touches buries area on both sides
    assert np.all(got.pair_areas[touch][:, 4:] > 0)


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_the_batch_entry_lists_the_same_rows_and_the_others_are_rounding_noise(system, sel, alg):
    b, ids, frames, touch = system
    _, got = runs(system, sel, alg)
    a, res = ALGS[alg]
    offs = np.arange(F + 1, dtype=np.int64) * N
    ref = fa.calc_interfaces(frames.reshape(-1, 3), np.tile(b.radii, F), offs, np.tile(ids, F), np.full(F, G, np.int32), alg=a, resolution=res,
                             device=0, per_atom=True)
    P, M = ref.n_pairs, int(ref.side_offsets[-1])
    assert M >= 128 * P and M == 258 * P                # (that entry sums its sides by the totals kernel, as the trajectory always does)
    index = {(int(g), int(h)): k for k, (g, h) in enumerate(PAIRS)}
    listed = np.zeros((F, K), bool)
    for p in range(P):
        f, k = int(ref.pair_struct[p]), index[tuple(int(x) for x in ref.pair_groups[p])]
        listed[f, k] = True
        assert got.pair_areas[f, k].tobytes() == ref.pair_areas[p].tobytes(), (f, k, got.pair_areas[f, k], ref.pair_areas[p])
    assert np.array_equal(listed, touch)
    assert not listed[list(AWAY)][:, D_PAIRS].any() and P == touch.sum() >= 2 * (F - len(AWAY))
    for f, k in zip(*np.nonzero(~listed)):
        row = got.pair_areas[f, k]
        print("no contact: frame %d pair %d buried %.3e %.3e bound %.3e %.3e" % (f, k, row[4], row[5], 129 * 2.0 ** -53 * row[0], 129 * 2.0 ** -53 * row[1]))
        assert abs(row[4]) <= 129 * 2.0 ** -53 * row[0] and abs(row[5]) <= 129 * 2.0 ** -53 * row[1], (f, k, row)


def test_solute_scattered_among_decoys(system, sel):
    """the `full` / `index` of tests/test_traj_groups_gpu.py: 150 decoy atoms, the real ones scattered among them"""
    b, ids, frames, _ = system
    _, want = runs(system, sel, "lr20")
    rng = np.random.default_rng(5)
    index = rng.permutation(N + 150)[:N].astype(np.int32)
    full = rng.uniform(b.xyz.min(0), b.xyz.max(0), (F, N + 150, 3))
    full[:, index] = frames
    assert np.any(np.diff(index) < 0)
    got = fa.trajectory_topology(full, b, atom_index=index, selection=sel, per_atom=True, frames_per_batch=FPB, devices=DEVS,
                                 group=ids, n_groups=G, interface_pairs=PAIRS)
    same_shared(got, want)
    assert got.pair_areas.tobytes() == want.pair_areas.tobytes()


def test_an_empty_groups_sides_are_zero(system):
    b, _, frames, _ = system
    acb, ng, st = b.chain_groups("AC+B")
    assert ng[0] == 2 and st[0] == 0
    pairs = [(0, 1), (1, 2), (0, 2)]
    kw = dict(frames_per_batch=FPB, devices=DEVS, group=acb, n_groups=3)
    got = fa.trajectory_topology(frames, b, interface_pairs=pairs, **kw)
    without = fa.trajectory_topology(frames, b, **kw)
    assert np.array_equal(got.group_atoms, [258, 129, 0]) and got.pair_areas.shape == (F, 3, 6)
    assert got.group_areas.tobytes() == without.group_areas.tobytes() and got.totals.tobytes() == without.totals.tobytes()
    # group 2 is side h of pairs 1 and 2: iso, in_pair and buried exactly 0 (+0.0)
    assert got.pair_areas[:, 1:, 1::2].tobytes() == np.zeros((F, 2, 3)).tobytes()
    # the other side of those pairs is alone in its pair structure: the terms of its iso in another order.  Each of the two sums
    # of N non-negative terms has at most N - 1 rounded additions, each within 2^-53 of a partial sum <= the total: both are
    # within (N - 1) 2^-53 (1 + O(2^-53)) of the exact sum relative to it, their difference within 2 N 2^-53 of iso
    for k, g, atoms in ((1, 1, 129), (2, 0, 258)):
        row = got.pair_areas[:, k]
        assert np.array_equal(row[:, 0], got.group_areas[:, g, 0]) and np.all(row[:, 0] > 0)
        assert np.all(np.abs(row[:, 4]) <= 2 * atoms * 2.0 ** -53 * row[:, 0])
    # A and C against B
    assert np.array_equal(got.pair_areas[:, 0, :2], got.group_areas[:, :2, 0]) and np.all(got.pair_areas[:, 0, 4:] > 0)
    assert np.all(got.pair_areas[:, :, 4] == got.pair_areas[:, :, 0] - got.pair_areas[:, :, 2])


def test_the_file_form_resumes_equals_the_arrays_and_refuses_other_pairs(system, sel, tmp_path):
    b, ids, frames, _ = system
    _, want = runs(system, sel, "lr20")
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    p = {k: str(tmp_path / k) for k in ("totals", "sasa", "groups", "iso", "pairs", "done")}

    def run(pairs, **kw):
        return fa.trajectory_file_topology(path, b, p["totals"], sasa_path=p["sasa"], done_path=p["done"], frames_per_batch=FPB, group=ids,
                                           n_groups=G, group_areas_path=p["groups"], isolated_path=p["iso"], interface_pairs=pairs,
                                           pair_areas_path=p["pairs"], **kw)

    done, n_frames, _ = run("all", devices=DEVS, max_new_shards=1)
    assert not done and n_frames == F and open(p["done"]).read().count("shard ") == 1
    done, n_frames, _ = run("all", devices=[0])
    assert done and open(p["done"]).read().count("shard ") == 3
    for k, w in (("totals", want.totals), ("sasa", want.sasa), ("groups", want.group_areas), ("iso", want.isolated), ("pairs", want.pair_areas)):
        assert open(p[k], "rb").read() == np.ascontiguousarray(w).tobytes(), k
    # the first line: outputs= carries the pairs' bit, and at its end the digest of K and the pairs
    head = open(p["done"]).readline()
    digest = fnv1a(PAIRS.tobytes(), fnv1a(np.int32(K).tobytes()))
    assert " outputs=%d " % (1 + 16 + 32 + 256) in head and head.endswith(" pairs=%016x\n" % digest) and " groups=" in head
    # a list written for other pairs, or without them, belongs to another run - and so does this one for a run without pairs
    before = {k: open(p[k], "rb").read() for k in p}
    with pytest.raises(RuntimeError, match="done-list belongs"):
        run(PAIRS[:5], devices=DEVS)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        run(PAIRS[::-1].copy(), devices=DEVS)
    with pytest.raises(RuntimeError, match="done-list belongs"):
        fa.trajectory_file_topology(path, b, p["totals"], sasa_path=p["sasa"], done_path=p["done"], frames_per_batch=FPB, group=ids, n_groups=G,
                                    group_areas_path=p["groups"], isolated_path=p["iso"], devices=DEVS)
    assert before == {k: open(p[k], "rb").read() for k in p}
    q = {k: str(tmp_path / ("nopairs." + k)) for k in ("totals", "groups", "done")}
    done, _, _ = fa.trajectory_file_topology(path, b, q["totals"], done_path=q["done"], frames_per_batch=FPB, group=ids, n_groups=G,
                                             group_areas_path=q["groups"], devices=DEVS)
    assert done and "pairs=" not in open(q["done"]).readline()
    with pytest.raises(RuntimeError, match="done-list belongs"):
        fa.trajectory_file_topology(path, b, q["totals"], done_path=q["done"], frames_per_batch=FPB, group=ids, n_groups=G,
                                    group_areas_path=q["groups"], devices=DEVS, interface_pairs="all", pair_areas_path=str(tmp_path / "nopairs.pairs"))
    assert not os.path.exists(tmp_path / "nopairs.pairs")


def test_statistics_beside_the_pairs(system, sel):
    b, ids, frames, _ = system
    _, want = runs(system, sel, "lr20")
    kw = dict(frames_per_batch=FPB, devices=DEVS, separate_chains=True, stats=("groups",))
    without = fa.trajectory_topology(frames, b, **kw)
    got = fa.trajectory_topology(frames, b, interface_pairs="all", **kw)
    assert got.stats.raw.tobytes() == without.stats.raw.tobytes() and got.stats.partials.tobytes() == without.stats.partials.tobytes()
    assert got.stats["groups"].shape == (4, G, 3)
    assert got.pair_areas.tobytes() == want.pair_areas.tobytes() and got.group_areas.tobytes() == want.group_areas.tobytes()
    # computed for the statistics alone: the pairs come down, the groups' areas do not
    only = fa.trajectory_topology(frames, b, interface_pairs="all", per_frame=False, **kw)
    assert only.group_areas is None and only.pair_areas.tobytes() == want.pair_areas.tobytes()
    assert only.stats.raw.tobytes() == without.stats.raw.tobytes()
