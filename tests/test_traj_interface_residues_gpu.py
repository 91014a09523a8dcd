"""Per-residue interface tables per frame of a trajectory (freesasa_gpu_trajectory_interface_residues / _file_interface_residues)
on the device.  The system is that of tests/test_traj_interfaces_gpu.py: 2jo4 with its four chains a group each and all six
pairs, 7 frames in shards of 3, chain D moved away in frames 2 and 5.  The dense table is held to the restatement
(tests/traj_interface_residues_ref.py) with == in all four columns, fed with the run's own isolated per-atom output and with the
plain entry (calc_batch) on the pair structures cut on the host; the batch entry (calc_interfaces with res_first) on the frames
tiled into one batch is the yardstick for the rows it lists; every output shared with the interfaces run must be that run's byte
for byte; the two new statistics outputs are held to the statistics definition restated on the delivered tables.

min_buried is 0.0 for Shrake-Rupley and 1.0 A^2 for Lee-Richards: a last bit of an arc sum must not flip the flag of a residue
that is not in the interface, and 1.0 A^2 is far above the 1e-8 per atom the project asserts for that algorithm."""
import os

import numpy as np
import pytest

import freesasa_amd as fa
import traj_interface_residues_ref as tq
import traj_interfaces_ref as tr
from test_dcd import write_dcd
from test_traj_groups_gpu import ALGS
from test_traj_interfaces_gpu import AWAY, D_PAIRS, DEVS, F, FPB, G, K, N, PAIRS, runs, same_shared, sel, system  # noqa: F401  (sel, system: fixtures)
from test_traj_stats import cut_ref, same_bits

pytestmark = pytest.mark.gpu

MIN_BURIED = {"lr20": 1.0, "sr100": 0.0}
SHARDS = [3, 3, 1]
_RES = {}


def res_first_of(b):
    assert b.offsets[0] == 0 and b.res_offsets[0] == 0
    return b.res_first[:int(b.res_offsets[1]) + 1].copy()


def res_run(system, sel, alg):  # noqa: F811
    """the run with all pairs and their per-residue table, every output asked for (once per algorithm)"""
    if alg not in _RES:
        b, ids, frames, _ = system
        a, res = ALGS[alg]
        _RES[alg] = fa.trajectory_topology(frames, b, selection=sel, per_atom=True, alg=a, resolution=res, frames_per_batch=FPB, devices=DEVS,
                                           separate_chains=True, interface_pairs="all", interface_residues=True, min_buried=MIN_BURIED[alg])
    return _RES[alg]


def segs(system):
    b, ids, _, _ = system
    return tq.segments(ids, G, PAIRS, res_first_of(b))


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_the_shared_outputs_are_the_interfaces_runs(system, sel, alg):  # noqa: F811
    _, want = runs(system, sel, alg)
    got = res_run(system, sel, alg)
    same_shared(got, want)
    assert got.pair_areas.tobytes() == want.pair_areas.tobytes() and np.array_equal(got.pair_groups, PAIRS)
    assert want.pair_residues is None and want.pair_res_offsets is None


def test_the_segments_the_run_reports_are_the_segments_entrys(system, sel):  # noqa: F811
    b, ids, _, _ = system
    got = res_run(system, sel, "sr100")
    offs, res, atoms = fa.traj_pair_segments(b, ids, G, PAIRS)
    first, seg_res, seg_side, pside, psrc = segs(system)
    S = seg_res.size
    assert got.pair_residues.shape == (F, S, 4) and S > 2 * K
    assert np.array_equal(got.pair_res_offsets, offs) and np.array_equal(got.pair_res_index, res) and np.array_equal(got.pair_res_atoms, atoms)
    assert np.array_equal(res, seg_res) and np.array_equal(atoms, np.diff(first)) and np.array_equal(offs, tq.side_offsets(seg_side, K))
    for k in range(K):
        for q in (0, 1):
            assert np.all(seg_side[got.side_segments(k, q)] == 2 * k + q)


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_the_dense_table_is_the_restatement(system, sel, alg):  # noqa: F811
    b, ids, frames, touch = system
    got = res_run(system, sel, alg)
    a, res = ALGS[alg]
    first, seg_res, seg_side, pside, psrc = segs(system)
    pfirst, psrc2 = tr.cut(ids, PAIRS)
    assert np.array_equal(psrc, psrc2)
    n_pair = psrc.size
    # the pair structures of every frame cut on the host: one batch of F K structures through the plain entry
    offs = np.concatenate([f * n_pair + pfirst[:-1] for f in range(F)] + [[F * n_pair]]).astype(np.int64)
    areas, _, _ = fa.calc_batch(frames[:, psrc].reshape(-1, 3), np.tile(b.radii[psrc], F), offs, alg=a, resolution=res, device=0)
    want = np.stack([tq.frame_table(got.isolated[f], areas[f * n_pair:(f + 1) * n_pair], first, psrc, MIN_BURIED[alg]) for f in range(F)])
    for c, name in enumerate(("iso_res", "in_pair_res", "buried_res", "in_interface")):
        assert np.all(got.pair_residues[:, :, c] == want[:, :, c]), (name, np.argwhere(got.pair_residues[:, :, c] != want[:, :, c])[:5])
    # what touches has residues in the interface on both sides; the flags are flags
    flags = got.pair_residues[:, :, 3]
    assert set(np.unique(flags)) == {0.0, 1.0}
    for f, k in zip(*np.nonzero(touch)):
        for q in (0, 1):
            assert flags[f, got.side_segments(k, q)].sum() >= 1, (f, k, q)
    # a side's segments are its atoms: their iso sums are the group's isolated total to rounding
    for k, (g, h) in enumerate(PAIRS):
        for q, x in enumerate((g, h)):
            tot = got.pair_residues[:, got.side_segments(k, q), 0].sum(1)
            assert np.all(np.abs(tot - got.group_areas[:, x, 0]) <= 129 * 2.0 ** -52 * got.group_areas[:, x, 0])


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_the_batch_entry_lists_the_rows_that_are_in_the_interface(system, sel, alg):  # noqa: F811
    b, ids, frames, touch = system
    got = res_run(system, sel, alg)
    a, res = ALGS[alg]
    rf = res_first_of(b)
    R = rf.size - 1
    tiled = np.concatenate([rf[:-1] + f * N for f in range(F)] + [[F * N]]).astype(np.int64)
    offs = np.arange(F + 1, dtype=np.int64) * N
    ref = fa.calc_interfaces(frames.reshape(-1, 3), np.tile(b.radii, F), offs, np.tile(ids, F), np.full(F, G, np.int32), alg=a, resolution=res,
                             device=0, res_first=tiled, min_buried=MIN_BURIED[alg])
    index = {(int(g), int(h)): k for k, (g, h) in enumerate(PAIRS)}
    dense = got.pair_residues
    listed_pair = np.zeros((F, K), bool)
    listed_row = np.zeros(dense.shape[:2], bool)
    for p in range(ref.n_pairs):
        f, k = int(ref.pair_struct[p]), index[tuple(int(x) for x in ref.pair_groups[p])]
        listed_pair[f, k] = True
        for q in (0, 1):
            mine = got.side_segments(k, q)
            seg_of = {int(r): s for s, r in zip(range(mine.start, mine.stop), got.pair_res_index[mine])}
            assert len(seg_of) == mine.stop - mine.start
            rows = ref.side_rows(p, q)
            for row in range(rows.start, rows.stop):
                r = int(ref.res_index[row]) - f * R
                s = seg_of[r]
                assert ref.res_atoms[row] == got.pair_res_atoms[s]
                assert np.all(ref.res_areas[row] == dense[f, s, :3]), (f, k, q, r, ref.res_areas[row], dense[f, s])
                assert dense[f, s, 3] == 1.0
                listed_row[f, s] = True
    # not vacuous: rows for every (frame, pair) that touches
    assert np.array_equal(listed_pair, touch) and listed_row.sum() == ref.n_res_rows >= 2 * touch.sum()
    for f, k in zip(*np.nonzero(touch)):
        both = slice(got.side_segments(k, 0).start, got.side_segments(k, 1).stop)
        assert listed_row[f, both].any(), (f, k)
    # every dense row in the interface of a pair that entry lists is listed; of the others, none is listed
    for f in range(F):
        for k in range(K):
            both = slice(got.side_segments(k, 0).start, got.side_segments(k, 1).stop)
            if listed_pair[f, k]:
                assert np.array_equal(listed_row[f, both], dense[f, both, 3] == 1.0), (f, k)
            else:
                assert not listed_row[f, both].any()


@pytest.mark.parametrize("alg", ["lr20", "sr100"])
def test_a_chain_moved_away_is_in_no_interface(system, sel, alg):  # noqa: F811
    got = res_run(system, sel, alg)
    for f in AWAY:
        for k in D_PAIRS:
            both = slice(got.side_segments(k, 0).start, got.side_segments(k, 1).stop)
            assert both.stop - both.start >= 2
            assert np.all(got.pair_residues[f, both, 3] == 0.0), (f, k)
            if alg == "sr100":      # (the same points are free in the pair as in the group taken on its own: the same areas, added in the same order)
                assert np.all(got.pair_residues[f, both, 2] == 0.0), (f, k)
    assert got.pair_residues[:, :, 3].sum() > 0


def stat_columns(r):
    return np.concatenate([r.pair_areas.reshape(F, -1), r.pair_residues.reshape(F, -1)], axis=1)


def test_statistics_of_both_pair_outputs(system, sel, tmp_path):  # noqa: F811
    b, ids, frames, _ = system
    base = res_run(system, sel, "lr20")
    S = base.pair_res_index.size
    kw = dict(frames_per_batch=FPB, separate_chains=True, interface_pairs="all", interface_residues=True, min_buried=MIN_BURIED["lr20"],
              stats=("pairs", "pair_residues"))
    got = fa.trajectory_topology(frames, b, devices=DEVS, **kw)
    assert got.pair_areas.tobytes() == base.pair_areas.tobytes() and got.pair_residues.tobytes() == base.pair_residues.tobytes()
    want, parts = cut_ref(stat_columns(got), SHARDS)
    assert got.stats.raw.shape == (4, 6 * K + 4 * S)
    assert same_bits(got.stats.raw, want) and same_bits(got.stats.partials, parts)
    assert same_bits(got.stats["pairs"], want[:, :6 * K].reshape(4, K, 6)) and same_bits(got.stats["pair_residues"], want[:, 6 * K:].reshape(4, S, 4))
    # occupancy: the mean of the fourth column is the fraction of the frames in which the residue is in the interface
    occ = got.stats["pair_residues"][0, :, 3]
    count = got.pair_residues[:, :, 3].sum(0)
    assert np.all(np.abs(occ * F - count) < 1e-6) and 0 < count.sum() < F * S and count.max() == F
    # beside the other outputs' statistics the columns lie behind the groups'
    mixed = fa.trajectory_topology(frames, b, devices=DEVS, **dict(kw, stats=("totals", "groups", "pairs", "pair_residues")))
    assert same_bits(mixed.stats.raw[:, 1 + 3 * G:], want) and mixed.stats["groups"].shape == (4, G, 3)
    # one device, and nothing delivered: the same bytes
    one = fa.trajectory_topology(frames, b, devices=[0], **kw)
    assert one.stats.raw.tobytes() == got.stats.raw.tobytes() and one.stats.partials.tobytes() == got.stats.partials.tobytes()
    none = fa.trajectory_topology(frames, b, devices=DEVS, per_frame=False, **kw)
    assert none.pair_areas is None and none.pair_residues is None and none.group_areas is None
    assert none.stats.raw.tobytes() == got.stats.raw.tobytes() and none.stats.partials.tobytes() == got.stats.partials.tobytes()
    # a file run cut by max_new_shards = 1 and resumed, its outputs in the statistics word alone
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    p = {k: str(tmp_path / k) for k in ("totals", "stats", "parts", "done")}

    def run(**more):
        return fa.trajectory_file_topology(path, b, p["totals"], done_path=p["done"], frames_per_batch=FPB, separate_chains=True,
                                           interface_pairs="all", min_buried=MIN_BURIED["lr20"], stats=("pairs", "pair_residues"),
                                           stats_path=p["stats"], partials_path=p["parts"], **more)

    done, n_frames, _ = run(devices=DEVS, max_new_shards=1)
    assert not done and n_frames == F and not os.path.exists(p["stats"])
    done, _, _ = run(devices=[0])
    assert done
    assert open(p["stats"], "rb").read() == got.stats.raw.tobytes() and open(p["parts"], "rb").read() == got.stats.partials.tobytes()
    head = open(p["done"]).readline()
    assert " outputs=0 " in head and " minburied=%016x" % np.float64(MIN_BURIED["lr20"]).view(np.uint64) in head and head.endswith(" stats=384\n")
    rs = fa.traj_stats_read(p["stats"], ("pairs", "pair_residues"), N, n_groups=G, n_pairs=K, n_segments=S)
    assert same_bits(rs["pair_residues"], got.stats["pair_residues"])


def test_the_file_form_equals_the_arrays_resumes_and_refuses_other_lists(system, sel, tmp_path):  # noqa: F811
    b, ids, frames, _ = system
    want = res_run(system, sel, "lr20")
    mb = MIN_BURIED["lr20"]
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    p = {k: str(tmp_path / k) for k in ("totals", "sasa", "groups", "iso", "pairs", "pres", "done")}

    def run(pairs="all", min_buried=mb, **kw):
        return fa.trajectory_file_topology(path, b, p["totals"], sasa_path=p["sasa"], done_path=p["done"], frames_per_batch=FPB, group=ids,
                                           n_groups=G, group_areas_path=p["groups"], isolated_path=p["iso"], interface_pairs=pairs,
                                           pair_areas_path=p["pairs"], pair_residues_path=p["pres"], min_buried=min_buried, **kw)

    done, n_frames, _ = run(devices=DEVS, max_new_shards=1)
    assert not done and n_frames == F and open(p["done"]).read().count("shard ") == 1
    done, _, _ = run(devices=[0])
    assert done and open(p["done"]).read().count("shard ") == 3
    for k, w in (("totals", want.totals), ("sasa", want.sasa), ("groups", want.group_areas), ("iso", want.isolated), ("pairs", want.pair_areas),
                 ("pres", want.pair_residues)):
        assert open(p[k], "rb").read() == np.ascontiguousarray(w).tobytes(), k
    head = open(p["done"]).readline()
    assert " outputs=%d " % (1 + 16 + 32 + 256 + 512) in head and " pairs=" in head
    assert head.endswith(" minburied=%016x\n" % np.float64(mb).view(np.uint64))
    # another min_buried, other pairs, the plain interfaces run: each is another run
    before = {k: open(p[k], "rb").read() for k in p}
    with pytest.raises(RuntimeError, match="done-list belongs.*min_buried"):
        run(min_buried=0.5, devices=DEVS)
    with pytest.raises(RuntimeError, match="done-list belongs.*interface pairs"):
        run(pairs=PAIRS[:5], devices=DEVS)
    with pytest.raises(RuntimeError, match="done-list belongs.*interface pairs"):
        fa.trajectory_file_topology(path, b, p["totals"], sasa_path=p["sasa"], done_path=p["done"], frames_per_batch=FPB, group=ids, n_groups=G,
                                    group_areas_path=p["groups"], isolated_path=p["iso"], interface_pairs="all", pair_areas_path=p["pairs"],
                                    devices=DEVS)
    assert before == {k: open(p[k], "rb").read() for k in p}
    # ... and the list of the plain interfaces run is refused by this one
    q = {k: str(tmp_path / ("plain." + k)) for k in ("totals", "pairs", "pres", "done")}
    done, _, _ = fa.trajectory_file_topology(path, b, q["totals"], done_path=q["done"], frames_per_batch=FPB, group=ids, n_groups=G,
                                             interface_pairs="all", pair_areas_path=q["pairs"], devices=DEVS)
    assert done and "minburied=" not in open(q["done"]).readline()
    assert open(q["pairs"], "rb").read() == want.pair_areas.tobytes()
    with pytest.raises(RuntimeError, match="done-list belongs.*min_buried"):
        fa.trajectory_file_topology(path, b, q["totals"], done_path=q["done"], frames_per_batch=FPB, group=ids, n_groups=G,
                                    interface_pairs="all", pair_areas_path=q["pairs"], pair_residues_path=q["pres"], min_buried=mb, devices=DEVS)
    assert not os.path.exists(q["pres"])


def test_a_dcd_run_equals_the_raw_run_of_the_same_values(system, tmp_path):  # noqa: F811
    b, ids, frames, _ = system
    f32 = frames.astype(np.float32)
    raw, dcd = tmp_path / "frames.f32", tmp_path / "frames.dcd"
    f32.tofile(raw)
    write_dcd(dcd, f32)
    out = {}
    for tag, path, kw in (("raw", raw, dict(f32=True)), ("dcd", dcd, dict(dcd=True))):
        p = {k: str(tmp_path / (tag + "." + k)) for k in ("totals", "pairs", "pres")}
        done, n_frames, _ = fa.trajectory_file_topology(path, b, p["totals"], frames_per_batch=FPB, group=ids, n_groups=G, interface_pairs="all",
                                                        pair_areas_path=p["pairs"], pair_residues_path=p["pres"], min_buried=1.0, devices=DEVS, **kw)
        assert done and n_frames == F
        out[tag] = {k: open(p[k], "rb").read() for k in p}
    assert out["raw"] == out["dcd"] and len(out["raw"]["pres"]) == 8 * F * 4 * segs(system)[1].size


def test_the_occupancy_tool_writes_the_statistics(system, sel, tmp_path):  # noqa: F811
    """tools/interface_occupancy.py on two frame files taken as one run: its columns are the merged statistics of the dense table"""
    import tools.interface_occupancy as tool
    from conftest import ROOT
    b, ids, frames, _ = system
    base = res_run(system, sel, "lr20")
    first, second = tmp_path / "a.f64", tmp_path / "b.f64"
    frames[:4].tofile(first)
    frames[4:].tofile(second)
    out = tmp_path / "occ.tsv"
    tool.main([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb"), str(first), str(second), "-o", str(out), "--min-buried", "1.0",
               "--frames-per-batch", "3", "--devices", "0,0"])
    lines = open(out).read().split("\n")
    S = base.pair_res_index.size
    assert lines[0] == tool.HEADER and len(lines) == S + 2 and lines[-1] == ""
    table = base.pair_residues
    for s in (0, 1, S // 2, S - 1):
        cols = lines[1 + s].split("\t")
        assert int(cols[6]) == base.pair_res_atoms[s]
        assert abs(float(cols[7]) - table[:, s, 2].mean()) <= 1e-3 and abs(float(cols[8]) - table[:, s, 2].std()) <= 1e-3
        assert abs(float(cols[9]) - table[:, s, 2].min()) <= 1e-3 and abs(float(cols[10]) - table[:, s, 2].max()) <= 1e-3
        assert abs(float(cols[11]) - table[:, s, 0].mean()) <= 1e-3 and abs(float(cols[12]) - table[:, s, 3].mean()) <= 1e-4
    assert lines[1].split("\t")[:3] == ["A", "B", "A"] and lines[S].split("\t")[:3] == ["C", "D", "D"]
