"""The residue contact occupancy map over a trajectory's interfaces on the device (include/freesasa_gpu.h:
freesasa_gpu_contact_occupancy_open, _add_frames, _add_rows, _table, freesasa_gpu_calc_contact_occupancy) against the plain-Python
reduction of tests/contact_occupancy_ref.py: synthetic row lists through add_rows in several cuts, the TRAJ fixture through
add_frames at 100 and 128 points against the numpy-restated rows, cut independence, snapshots, agreement with
calc_interface_contacts(res_first=) on TRAJ and on one larger shape, the table's invariants, refusals and the poisoned handle.

Everything is compared byte for byte: the counts are integers and the areas are sums in a defined order, so no tolerance is needed."""
import numpy as np
import pytest

import contact_occupancy_ref as occ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0, "no HIP device: the GPU tests cannot run"
    return freesasa_amd


def _bytes(t):
    return b"".join(np.ascontiguousarray(getattr(t, k) if not isinstance(t, dict) else t[k]).tobytes() for k in occ.COLUMNS)


def _same(got, want, what=""):
    assert got.n_frames == want["n_frames"], what
    for k in occ.COLUMNS:
        g, w = getattr(got, k), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


def _as_dict(t):
    return {k: getattr(t, k) for k in occ.COLUMNS}


def _cuts(F):
    return {"all at once": [F], "one frame per call": [1] * F, "[1, F - 1]": [1, F - 1], "uneven": [2, 5, 1, F - 8]}


def _system():
    radii, group, n_groups, res_first = occ.traj_system()
    return np.array(radii), np.array(group), n_groups, np.array(res_first)


def _run_frames(fa, xyz, cuts, n_points, frames_per_batch=0, system=None):
    radii, group, n_groups, res_first = system or _system()
    counts = []
    with fa.ContactOccupancy(radii, group, n_groups, res_first, n_points=n_points, frames_per_batch=frames_per_batch) as acc:
        f0 = 0
        for c in cuts:
            counts.append(acc.add(xyz[f0:f0 + c]))
            f0 += c
        assert f0 == len(xyz)
        return acc.table(), np.concatenate(counts)


# ------------------------------------------------------------------ 1. LISTS through add_rows

@pytest.fixture(scope="module")
def lists_want():
    return occ.reduce(occ.lists_frames())


@pytest.mark.parametrize("cut", ["all at once", "one frame per call", "[1, F - 1]", "uneven"])
def test_lists_through_add_rows(fa, lists_want, cut):
    frames = occ.lists_frames()
    with fa.ContactOccupancy(None) as acc:
        f0 = 0
        for c in _cuts(len(frames))[cut]:
            acc.add_rows(*occ.row_arrays(frames[f0:f0 + c]))
            f0 += c
        got = acc.table()
    _same(got, lists_want, cut)
    assert occ.invariants(_as_dict(got)) == []
    assert int(got.frames.sum()) == sum(len(r) for r in frames)


def test_lists_in_small_chunks(fa, lists_want):
    """frames_per_batch of a rows-only accumulator: the chunks of one call"""
    for fpb in (1, 4):
        with fa.ContactOccupancy(None, frames_per_batch=fpb) as acc:
            acc.add_rows(*occ.row_arrays(occ.lists_frames()))
            _same(acc.table(), lists_want, fpb)


# ------------------------------------------------------------------ 2. TRAJ through add_frames

@pytest.mark.parametrize("n_points", occ.TRAJ_POINTS)
def test_traj_through_add_frames(fa, n_points):
    frames, counts = occ.traj_rows(n_points)
    want = occ.reduce(frames)
    got, got_counts = _run_frames(fa, np.array(occ.traj_frames()), [occ.N_FRAMES], n_points)
    assert got_counts.dtype == np.int64 and np.array_equal(got_counts, counts)
    _same(got, want, n_points)
    assert occ.invariants(_as_dict(got), got_counts) == []
    assert np.array_equal(got.occupancy(), want["frames"] / occ.N_FRAMES) and np.array_equal(got.mean_area(), want["area"][:, 0] / want["frames"])
    assert np.array_equal(got.occupancy_either(), want["frames_either"] / occ.N_FRAMES)
    rows = got.pair_rows(0, 1, 1)
    assert len(rows) > 0 and all(tuple(got.keys[k][:3]) == (0, 1, 1) for k in rows) and len(rows) == int(((want["keys"][:, :3] == (0, 1, 1)).all(axis=1)).sum())
    one_shot, c2 = fa.contact_occupancy(np.array(occ.traj_frames()), *_system(), n_points=n_points, frame_counts=True)
    assert _bytes(one_shot) == _bytes(got) and np.array_equal(c2, counts)


# ------------------------------------------------------------------ 3. cut independence

def test_cut_independence_on_traj(fa):
    xyz, F = np.array(occ.traj_frames()), occ.N_FRAMES
    first, first_counts = _run_frames(fa, xyz, [F], 100)
    assert first.n_rows > 0
    for fpb in (1, 2, 5, F, F + 1):
        for name, cuts in _cuts(F).items():
            got, counts = _run_frames(fa, xyz, cuts, 100, frames_per_batch=fpb)
            assert got.n_frames == F and _bytes(got) == _bytes(first), (fpb, name)
            assert np.array_equal(counts, first_counts), (fpb, name)


# ------------------------------------------------------------------ 4. snapshot

def test_a_snapshot_leaves_the_run_alone(fa):
    xyz, F = np.array(occ.traj_frames()), occ.N_FRAMES
    full, _ = _run_frames(fa, xyz, [F], 100)
    fresh, _ = _run_frames(fa, xyz[:5], [5], 100)
    radii, group, n_groups, res_first = _system()
    with fa.ContactOccupancy(radii, group, n_groups, res_first, frames_per_batch=3) as acc:
        assert acc.table().n_rows == 0 and acc.table().n_frames == 0
        acc.add(xyz[:5])
        snap = acc.table()
        assert snap.n_frames == 5 and _bytes(snap) == _bytes(fresh)
        assert _bytes(acc.table()) == _bytes(snap)
        acc.add(xyz[5:])
        end = acc.table()
    assert end.n_frames == F and _bytes(end) == _bytes(full)
    assert _bytes(snap) == _bytes(fresh)          # (the snapshot's arrays are the caller's own)


# ------------------------------------------------------------------ 5. agreement with the batch entry

def _batch_reduction(fa, xyz, radii, group, n_groups, res_first, n_points):
    """the frames as ONE batch through calc_interface_contacts(res_first=), its folded rows re-keyed and reduced in Python"""
    F, n = xyz.shape[:2]
    n_res = len(res_first) - 1
    brf = np.concatenate([res_first[:-1] + f * n for f in range(F)] + [[F * n]]).astype(np.int64)
    got = fa.calc_interface_contacts(xyz.reshape(-1, 3), np.tile(radii, F), np.arange(F + 1, dtype=np.int64) * n, np.tile(group, F),
                                     np.full(F, n_groups, np.int32), n_points=n_points, res_first=brf)
    frames = occ.frames_of_batch(F, n_res, got.pair_struct, got.pair_groups, got.rescontact_offsets, got.rescontact_residues,
                                 got.rescontact_counts, got.rescontact_area)
    counts = np.zeros((F, 2), np.int64)
    for s in got.pair_struct:
        counts[s, 0] += 1
    counts[:, 1] = [len(r) for r in frames]
    return occ.reduce(frames), counts


def test_agreement_with_the_batch_entry_on_traj(fa):
    radii, group, n_groups, res_first = _system()
    xyz = np.array(occ.traj_frames())
    want, counts = _batch_reduction(fa, xyz, radii, group, n_groups, res_first, 100)
    got, got_counts = _run_frames(fa, xyz, [5, 7], 100, frames_per_batch=4)
    _same(got, want)
    assert np.array_equal(got_counts, counts)


def test_agreement_with_the_batch_entry_on_a_larger_system(fa):
    """40 frames of 600 atoms in 3 groups interleaved in one jittering cloud: U well above 1024, chunks of 7 frames"""
    rng = np.random.default_rng(20261022)
    n, F = 600, 40
    base = rng.uniform(0, np.cbrt(40.0 * n), (n, 3))
    radii, group = rng.uniform(1.0, 2.0, n), (np.arange(n) // 5 % 3).astype(np.int32)
    res_first = np.arange(0, n + 1, 5, dtype=np.int64)
    xyz = np.array([base + rng.normal(0, 0.4, (n, 3)) for _ in range(F)])
    xyz[7] = xyz[6]
    want, counts = _batch_reduction(fa, xyz, radii, group, 3, res_first, 100)
    assert len(want["keys"]) > 2048
    got, got_counts = _run_frames(fa, xyz, [13, 27], 100, frames_per_batch=7, system=(radii, group, 3, res_first))
    _same(got, want)
    assert np.array_equal(got_counts, counts)
    assert occ.invariants(_as_dict(got), got_counts) == []


# ------------------------------------------------------------------ 7. refusals and the poisoned handle

def test_a_failed_add_poisons_the_handle(fa):
    radii, group, n_groups, res_first = _system()
    xyz = np.array(occ.traj_frames())
    bad = xyz[3:9].copy()
    bad[4, 17, 1] = np.nan                                  # frame 7 of the run
    acc = fa.ContactOccupancy(radii, group, n_groups, res_first, frames_per_batch=4)
    acc.add(xyz[:3])
    before = _bytes(acc.table())
    # an argument error before the device is touched leaves the handle usable
    with pytest.raises(RuntimeError, match="frame 0, row 0: side must be 0 or 1"):
        acc.add_rows([0, 1], [[0, 1, 2, 0, 0]], [[1, 1]], [1.0])
    assert _bytes(acc.table()) == before
    with pytest.raises(RuntimeError) as e:
        acc.add(bad)
    first = str(e.value)
    assert "frame 7 of the run" in first and "non-finite coordinate" in first
    for call in (lambda: acc.add(xyz[:1]), acc.table, lambda: acc.add_rows([0], np.zeros((0, 5)), np.zeros((0, 2)), np.zeros(0))):
        with pytest.raises(RuntimeError) as e2:
            call()
        assert "frame 7 of the run" in str(e2.value)
    acc.close()
    acc.close()
    # the context went back to the pool in working order
    got, _ = _run_frames(fa, xyz, [occ.N_FRAMES], 100)
    assert got.n_rows > 0


def test_add_rows_validates_on_the_host(fa):
    """every refusal names the frame and the row, and leaves the accumulator as it was"""
    good = ([0, 2, 3], [[0, 1, 0, 4, 5], [0, 1, 1, 5, 4], [0, 1, 0, 4, 5]], [[1, 2], [3, 4], [1, 1]], [1.5, 2.5, 0.5])
    bad = [(dict(first=[1, 2, 3]), "frame_first[0] must be 0"), (dict(first=[0, 3, 2]), "frame_first must be non-decreasing (frame 1)"),
           (dict(key=(2, [1, 1, 0, 4, 5])), "frame 1, row 0: the groups must be 0 <= g < h (they are 1, 1)"),
           (dict(key=(0, [-1, 1, 0, 4, 5])), "frame 0, row 0: the groups must be 0 <= g < h (they are -1, 1)"),
           (dict(key=(1, [0, 1, 2, 5, 4])), "frame 0, row 1: side must be 0 or 1 (it is 2)"),
           (dict(key=(1, [0, 1, 1, -5, 4])), "frame 0, row 1: the residues must be >= 0 (they are -5, 4)"),
           (dict(key=(1, [0, 1, 0, 4, 5])), "frame 0, row 1: the keys of a frame must be strictly ascending"),
           (dict(key=(1, [0, 1, 0, 4, 4])), "frame 0, row 1: the keys of a frame must be strictly ascending"),
           (dict(count=(2, [1, 0])), "frame 1, row 0: both counts must be >= 1 (they are 1, 0)"),
           (dict(area=(1, np.inf)), "frame 0, row 1: the area is not finite"), (dict(area=(2, np.nan)), "frame 1, row 0: the area is not finite")]
    with fa.ContactOccupancy(None) as acc:
        acc.add_rows(*good)
        before = _bytes(acc.table())
        for change, text in bad:
            first, keys, counts, area = [np.array(a) for a in good]
            if "first" in change:
                first = np.array(change["first"])
            if "key" in change:
                keys[change["key"][0]] = change["key"][1]
            if "count" in change:
                counts[change["count"][0]] = change["count"][1]
            if "area" in change:
                area[change["area"][0]] = change["area"][1]
            with pytest.raises(RuntimeError) as e:
                acc.add_rows(first, keys, counts, area)
            assert str(e.value).split(": ", 1)[1] == text
            t = acc.table()
            assert t.n_frames == 2 and _bytes(t) == before
        acc.add_rows(*good)
        t = acc.table()
    assert t.n_frames == 4 and t.frames.tolist() == [4, 2] and t.frames_either.tolist() == [4, 4] and t.reverse.tolist() == [1, 0]
    assert t.area.tolist() == [[(1.5 + 0.5) + 1.5 + 0.5, 0.5, 1.5], [5.0, 2.5, 2.5]] and t.span.tolist() == [[0, 3], [0, 2]]
    assert t.counts.tolist() == [[4, 6], [6, 8]]


def test_rows_only_accumulators_refuse_frames(fa):
    with fa.ContactOccupancy(None) as acc:
        with pytest.raises(RuntimeError, match="takes rows, not frames"):
            acc.add(np.zeros((0, 3)))
        acc.add_rows([0, 0, 0], np.zeros((0, 5)), np.zeros((0, 2)), np.zeros(0))
        t = acc.table()
        assert t.n_frames == 2 and t.n_rows == 0 and t.keys.shape == (0, 5)
