"""The residue contact occupancy map over a trajectory's interfaces without a GPU (include/freesasa_gpu.h,
freesasa_gpu_contact_occupancy_open): what the fixtures hold; the kernels' phase functions (csrc/occupancy_kernels.h) emulated on the
CPU against the plain-Python reduction (tests/contact_occupancy_ref.py), byte for byte, on the synthetic row lists and on the
numpy-restated rows of the trajectory fixture, in several cuts; the same phases under AddressSanitizer + UBSan in a program of their
own; the exports; the refusals made before a device is touched; the result class; and the record format of
tools/contact_occupancy.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import contact_occupancy_ref as occ
import freesasa_amd as fa
from emu import occupancy_emu

# what the restatements give for the trajectory fixture: pairs and folded rows per frame, and the rows of the run table
EXPECTED_COUNTS = {100: [[0, 0], [2, 13], [2, 21], [3, 50], [2, 35], [2, 32], [2, 32], [3, 49], [3, 39], [2, 15], [1, 1], [0, 0]]}
EXPECTED_ROWS = {100: 85}


def test_the_fixtures_hold_every_kind():
    cov = occ.coverage()
    assert len(cov) >= 16 and all(cov.values()), [k for k, v in cov.items() if not v]
    frames, counts = occ.traj_rows(100)
    assert counts.tolist() == EXPECTED_COUNTS[100] and len(occ.reduce(frames)["keys"]) == EXPECTED_ROWS[100]
    for rows in frames + occ.lists_frames():
        keys = [r[0] for r in rows]
        assert all(a < b for a, b in zip(keys, keys[1:]))
    for n_points in occ.TRAJ_POINTS:
        f, c = occ.traj_rows(n_points)
        assert occ.invariants(occ.reduce(f), c) == []
    assert occ.invariants(occ.reduce(occ.lists_frames())) == []


def _same(got, want, what=""):
    assert got["n_frames"] == want["n_frames"], what
    for k in occ.COLUMNS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


def _cuts(F):
    return {"all at once": [F], "one frame per call": [1] * F, "[1, F - 1]": [1, F - 1], "uneven": [2, 5, 1, F - 8]}


@pytest.mark.parametrize("fixture", ["LISTS", "TRAJ 100", "TRAJ 128"])
def test_the_emulated_phases_equal_the_reduction(fixture):
    frames = occ.lists_frames() if fixture == "LISTS" else occ.traj_rows(int(fixture.split()[1]))[0]
    want = occ.reduce(frames)
    for name, cuts in _cuts(len(frames)).items():
        for fpb in (1, 3, 256):
            with occupancy_emu.Accumulator() as acc:
                f0 = 0
                for c in cuts:
                    acc.add_rows(*occ.row_arrays(frames[f0:f0 + c]), frames_per_batch=fpb)
                    if f0 == 0:
                        acc.table()          # (a snapshot on the way changes nothing)
                    f0 += c
                _same(acc.table(), want, (fixture, name, fpb))
            if fixture == "LISTS" and name != "all at once":
                break                        # (the long lists in every cut, in chunks of one frame)


@pytest.mark.parametrize("n_points", occ.TRAJ_POINTS)
def test_the_emulated_keys_of_a_folded_table(n_points):
    """occ_keys: the restated folded table of the frames as ONE chunk, and cut into two batches"""
    frames, counts = occ.traj_rows(n_points)
    want = occ.reduce(frames)
    ps, pg, f = occ.traj_folded(n_points)
    n_res = len(occ.traj_system()[3]) - 1
    args = (f["rescontact_offsets"], f["rescontact_residues"], f["rescontact_counts"], f["rescontact_area"])
    with occupancy_emu.Accumulator() as acc:
        got_counts = acc.add_table(occ.N_FRAMES, n_res, ps, pg, *args)
        assert np.array_equal(got_counts, counts)
        _same(acc.table(), want)
    # frames 0 .. 4 and 5 .. 11 as two batches of their own: pairs and rows renumbered from the cut
    cut = 5
    p0 = int(np.searchsorted(ps, cut))
    q0 = int(f["rescontact_offsets"][2 * p0])
    with occupancy_emu.Accumulator() as acc:
        a = acc.add_table(cut, n_res, ps[:p0], pg[:p0], args[0][:2 * p0 + 1], args[1][:q0], args[2][:q0], args[3][:q0])
        b = acc.add_table(occ.N_FRAMES - cut, n_res, ps[p0:] - cut, pg[p0:], args[0][2 * p0:] - q0, args[1][q0:] - cut * n_res, args[2][q0:], args[3][q0:])
        assert np.array_equal(np.concatenate([a, b]), counts)
        _same(acc.table(), want)


def test_the_phases_under_sanitizers():
    """tests/emu/occ_check: a program of its own built with -fsanitize=address,undefined; one line per case"""
    out = subprocess.run([occupancy_emu.build_check()], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(lines) >= 7 and all(" ok " in l for l in lines), out.stdout
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr


def test_the_entries_are_exported_and_bound():
    L = fa.lib()
    for name, n_args in (("freesasa_gpu_contact_occupancy_open", 12), ("freesasa_gpu_contact_occupancy_add_frames", 4),
                         ("freesasa_gpu_contact_occupancy_add_rows", 6), ("freesasa_gpu_contact_occupancy_table", 2),
                         ("freesasa_gpu_contact_occupancy_table_free", 1), ("freesasa_gpu_contact_occupancy_close", 1),
                         ("freesasa_gpu_contact_occupancy_error", 1), ("freesasa_gpu_calc_contact_occupancy", 16)):
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("add", "add_rows", "table", "close", "__enter__", "__exit__"):
        assert callable(getattr(fa.ContactOccupancy, name))
    for name in ("occupancy", "occupancy_either", "mean_area", "pair_rows"):
        assert callable(getattr(fa.ContactOccupancyTable, name))
    assert callable(fa.contact_occupancy)
    L.freesasa_gpu_contact_occupancy_close(None)
    assert L.freesasa_gpu_contact_occupancy_error(None) == b"no accumulator"


def _open(radii, group, n_groups, res_first, n_points=100, null=()):
    L = fa.lib()
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    radii, group, res_first = np.ascontiguousarray(radii, np.float64), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(res_first, np.int64)
    err = C.create_string_buffer(512)
    args = [radii.ctypes.data_as(dp), radii.size, group.ctypes.data_as(ip), n_groups, res_first.ctypes.data_as(lp), res_first.size - 1, 1.4, n_points,
            0, -1, err, 512]
    for k in null:
        args[k] = None
    h = L.freesasa_gpu_contact_occupancy_open(*args)
    if h:
        L.freesasa_gpu_contact_occupancy_close(h)
    return h, err.value.decode()


def test_arguments_are_checked_before_a_device_is_touched():
    """every refusal below comes with its own message, not with the one about the missing device, with or without a GPU"""
    radii, g, rf = np.ones(6), [0, 0, 1, 1, -1, 1], [0, 2, 4, 6]
    for k in (0, 2, 4):
        h, msg = _open(radii, g, 2, rf, null=(k,))
        assert not h and msg == "null argument", (k, msg)
    # what the residue-residue contact entry refuses about the groups, the resolution and res_first, with its messages
    h, msg = _open(radii, g, 4097, rf)
    assert not h and "structure 0" in msg and "4097" in msg
    h, msg = _open(radii, g, 2, rf, n_points=129)
    assert not h and "128" in msg and "129" in msg
    h, msg = _open(radii, g, 2, rf, n_points=0)
    assert not h and msg == "resolution must be > 0"
    for bad_rf, text in (([1, 4, 6], "res_first[0] must be 0"), ([0, 4, 3, 6], "res_first must be non-decreasing"),
                         ([0, 4, 5], "res_first[n_res] is 5: the batch has 6 atoms")):
        h, msg = _open(radii, g, 2, bad_rf)
        assert not h and msg == text, msg
    h, msg = _open(radii, g, 2, [0])
    assert not h and msg == "n_res must be > 0"
    # its own: a group id outside -1 .. n_groups - 1, a system without atoms
    h, msg = _open(radii, [0, 0, 1, 2, -1, 1], 2, rf)
    assert not h and msg == "atom 3 has group id 2: ids are -1 (in no group) or 0 .. 1"
    h, msg = _open(radii, [0, 0, 1, -2, -1, 1], 2, rf)
    assert not h and "atom 3 has group id -2" in msg
    L = fa.lib()
    err = C.create_string_buffer(512)
    assert not L.freesasa_gpu_contact_occupancy_open(radii.ctypes.data_as(C.POINTER(C.c_double)), 0, None, 0, None, 0, 1.4, 100, 0, -1, err, 512)
    assert err.value == b"n_atoms must be > 0"
    # the one-shot form: its own NULLs, then the open's refusals
    t = fa._OccupancyTable()
    assert L.freesasa_gpu_calc_contact_occupancy(None, 0, None, 0, None, 0, None, 0, 1.4, 100, 0, None, C.byref(t), -1, err, 512) == -1
    assert err.value == b"null argument"
    with pytest.raises(RuntimeError, match="res_first\\[0\\] must be 0"):
        fa.contact_occupancy(np.zeros((2, 6, 3)), radii, g, 2, [1, 4, 6])
    with pytest.raises(ValueError):
        fa.contact_occupancy(np.zeros((2, 5, 3)), radii, g, 2, rf)
    with pytest.raises(ValueError):
        fa.ContactOccupancy(radii, g[:5], 2, rf)


def test_the_result_class():
    keys = np.array([[0, 1, 0, 2, 5], [0, 1, 0, 3, 5], [0, 1, 1, 5, 2], [0, 2, 0, 2, 9]], np.int32)
    t = fa.ContactOccupancyTable(8, keys, np.array([4, 2, 1, 8]), np.array([5, 2, 5, 8]), np.array([[4, 8], [2, 2], [1, 3], [8, 80]]),
                                 np.array([[10.0, 1.0, 4.0], [3.0, 1.0, 2.0], [0.5, 0.5, 0.5], [16.0, 2.0, 2.0]]), np.zeros((4, 2), np.int64),
                                 np.array([2, -1, 0, -1], np.int32))
    assert t.n_frames == 8 and t.n_rows == 4
    assert t.occupancy().tolist() == [0.5, 0.25, 0.125, 1.0] and t.occupancy_either().tolist() == [0.625, 0.25, 0.625, 1.0]
    assert t.mean_area().tolist() == [2.5, 1.5, 0.5, 2.0]
    assert t.pair_rows(0, 1, 0) == range(0, 2) and t.pair_rows(0, 1, 1) == range(2, 3) and t.pair_rows(0, 2, 0) == range(3, 4)
    assert t.pair_rows(0, 2, 1) == range(0, 0) and t.pair_rows(1, 2, 0) == range(0, 0)


def test_the_tool_formats_its_records():
    from tools import contact_occupancy as tool
    labels = ["A", "B", "C"]
    res_chain, res_name, res_number = ["A", "A", "B", "B", " "], ["ALA", "GLY", "SER", "TRP", "HOH"], ["1", "2A", "-3", "4", "9"]
    # pair (A, B): 0 -> 2 with its reverse, 1 -> 3 without; side B: 2 -> 0, 3 -> 0 without; pair (A, C): only side C, 4 -> 1
    keys = np.array([[0, 1, 0, 0, 2], [0, 1, 0, 1, 3], [0, 1, 1, 2, 0], [0, 1, 1, 3, 0], [0, 2, 1, 4, 1]], np.int32)
    frames, either = np.array([4, 1, 2, 8, 3]), np.array([5, 1, 5, 8, 3])
    counts = np.array([[4, 10], [1, 7], [2, 3], [8, 8], [3, 9]])
    area = np.array([[14.0, 0, 0], [0.25, 0, 0], [1.0, 0, 0], [2.0004, 0, 0], [6.0, 0, 0]])
    reverse = np.array([2, -1, 0, -1, -1], np.int32)
    lines = tool.format_rows(labels, 8, keys, frames, either, counts, area, reverse, res_chain, res_name, res_number)
    assert lines == ["A\tB\tA\tALA\t1\tB\tSER\t-3\t0.6250\t0.5000\t2.50\t3.500\t0.2500\t1.50\t0.500",
                     "A\tB\tA\tALA\t1\tB\tTRP\t4\t1.0000\t0.0000\t0.00\t0.000\t1.0000\t1.00\t0.250",
                     "A\tB\tA\tGLY\t2A\tB\tTRP\t4\t0.1250\t0.1250\t7.00\t0.250\t0.0000\t0.00\t0.000",
                     "A\tC\tA\tGLY\t2A\t_\tHOH\t9\t0.3750\t0.0000\t0.00\t0.000\t0.3750\t3.00\t2.000"]
    assert len(tool.HEADER.split("\t")) == len(lines[0].split("\t")) == 15
    with pytest.raises(SystemExit) as e:
        tool.main(["x.pdb", "run.dcd", "-o", "o.tsv"])
    assert "reader of your own" in str(e.value)
