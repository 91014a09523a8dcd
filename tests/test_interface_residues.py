"""Per-residue tables of the interfaces between chain groups without a GPU (include/freesasa_gpu.h,
freesasa_gpu_interface_residues_dev): the kernels' phase functions (csrc/iface_kernels.h, IfaceResArgs) emulated on the CPU against
the numpy restatement (tests/interface_residues_ref.py) on the residue edge batch with synthetic per-atom areas, the block scan
at the sizes where it takes another path, the same phases under AddressSanitizer + UBSan in a program of their own, the argument
checks the host entry makes before a device is touched, and the record format of tools/interfaces.py --residues."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import freesasa_amd as fa
import interface_residues_ref as rr
from emu import iface_res_emu


@pytest.fixture(scope="module")
def synthetic():
    """(side_offsets, pair_atom, res_first, iso [n], pair areas [M]): the edge batch's table with areas of which about half the
    atoms keep theirs in the pair, so that many segments lose nothing"""
    xyz, radii, offsets, group, n_groups, names, res_first = rr.residue_edge_batch()
    _, _, so, pa = rr.edge_table()
    rng = np.random.default_rng(11)
    iso = rng.uniform(0.0, 60.0, len(radii))
    keep = rng.uniform(size=len(pa)) < 0.5
    ps = np.where(keep, iso[pa], iso[pa] * rng.uniform(0.0, 1.0, len(pa)))
    # whole residues that lose nothing
    res = rr.residue_of(res_first, pa)
    ps = np.where(res % 3 == 0, iso[pa], ps)
    return so, pa, res_first, iso, ps


def test_the_residue_edge_batch_holds_every_kind():
    assert iface_res_emu.shape()[0] == rr.WORKGROUP
    cov = rr.coverage()
    assert all(cov.values()), [k for k, v in cov.items() if not v]


def _same(got, want):
    off, index, atoms, areas = want
    assert got["n_res_rows"] == len(index)
    assert np.array_equal(got["res_offsets"], off) and np.array_equal(got["res_index"], index) and np.array_equal(got["res_atoms"], atoms)
    assert got["res_areas"].tobytes() == areas.tobytes()


def test_heads_segments_rows_and_offsets_equal_the_restatement(synthetic):
    so, pa, res_first, iso, ps = synthetic
    heads, first, seg_res, seg_side = rr.segments(so, pa, res_first)
    got = iface_res_emu.table(so, pa, res_first, iso, ps, 0.0)
    assert np.array_equal(got["heads"], heads) and np.array_equal(got["seg_first"], first) and got["n_segments"] == len(seg_res)
    want = rr.rows(iso, ps, so, pa, res_first, 0.0)
    _same(got, want)
    R = len(want[1])
    assert 0 < R < len(seg_res)                                            # segments that lose nothing get no row
    for q in range(len(so) - 1):
        assert want[2][want[0][q]:want[0][q + 1]].sum() <= so[q + 1] - so[q]


def test_min_buried_is_strict_and_can_empty_the_table(synthetic):
    so, pa, res_first, iso, ps = synthetic
    off0, index0, atoms0, areas0 = rr.rows(iso, ps, so, pa, res_first, 0.0)
    k = len(index0) // 2
    cut = float(areas0[k, 2])
    want = rr.rows(iso, ps, so, pa, res_first, cut)
    gone = areas0[:, 2] <= cut
    assert gone[k] and np.array_equal(want[1], index0[~gone]) and want[3].tobytes() == areas0[~gone].tobytes()
    _same(iface_res_emu.table(so, pa, res_first, iso, ps, cut), want)
    below = iface_res_emu.table(so, pa, res_first, iso, ps, float(np.nextafter(cut, 0.0)))
    assert below["n_res_rows"] == len(want[1]) + int(np.sum(areas0[:, 2] == cut))
    none = iface_res_emu.table(so, pa, res_first, iso, ps, 1e300)
    assert none["n_res_rows"] == 0 and np.all(none["res_offsets"] == 0)


def test_a_short_capacity_writes_nothing(synthetic):
    so, pa, res_first, iso, ps = synthetic
    R = len(rr.rows(iso, ps, so, pa, res_first, 0.0)[1])
    K = len(rr.segments(so, pa, res_first)[2])
    assert iface_res_emu.table(so, pa, res_first, iso, ps, 0.0, res_cap=R - 1) == (K, R)
    assert iface_res_emu.table(so, pa, res_first, iso, ps, 0.0, res_cap=R)["n_res_rows"] == R


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 256 * 256, 256 * 256 + 1])
def test_the_scan_at_the_sizes_where_it_takes_another_path(n):
    """one workgroup holds 256 elements, a second level 256 blocks' sums: 65 537 elements need a third"""
    counts = np.random.default_rng(n).integers(0, 2, n).astype(np.int32)
    got, top = iface_res_emu.scan(counts)
    assert np.array_equal(got, np.concatenate([[0], np.cumsum(counts)]))
    assert top == (0 if n <= 256 else 1 if n <= 256 * 256 else 2)


def test_the_phases_under_sanitizers():
    """tests/emu/iface_res_check: a program of its own built with -fsanitize=address,undefined; one line per case"""
    out = subprocess.run([iface_res_emu.build_check()], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(lines) >= 12 and all(" ok " in l for l in lines), out.stdout
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr


def _call(xyz, radii, offsets, group, n_groups, res_first, min_buried=0.0, pcap=4, mcap=16, rcap=16, null=(), n_res=None, refused=True):
    L = fa.lib()
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    xyz, radii = np.ascontiguousarray(xyz, np.float64).reshape(-1), np.ascontiguousarray(radii, np.float64)
    offsets, group, n_groups = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
    res_first = np.ascontiguousarray(res_first, np.int64)
    n = radii.size
    sasa, iso, areas, rareas = np.full(n, -7.0), np.full(n, -7.0), np.full(6 * max(pcap, 1), -7.0), np.full(3 * max(rcap, 1), -7.0)
    P, M, R, err = C.c_longlong(-5), C.c_longlong(-5), C.c_longlong(-5), C.create_string_buffer(512)
    args = [xyz.ctypes.data_as(dp), radii.ctypes.data_as(dp), offsets.ctypes.data_as(lp), offsets.size - 1, group.ctypes.data_as(ip),
            n_groups.ctypes.data_as(ip), res_first.ctypes.data_as(lp), res_first.size - 1 if n_res is None else n_res, 0, 1.4, 20, min_buried,
            sasa.ctypes.data_as(dp), iso.ctypes.data_as(dp), None, None, pcap, mcap, rcap, C.byref(P), C.byref(M), C.byref(R), None, None,
            areas.ctypes.data_as(dp), None, None, None, None, None, None, rareas.ctypes.data_as(dp), -1, err, 512]
    for k in null:
        args[k] = None
    rc = L.freesasa_gpu_calc_interface_residues(*args)
    if refused:
        assert np.all(sasa == -7.0) and np.all(areas == -7.0) and np.all(rareas == -7.0) and (P.value, M.value, R.value) == (-5, -5, -5)
    return rc, err.value.decode()


def test_arguments_are_checked_before_a_device_is_touched():
    """every refusal below comes with its own message, not with the one about the missing device, with or without a GPU"""
    xyz, radii = np.zeros((6, 3)), np.ones(6)
    off, g, ng, rf = [0, 4, 6], [0, 0, 1, 1, 0, 1], [2, 2], [0, 2, 4, 6]
    for k in (0, 1, 2, 4, 5, 6, 19, 20, 21, 24, 31):
        rc, msg = _call(xyz, radii, off, g, ng, rf, null=(k,))
        assert rc == -1 and msg == "null argument", (k, msg)
    # what the interface entries refuse, with their messages
    for bad_off, text in (([1, 6], "offsets[0] must be 0"), ([0, 6, 5], "non-decreasing"), ([0, 0], "empty batch")):
        rc, msg = _call(xyz, radii, bad_off, g, [2] * (len(bad_off) - 1), rf)
        assert rc == -1 and text in msg, msg
    rc, msg = _call(xyz, radii, off, g, [2, 4097], rf)
    assert rc == -1 and "structure 1" in msg and "4097" in msg
    rc, msg = _call(xyz, radii, off, g, ng, rf, pcap=-2)
    assert rc == -1 and "pair_capacity" in msg and "-2" in msg
    rc, msg = _call(xyz, radii, off, g, ng, rf, mcap=-3)
    assert rc == -1 and "atom_capacity" in msg and "-3" in msg
    # the residue table's own
    rc, msg = _call(xyz, radii, off, g, ng, rf, rcap=-4)
    assert rc == -1 and "res_capacity" in msg and "-4" in msg
    rc, msg = _call(xyz, radii, off, g, ng, rf, n_res=0)
    assert rc == -1 and "n_res" in msg
    rc, msg = _call(xyz, radii, off, g, ng, [1, 2, 4, 6])
    assert rc == -1 and "res_first[0] must be 0" in msg
    rc, msg = _call(xyz, radii, off, g, ng, [0, 3, 2, 6])
    assert rc == -1 and "non-decreasing" in msg and "res_first" in msg
    rc, msg = _call(xyz, radii, off, g, ng, [0, 2, 4, 5])
    assert rc == -1 and "res_first[n_res]" in msg and "5" in msg and "6" in msg
    rc, msg = _call(xyz, radii, off, g, ng, [0, 3, 5, 6])
    assert rc == -1 and "residue 1" in msg and "structures 0 and 1" in msg
    rc, msg = _call(xyz, radii, off, g, ng, [0, 0, 4, 4, 6, 6], refused=False)   # empty residues, one on the boundary: fine as arguments
    assert "residue" not in msg and "res_first" not in msg
    for bad in (-1e-300, float("nan"), float("inf"), -float("inf")):
        rc, msg = _call(xyz, radii, off, g, ng, rf, min_buried=bad)
        assert rc == -1 and "min_buried" in msg, (bad, msg)


def test_python_entry_checks_res_first():
    with pytest.raises(ValueError):
        fa.calc_interfaces(np.zeros((4, 3)), np.ones(4), [0, 4], [0, 1, 0], [2], res_first=[0, 4])
    got = fa.Interfaces(*([np.zeros(0)] * 10))
    assert got.res_offsets is None and got.res_index is None and got.res_atoms is None and got.res_areas is None and got.n_res_rows is None
    with pytest.raises(ValueError):
        got.side_rows(0, 0)


def test_the_tool_formats_its_residue_records():
    from tools import interfaces
    files, labels = ["a.pdb"], [["A", "B"]]
    res_chain, res_name, res_number = ["A", "A", "B", "B"], ["ALA", "GLY", "SER", "TRP"], ["1", "2A", "-3", "10"]
    lines = interfaces.format_residue_rows(files, labels, np.array([0], np.int32), np.array([[0, 1]], np.int32), np.array([0, 1, 3]),
                                           np.array([1, 2, 3], np.int32), np.array([5, 2, 14], np.int32),
                                           np.array([[50.0, 40.5, 9.5], [10.0, 9.9996, 0.0004], [200.0, 100.0, 100.0]]),
                                           res_chain, res_name, res_number)
    assert lines == ["a.pdb\tA\tB\tA\tA\tGLY\t2A\t5\t50.000\t40.500\t9.500",
                     "a.pdb\tA\tB\tB\tB\tSER\t-3\t2\t10.000\t10.000\t0.000",
                     "a.pdb\tA\tB\tB\tB\tTRP\t10\t14\t200.000\t100.000\t100.000"]
    assert len(interfaces.RESIDUE_HEADER.split("\t")) == len(lines[0].split("\t")) == 11
