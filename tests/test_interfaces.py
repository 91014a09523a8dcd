"""Interfaces between chain groups without a GPU (include/freesasa_gpu.h, freesasa_gpu_interfaces_dev): the kernels' phase
functions (csrc/iface_kernels.h) emulated on the CPU against the numpy restatement (tests/interfaces_ref.py) on the edge batch,
the same phases under AddressSanitizer + UBSan in a program of their own, the argument checks the entries make before a device
is touched, and the record format of tools/interfaces.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import freesasa_amd as fa
import interfaces_ref as ir
from emu import iface_emu


@pytest.fixture(scope="module")
def edge():
    return ir.edge_batch()[:5]


@pytest.fixture(scope="module")
def emulated(edge):
    return iface_emu.screen(*edge)


def test_the_edge_batch_holds_every_kind():
    assert iface_emu.shape() == (ir.WORKGROUP, ir.LDS_ATOMS)
    cov = ir.coverage()
    assert all(cov.values()), [k for k, v in cov.items() if not v]


def test_boxes_candidates_and_contacts_equal_the_restatement(edge, emulated):
    xyz, radii, offsets, group, n_groups = edge
    box, cand, flag = emulated
    tests, want_cand, want_hit = ir.screen(*edge)
    k = 0
    for s in range(len(n_groups)):
        for g in range(n_groups[s]):
            lo, hi, rmax = ir.box(xyz, radii, ir.members(offsets, group, s, g))
            assert np.array_equal(box[k, :3], lo) and np.array_equal(box[k, 3:6], hi) and box[k, 6] == rmax, (s, g)
            k += 1
    assert np.array_equal(cand, want_cand)
    assert np.array_equal(flag, want_hit)
    assert want_hit.sum() >= 8 and (~want_hit).sum() >= 8


def test_order_side_offsets_gather_and_finish_equal_the_restatement(edge, emulated):
    xyz, radii, offsets, group, n_groups = edge
    ps, pg, so, pa = ir.table(*edge)
    P, M = len(ps), len(pa)
    rng = np.random.default_rng(3)
    n, G = len(radii), int(n_groups.sum())
    n_iso = int((group >= 0).sum())
    csasa, ctot, psasa = rng.uniform(0, 60, n + n_iso), rng.uniform(0, 9000, len(n_groups) + G), rng.uniform(0, 60, M)
    got = iface_emu.table(*edge, emulated[2], P, M, csasa, ctot, psasa)
    assert got["n_pairs"] == P and got["n_pair_atoms"] == M
    assert np.array_equal(got["pair_struct"], ps) and np.array_equal(got["pair_groups"], pg)
    assert np.array_equal(got["side_offsets"], so) and np.array_equal(got["pair_atom"], pa)
    px, pr, _ = ir.pair_structures(xyz, radii, so, pa)
    assert np.array_equal(got["pxyz"], px) and np.array_equal(got["pradii"], pr)
    # the combined batch's atom of every pair-structure atom: the groups in structure-major order behind the n input atoms
    gbase = np.concatenate([[0], np.cumsum(n_groups)])
    key = np.where(group >= 0, gbase[np.searchsorted(offsets, np.arange(n), side="right") - 1] + group, -1)
    order = np.argsort(np.where(key < 0, G, key), kind="stable")[:n_iso]
    comb_of = np.full(n, -1)
    comb_of[order] = n + np.arange(n_iso)
    assert np.array_equal(got["pair_buried"], csasa[comb_of[pa]] - psasa)
    for p in range(P):
        kg, kh = gbase[ps[p]] + pg[p]
        a = got["pair_areas"][p]
        assert a[0] == ctot[len(n_groups) + kg] and a[1] == ctot[len(n_groups) + kh]
        for side in (0, 1):
            want = 0.0
            for v in psasa[so[2 * p + side]:so[2 * p + side + 1]]:
                want += v
            assert a[2 + side] == want and a[4 + side] == a[side] - a[2 + side]


def test_a_short_capacity_writes_nothing(edge, emulated):
    ps, pg, so, pa = ir.table(*edge)
    assert iface_emu.table(*edge, emulated[2], len(ps) - 1, len(pa)) is None
    assert iface_emu.table(*edge, emulated[2], len(ps), len(pa) - 1) is None
    assert iface_emu.table(*edge, emulated[2], len(ps), len(pa))["n_pairs"] == len(ps)


def test_the_phases_under_sanitizers():
    """tests/emu/iface_check: a program of its own built with -fsanitize=address,undefined; one line per case"""
    out = subprocess.run([iface_emu.build_check()], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(lines) >= 6 and all(" ok " in l for l in lines), out.stdout
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr


def _call_pairs(xyz, radii, offsets, group, n_groups, alg=0, resolution=20, cap=0, null=()):
    L = fa.lib()
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    xyz, radii = np.ascontiguousarray(xyz, np.float64).reshape(-1), np.ascontiguousarray(radii, np.float64)
    offsets, group, n_groups = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
    P, M, err = C.c_longlong(-5), C.c_longlong(-5), C.create_string_buffer(512)
    args = [xyz.ctypes.data_as(dp), radii.ctypes.data_as(dp), offsets.ctypes.data_as(lp), offsets.size - 1, group.ctypes.data_as(ip),
            n_groups.ctypes.data_as(ip), alg, 1.4, resolution, cap, C.byref(P), C.byref(M), None, None, None, -1, err, 512]
    for k in null:
        args[k] = None
    return L.freesasa_gpu_calc_interface_pairs(*args), err.value.decode(), P.value


def _call_whole(xyz, radii, offsets, group, n_groups, pcap=4, mcap=16, null=()):
    L = fa.lib()
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    xyz, radii = np.ascontiguousarray(xyz, np.float64).reshape(-1), np.ascontiguousarray(radii, np.float64)
    offsets, group, n_groups = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
    n = radii.size
    sasa, iso, areas = np.full(n, -7.0), np.full(n, -7.0), np.full(6 * max(pcap, 1), -7.0)
    P, M, err = C.c_longlong(-5), C.c_longlong(-5), C.create_string_buffer(512)
    args = [xyz.ctypes.data_as(dp), radii.ctypes.data_as(dp), offsets.ctypes.data_as(lp), offsets.size - 1, group.ctypes.data_as(ip),
            n_groups.ctypes.data_as(ip), 0, 1.4, 20, sasa.ctypes.data_as(dp), iso.ctypes.data_as(dp), None, None, pcap, mcap,
            C.byref(P), C.byref(M), None, None, areas.ctypes.data_as(dp), None, None, None, -1, err, 512]
    for k in null:
        args[k] = None
    rc = L.freesasa_gpu_calc_interfaces(*args)
    assert np.all(sasa == -7.0) and np.all(areas == -7.0)
    return rc, err.value.decode()


def test_arguments_are_checked_before_a_device_is_touched():
    """every refusal below comes with its own message, not with the one about the missing device, with or without a GPU"""
    xyz, radii = np.zeros((4, 3)), np.ones(4)
    off, g, ng = [0, 4], [0, 0, 1, 1], [2]
    for call, nulls in ((_call_pairs, (0, 1, 2, 4, 5, 10, 11)), (_call_whole, (0, 1, 2, 4, 5, 15, 16, 19))):
        for k in nulls:
            rc, msg, *_ = call(xyz, radii, off, g, ng, null=(k,))
            assert rc == -1 and msg == "null argument", (call.__name__, k, msg)
        for bad_off, text in (([1, 4], "offsets[0] must be 0"), ([0, 4, 3], "non-decreasing"), ([0, 0], "empty batch")):
            rc, msg, *_ = call(xyz, radii, bad_off, g, [2] * (len(bad_off) - 1))
            assert rc == -1 and text in msg, msg
        rc, msg, *_ = call(xyz, radii, [0, 2, 4], g, [2, 4097])
        assert rc == -1 and "structure 1" in msg and "4097" in msg and "4096" in msg, msg
        # 9 structures of 4096 groups: 75 479 040 pairs in the first nine, 134 184 960 with the 16 that pass 2^27
        rc, msg, *_ = call(np.zeros((17, 3)), np.ones(17), np.arange(18), np.zeros(17, np.int32), [4096] * 17)
        assert rc == -1 and "2^27" not in msg and "134217728" in msg and "structures 0 .. 16" in msg, msg
    rc, msg, _ = _call_pairs(xyz, radii, off, g, ng, cap=-1)
    assert rc == -1 and "pair_capacity" in msg and "-1" in msg
    rc, msg = _call_whole(xyz, radii, off, g, ng, pcap=-2)
    assert rc == -1 and "pair_capacity" in msg and "-2" in msg
    rc, msg = _call_whole(xyz, radii, off, g, ng, mcap=-3)
    assert rc == -1 and "atom_capacity" in msg and "-3" in msg
    rc, msg, _ = _call_pairs(xyz, radii, off, g, ng, alg=2)
    assert rc == -1 and "unknown algorithm 2" in msg
    rc, msg, _ = _call_pairs(xyz, radii, off, g, ng, resolution=0)
    assert rc == -1 and "resolution" in msg


def test_python_entries_check_their_shapes():
    with pytest.raises(ValueError):
        fa.calc_interfaces(np.zeros((4, 3)), np.ones(4), [0, 4], [0, 1, 0], [2])
    with pytest.raises(ValueError):
        fa.interface_pairs(np.zeros((4, 3)), np.ones(4), [0, 4], [0, 1, 0, 1], [2, 2])


def test_the_tool_formats_its_records():
    from tools import interfaces
    files, labels, atoms = ["a.pdb", "b.cif"], [["A", "B", "CD"], ["H/L", "AG1"]], [[10, 20, 30], [400, 5000]]
    areas = np.array([[100.0, 200.0, 90.0, 185.5, 10.0, 14.5], [1.0004, 2.0, 1.0, 2.0, 0.0004, 0.0], [5e4, 6e4, 4.9e4, 5.9e4, 1e3, 1e3]])
    lines = interfaces.format_rows(files, labels, atoms, np.array([0, 0, 1], np.int32), np.array([[0, 1], [1, 2], [0, 1]], np.int32), areas)
    assert lines == ["a.pdb\tA\tB\t10\t20\t100.000\t200.000\t90.000\t185.500\t10.000\t14.500",
                     "a.pdb\tB\tCD\t20\t30\t1.000\t2.000\t1.000\t2.000\t0.000\t0.000",
                     "b.cif\tH/L\tAG1\t400\t5000\t50000.000\t60000.000\t49000.000\t59000.000\t1000.000\t1000.000"]
    assert len(interfaces.HEADER.split("\t")) == len(lines[0].split("\t")) == 11
    assert interfaces.format_rows(files, labels, atoms, np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 6))) == []
