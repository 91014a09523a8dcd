"""Atom-atom contact tables of the interfaces between chain groups without a GPU (include/freesasa_gpu.h,
freesasa_gpu_interface_contacts_dev): the kernels' phase functions (csrc/contact_kernels.h) emulated on the CPU against the numpy
restatement (tests/interface_contacts_ref.py) on the contact edge batch, bit for bit, at every point count of the GPU tests; the
same phases under AddressSanitizer + UBSan in a program of their own; the exports; the argument checks the host entry makes
before a device is touched; and the record formats of tools/interfaces.py --contacts / --residue-contacts."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import freesasa_amd as fa
import dots_ref as dr
import interfaces_ref as ir
import interface_contacts_ref as cr
from emu import contacts_emu

KEYS = ("buried_masks", "dot_first", "dot_partner", "contact_first", "contact_partner", "contact_points", "contact_area")


def test_the_contact_edge_batch_holds_every_kind():
    assert contacts_emu.shape() == cr.WORKGROUP
    cov = cr.coverage()
    assert len(cov) >= 13 and all(cov.values()), [k for k, v in cov.items() if not v]


def _pair_batch():
    xyz, radii, offsets, group, n_groups, _ = cr.contacts_edge_batch()
    _, _, so, pa = cr.edge_table()
    px, pr, _ = ir.pair_structures(xyz, radii, so, pa)
    return so, px, pr


@pytest.mark.parametrize("n_points", cr.N_POINTS)
def test_the_emulated_phases_equal_the_restatement(n_points):
    so, px, pr = _pair_batch()
    side, pair, want = cr.edge_contacts(n_points)
    got = contacts_emu.table(so, px, pr, cr.PROBE, cr.unit_points(n_points), dr.masks_of(side), dr.masks_of(pair))
    assert got["flag"] == 0
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    M = len(pr)
    assert got["n_dots"] == want["dot_first"][M] == len(want["dot_partner"]) and got["n_contacts"] == want["contact_first"][M]
    # the integer identity on the restatement's own masks, and the buried masks' stray bits
    per_atom = np.bincount(np.repeat(np.arange(M), np.diff(want["contact_first"])), weights=want["contact_points"], minlength=M).astype(np.int64)
    assert np.array_equal(per_atom, side.sum(axis=1) - pair.sum(axis=1))
    assert not (got["buried_masks"] & ~dr.full_words(n_points)).any()
    # rows ascend in j within an atom, and every partner lies on the other side of the same pair
    cf, cp = want["contact_first"], want["contact_partner"]
    rows_atom = np.repeat(np.arange(M), np.diff(cf))
    q_i, q_j = np.searchsorted(so, rows_atom, side="right") - 1, np.searchsorted(so, cp, side="right") - 1
    assert np.array_equal(q_j, q_i ^ 1)
    same = rows_atom[1:] == rows_atom[:-1]
    assert np.all(cp[1:][same] > cp[:-1][same])


def test_a_dot_without_a_cover_raises_the_flag_and_gets_no_partner():
    """masks that claim a buried point where the partner covers none: -1 for the dot, the flag names the atom"""
    so = np.array([0, 1, 2], np.int64)
    px, pr = np.array([[0.0, 0, 0], [50.0, 0, 0]]), np.array([1.5, 1.5])
    full = dr.masks_of(np.ones((2, 33), bool))
    lies = full.copy(); lies[1, 0] &= ~np.uint32(4)            # atom 1's point 2 "buried in the pair"
    got = contacts_emu.table(so, px, pr, cr.PROBE, cr.unit_points(33), full, lies)
    assert got["n_dots"] == 1 and got["flag"] == 2 and np.array_equal(got["dot_partner"], [-1])


def test_a_short_capacity_writes_nothing():
    so, px, pr = _pair_batch()
    side, pair, want = cr.edge_contacts(33)
    D, Cn = len(want["dot_partner"]), len(want["contact_partner"])
    sm, pm, unit = dr.masks_of(side), dr.masks_of(pair), cr.unit_points(33)
    assert contacts_emu.table(so, px, pr, cr.PROBE, unit, sm, pm, dot_cap=D, row_cap=Cn - 1) == (D, Cn)
    assert contacts_emu.table(so, px, pr, cr.PROBE, unit, sm, pm, dot_cap=D - 1, row_cap=Cn) == (D, Cn)
    assert contacts_emu.table(so, px, pr, cr.PROBE, unit, sm, pm, dot_cap=D, row_cap=Cn)["n_contacts"] == Cn


def test_the_phases_under_sanitizers():
    """tests/emu/contacts_check: a program of its own built with -fsanitize=address,undefined; one line per case"""
    out = subprocess.run([contacts_emu.build_check()], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(lines) >= 6 and all(" ok " in l for l in lines), out.stdout
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr


def test_the_entries_are_exported_and_bound():
    L = fa.lib()
    for name, n_args in (("freesasa_gpu_interface_contacts_dev", 34), ("freesasa_gpu_calc_interface_contacts", 36)):
        assert len(getattr(L, name).argtypes) == n_args, name
    assert callable(fa.calc_interface_contacts) and callable(fa.GpuContext.interface_contacts)
    assert issubclass(fa.InterfaceContacts, fa.Interfaces)


def _call(xyz, radii, offsets, group, n_groups, alg=1, n_points=100, pcap=4, mcap=16, ccap=16, dcap=16, null=()):
    L = fa.lib()
    dp, lp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    xyz, radii = np.ascontiguousarray(xyz, np.float64).reshape(-1), np.ascontiguousarray(radii, np.float64)
    offsets, group, n_groups = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
    n = radii.size
    sasa, iso, areas = np.full(n, -7.0), np.full(n, -7.0), np.full(6 * max(pcap, 1), -7.0)
    cf, cp, cn, ca = np.full(max(mcap, 0) + 1, -7, np.int64), np.full(max(ccap, 1), -7, np.int32), np.full(max(ccap, 1), -7, np.int32), np.full(max(ccap, 1), -7.0)
    bm, dpart = np.full(4 * max(mcap, 1), 7, np.uint32), np.full(max(dcap, 1), -7, np.int32)
    P, M, Cn, D, err = C.c_longlong(-5), C.c_longlong(-5), C.c_longlong(-5), C.c_longlong(-5), C.create_string_buffer(512)
    args = [xyz.ctypes.data_as(dp), radii.ctypes.data_as(dp), offsets.ctypes.data_as(lp), offsets.size - 1, group.ctypes.data_as(ip),
            n_groups.ctypes.data_as(ip), alg, 1.4, n_points, sasa.ctypes.data_as(dp), iso.ctypes.data_as(dp), None, None, pcap, mcap, ccap, dcap,
            C.byref(P), C.byref(M), C.byref(Cn), C.byref(D), None, None, areas.ctypes.data_as(dp), None, None, None, cf.ctypes.data_as(lp),
            cp.ctypes.data_as(ip), cn.ctypes.data_as(ip), ca.ctypes.data_as(dp), bm.ctypes.data_as(up), dpart.ctypes.data_as(ip), -1, err, 512]
    for k in null:
        args[k] = None
    rc = L.freesasa_gpu_calc_interface_contacts(*args)
    assert np.all(sasa == -7.0) and np.all(areas == -7.0) and np.all(cf == -7) and np.all(cp == -7) and np.all(cn == -7) and np.all(ca == -7.0)
    assert np.all(bm == 7) and np.all(dpart == -7) and (P.value, M.value, Cn.value, D.value) == (-5, -5, -5, -5)
    return rc, err.value.decode()


def test_arguments_are_checked_before_a_device_is_touched():
    """every refusal below comes with its own message, not with the one about the missing device, with or without a GPU"""
    xyz, radii = np.zeros((6, 3)), np.ones(6)
    off, g, ng = [0, 4, 6], [0, 0, 1, 1, 0, 1], [2, 2]
    for k in (0, 1, 2, 4, 5, 17, 18, 19, 23):
        rc, msg = _call(xyz, radii, off, g, ng, null=(k,))
        assert rc == -1 and msg == "null argument", (k, msg)
    # what the interface entries refuse, with their messages
    for bad_off, text in (([1, 6], "offsets[0] must be 0"), ([0, 6, 5], "non-decreasing"), ([0, 0], "empty batch")):
        rc, msg = _call(xyz, radii, bad_off, g, [2] * (len(bad_off) - 1))
        assert rc == -1 and text in msg, msg
    rc, msg = _call(xyz, radii, off, g, [2, 4097])
    assert rc == -1 and "structure 1" in msg and "4097" in msg
    rc, msg = _call(xyz, radii, off, g, ng, pcap=-2)
    assert rc == -1 and "pair_capacity" in msg and "-2" in msg
    rc, msg = _call(xyz, radii, off, g, ng, mcap=-3)
    assert rc == -1 and "atom_capacity" in msg and "-3" in msg
    # the contact table's own
    rc, msg = _call(xyz, radii, off, g, ng, alg=0)
    assert rc == -1 and "Lee-Richards" in msg and "Shrake-Rupley" in msg
    rc, msg = _call(xyz, radii, off, g, ng, n_points=129)
    assert rc == -1 and "128" in msg and "129" in msg
    rc, msg = _call(xyz, radii, off, g, ng, ccap=-4)
    assert rc == -1 and "contact_capacity" in msg and "-4" in msg
    rc, msg = _call(xyz, radii, off, g, ng, dcap=-6)
    assert rc == -1 and "dot_capacity" in msg and "-6" in msg


def test_the_result_class_gives_row_ranges():
    z = np.zeros(0)
    base = (z, z, z, z, np.zeros(1, np.int32), np.zeros((1, 2), np.int32), np.zeros((1, 6)), np.array([0, 2, 3]), np.array([0, 1, 2], np.int32), np.zeros(3))
    got = fa.InterfaceContacts(base, np.array([0, 2, 2, 5]), np.array([2, 2, 0, 0, 1], np.int32), np.ones(5, np.int32), np.ones(5), np.zeros((3, 4), np.uint32), 5)
    assert got.n_contacts == 5 and got.n_buried_dots == 5 and got.n_pairs == 1
    assert got.atom_rows(0) == slice(0, 2) and got.atom_rows(1) == slice(2, 2) and got.atom_rows(2) == slice(2, 5)
    assert got.side_rows(0, 0) == slice(0, 2) and got.side_rows(0, 1) == slice(2, 5)


def test_the_tool_formats_and_folds_its_contact_records():
    from tools import interfaces
    files, labels = ["a.pdb"], [["A", "B"]]
    res_chain, res_name, res_number = ["A", "A", "B"], ["ALA", "GLY", "SER"], ["1", "2A", "-3"]
    atom_res, atom_name = np.array([0, 0, 1, 2, 2]), [" N  ", " CA ", " O  ", " OG ", " CB "]
    so, pa = np.array([0, 3, 5]), np.array([0, 1, 2, 3, 4], np.int32)
    cf, cp = np.array([0, 1, 3, 3, 4, 5]), np.array([3, 3, 4, 1, 1], np.int32)
    points, area = np.array([2, 1, 4, 3, 1], np.int32), np.array([1.0, 0.5, 2.0004, 1.5, 0.25])
    row_pair, ai, aj = interfaces.contact_row_keys(so, pa, cf, cp)
    assert np.array_equal(row_pair, [0] * 5) and np.array_equal(ai, [0, 1, 1, 3, 4]) and np.array_equal(aj, [3, 3, 4, 1, 1])
    lines = interfaces.format_contact_rows(files, labels, np.array([0]), np.array([[0, 1]]), row_pair, ai, aj, points, area, atom_res, atom_name,
                                           res_chain, res_name, res_number)
    assert lines[0] == "a.pdb\tA\tB\tA\tALA\t1\tN\tB\tSER\t-3\tOG\t2\t1.000"
    assert lines[2] == "a.pdb\tA\tB\tA\tALA\t1\tCA\tB\tSER\t-3\tCB\t4\t2.000"
    assert lines[4] == "a.pdb\tA\tB\tB\tSER\t-3\tCB\tA\tALA\t1\tCA\t1\t0.250"
    assert len(interfaces.CONTACT_HEADER.split("\t")) == len(lines[0].split("\t")) == 13
    fold = interfaces.fold_contact_rows(row_pair, atom_res[ai], atom_res[aj], points, area)
    assert np.array_equal(fold[1], [0, 2]) and np.array_equal(fold[2], [2, 0]) and np.array_equal(fold[3], [7, 4])
    assert fold[4][0] == (1.0 + 0.5) + 2.0004 and fold[4][1] == 1.5 + 0.25          # added in row order
    rlines = interfaces.format_residue_contact_rows(files, labels, np.array([0]), np.array([[0, 1]]), fold, res_chain, res_name, res_number)
    assert rlines == ["a.pdb\tA\tB\tA\tALA\t1\tB\tSER\t-3\t7\t3.500", "a.pdb\tA\tB\tB\tSER\t-3\tA\tALA\t1\t4\t1.750"]
    assert len(interfaces.RESIDUE_CONTACT_HEADER.split("\t")) == len(rlines[0].split("\t")) == 11
    with pytest.raises(SystemExit) as e:
        interfaces.main(["x.pdb", "-o", "o.tsv", "--alg", "lr", "--contacts", "c.tsv"])
    assert "Shrake-Rupley" in str(e.value)
