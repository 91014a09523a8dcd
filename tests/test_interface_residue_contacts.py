"""Residue-residue contact tables of the interfaces between chain groups without a GPU (include/freesasa_gpu.h,
freesasa_gpu_interface_residue_contacts_dev): what the batch holds; the kernels' phase functions (csrc/rescontact_kernels.h)
emulated on the CPU against the numpy restatement (tests/interface_residue_contacts_ref.py), bit for bit, at every point count of
the GPU tests; the same phases under AddressSanitizer + UBSan in a program of their own; the exports; the argument checks the
host entry makes before a device is touched; the result class's row ranges; and the record format of tools/interfaces.py
--contact-map."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import freesasa_amd as fa
import interface_residue_contacts_ref as qr
from emu import rescontacts_emu

# what the issue's author counted on the project's own restatements: n atoms, residues, P, M, K, and C and Q per point count
EXPECTED = dict(n=1266, n_res=202, P=24, M=1434, K=251, C={1: 94, 31: 977, 32: 991, 33: 998, 100: 1291, 128: 1388},
                Q={1: 48, 31: 372, 32: 372, 33: 376, 100: 467, 128: 501})


def test_the_batch_holds_every_kind():
    wave, stage = rescontacts_emu.shape()
    assert wave == qr.WAVE
    cov = qr.coverage(stage)
    assert len(cov) >= 9 and all(cov.values()), [k for k, v in cov.items() if not v]
    b, (ps, pg, so, pa) = qr.rescontacts_batch(), qr.batch_table()
    assert (int(b[2][-1]), len(b[6]) - 1, len(ps), len(pa)) == (EXPECTED["n"], EXPECTED["n_res"], EXPECTED["P"], EXPECTED["M"])
    # the large segments the issue names: 300 rows to 100 partner residues, 384 to 128
    for n, rows in ((100, 300), (128, 384)):
        f = qr.batch_fold(n)
        a = int(np.argmax(f["seg_rows"]))
        assert f["seg_rows"][a] == rows and np.count_nonzero(f["row_seg"] == a) == n


def _inputs(n_points):
    _, _, so, pa = qr.batch_table()
    c = qr.batch_contacts(n_points)
    return so, pa, qr.rescontacts_batch()[6], c["contact_first"], c["contact_partner"], c["contact_points"], c["contact_area"]


@pytest.mark.parametrize("n_points", qr.N_POINTS)
def test_the_emulated_phases_equal_the_restatement(n_points):
    want = qr.batch_fold(n_points)
    got = rescontacts_emu.table(*_inputs(n_points))
    assert (len(qr.batch_contacts(n_points)["contact_partner"]), got["n_rescontacts"]) == (EXPECTED["C"][n_points], EXPECTED["Q"][n_points])
    assert got["n_segments"] == len(want["seg_rows"]) == EXPECTED["K"]
    for k in qr.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    # the restatement's own identities: rows and points are conserved, reverse is an involution with swapped residues
    c = qr.batch_contacts(n_points)
    assert want["rescontact_counts"][:, 0].sum() == len(c["contact_partner"]) and want["rescontact_counts"][:, 1].sum() == c["contact_points"].sum()
    rev, res = want["rescontact_reverse"], want["rescontact_residues"]
    has = np.nonzero(rev >= 0)[0]
    assert np.array_equal(rev[rev[has]], has) and np.array_equal(res[rev[has]], res[has][:, ::-1])
    assert want["rescontact_offsets"][-1] == len(rev) and np.all(np.diff(want["rescontact_offsets"]) >= 0)


def test_one_atom_residues_fold_to_the_atom_table():
    """res_first = arange(n + 1): every folded row is one contact row"""
    so, pa, _, cf, cp, cn, ca = _inputs(33)
    n = int(qr.rescontacts_batch()[2][-1])
    got = rescontacts_emu.table(so, pa, np.arange(n + 1), cf, cp, cn, ca)
    rows_atom = np.repeat(np.arange(len(pa)), np.diff(cf))
    assert got["n_rescontacts"] == len(cp) and got["n_segments"] == len(pa)
    assert np.array_equal(got["rescontact_residues"], np.stack([pa[rows_atom], pa[cp]], axis=1))
    assert np.array_equal(got["rescontact_counts"], np.stack([np.ones(len(cp), np.int32), cn], axis=1))
    assert got["rescontact_area"].tobytes() == ca.tobytes()
    assert np.array_equal(got["rescontact_offsets"], cf[so])


def test_a_short_capacity_writes_nothing():
    args = _inputs(33)
    K, Q = EXPECTED["K"], EXPECTED["Q"][33]
    assert rescontacts_emu.table(*args, row_cap=Q - 1) == (K, Q)
    assert rescontacts_emu.table(*args, row_cap=0) == (K, Q)
    assert rescontacts_emu.table(*args, row_cap=Q)["n_rescontacts"] == Q


def test_the_phases_under_sanitizers():
    """tests/emu/rescontacts_check: a program of its own built with -fsanitize=address,undefined; one line per case"""
    out = subprocess.run([rescontacts_emu.build_check()], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(lines) >= 7 and all(" ok " in l for l in lines), out.stdout
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr


def test_the_entries_are_exported_and_bound():
    L = fa.lib()
    for name, n_args in (("freesasa_gpu_interface_residue_contacts_dev", 43), ("freesasa_gpu_calc_interface_residue_contacts", 45)):
        assert len(getattr(L, name).argtypes) == n_args, name
    assert callable(fa.GpuContext.interface_residue_contacts)
    import inspect
    assert inspect.signature(fa.calc_interface_contacts).parameters["res_first"].default is None


def _call(xyz, radii, offsets, group, n_groups, res_first, alg=1, n_points=100, pcap=4, mcap=16, ccap=16, dcap=16, qcap=16, null=()):
    L = fa.lib()
    dp, lp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    xyz, radii = np.ascontiguousarray(xyz, np.float64).reshape(-1), np.ascontiguousarray(radii, np.float64)
    offsets, group, n_groups = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
    res_first = np.ascontiguousarray(res_first, np.int64)
    n = radii.size
    sasa, iso, areas = np.full(n, -7.0), np.full(n, -7.0), np.full(6 * max(pcap, 1), -7.0)
    cf, cp, cn, ca = np.full(max(mcap, 0) + 1, -7, np.int64), np.full(max(ccap, 1), -7, np.int32), np.full(max(ccap, 1), -7, np.int32), np.full(max(ccap, 1), -7.0)
    bm, dpart = np.full(4 * max(mcap, 1), 7, np.uint32), np.full(max(dcap, 1), -7, np.int32)
    q = max(qcap, 1)
    qo, qr_, qc, qa, qv = np.full(2 * max(pcap, 0) + 1, -7, np.int64), np.full(2 * q, -7, np.int32), np.full(2 * q, -7, np.int32), np.full(q, -7.0), np.full(q, -7, np.int32)
    P, M, Cn, D, Q, err = C.c_longlong(-5), C.c_longlong(-5), C.c_longlong(-5), C.c_longlong(-5), C.c_longlong(-5), C.create_string_buffer(512)
    args = [xyz.ctypes.data_as(dp), radii.ctypes.data_as(dp), offsets.ctypes.data_as(lp), offsets.size - 1, group.ctypes.data_as(ip),
            n_groups.ctypes.data_as(ip), alg, 1.4, n_points, sasa.ctypes.data_as(dp), iso.ctypes.data_as(dp), None, None, pcap, mcap, ccap, dcap,
            C.byref(P), C.byref(M), C.byref(Cn), C.byref(D), None, None, areas.ctypes.data_as(dp), None, None, None, cf.ctypes.data_as(lp),
            cp.ctypes.data_as(ip), cn.ctypes.data_as(ip), ca.ctypes.data_as(dp), bm.ctypes.data_as(up), dpart.ctypes.data_as(ip),
            res_first.ctypes.data_as(lp), res_first.size - 1, qcap, C.byref(Q), qo.ctypes.data_as(lp), qr_.ctypes.data_as(ip), qc.ctypes.data_as(ip),
            qa.ctypes.data_as(dp), qv.ctypes.data_as(ip), -1, err, 512]
    for k in null:
        args[k] = None
    rc = L.freesasa_gpu_calc_interface_residue_contacts(*args)
    assert np.all(sasa == -7.0) and np.all(areas == -7.0) and np.all(cf == -7) and np.all(cp == -7) and np.all(cn == -7) and np.all(ca == -7.0)
    assert np.all(bm == 7) and np.all(dpart == -7) and np.all(qo == -7) and np.all(qr_ == -7) and np.all(qc == -7) and np.all(qa == -7.0) and np.all(qv == -7)
    assert (P.value, M.value, Cn.value, D.value, Q.value) == (-5, -5, -5, -5, -5)
    return rc, err.value.decode()


def test_arguments_are_checked_before_a_device_is_touched():
    """every refusal below comes with its own message, not with the one about the missing device, with or without a GPU"""
    xyz, radii = np.zeros((6, 3)), np.ones(6)
    off, g, ng, rf = [0, 4, 6], [0, 0, 1, 1, 0, 1], [2, 2], [0, 2, 4, 6]
    for k in (0, 1, 2, 4, 5, 17, 18, 19, 23, 33, 36, 40):          # ... res_first, n_rescontacts_out, rescontact_area
        rc, msg = _call(xyz, radii, off, g, ng, rf, null=(k,))
        assert rc == -1 and msg == "null argument", (k, msg)
    # what the interface entries and the contact entry refuse, with their messages
    for bad_off, text in (([1, 6], "offsets[0] must be 0"), ([0, 6, 5], "non-decreasing"), ([0, 0], "empty batch")):
        rc, msg = _call(xyz, radii, bad_off, g, [2] * (len(bad_off) - 1), rf)
        assert rc == -1 and text in msg, msg
    rc, msg = _call(xyz, radii, off, g, [2, 4097], rf)
    assert rc == -1 and "structure 1" in msg and "4097" in msg
    for kw, words in ((dict(pcap=-2), ("pair_capacity", "-2")), (dict(mcap=-3), ("atom_capacity", "-3")), (dict(alg=0), ("Lee-Richards", "Shrake-Rupley")),
                      (dict(n_points=129), ("128", "129")), (dict(ccap=-4), ("contact_capacity", "-4")), (dict(dcap=-6), ("dot_capacity", "-6"))):
        rc, msg = _call(xyz, radii, off, g, ng, rf, **kw)
        assert rc == -1 and all(w in msg for w in words), msg
    # what the per-residue entry refuses about res_first, with its messages
    for bad_rf, text in (([1, 4, 6], "res_first[0] must be 0"), ([0, 4, 3, 6], "res_first must be non-decreasing"),
                         ([0, 4, 5], "res_first[n_res] is 5: the batch has 6 atoms"), ([0, 3, 6], "residue 1 spans the boundary between structures 0 and 1")):
        rc, msg = _call(xyz, radii, off, g, ng, bad_rf)
        assert rc == -1 and msg == text, msg
    rc, msg = _call(xyz, radii, off, g, ng, [0])
    assert rc == -1 and msg == "n_res must be > 0"
    # its own
    rc, msg = _call(xyz, radii, off, g, ng, rf, qcap=-8)
    assert rc == -1 and msg == "rescontact_capacity must be >= 0 (it is -8)"


def test_the_result_class_gives_residue_row_ranges():
    z = np.zeros(0)
    base = (z, z, z, z, np.zeros(2, np.int32), np.zeros((2, 2), np.int32), np.zeros((2, 6)), np.array([0, 2, 3, 4, 6]), np.arange(6, dtype=np.int32), np.zeros(6))
    contacts = (np.array([0, 2, 2, 5, 5, 5, 5]), np.array([2, 2, 0, 0, 1], np.int32), np.ones(5, np.int32), np.ones(5), np.zeros((6, 4), np.uint32), 5)
    folded = (np.array([0, 1, 3, 3, 3]), np.zeros((3, 2), np.int32), np.ones((3, 2), np.int32), np.ones(3), np.array([1, 0, -1], np.int32))
    got = fa.InterfaceContacts(base, *contacts, folded)
    assert got.n_rescontacts == 3 and got.n_contacts == 5
    assert got.residue_side_rows(0, 0) == range(0, 1) and got.residue_side_rows(0, 1) == range(1, 3)
    assert got.residue_side_rows(1, 0) == range(3, 3) and got.residue_side_rows(1, 1) == range(3, 3)
    plain = fa.InterfaceContacts(base, *contacts)
    assert plain.n_rescontacts is None and plain.rescontact_area is None and plain.atom_rows(0) == slice(0, 2)
    with pytest.raises(ValueError):
        plain.residue_side_rows(0, 0)


def test_the_tool_formats_its_contact_map():
    from tools import interfaces
    files, labels = ["a.pdb"], [["A", "B", "C"]]
    res_chain, res_name, res_number = ["A", "A", "B", "B", " "], ["ALA", "GLY", "SER", "TRP", "HOH"], ["1", "2A", "-3", "4", "9"]
    pair_struct, pair_groups = np.array([0, 0]), np.array([[0, 1], [0, 2]])
    # pair (A, B): 0 -> 2 (with its reverse), 0 -> 3 (without), 1 -> 2 (with); side B: 2 -> 0, 2 -> 1, 3 -> 1 (without)
    # pair (A, C): nothing from A; side C: 4 -> 1 (without)
    offsets = np.array([0, 3, 6, 6, 7])
    residues = np.array([[0, 2], [0, 3], [1, 2], [2, 0], [2, 1], [3, 1], [4, 1]], np.int32)
    counts = np.array([[2, 7], [1, 1], [1, 3], [1, 4], [2, 2], [1, 5], [3, 9]], np.int32)
    area = np.array([3.5, 0.25, 1.0004, 1.75, 0.5, 2.0, 6.0])
    reverse = np.array([3, -1, 4, 0, 2, -1, -1], np.int32)
    lines = interfaces.format_contact_map_rows(files, labels, pair_struct, pair_groups, offsets, residues, counts, area, reverse, res_chain, res_name, res_number)
    assert lines == ["a.pdb\tA\tB\tA\tALA\t1\tB\tSER\t-3\t2\t7\t3.500\t1\t4\t1.750",
                     "a.pdb\tA\tB\tA\tALA\t1\tB\tTRP\t4\t1\t1\t0.250\t0\t0\t0.000",
                     "a.pdb\tA\tB\tA\tGLY\t2A\tB\tSER\t-3\t1\t3\t1.000\t2\t2\t0.500",
                     "a.pdb\tA\tB\tA\tGLY\t2A\tB\tTRP\t4\t0\t0\t0.000\t1\t5\t2.000",
                     "a.pdb\tA\tC\tA\tGLY\t2A\t_\tHOH\t9\t0\t0\t0.000\t3\t9\t6.000"]
    assert len(interfaces.CONTACT_MAP_HEADER.split("\t")) == len(lines[0].split("\t")) == 15
    with pytest.raises(SystemExit) as e:
        interfaces.main(["x.pdb", "-o", "o.tsv", "--alg", "lr", "--contact-map", "m.tsv"])
    assert "Shrake-Rupley" in str(e.value)
