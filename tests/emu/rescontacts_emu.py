"""TESTS ONLY: ctypes front-end of the CPU emulation of the interfaces' residue-residue contact tables (tests/emu/emu_rescontacts.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CHECK = os.path.join(HERE, "rescontacts_check")
_lib = None
_dp, _lp, _ip, _llp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/librescontacts_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "librescontacts_emu.so"))
        _lib.emu_rescontacts_table.argtypes = [_lp, C.c_longlong, _ip, C.c_longlong, _lp, C.c_int, _lp, _ip, _ip, _dp, C.c_longlong, C.c_longlong,
                                               _llp, _llp, _lp, _ip, _ip, _dp, _ip]
        _lib.emu_rescontacts_table.restype = C.c_longlong
        _lib.emu_rescontacts_shape.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return _lib


def build_check():
    """tests/emu/rescontacts_check (the phases under AddressSanitizer + UBSan, a program of its own): its path"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/rescontacts_check"], check=True, stdout=subprocess.DEVNULL)
    return CHECK


def shape():
    """(the lanes of a wave, RC_STAGE: the rows of a segment whose keys the fold kernels keep in LDS)"""
    w, s = C.c_int(0), C.c_int(0)
    _load().emu_rescontacts_shape(C.byref(w), C.byref(s))
    return w.value, s.value


def table(side_offsets, pair_atom, res_first, contact_first, contact_partner, contact_points, contact_area, row_cap=None):
    """the stage from the pair table, the residue boundaries and the atom-atom contact table, into arrays of row_cap rows (None: C,
    which always suffices) with a guard element behind each: a dict, or (K, Q) when the capacity is too small - then with none of
    the arrays written"""
    so, pa, rf = np.ascontiguousarray(side_offsets, np.int64), np.ascontiguousarray(pair_atom, np.int32), np.ascontiguousarray(res_first, np.int64)
    cf, cp = np.ascontiguousarray(contact_first, np.int64), np.ascontiguousarray(contact_partner, np.int32)
    cn, ca = np.ascontiguousarray(contact_points, np.int32), np.ascontiguousarray(contact_area, np.float64)
    M, S, Cn = pa.size, so.size - 1, cp.size
    cap = Cn if row_cap is None else row_cap
    off, res, cnt = np.full(S + 2, -7, np.int64), np.full(2 * cap + 1, -7, np.int32), np.full(2 * cap + 1, -7, np.int32)
    area, rev = np.full(cap + 1, -7.0), np.full(cap + 1, -7, np.int32)
    K, Q = C.c_longlong(-1), C.c_longlong(-1)
    got = _load().emu_rescontacts_table(so.ctypes.data_as(_lp), S, pa.ctypes.data_as(_ip), M, rf.ctypes.data_as(_lp), rf.size - 1,
                                        cf.ctypes.data_as(_lp), cp.ctypes.data_as(_ip), cn.ctypes.data_as(_ip), ca.ctypes.data_as(_dp), Cn, cap,
                                        C.byref(K), C.byref(Q), off.ctypes.data_as(_lp), res.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip),
                                        area.ctypes.data_as(_dp), rev.ctypes.data_as(_ip))
    if got == -1:
        raise RuntimeError("emu_rescontacts_table: bad argument")
    assert off[S + 1] == -7 and res[2 * cap] == -7 and cnt[2 * cap] == -7 and area[cap] == -7.0 and rev[cap] == -7
    k, q = int(K.value), int(Q.value)
    if got == -2:
        assert np.all(off == -7) and np.all(res == -7) and np.all(cnt == -7) and np.all(area == -7.0) and np.all(rev == -7)
        return k, q
    assert got == q and np.all(res[2 * q:] == -7) and np.all(cnt[2 * q:] == -7) and np.all(area[q:] == -7.0) and np.all(rev[q:] == -7)
    return dict(rescontact_offsets=off[:S + 1], rescontact_residues=res[:2 * q].reshape(q, 2), rescontact_counts=cnt[:2 * q].reshape(q, 2),
                rescontact_area=area[:q], rescontact_reverse=rev[:q], n_segments=k, n_rescontacts=q)
