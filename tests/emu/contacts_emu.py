"""TESTS ONLY: ctypes front-end of the CPU emulation of the interfaces' atom-atom contact tables (tests/emu/emu_contacts.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CHECK = os.path.join(HERE, "contacts_check")
_lib = None
_dp, _lp, _ip, _up, _llp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_longlong)


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libcontacts_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libcontacts_emu.so"))
        _lib.emu_contacts_table.argtypes = [_lp, C.c_longlong, _dp, _dp, C.c_longlong, C.c_double, C.c_int, _dp, _up, _up, C.c_longlong,
                                            C.c_longlong, _up, _lp, _ip, _lp, _ip, _ip, _dp, _llp, _llp, C.POINTER(C.c_int)]
        _lib.emu_contacts_table.restype = C.c_longlong
        _lib.emu_contacts_shape.argtypes = [C.POINTER(C.c_int)]
    return _lib


def build_check():
    """tests/emu/contacts_check (the phases under AddressSanitizer + UBSan, a program of its own): its path"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/contacts_check"], check=True, stdout=subprocess.DEVNULL)
    return CHECK


def shape():
    t = C.c_int(0)
    _load().emu_contacts_shape(C.byref(t))
    return t.value


def table(side_offsets, pxyz, pradii, probe, unit, side_masks, pair_masks, dot_cap=None, row_cap=None):
    """the stage from the pair batch and the two sets of masks ([M, 4] uint32), into arrays of dot_cap dots and row_cap rows (None:
    what the masks' popcounts allow) with a guard element behind each: a dict, or (D_b, C) when a capacity is too small - then with
    none of the arrays behind the capacities written"""
    so = np.ascontiguousarray(side_offsets, np.int64)
    x, r, u = np.ascontiguousarray(pxyz, np.float64).reshape(-1), np.ascontiguousarray(pradii, np.float64), np.ascontiguousarray(unit, np.float64).reshape(-1)
    sm, pm = np.ascontiguousarray(side_masks, np.uint32).reshape(-1), np.ascontiguousarray(pair_masks, np.uint32).reshape(-1)
    M, S, N = r.size, so.size - 1, u.size // 3
    most = int(sum(bin(int(v)).count("1") for v in (sm & ~pm)))
    dcap = most if dot_cap is None else dot_cap
    rcap = most if row_cap is None else row_cap
    buried, dfirst = np.full(4 * M + 1, 7, np.uint32), np.full(M + 2, -7, np.int64)
    dpart, first = np.full(dcap + 1, -7, np.int32), np.full(M + 2, -7, np.int64)
    partner, points, area = np.full(rcap + 1, -7, np.int32), np.full(rcap + 1, -7, np.int32), np.full(rcap + 1, -7.0)
    D, Cn, flag = C.c_longlong(-1), C.c_longlong(-1), C.c_int(-1)
    got = _load().emu_contacts_table(so.ctypes.data_as(_lp), S, x.ctypes.data_as(_dp), r.ctypes.data_as(_dp), M, probe, N, u.ctypes.data_as(_dp),
                                     sm.ctypes.data_as(_up), pm.ctypes.data_as(_up), dcap, rcap, buried.ctypes.data_as(_up),
                                     dfirst.ctypes.data_as(_lp), dpart.ctypes.data_as(_ip), first.ctypes.data_as(_lp), partner.ctypes.data_as(_ip),
                                     points.ctypes.data_as(_ip), area.ctypes.data_as(_dp), C.byref(D), C.byref(Cn), C.byref(flag))
    if got == -1:
        raise RuntimeError("emu_contacts_table: bad argument")
    assert buried[4 * M] == 7 and dfirst[M + 1] == -7 and dpart[dcap] == -7 and first[M + 1] == -7
    assert partner[rcap] == -7 and points[rcap] == -7 and area[rcap] == -7.0
    d, c = int(D.value), int(Cn.value)
    if got == -2:
        assert np.all(dpart == -7) and np.all(first == -7) and np.all(partner == -7) and np.all(points == -7) and np.all(area == -7.0)
        return d, c
    assert got == c and np.all(dpart[d:] == -7) and np.all(partner[c:] == -7) and np.all(points[c:] == -7) and np.all(area[c:] == -7.0)
    return dict(buried_masks=buried[:4 * M].reshape(M, 4), dot_first=dfirst[:M + 1], dot_partner=dpart[:d], contact_first=first[:M + 1],
                contact_partner=partner[:c], contact_points=points[:c], contact_area=area[:c], n_dots=d, n_contacts=c, flag=int(flag.value))
