"""TESTS ONLY: ctypes front-end of the CPU emulation of the per-residue interface tables (tests/emu/emu_iface_res.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CHECK = os.path.join(HERE, "iface_res_check")
_lib = None
_dp, _lp, _ip, _bp, _llp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong)


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libiface_res_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libiface_res_emu.so"))
        _lib.emu_iface_res_scan.argtypes = [_ip, C.c_longlong]
        _lib.emu_iface_res_table.argtypes = [_lp, C.c_longlong, _ip, C.c_longlong, _lp, C.c_int, _dp, _dp, C.c_double, C.c_longlong,
                                             _bp, _lp, _llp, _llp, _lp, _ip, _ip, _dp]
        _lib.emu_iface_res_table.restype = C.c_longlong
        _lib.emu_iface_res_shape.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return _lib


def build_check():
    """tests/emu/iface_res_check (the phases under AddressSanitizer + UBSan, a program of its own): its path"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/iface_res_check"], check=True, stdout=subprocess.DEVNULL)
    return CHECK


def shape():
    t, l = C.c_int(0), C.c_int(0)
    _load().emu_iface_res_shape(C.byref(t), C.byref(l))
    return t.value, l.value


def scan(counts):
    """(the exclusive prefix sums [n + 1] of the int32 counts, the levels above the first) as kl_iface_res_scan makes them"""
    counts = np.asarray(counts, np.int32)
    a = np.concatenate([counts, [-7, -9]]).astype(np.int32)      # the slot of the total, and a guard behind it
    top = _load().emu_iface_res_scan(a.ctypes.data_as(_ip), counts.size)
    assert top >= 0 and a[-1] == -9
    return a[:-1], top


def table(side_offsets, pair_atom, res_first, iso, psasa, min_buried, res_cap=None):
    """the stage from the pair table and the areas, into row arrays of res_cap rows (None: M) with a guard element behind each:
    a dict, or (K, R) when res_cap is too small - then with none of the row arrays written"""
    so, pa = np.ascontiguousarray(side_offsets, np.int64), np.ascontiguousarray(pair_atom, np.int32)
    rf, iso, ps = np.ascontiguousarray(res_first, np.int64), np.ascontiguousarray(iso, np.float64), np.ascontiguousarray(psasa, np.float64)
    M, S = pa.size, so.size - 1
    cap = M if res_cap is None else res_cap
    heads, first = np.full(M + 1, 7, np.uint8), np.full(M + 2, -7, np.int64)
    off, index, atoms, areas = np.full(S + 2, -7, np.int64), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32), np.full(3 * cap + 1, -7.0)
    K, R = C.c_longlong(-1), C.c_longlong(-1)
    got = _load().emu_iface_res_table(so.ctypes.data_as(_lp), S, pa.ctypes.data_as(_ip), M, rf.ctypes.data_as(_lp), rf.size - 1,
                                      iso.ctypes.data_as(_dp), ps.ctypes.data_as(_dp), min_buried, cap, heads.ctypes.data_as(_bp),
                                      first.ctypes.data_as(_lp), C.byref(K), C.byref(R), off.ctypes.data_as(_lp), index.ctypes.data_as(_ip),
                                      atoms.ctypes.data_as(_ip), areas.ctypes.data_as(_dp))
    if got == -1:
        raise RuntimeError("emu_iface_res_table: bad argument")
    assert heads[M] == 7 and first[M + 1] == -7 and off[S + 1] == -7 and index[cap] == -7 and atoms[cap] == -7 and areas[3 * cap] == -7.0
    k, r = int(K.value), int(R.value)
    if got == -2:
        assert np.all(off == -7) and np.all(index == -7) and np.all(atoms == -7) and np.all(areas == -7.0)
        return k, r
    assert got == r and np.all(index[r:] == -7) and np.all(atoms[r:] == -7) and np.all(areas[3 * r:] == -7.0)
    return dict(heads=heads[:M].astype(bool), seg_first=first[:k + 1], n_segments=k, n_res_rows=r, res_offsets=off[:S + 1],
                res_index=index[:r], res_atoms=atoms[:r], res_areas=areas[:3 * r].reshape(r, 3))
