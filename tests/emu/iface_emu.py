"""TESTS ONLY: ctypes front-end of the CPU emulation of the interface kernels (tests/emu/emu_iface.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CHECK = os.path.join(HERE, "iface_check")
_lib = None
_dp, _lp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_ubyte)


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libiface_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libiface_emu.so"))
        _lib.emu_iface_screen.argtypes = [_dp, _dp, _lp, C.c_int, _ip, _ip, C.c_double, _dp, _bp, _bp, C.c_longlong]
        _lib.emu_iface_screen.restype = C.c_longlong
        _lib.emu_iface_table.argtypes = [_dp, _dp, _lp, C.c_int, _ip, _ip, _bp, _dp, _dp, _dp, C.c_longlong, C.c_longlong,
                                         C.POINTER(C.c_longlong), _ip, _ip, _lp, _dp, _dp, _ip, _dp, _dp]
        _lib.emu_iface_table.restype = C.c_longlong
        _lib.emu_iface_shape.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return _lib


def build_check():
    """tests/emu/iface_check (the phases under AddressSanitizer + UBSan, a program of its own): its path"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/iface_check"], check=True, stdout=subprocess.DEVNULL)
    return CHECK


def shape():
    t, l = C.c_int(0), C.c_int(0)
    _load().emu_iface_shape(C.byref(t), C.byref(l))
    return t.value, l.value


def _batch(xyz, radii, offsets, group, n_groups):
    return (np.ascontiguousarray(xyz, np.float64).reshape(-1), np.ascontiguousarray(radii, np.float64), np.ascontiguousarray(offsets, np.int64),
            np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32))


def screen(xyz, radii, offsets, group, n_groups, probe=1.4):
    """(box [G, 8], candidate [T] bool, contact [T] bool) as k_iface_box, k_iface_candidates and k_iface_contact make them"""
    x, r, o, g, ng = _batch(xyz, radii, offsets, group, n_groups)
    G, T = int(ng.sum()), int((ng.astype(np.int64) * (ng - 1) // 2).sum())
    box, cand, flag = np.full((G + 1, 8), np.nan), np.full(T + 1, 7, np.uint8), np.full(T + 1, 7, np.uint8)
    got = _load().emu_iface_screen(x.ctypes.data_as(_dp), r.ctypes.data_as(_dp), o.ctypes.data_as(_lp), o.size - 1, g.ctypes.data_as(_ip),
                                   ng.ctypes.data_as(_ip), probe, box.ctypes.data_as(_dp), cand.ctypes.data_as(_bp), flag.ctypes.data_as(_bp), T)
    if got != T:
        raise RuntimeError("emu_iface_screen: bad argument")
    assert np.all(np.isnan(box[G])) and cand[T] == 7 and flag[T] == 7
    return box[:G], cand[:T].astype(bool), flag[:T].astype(bool)


def table(xyz, radii, offsets, group, n_groups, flag, p_cap, m_cap, csasa=None, ctot=None, psasa=None):
    """the table, the gather and the finish from the flags, into arrays of p_cap rows and m_cap atoms (one guard element behind
    each): a dict, or None when a capacity is too small (then with nothing written: the guards and the fill are checked)"""
    x, r, o, g, ng = _batch(xyz, radii, offsets, group, n_groups)
    f = np.ascontiguousarray(flag, np.uint8)
    ps, pg, so = np.full(p_cap + 1, -7, np.int32), np.full(2 * p_cap + 1, -7, np.int32), np.full(2 * p_cap + 2, -7, np.int64)
    px, pr, pa = np.full(3 * m_cap + 1, -7.0), np.full(m_cap + 1, -7.0), np.full(m_cap + 1, -7, np.int32)
    pb, ar = np.full(m_cap + 1, -7.0), np.full(6 * p_cap + 1, -7.0)
    opt = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(_dp)
    keep = [np.ascontiguousarray(a, np.float64) for a in (csasa, ctot, psasa) if a is not None]
    P = C.c_longlong(-1)
    M = _load().emu_iface_table(x.ctypes.data_as(_dp), r.ctypes.data_as(_dp), o.ctypes.data_as(_lp), o.size - 1, g.ctypes.data_as(_ip),
                                ng.ctypes.data_as(_ip), f.ctypes.data_as(_bp), *(k.ctypes.data_as(_dp) for k in keep) if len(keep) == 3 else (None, None, None),
                                p_cap, m_cap, C.byref(P), ps.ctypes.data_as(_ip), pg.ctypes.data_as(_ip), so.ctypes.data_as(_lp),
                                px.ctypes.data_as(_dp), pr.ctypes.data_as(_dp), pa.ctypes.data_as(_ip), pb.ctypes.data_as(_dp), ar.ctypes.data_as(_dp))
    if M == -1:
        raise RuntimeError("emu_iface_table: bad argument")
    assert ps[p_cap] == -7 and pg[2 * p_cap] == -7 and so[2 * p_cap + 1] == -7 and px[3 * m_cap] == -7.0 and pr[m_cap] == -7.0
    assert pa[m_cap] == -7 and pb[m_cap] == -7.0 and ar[6 * p_cap] == -7.0
    if M == -2:
        assert np.all(ps == -7) and np.all(so == -7) and np.all(pa == -7) and np.all(ar == -7.0) and np.all(px == -7.0)
        return None
    n = int(P.value)
    return dict(n_pairs=n, n_pair_atoms=int(M), pair_struct=ps[:n], pair_groups=pg[:2 * n].reshape(n, 2), side_offsets=so[:2 * n + 1],
                pxyz=px[:3 * M].reshape(M, 3), pradii=pr[:M], pair_atom=pa[:M], pair_buried=pb[:M], pair_areas=ar[:6 * n].reshape(n, 6))
