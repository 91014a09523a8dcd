"""TESTS ONLY: ctypes front-end of the CPU emulation of the triclinic periodic-image kernels (tests/emu/emu_pbc_tri.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libpbc_tri_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libpbc_tri_emu.so"))
        for f in (_lib.emu_pbc_tri_expand, _lib.emu_pbc_expand):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
            f.restype = C.c_longlong
    return _lib


def expand(xyz, radii, offsets, cell9, probe=1.4, n_fixed=0, orthorhombic=False):
    """k_pbc_tri_count and k_pbc_tri_emit over a batch -> (expanded xyz [N, 3], expanded radii [N], expanded offsets, image counts,
    max radii, image bases).  cell9 [n_structs, 9]: the six numbers of every cell and its three widths.  offsets None with n_fixed:
    structures of n_fixed atoms that share the n_fixed radii (a shard's frames).  What no thread wrote is NaN.  orthorhombic: cell9
    is [n_structs, 3] edges and the kernels are the orthorhombic ones, as this library holds them."""
    w = 3 if orthorhombic else 9
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    cell9 = np.ascontiguousarray(cell9, dtype=np.float64).reshape(-1, w)
    ns, n = cell9.shape[0], xyz.shape[0]
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    n_img, rmax = np.full(ns, -1, dtype=np.int64), np.full(ns, np.nan)
    ibase, eoff = np.full(n, -1, dtype=np.int32), np.zeros(ns + 1, dtype=np.int64)
    cap = 27 * n
    exyz, eradii = np.full((cap, 3), np.nan), np.full(cap, np.nan)
    fn = _load().emu_pbc_expand if orthorhombic else _load().emu_pbc_tri_expand
    N = fn(xyz.ctypes.data, radii.ctypes.data, None if off is None else off.ctypes.data, ns, n_fixed, int(off is None), cell9.ctypes.data,
           probe, n_img.ctypes.data, rmax.ctypes.data, ibase.ctypes.data, eoff.ctypes.data, exyz.ctypes.data, eradii.ctypes.data, cap)
    if N < 0:
        raise RuntimeError("emu_pbc_tri_expand: bad argument")
    assert np.all(np.isnan(exyz[N:])) and np.all(np.isnan(eradii[N:])), "a thread wrote behind the expanded batch"
    return exyz[:N].copy(), eradii[:N].copy(), eoff, n_img, rmax, ibase
