"""TESTS ONLY: ctypes front-end of the CPU emulation of the periodic-image kernels (tests/emu/emu_pbc.cpp)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libpbc_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libpbc_emu.so"))
        _lib.emu_pbc_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
        _lib.emu_pbc_expand.restype = C.c_longlong
        _lib.emu_pbc_collect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def expand(xyz, radii, offsets, cells, probe=1.4, n_fixed=0):
    """k_pbc_count and k_pbc_emit over a batch -> (expanded xyz [N, 3], expanded radii [N], expanded offsets, image counts, max
    radii, image bases).  offsets None with n_fixed: structures of n_fixed atoms that share the n_fixed radii (a shard's frames).
    What no thread wrote is NaN."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 3)
    ns, n = cells.shape[0], xyz.shape[0]
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    n_img, rmax = np.full(ns, -1, dtype=np.int64), np.full(ns, np.nan)
    ibase, eoff = np.full(n, -1, dtype=np.int32), np.zeros(ns + 1, dtype=np.int64)
    cap = 27 * n
    exyz, eradii = np.full((cap, 3), np.nan), np.full(cap, np.nan)
    N = _load().emu_pbc_expand(xyz.ctypes.data, radii.ctypes.data, None if off is None else off.ctypes.data, ns, n_fixed,
                               int(off is None), cells.ctypes.data, probe, n_img.ctypes.data, rmax.ctypes.data, ibase.ctypes.data,
                               eoff.ctypes.data, exyz.ctypes.data, eradii.ctypes.data, cap)
    if N < 0:
        raise RuntimeError("emu_pbc_expand: bad argument")
    assert np.all(np.isnan(exyz[N:])) and np.all(np.isnan(eradii[N:])), "a thread wrote behind the expanded batch"
    return exyz[:N].copy(), eradii[:N].copy(), eoff, n_img, rmax, ibase


def collect(offsets, eoff, esasa, n_fixed=0):
    """k_pbc_collect: the real atoms' areas out of the expanded batch's"""
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    eoff = np.ascontiguousarray(eoff, dtype=np.int64)
    esasa = np.ascontiguousarray(esasa, dtype=np.float64)
    ns = eoff.size - 1
    n = int(off[-1]) if off is not None else ns * n_fixed
    out = np.full(n, np.nan)
    if _load().emu_pbc_collect(None if off is None else off.ctypes.data, ns, n_fixed, eoff.ctypes.data, esasa.ctypes.data, out.ctypes.data):
        raise RuntimeError("emu_pbc_collect: bad argument")
    return out
