"""TESTS ONLY: ctypes front-end of the CPU emulation of the kernels of chain groups among periodic images
(tests/emu/emu_groups_pbc.cpp): the cells of the combined structures, the expansion of the combined batch (the periodic
kernels, orthorhombic or triclinic), the fused collect-and-finish."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libgroups_pbc_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libgroups_pbc_emu.so"))
        for f in (_lib.emu_pbc_tri_expand, _lib.emu_pbc_expand):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
            f.restype = C.c_longlong
        _lib.emu_gpbc_cells.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.emu_gpbc_finish.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def cells(cells_in, n_comb, gbase=None, g_fixed=0):
    """k_gpbc_cells: cells_in [n_cplx, W] (W = 3 or 9) -> [n_comb, W]; gbase [n_cplx + 1] (the batch entries) or g_fixed groups
    per complex (a shard's frames).  What no thread wrote is NaN."""
    cells_in = np.ascontiguousarray(cells_in, dtype=np.float64)
    n_cplx, W = cells_in.shape
    gb = None if gbase is None else np.ascontiguousarray(gbase, dtype=np.int64)
    out = np.full((n_comb + 1, W), np.nan)
    if _load().emu_gpbc_cells(n_cplx, n_comb, _p(gb), g_fixed, W, cells_in.ctypes.data, out.ctypes.data):
        raise RuntimeError("emu_gpbc_cells: bad argument")
    assert np.all(np.isnan(out[n_comb])), "a thread wrote behind the cells"
    return out[:n_comb].copy()


def expand(cxyz, cradii, coff, ccells, probe=1.4):
    """the periodic count and emit kernels over the combined batch -> (expanded xyz, expanded radii, expanded offsets, image
    counts); ccells [n_comb, 3]: the orthorhombic kernels, [n_comb, 9]: the triclinic ones"""
    cxyz = np.ascontiguousarray(cxyz, dtype=np.float64).reshape(-1, 3)
    cradii = np.ascontiguousarray(cradii, dtype=np.float64)
    ccells = np.ascontiguousarray(ccells, dtype=np.float64)
    coff = np.ascontiguousarray(coff, dtype=np.int64)
    ns, n = ccells.shape[0], cxyz.shape[0]
    n_img, rmax = np.full(ns, -1, dtype=np.int64), np.full(ns, np.nan)
    ibase, eoff = np.full(max(n, 1), -1, dtype=np.int32), np.zeros(ns + 1, dtype=np.int64)
    cap = 27 * n + 1
    exyz, eradii = np.full((cap, 3), np.nan), np.full(cap, np.nan)
    fn = _load().emu_pbc_expand if ccells.shape[1] == 3 else _load().emu_pbc_tri_expand
    N = fn(cxyz.ctypes.data, cradii.ctypes.data, coff.ctypes.data, ns, 0, 0, ccells.ctypes.data, probe, n_img.ctypes.data,
           rmax.ctypes.data, ibase.ctypes.data, eoff.ctypes.data, exyz.ctypes.data, eradii.ctypes.data, cap)
    if N < 0:
        raise RuntimeError("emu_pbc_expand: bad argument")
    assert np.all(np.isnan(exyz[N:])) and np.all(np.isnan(eradii[N:])), "a thread wrote behind the expanded batch"
    return exyz[:N].copy(), eradii[:N].copy(), eoff, n_img


def finish(n_cplx, coff, eoff, esasa, src, key, gbase=None, g_fixed=0, n_fixed=0, n_iso_fixed=0):
    """k_gpbc_finish -> (sasa [n], iso [n], carea [N], cgath [N]); what no thread wrote is NaN"""
    coff, eoff = np.ascontiguousarray(coff, dtype=np.int64), np.ascontiguousarray(eoff, dtype=np.int64)
    esasa = np.ascontiguousarray(esasa, dtype=np.float64)
    src, key = np.ascontiguousarray(src, dtype=np.int32), np.ascontiguousarray(key, dtype=np.int32)
    gb = None if gbase is None else np.ascontiguousarray(gbase, dtype=np.int64)
    n_comb = coff.size - 1
    n, N = int(coff[n_cplx]), int(coff[n_comb])
    sasa, iso = np.full(n + 1, np.nan), np.full(n + 1, np.nan)
    carea, cgath = np.full(N + 1, np.nan), np.full(N + 1, np.nan)
    if _load().emu_gpbc_finish(n_cplx, n_comb, coff.ctypes.data, eoff.ctypes.data, _p(gb), g_fixed, src.ctypes.data, n_fixed, n_iso_fixed,
                               key.ctypes.data, esasa.ctypes.data, carea.ctypes.data, cgath.ctypes.data, sasa.ctypes.data, iso.ctypes.data):
        raise RuntimeError("emu_gpbc_finish: bad argument")
    assert np.isnan(sasa[n]) and np.isnan(iso[n]) and np.isnan(carea[N]) and np.isnan(cgath[N]), "a thread wrote behind its array"
    return sasa[:n].copy(), iso[:n].copy(), carea[:N].copy(), cgath[:N].copy()
