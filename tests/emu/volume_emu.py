"""TESTS ONLY: ctypes front-end of the CPU emulation of the molecular-volume kernels (tests/emu/emu_volume.cpp) and of the
Shrake-Rupley tile kernel's phases with the store phase that keeps the exposed-point vectors (the same file: emu.cpp compiled
into it once more, emu_set_sr_evec)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libvolume_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libvolume_emu.so"))
        _lib.emu_volume.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 5
    return _lib


def volume(xyz, radii, offsets, counts, evec, probe=1.4, n_points=100, shared_radii=False):
    """k_vol_origin, k_vol_atom and the totals over the terms -> (origin [n_structs, 3], vol [n], volumes [n_structs]); what no
    thread wrote is NaN"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    evec = np.ascontiguousarray(evec, dtype=np.float64).reshape(-1, 3)
    ns, n = off.size - 1, xyz.shape[0]
    origin, vol, volumes = np.full((ns, 3), np.nan), np.full(n, np.nan), np.full(ns, np.nan)
    rc = _load().emu_volume(xyz.ctypes.data, radii.ctypes.data, off.ctypes.data, ns, int(shared_radii), probe, n_points,
                            counts.ctypes.data, evec.ctypes.data, origin.ctypes.data, vol.ctypes.data, volumes.ctypes.data)
    if rc:
        raise RuntimeError("emu_volume: bad argument")
    return origin, vol, volumes


def sr_batch_with_evec(xyz, radii, offsets, unit, probe=1.4, cap_idx=0):
    """the emulated Shrake-Rupley batch (emu.run_batch's call, into this library's own copy of emu.cpp) with the vectors asked
    for -> (sasa, counts, totals, stats, evec [n, 3]); vectors no store phase wrote are NaN.  cap_idx: records per atom of the
    main launch (0: the production shape)"""
    lib = _load()
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64)
    lib.emu_run_batch.argtypes = [C.c_int, dp, dp, lp, C.c_int, C.c_double, C.c_int, dp, dp, ip, dp, C.POINTER(C.c_longlong)] + [C.c_int] * 9
    lib.emu_set_sr_evec.argtypes = [C.c_void_p]
    lib.emu_set_sr_evec.restype = None
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    up = np.ascontiguousarray(unit, dtype=np.float64).reshape(-1)
    n = radii.size
    sasa, counts, totals = np.full(n, np.nan), np.full(n, -1, dtype=np.int32), np.zeros(offsets.size - 1)
    evec = np.full((n, 3), np.nan)
    stats = (C.c_longlong * 10)()
    lib.emu_set_sr_evec(evec.ctypes.data)
    try:
        ret = lib.emu_run_batch(0, xyz.ctypes.data_as(dp), radii.ctypes.data_as(dp), offsets.ctypes.data_as(lp), offsets.size - 1, probe,
                                up.size // 3, up.ctypes.data_as(dp), sasa.ctypes.data_as(dp), counts.ctypes.data_as(ip), totals.ctypes.data_as(dp),
                                stats, cap_idx, 0, -1, 0, 0, 0, 0, 0, -1)
    finally:
        lib.emu_set_sr_evec(None)
    st = dict(zip(("error", "fallback_tiles", "max_nn", "TA", "B", "lds", "cells", "items", "slab_tiles", "unused"), list(stats)))
    if ret:
        raise RuntimeError(f"emulated batch failed: {st}")
    return sasa, counts, totals, st, evec
