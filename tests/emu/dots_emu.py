"""TESTS ONLY: ctypes front-end of the CPU emulation of the surface-dot kernels (tests/emu/emu_dots.cpp) and of the
Shrake-Rupley tile kernel's phases with the store phase that keeps the exposure masks (the same file: emu.cpp compiled into it
once more, emu_set_sr_masks)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libdots_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libdots_emu.so"))
        _lib.emu_dots_count.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
        _lib.emu_dots_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.emu_dots_shape.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.emu_dots_shape.restype = None
    return _lib


def pair_misses():
    """dots_pair (the expansion's atom and point of a pair, made without a 64-bit division) against // and % at the atoms' boundaries up
    to 2^30 atoms, every point count: the number of misses"""
    lib = _load()
    lib.emu_dots_pair_misses.restype = C.c_longlong
    return int(lib.emu_dots_pair_misses())


def shape():
    """(atoms per block of the scan, threads of its workgroups)"""
    b, t = C.c_int(0), C.c_int(0)
    _load().emu_dots_shape(C.byref(b), C.byref(t))
    return b.value, t.value


def count(masks, n_points):
    """the scan's three launches -> dot_first [n + 1] int64; what no thread wrote is -1"""
    masks = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1, 4)
    first = np.full(len(masks) + 1, -1, dtype=np.int64)
    if _load().emu_dots_count(masks.ctypes.data, len(masks), n_points, first.ctypes.data):
        raise RuntimeError("emu_dots_count: bad argument")
    return first


def expand(xyz, radii, probe, unit, masks, dot_first, capacity, guard=16):
    """k_dots_expand into arrays of capacity + guard dots, all of them filled with a sentinel first ->
    (dot_xyz [capacity + guard, 3], dot_atom, dot_point [capacity + guard]): NaN / -7 where no thread wrote"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    unit = np.ascontiguousarray(unit, dtype=np.float64).reshape(-1, 3)
    masks = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1, 4)
    first = np.ascontiguousarray(dot_first, dtype=np.int64)
    dx = np.full((capacity + guard, 3), np.nan)
    da, dp = np.full(capacity + guard, -7, dtype=np.int32), np.full(capacity + guard, -7, dtype=np.int32)
    rc = _load().emu_dots_expand(xyz.ctypes.data, radii.ctypes.data, len(radii), probe, len(unit), unit.ctypes.data, masks.ctypes.data,
                                 first.ctypes.data, capacity, dx.ctypes.data, da.ctypes.data, dp.ctypes.data)
    if rc:
        raise RuntimeError("emu_dots_expand: bad argument")
    return dx, da, dp


def sr_batch_with_masks(xyz, radii, offsets, unit, probe=1.4, cap_idx=0):
    """the emulated Shrake-Rupley batch (emu.run_batch's call, into this library's own copy of emu.cpp) with the masks asked for ->
    (sasa, counts, totals, stats, masks [n, 4]); masks no store phase wrote are 0xdeadbeef.  cap_idx: records per atom of the
    main launch (0: the production shape)"""
    lib = _load()
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64)
    lib.emu_run_batch.argtypes = [C.c_int, dp, dp, lp, C.c_int, C.c_double, C.c_int, dp, dp, ip, dp, C.POINTER(C.c_longlong)] + [C.c_int] * 9
    lib.emu_set_sr_masks.argtypes = [C.c_void_p]
    lib.emu_set_sr_masks.restype = None
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    up = np.ascontiguousarray(unit, dtype=np.float64).reshape(-1)
    n = radii.size
    sasa, counts, totals = np.full(n, np.nan), np.full(n, -1, dtype=np.int32), np.zeros(offsets.size - 1)
    # (aligned to 16 bytes: the store phase writes an atom's four words in one store)
    raw = np.full(4 * n + 4, 0xdeadbeef, dtype=np.uint32)
    shift = (-raw.ctypes.data % 16) // 4
    masks = raw[shift:shift + 4 * n].reshape(n, 4)
    stats = (C.c_longlong * 10)()
    lib.emu_set_sr_masks(masks.ctypes.data)
    try:
        ret = lib.emu_run_batch(0, xyz.ctypes.data_as(dp), radii.ctypes.data_as(dp), offsets.ctypes.data_as(lp), offsets.size - 1, probe,
                                up.size // 3, up.ctypes.data_as(dp), sasa.ctypes.data_as(dp), counts.ctypes.data_as(ip), totals.ctypes.data_as(dp),
                                stats, cap_idx, 0, -1, 0, 0, 0, 0, 0, -1)
    finally:
        lib.emu_set_sr_masks(None)
    st = dict(zip(("error", "fallback_tiles", "max_nn", "TA", "B", "lds", "cells", "items", "slab_tiles", "unused"), list(stats)))
    if ret:
        raise RuntimeError(f"emulated batch failed: {st}")
    return sasa, counts, totals, st, masks.copy()
