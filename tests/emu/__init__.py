"""TESTS ONLY: ctypes front-end of the CPU emulation of the kernel phase functions."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_SO = os.environ.get("SASA_EMU_SO") or os.path.join(HERE, "libsasa_emu.so")  # (SASA_EMU_SO: a variant build, see test_emulation.py)
_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64)
_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.environ.get("SASA_EMU_SO"):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(_SO)
        _lib.emu_run_batch.argtypes = [C.c_int, _dp, _dp, _lp, C.c_int, C.c_double, C.c_int, _dp,
                                       _dp, _ip, _dp, C.POINTER(C.c_longlong)] + [C.c_int] * 9
        _lib.emu_set_lr2_opts.argtypes = [C.c_int]
    return _lib


def set_lr2_opts(shape_builds=False, compact_cells=False):
    """Run the Lee-Richards tile kernel's shape-specialised builds where the device would, and / or look cells up in the
    compact cell table (single-structure batches)."""
    _load().emu_set_lr2_opts((1 if shape_builds else 0) | (2 if compact_cells else 0))


def run_batch(lr, xyz, radii, offsets=None, probe=1.4, resolution=20, unit_pts=None,
              cap_idx=0, pool=0, ds=-1, fb_cap_idx=0, fb_pool=0, fb_ds=0, mid_cap_idx=0, mid_pool=0,
              mid_ds=-1, check=True):
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    n = radii.size
    if offsets is None:
        offsets = [0, n]
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    sasa = np.full(n, np.nan)
    counts = np.full(n, -1, dtype=np.int32)
    totals = np.zeros(offsets.size - 1)
    stats = (C.c_longlong * 10)()
    up = None
    if unit_pts is not None:
        up = np.ascontiguousarray(unit_pts, dtype=np.float64).reshape(-1)
    ret = _load().emu_run_batch(1 if lr else 0, xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp),
                                offsets.ctypes.data_as(_lp), offsets.size - 1, probe, resolution,
                                up.ctypes.data_as(_dp) if up is not None else None,
                                sasa.ctypes.data_as(_dp), counts.ctypes.data_as(_ip),
                                totals.ctypes.data_as(_dp), stats, cap_idx, pool, ds,
                                fb_cap_idx, fb_pool, fb_ds, mid_cap_idx, mid_pool, mid_ds)
    st = dict(zip(("error", "fallback_tiles", "max_nn", "TA", "B", "lds", "cells", "items", "slab_tiles", "unused"), list(stats)))
    if check and ret:
        raise RuntimeError(f"emulated batch failed: {st}")
    return sasa, counts, totals, st


def cell_sort(xyz, radii, offsets, probe=1.4, cells_cap=0, shared_radii=False):
    """The emulated general cell sort on its own (emu_cell_sort), in the shape of GpuContext.cell_sort's result for
    arrangement 0; cells_cap 0: the engine's sizing of a first batch; what nobody wrote is all-ones bytes."""
    import cell_sort_ref as ref
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    ns, n = offsets.size - 1, int(offsets[-1])
    cap = int(cells_cap) or 10 * n + 256 * ns
    stride = n // 256 if n >= 256 else 1
    status = np.full(ref.STATUS_WORDS, -1, dtype=np.int32)
    grid = np.full(6 * ns, -1, dtype=np.int64).view(ref.GRID)
    ncells = np.full(ns, -1, dtype=np.int64)
    sq = np.full(4 * n, -1, dtype=np.int64).view(np.float64)
    s_idx = np.full(2 * n, -1, dtype=np.int64).view(ref.IDX)
    cell_start = np.full(cap + 2, -1, dtype=np.int32)
    L = _load()
    L.emu_cell_sort.argtypes = [_dp, _dp, _lp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 6
    L.emu_cell_sort(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns, probe, 1 if shared_radii else 0,
                    stride, cap, status.ctypes.data, grid.ctypes.data, ncells.ctypes.data, sq.ctypes.data, s_idx.ctypes.data, cell_start.ctypes.data)
    return {"status": status, "error": int(status[ref.ST_ERROR]), "retry": int(status[ref.ST_RETRY]), "occ_sum": int(status[ref.ST_OCC_SUM]),
            "occ_n": int(status[ref.ST_OCC_N]), "cells": int(status[ref.ST_CELLS:ref.ST_CELLS + 2].view(np.int64)[0]), "occ_stride": stride,
            "cells_cap": cap, "grid": grid, "ncells": ncells, "sq": sq.reshape(-1, 4), "s_idx": s_idx, "cell_start": cell_start}


def kat_elementwise(op, a=None, b=None, c=None, k=0.0, n=None, outputs=2):
    """The emulated elementwise known-answer kernel (emu_kat_elementwise), with GpuContext.kat_elementwise's arguments, result
    and refusals."""
    arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (a, b, c)]
    if n is None:
        n = max([x.size for x in arrs if x is not None] or [0])
    if any(x is not None and x.size < min(max(int(n), 0), 1 << 20) for x in arrs):
        raise ValueError("kat_elementwise: an array is shorter than n")
    outs = [np.full(max(int(n), 0), np.nan) if j < outputs else None for j in range(2)]
    ptr = lambda x: x.ctypes.data if x is not None else None
    L = _load()
    L.emu_kat_elementwise.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_void_p, C.c_void_p]
    if L.emu_kat_elementwise(int(op), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), int(n), float(k), ptr(outs[0]), ptr(outs[1])):
        raise ValueError("emu_kat_elementwise: refused")
    return outs[0], outs[1]


def kat_wave(op, words, rows=None):
    """The emulated wave known-answer kernel (emu_kat_wave): uint64 [rows, 64] in and out, as GpuContext.kat_wave."""
    w = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 64)
    if rows is None:
        rows = 0 if w is None else w.shape[0]
    if w is not None and w.shape[0] < min(max(int(rows), 0), 4096):
        raise ValueError("kat_wave: fewer rows than said")
    out = None if w is None else np.zeros_like(w)
    L = _load()
    L.emu_kat_wave.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    if L.emu_kat_wave(int(op), None if w is None else w.ctypes.data, int(rows), None if out is None else out.ctypes.data):
        raise ValueError("emu_kat_wave: refused")
    return out
