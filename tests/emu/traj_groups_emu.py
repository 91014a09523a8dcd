"""TESTS ONLY: ctypes front-end of the CPU emulation of chain groups per frame (tests/emu/emu_traj_groups.cpp): the host cut and
the traj_group_* phase functions of csrc/traj_kernels.h, and the chain-group entry's own phase functions (group_kernels.h) on
one frame as a batch of one structure."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libtraj_groups_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libtraj_groups_emu.so"))
        p = C.c_void_p
        _lib.emu_tg_cut.argtypes = [p, C.c_int, C.c_int, p, p, C.POINTER(C.c_longlong)]
        _lib.emu_tg_cut.restype = C.c_longlong
        _lib.emu_tg_shard.argtypes = [p, C.c_int, C.c_int, p, C.c_int, p, p, p, p, p, p]
        _lib.emu_grp_one.argtypes = [p, p, p, C.c_int, C.c_int, p, p, p, p, p, p, p, p]
        _lib.emu_grp_one.restype = C.c_longlong
    return _lib


def cut(group, n_groups):
    """traj_group_cut: (gfirst [G + 1], src [n_iso]); ValueError naming the atom for a bad id"""
    group = np.ascontiguousarray(group, dtype=np.int32)
    gfirst = np.full(n_groups + 1, -7, dtype=np.int64)
    src = np.full(group.size, -7, dtype=np.int32)
    bad = C.c_longlong(-1)
    n_iso = _load().emu_tg_cut(group.ctypes.data, group.size, n_groups, gfirst.ctypes.data, src.ctypes.data, C.byref(bad))
    if n_iso < 0:
        raise ValueError("atom %d has a bad group id" % bad.value)
    return gfirst, src[:n_iso].copy()


def shard(group, n_groups, radii, frames, csasa, want_iso=True):
    """One shard as the driver runs it.  frames [nf, n, 3]: the compact frames; csasa [nf (n + n_iso)]: the areas of the combined
    batch.  Returns (xyz [nf (n + n_iso), 3] the combined batch's coordinates, cradii, iso [nf, n] or None, totals [nf],
    group_areas [nf, G, 3])."""
    group = np.ascontiguousarray(group, dtype=np.int32)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    csasa = np.ascontiguousarray(csasa, dtype=np.float64)
    nf, n = frames.shape[:2]
    n_iso = int(np.count_nonzero(group >= 0))
    assert csasa.size == nf * (n + n_iso) and radii.size == n == group.size
    xyz = np.full((nf * (n + n_iso), 3), np.nan)
    xyz[:nf * n] = frames.reshape(-1, 3)
    cradii = np.full(nf * (n + n_iso), np.nan)
    iso = np.full((nf, n), np.nan) if want_iso else None
    totals, out = np.full(nf, np.nan), np.full((nf, n_groups, 3), np.nan)
    rc = _load().emu_tg_shard(group.ctypes.data, n, n_groups, radii.ctypes.data, nf, xyz.ctypes.data, cradii.ctypes.data,
                              csasa.ctypes.data, None if iso is None else iso.ctypes.data, totals.ctypes.data, out.ctypes.data)
    if rc:
        raise RuntimeError("emu_tg_shard: bad argument")
    return xyz, cradii, iso, totals, out


def groups_one(xyz, radii, group, n_groups, csasa=None):
    """freesasa_gpu_groups_dev's kernels on ONE structure.  Without csasa: (src [n_iso], cxyz [n + n_iso, 3], cradii) - the
    combined batch the rank kernel makes; with csasa [n + n_iso], its areas: (sasa [n], iso [n], total, group_totals [G, 3])."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    group = np.ascontiguousarray(group, dtype=np.int32)
    n = radii.size
    n_iso = int(np.count_nonzero(group >= 0))
    src = np.full(n, -7, dtype=np.int32)
    cxyz, cradii = np.full((n + n_iso, 3), np.nan), np.full(n + n_iso, np.nan)
    if csasa is None:
        rc = _load().emu_grp_one(xyz.ctypes.data, radii.ctypes.data, group.ctypes.data, n, n_groups, None, src.ctypes.data,
                                 cxyz.ctypes.data, cradii.ctypes.data, None, None, None, None)
        if rc != n_iso:
            raise RuntimeError("emu_grp_one: bad argument")
        return src[:n_iso].copy(), cxyz, cradii
    csasa = np.ascontiguousarray(csasa, dtype=np.float64)
    assert csasa.size == n + n_iso
    sasa, iso, total, gtot = np.full(n, np.nan), np.full(n, np.nan), np.full(1, np.nan), np.full((n_groups, 3), np.nan)
    rc = _load().emu_grp_one(xyz.ctypes.data, radii.ctypes.data, group.ctypes.data, n, n_groups, csasa.ctypes.data, src.ctypes.data,
                             None, None, sasa.ctypes.data, iso.ctypes.data, total.ctypes.data, gtot.ctypes.data)
    if rc != n_iso:
        raise RuntimeError("emu_grp_one: bad argument")
    return sasa, iso, total[0], gtot
