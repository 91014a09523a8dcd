"""TESTS ONLY: ctypes front-end of the CPU emulation of the interfaces between chain groups per frame
(tests/emu/emu_traj_pairs.cpp): the host cuts and the traj_group_* / traj_pair_* phase functions of csrc/traj_kernels.h in the
driver's launch order, and k_totals (totals_phase0 / totals_phase1, csrc/sasa_kernels.h) over one segment."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libtraj_pairs_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libtraj_pairs_emu.so"))
        p = C.c_void_p
        _lib.emu_tp_tot_b.restype = C.c_int
        _lib.emu_tp_ktotals.argtypes = [p, C.c_longlong]
        _lib.emu_tp_ktotals.restype = C.c_double
        _lib.emu_tp_cut.argtypes = [p, C.c_int, C.c_int, p, C.c_int, p, p, p, p, p, C.c_longlong]
        _lib.emu_tp_cut.restype = C.c_longlong
        _lib.emu_tp_shard.argtypes = [p, C.c_int, C.c_int, p, C.c_int, p, C.c_int, p, p, p, p, p, p, p, p]
    return _lib


def tot_b():
    """SASA_TOT_B"""
    return int(_load().emu_tp_tot_b())


def k_totals(v):
    """k_totals over the one segment v"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    return float(_load().emu_tp_ktotals(v.ctypes.data, v.size))


def cut(group, n_groups, pairs):
    """traj_group_cut, then traj_pair_cut: (pfirst [K + 1], pside [2 K + 1], psrc [n_pair])"""
    group = np.ascontiguousarray(group, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    K = pairs.shape[0]
    gfirst, src = np.full(n_groups + 1, -7, dtype=np.int64), np.full(group.size, -7, dtype=np.int32)
    pfirst, pside = np.full(K + 1, -7, dtype=np.int64), np.full(2 * K + 1, -7, dtype=np.int64)
    cap = 2 * K * group.size
    psrc = np.full(cap + 1, -7, dtype=np.int32)
    n_pair = _load().emu_tp_cut(group.ctypes.data, group.size, n_groups, pairs.ctypes.data, K, gfirst.ctypes.data, src.ctypes.data,
                                pfirst.ctypes.data, pside.ctypes.data, psrc.ctypes.data, cap)
    if n_pair < 0:
        raise ValueError("bad group id or pair")
    assert np.all(psrc[n_pair:] == -7)
    return pfirst, pside, psrc[:n_pair].copy()


def shard(group, n_groups, pairs, radii, frames, csasa, want_iso=True):
    """One shard as the driver runs it with interface pairs.  frames [nf, n, 3]: the compact frames; csasa [nf (n + n_iso +
    n_pair)]: the areas of the combined batch.  Returns (xyz [nf nc, 3] the combined batch's coordinates, cradii [nf nc], iso
    [nf, n] or None, totals [nf], group_areas [nf, G, 3], pair_areas [nf, K, 6], side_off [2 K nf + 1])."""
    group = np.ascontiguousarray(group, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    csasa = np.ascontiguousarray(csasa, dtype=np.float64)
    nf, n = frames.shape[:2]
    K = pairs.shape[0]
    counts = np.bincount(group[group >= 0], minlength=n_groups)
    nc = n + int(counts.sum()) + int(sum(counts[g] + counts[h] for g, h in pairs))
    assert csasa.size == nf * nc and radii.size == n == group.size
    xyz = np.full((nf * nc, 3), np.nan)
    xyz[:nf * n] = frames.reshape(-1, 3)
    cradii = np.full(nf * nc, np.nan)
    iso = np.full((nf, n), np.nan) if want_iso else None
    totals, gout, pout = np.full(nf, np.nan), np.full((nf, n_groups, 3), np.nan), np.full((nf, K, 6), np.nan)
    side_off = np.full(2 * K * nf + 1, -7, dtype=np.int64)
    rc = _load().emu_tp_shard(group.ctypes.data, n, n_groups, pairs.ctypes.data, K, radii.ctypes.data, nf, xyz.ctypes.data,
                              cradii.ctypes.data, csasa.ctypes.data, None if iso is None else iso.ctypes.data, totals.ctypes.data,
                              gout.ctypes.data, pout.ctypes.data, side_off.ctypes.data)
    if rc:
        raise RuntimeError("emu_tp_shard: bad argument")
    return xyz, cradii, iso, totals, gout, pout, side_off
