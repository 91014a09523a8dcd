"""TESTS ONLY: ctypes front-end of the CPU emulation of the per-residue interface tables per frame
(tests/emu/emu_traj_pair_res.cpp): the host cut of the segments (traj_pair_res_cut) and the traj_pair_res phase function of
csrc/traj_kernels.h in the grid of its kernel."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libtraj_pair_res_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libtraj_pair_res_emu.so"))
        p = C.c_void_p
        _lib.emu_tpr_cut.argtypes = [p, C.c_int, C.c_int, p, C.c_int, p, C.c_int, C.c_longlong, p, p, p, p]
        _lib.emu_tpr_cut.restype = C.c_longlong
        _lib.emu_tpr_shard.argtypes = [p, C.c_int, C.c_int, p, C.c_int, p, C.c_int, C.c_int, p, C.c_double, p]
    return _lib


def _args(group, pairs, res_first):
    group = np.ascontiguousarray(group, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    res_first = np.ascontiguousarray(res_first, dtype=np.int64)
    return group, pairs, res_first


def cut(group, n_groups, pairs, res_first):
    """traj_group_cut, traj_pair_cut, then traj_pair_res_cut: (seg_first [S + 1], seg_res [S], seg_side [S], seg_iso [S])"""
    group, pairs, res_first = _args(group, pairs, res_first)
    a = (group.ctypes.data, group.size, n_groups, pairs.ctypes.data, pairs.shape[0], res_first.ctypes.data, res_first.size - 1)
    S = _load().emu_tpr_cut(*a, -1, None, None, None, None)
    if S < 0:
        raise ValueError("bad group id or pair")
    first, iso = np.full(S + 2, -7, dtype=np.int64), np.full(S + 1, -7, dtype=np.int64)
    res, side = np.full(S + 1, -7, dtype=np.int32), np.full(S + 1, -7, dtype=np.int32)
    assert _load().emu_tpr_cut(*a, S, first.ctypes.data, res.ctypes.data, side.ctypes.data, iso.ctypes.data) == S
    assert first[-1] == -7 and iso[-1] == -7 and res[-1] == -7 and side[-1] == -7
    return first[:-1].copy(), res[:-1].copy(), side[:-1].copy(), iso[:-1].copy()


def shard(group, n_groups, pairs, res_first, nf, csasa, min_buried):
    """one shard of nf frames: csasa [nf (n + n_iso + n_pair)] the areas of the combined batch -> [nf, S, 4]"""
    group, pairs, res_first = _args(group, pairs, res_first)
    csasa = np.ascontiguousarray(csasa, dtype=np.float64)
    S = cut(group, n_groups, pairs, res_first)[1].size
    counts = np.bincount(group[group >= 0], minlength=n_groups)
    nc = group.size + int(counts.sum()) + int(sum(counts[g] + counts[h] for g, h in pairs))
    assert csasa.size == nf * nc
    out = np.full((nf, S, 4), np.nan)
    rc = _load().emu_tpr_shard(group.ctypes.data, group.size, n_groups, pairs.ctypes.data, pairs.shape[0], res_first.ctypes.data,
                               res_first.size - 1, nf, csasa.ctypes.data, float(min_buried), out.ctypes.data)
    if rc:
        raise RuntimeError("emu_tpr_shard: bad argument")
    return out
