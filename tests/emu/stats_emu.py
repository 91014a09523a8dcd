"""TESTS ONLY: ctypes front-end of the CPU emulation of the run-statistics kernel (tests/emu/emu_stats.cpp)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libstats_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libstats_emu.so"))
        _lib.emu_traj_stats.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.c_int, C.c_int, C.c_void_p]
        _lib.emu_traj_stats.restype = C.c_longlong
    return _lib


def traj_stats(blocks):
    """k_traj_stats on the blocks [nf, w_k] of one shard (one segment each): its partial [4, sum w_k] - mean, M2, min, max"""
    blocks = [np.ascontiguousarray(b, dtype=np.float64) for b in blocks]
    nf = blocks[0].shape[0]
    assert all(b.ndim == 2 and b.shape[0] == nf for b in blocks)
    W = sum(b.shape[1] for b in blocks)
    out = np.full((4, W), np.nan)
    ptrs = (C.c_void_p * len(blocks))(*[b.ctypes.data for b in blocks])
    widths = (C.c_longlong * len(blocks))(*[b.shape[1] for b in blocks])
    rc = _load().emu_traj_stats(ptrs, widths, len(blocks), nf, out.ctypes.data)
    if rc != W:
        raise RuntimeError("emu_traj_stats: bad argument")
    return out
