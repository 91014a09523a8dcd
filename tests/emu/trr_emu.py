"""TESTS ONLY: ctypes front-end of the CPU emulation of the GROMACS TRR gather kernel (tests/emu/emu_trr.cpp)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libtrr_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libtrr_emu.so"))
        _lib.emu_traj_gather_trr.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
        _lib.emu_traj_gather_trr.restype = C.c_longlong
    return _lib


def gather(shard_bytes, n_atoms, n_frames, index=None):
    """k_traj_gather_trr over a shard - the bytes of a run of whole TRR records of n_atoms atoms, n_frames of them with
    coordinates: -> [n_frames, len(index) or n_atoms, 3] float64 in Angstrom, NaN where no thread wrote"""
    raw = np.frombuffer(shard_bytes, dtype=np.uint8)
    words = np.empty(raw.size // 4, dtype=np.uint32)           # (4-byte aligned, as the device buffer is)
    words.view(np.uint8)[:] = raw
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    n = n_atoms if idx is None else idx.size
    out = np.full((n_frames, n, 3), np.nan)
    rc = _load().emu_traj_gather_trr(words.ctypes.data, raw.size, None if idx is None else idx.ctypes.data, n, n_frames, out.ctypes.data)
    if rc != n_frames:
        raise RuntimeError(f"emu_traj_gather_trr: {rc} (wanted {n_frames} frames)")
    return out
