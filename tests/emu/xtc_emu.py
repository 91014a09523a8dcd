"""TESTS ONLY: ctypes front-end of the CPU emulation of the XTC decode kernels (tests/emu/emu_xtc.cpp)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libxtc_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libxtc_emu.so"))
        _lib.emu_xtc_shard.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return _lib


def decode(file_bytes, n_frames, n_atoms):
    """k_xtc_scan and k_xtc_unpack over n_frames whole frames at the beginning of file_bytes -> (records: per frame the
    [groups, 4] int32 array of (bit, atom, run, smallidx), status [n_frames], xyz [n_frames, n_atoms, 3] float32 with NaN where
    no thread wrote, writes [n_frames, n_atoms, 3]: how often each element was written is not observable, so the caller checks
    NaN-freeness).  ValueError with the host's reason for a header it refuses."""
    words = np.empty((len(file_bytes) + 3) // 4, dtype=np.uint32)          # (4-byte aligned, as the device buffer is)
    words.view(np.uint8)[:len(file_bytes)] = np.frombuffer(file_bytes, dtype=np.uint8)
    rec = np.zeros((n_frames, n_atoms, 4), dtype=np.int32)
    count = np.full((n_frames, 2), -1, dtype=np.int32)
    out = np.full((n_frames, n_atoms, 3), np.nan, dtype=np.float32)
    why = C.create_string_buffer(300)
    rc = _load().emu_xtc_shard(words.ctypes.data, len(file_bytes), n_frames, n_atoms, rec.ctypes.data, count.ctypes.data, out.ctypes.data, why, 300)
    if rc:
        raise ValueError(f"emu_xtc_shard {rc}: {why.value.decode()}")
    return [rec[f, :max(int(count[f, 0]), 0)] for f in range(n_frames)], count[:, 1].copy(), out
