"""TESTS ONLY: ctypes front-end of the CPU emulation of the DCD gather kernel (tests/emu/emu_dcd.cpp)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libdcd_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libdcd_emu.so"))
        _lib.emu_traj_gather_dcd.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return _lib


def gather(file_bytes, info, n_frames, index=None):
    """k_traj_gather_dcd over the first n_frames frames of a DCD file's bytes (info: freesasa_amd.dcd_info of it):
    -> [n_frames, len(index) or NATOM, 3] float64, NaN where no thread wrote"""
    raw = np.frombuffer(file_bytes, dtype=np.uint8)[info.first_frame:info.first_frame + n_frames * info.frame_bytes]
    frames = np.empty(raw.size // 4, dtype=np.uint32)            # (4-byte aligned, as the device buffer is)
    frames.view(np.uint8)[:] = raw
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    n = info.n_atoms if idx is None else idx.size
    out = np.full((n_frames, n, 3), np.nan)
    rc = _load().emu_traj_gather_dcd(frames.ctypes.data, n_frames, info.frame_bytes, info.x_off, info.plane_bytes, info.big_endian,
                                     None if idx is None else idx.ctypes.data, n, out.ctypes.data)
    if rc:
        raise RuntimeError("emu_traj_gather_dcd: bad argument")
    return out
