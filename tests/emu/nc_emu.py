"""TESTS ONLY: ctypes front-end of the CPU emulation of the AMBER NetCDF gather kernel (tests/emu/emu_nc.cpp)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libnc_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libnc_emu.so"))
        _lib.emu_traj_gather_nc.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]
    return _lib


def gather(file_bytes, info, n_frames, index=None):
    """k_traj_gather_nc over the first n_frames records of a NetCDF file's bytes (info: freesasa_amd.nc_info of it):
    -> [n_frames, len(index) or the file's atoms, 3] float64, NaN where no thread wrote"""
    raw = np.frombuffer(file_bytes, dtype=np.uint8)[info.first_record:info.first_record + n_frames * info.record_bytes]
    records = np.empty(raw.size // 4, dtype=np.uint32)           # (4-byte aligned, as the device buffer is)
    records.view(np.uint8)[:] = raw
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    n = info.n_atoms if idx is None else idx.size
    out = np.full((n_frames, n, 3), np.nan)
    rc = _load().emu_traj_gather_nc(records.ctypes.data, n_frames, info.record_bytes, info.coord_off,
                                    None if idx is None else idx.ctypes.data, n, out.ctypes.data)
    if rc:
        raise RuntimeError("emu_traj_gather_nc: bad argument")
    return out
