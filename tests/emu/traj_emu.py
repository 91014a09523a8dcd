"""TESTS ONLY: ctypes front-end of the CPU emulation of the trajectory-topology kernels (tests/emu/emu_traj.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from freesasa_amd import ingest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libtraj_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libtraj_emu.so"))
        _lib.emu_traj_gather.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.emu_traj_sums.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def gather(frames, index):
    """k_traj_gather: frames [F, frame_atoms, 3] (float64 or float32) -> [F, len(index), 3] float64"""
    frames = np.ascontiguousarray(frames)
    assert frames.dtype in (np.float32, np.float64)
    index = np.ascontiguousarray(index, dtype=np.int32)
    out = np.full((frames.shape[0], index.size, 3), np.nan)
    rc = _load().emu_traj_gather(frames.ctypes.data, int(frames.dtype == np.float32), frames.shape[0], frames.shape[1],
                                 index.ctypes.data, index.size, out.ctypes.data)
    if rc:
        raise RuntimeError("emu_traj_gather: bad argument")
    return out


def sums(batch, structure, sasa, selection=None):
    """The per-frame kernels on sasa [F, n]: (class_sums [F, 3], residues [F, R, 6]) and, with an ingest.Selection,
    (..., bits [n], areas [F, S], counts [F, S])."""
    sasa = np.ascontiguousarray(sasa, dtype=np.float64)
    F, n = sasa.shape
    R = int(batch.res_offsets[structure + 1] - batch.res_offsets[structure])
    cls, res = np.full((F, 3), np.nan), np.full((F, R, 6), np.nan)
    cb = batch._as_c()
    if selection is None:
        rc = _load().emu_traj_sums(C.byref(cb), structure, None, 0, 0, 0, sasa.ctypes.data, F, cls.ctypes.data, res.ctypes.data,
                                   None, None, None)
        if rc != R:
            raise RuntimeError("emu_traj_sums: bad argument")
        return cls, res
    L = ingest._selection_proto()
    nw, flags = C.c_int(0), C.c_int(0)
    prog = L.freesasa_ingest_selection_program(selection.handle, C.byref(nw), C.byref(flags))
    S = len(selection)
    bits = np.zeros(n, dtype=np.uint64)
    areas, counts = np.full((F, S), np.nan), np.zeros((F, S), dtype=np.int64)
    rc = _load().emu_traj_sums(C.byref(cb), structure, prog, nw.value, flags.value, S, sasa.ctypes.data, F, cls.ctypes.data,
                               res.ctypes.data, bits.ctypes.data, areas.ctypes.data, counts.ctypes.data)
    if rc != R:
        raise RuntimeError("emu_traj_sums: bad argument")
    return cls, res, bits, areas, counts
