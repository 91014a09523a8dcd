"""TESTS ONLY: ctypes front-end of the CPU emulation of the residue contact occupancy map (tests/emu/emu_occupancy.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CHECK = os.path.join(HERE, "occ_check")
_lib = None
_dp, _lp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libocc_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libocc_emu.so"))
        _lib.emu_occ_open.restype = C.c_void_p
        _lib.emu_occ_close.argtypes = [C.c_void_p]
        _lib.emu_occ_rows.argtypes = [C.c_void_p]
        _lib.emu_occ_rows.restype = C.c_longlong
        _lib.emu_occ_frames.argtypes = [C.c_void_p]
        _lib.emu_occ_frames.restype = C.c_longlong
        _lib.emu_occ_add_rows.argtypes = [C.c_void_p, C.c_int, _lp, _ip, _ip, _dp, C.c_int]
        _lib.emu_occ_add_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, _ip, _ip, _lp, _ip, _ip, _dp, _lp]
        _lib.emu_occ_table.argtypes = [C.c_void_p, _ip, _lp, _lp, _lp, _dp, _lp, _ip]
    return _lib


def build_check():
    """tests/emu/occ_check (the phases under AddressSanitizer + UBSan, a program of its own): its path"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/occ_check"], check=True, stdout=subprocess.DEVNULL)
    return CHECK


class Accumulator:
    """the emulated accumulator: add_rows(frame_first, keys, counts, area, frames_per_batch), add_table(...) for a chunk that comes
    as a folded table, table() -> a dict of the run table's arrays and n_frames"""

    def __init__(self):
        self.h = _load().emu_occ_open()

    def close(self):
        if self.h:
            _load().emu_occ_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_rows(self, frame_first, keys, counts, area, frames_per_batch=256):
        ff, k = np.ascontiguousarray(frame_first, np.int64), np.ascontiguousarray(keys, np.int32).reshape(-1)
        c, a = np.ascontiguousarray(counts, np.int32).reshape(-1), np.ascontiguousarray(area, np.float64)
        if _load().emu_occ_add_rows(self.h, ff.size - 1, ff.ctypes.data_as(_lp), k.ctypes.data_as(_ip), c.ctypes.data_as(_ip), a.ctypes.data_as(_dp),
                                    frames_per_batch):
            raise RuntimeError("emu_occ_add_rows: bad argument")

    def add_table(self, n_frames, n_res, pair_struct, pair_groups, offsets, residues, counts, area):
        ps, pg = np.ascontiguousarray(pair_struct, np.int32), np.ascontiguousarray(pair_groups, np.int32).reshape(-1)
        off, res = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(residues, np.int32).reshape(-1)
        cnt, ar = np.ascontiguousarray(counts, np.int32).reshape(-1), np.ascontiguousarray(area, np.float64)
        fc = np.full((n_frames, 2), -7, np.int64)
        if _load().emu_occ_add_table(self.h, n_frames, n_res, ps.size, ps.ctypes.data_as(_ip), pg.ctypes.data_as(_ip), off.ctypes.data_as(_lp),
                                     res.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip), ar.ctypes.data_as(_dp), fc.ctypes.data_as(_lp)):
            raise RuntimeError("emu_occ_add_table: bad argument")
        return fc

    def table(self):
        L = _load()
        U = int(L.emu_occ_rows(self.h))
        t = dict(keys=np.zeros((U, 5), np.int32), frames=np.zeros(U, np.int64), frames_either=np.zeros(U, np.int64), counts=np.zeros((U, 2), np.int64),
                 area=np.zeros((U, 3)), span=np.zeros((U, 2), np.int64), reverse=np.zeros(U, np.int32))
        L.emu_occ_table(self.h, t["keys"].ctypes.data_as(_ip), t["frames"].ctypes.data_as(_lp), t["frames_either"].ctypes.data_as(_lp),
                        t["counts"].ctypes.data_as(_lp), t["area"].ctypes.data_as(_dp), t["span"].ctypes.data_as(_lp), t["reverse"].ctypes.data_as(_ip))
        t["n_frames"] = int(L.emu_occ_frames(self.h))
        return t
