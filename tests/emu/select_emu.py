"""TESTS ONLY: ctypes front-end of the CPU emulation of the selection kernels (tests/emu/emu_select.cpp)."""
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
        subprocess.run(["make", "-C", ROOT, "tests/emu/libselect_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libselect_emu.so"))
        _lib.emu_select.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    return _lib


def run(selection, batch, sasa=None):
    """The set's program over every atom of the batch, as k_sel_mask / k_sel_sums run it: bits[n_atoms] uint64 and, with
    per-atom areas, (bits, areas[n_structs, S], counts[n_structs, S])."""
    L = ingest._selection_proto()
    nw, flags = C.c_int(0), C.c_int(0)
    prog = L.freesasa_ingest_selection_program(selection.handle, C.byref(nw), C.byref(flags))
    S = len(selection)
    bits = np.zeros(batch.n_atoms, dtype=np.uint64)
    areas, counts = np.zeros((batch.n_structs, S)), np.zeros((batch.n_structs, S), dtype=np.int64)
    cb = batch._as_c()
    w = None if sasa is None else np.ascontiguousarray(sasa, dtype=np.float64)
    rc = _load().emu_select(prog, nw.value, flags.value, S, C.byref(cb), w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
                            bits.ctypes.data_as(C.POINTER(C.c_uint64)), areas.ctypes.data_as(C.POINTER(C.c_double)),
                            counts.ctypes.data_as(C.POINTER(C.c_longlong)))
    if rc:
        raise RuntimeError("emu_select: bad argument")
    return bits if sasa is None else (bits, areas, counts)
