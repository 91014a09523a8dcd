"""TESTS ONLY: ctypes front-end of the CPU emulation of the two phases of chain groups among periodic images with the pair part of
a trajectory shard's combined batch (tests/emu/emu_traj_pairs_pbc.cpp; csrc/pbc_kernels.h, GpbcArgs with k_fixed): the cells of
the combined structures and the fused collect-and-finish.  Every output is pre-filled with SENTINEL and returned WHOLE, a guard of
PAD elements behind its end included, so a test sees what no thread wrote."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SENTINEL = -7777.5
PAD = 300                                                    # more than the idle threads of a kernel's last workgroup (PBC_B = 256)
_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libtraj_pairs_pbc_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libtraj_pairs_pbc_emu.so"))
        _lib.emu_gpbc_pair_cells.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.emu_gpbc_pair_finish.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # the groups' run's own entries (emu_groups_pbc.cpp): the yardstick of k_fixed = 0
        _lib.emu_gpbc_cells.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.emu_gpbc_finish.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def cells(cells_in, G, K, old=False):
    """k_gpbc_cells over a shard's nf frames with G groups and K pair structures each: cells_in [nf, W] (W = 3 or 9) ->
    [nf (1 + G + K) + PAD, W], the guard rows still SENTINEL.  old: the groups' run's entry (K must be 0)."""
    cells_in = np.ascontiguousarray(cells_in, dtype=np.float64)
    nf, W = cells_in.shape
    out = np.full((nf * (1 + G + K) + PAD, W), SENTINEL)
    rc = (_load().emu_gpbc_cells(nf, nf * (1 + G), None, G, W, cells_in.ctypes.data, out.ctypes.data) if old else
          _load().emu_gpbc_pair_cells(nf, G, K, W, cells_in.ctypes.data, out.ctypes.data))
    if rc:
        raise RuntimeError("emu_gpbc_pair_cells: bad argument")
    return out


def finish(nf, G, K, coff, eoff, esasa, src, key, old=False):
    """k_gpbc_finish over such a shard -> (sasa, iso, carea, cgath), EACH [n_all + PAD] and pre-filled with SENTINEL: sasa and iso
    own their first nf n elements, carea and cgath their first n_all.  src [n_iso], key [n]: the topology's.  old: the groups'
    run's entry (K must be 0)."""
    coff, eoff = np.ascontiguousarray(coff, dtype=np.int64), np.ascontiguousarray(eoff, dtype=np.int64)
    esasa = np.ascontiguousarray(esasa, dtype=np.float64)
    src, key = np.ascontiguousarray(src, dtype=np.int32), np.ascontiguousarray(key, dtype=np.int32)
    assert coff.size == eoff.size == nf * (1 + G + K) + 1 and esasa.size == eoff[-1]
    N = int(coff[-1])
    sasa, iso, carea, cgath = (np.full(N + PAD, SENTINEL) for _ in range(4))
    L = _load()
    if old:
        rc = L.emu_gpbc_finish(nf, nf * (1 + G), coff.ctypes.data, eoff.ctypes.data, None, G, src.ctypes.data, key.size, src.size,
                               key.ctypes.data, esasa.ctypes.data, carea.ctypes.data, cgath.ctypes.data, sasa.ctypes.data, iso.ctypes.data)
    else:
        rc = L.emu_gpbc_pair_finish(nf, G, K, coff.ctypes.data, eoff.ctypes.data, src.ctypes.data, key.size, src.size, key.ctypes.data,
                                    esasa.ctypes.data, carea.ctypes.data, cgath.ctypes.data, sasa.ctypes.data, iso.ctypes.data)
    if rc:
        raise RuntimeError("emu_gpbc_pair_finish: bad argument")
    return sasa, iso, carea, cgath
