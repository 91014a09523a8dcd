"""TESTS ONLY: ctypes front-end of the CPU emulation of the group-ids kernel (tests/emu/emu_groups.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

import freesasa_amd as fa
from freesasa_amd import ingest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MAX_LABELS = 4096
_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libgroups_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "libgroups_emu.so"))
        i32 = C.POINTER(C.c_int32)
        _lib.emu_group_ids.argtypes = [C.c_char_p, i32, C.c_int, C.c_int, C.c_void_p, i32, i32, i32]
    return _lib


def parse(spec, flags):
    """freesasa_ingest_chain_groups_parse of the product library: (labels bytes, groups, n_labels, n_groups); ValueError with
    its message"""
    L = ingest._proto()
    L.freesasa_ingest_chain_groups_parse.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int),
                                                     C.c_char_p, C.c_int]
    labels = C.create_string_buffer(4 * MAX_LABELS)
    groups = (C.c_int32 * MAX_LABELS)()
    n, err = C.c_int(0), C.create_string_buffer(256)
    G = L.freesasa_ingest_chain_groups_parse(spec.encode() if spec is not None else None, flags, labels, groups, C.byref(n), err, 256)
    if G < 0:
        raise ValueError(err.value.decode())
    return labels, groups, n.value, G


def run(batch, spec=None, long=False, separate_chains=False):
    """(group[n_atoms], n_groups[n_structs], status[n_structs]) as k_gid_struct makes them"""
    flags = (ingest.GROUPS_LONG if long else 0) | (ingest.SEPARATE_CHAINS if separate_chains else 0)
    labels, groups, n_lab, G = parse(spec, flags)
    group = np.full(batch.n_atoms, -7, dtype=np.int32)
    n_groups = np.full(batch.n_structs, -7, dtype=np.int32)
    status = np.full(batch.n_structs, -7, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    cb = batch._as_c()
    rc = _load().emu_group_ids(labels, groups, n_lab, G, C.byref(cb), group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32),
                               status.ctypes.data_as(i32))
    if rc:
        raise RuntimeError("emu_group_ids: bad argument")
    return group, n_groups, status
