#!/usr/bin/env python3
"""Mint tests/golden/chain_groups.json from the REAL reference (run in the build container, like make_golden.py).

For each case - a committed PDB fixture and a chain-group spec, or separate chains - the reference library cuts the
groups out as it does for its CLI's --chain-groups / --separate-chains (freesasa_structure_get_chains_lcl,
freesasa_structure_array with FREESASA_SEPARATE_CHAINS; oracle/_ref/libfreesasa_ref.so), and freesasa_calc_coord gives
the total area of the whole structure and of every group, Lee-Richards 20 slices and Shrake-Rupley 100 points, probe
1.4.  Totals only: tests/test_groups_gpu.py compares freesasa_gpu_groups_dev's totals with them.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PDB = os.path.join(OUT, "pdb")
CASES = [("1a0q.pdb", "H+L"), ("2jo4.pdb", "AB+CD"), ("3gnn.pdb", None)]   # None: separate chains


class ChainGroup(C.Structure):
    _fields_ = [("chains", C.POINTER(C.c_char_p)), ("n", C.c_size_t)]


ref = oracle.Reference()
L = ref.lib
L.freesasa_set_verbosity(2)
libc = C.CDLL(None)
libc.fopen.restype = C.c_void_p
libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
libc.fclose.argtypes = [C.c_void_p]
L.freesasa_structure_from_pdb.restype = C.c_void_p
L.freesasa_structure_from_pdb.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
L.freesasa_structure_array.restype = C.POINTER(C.c_void_p)
L.freesasa_structure_array.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
L.freesasa_structure_get_chains_lcl.restype = C.c_void_p
L.freesasa_structure_get_chains_lcl.argtypes = [C.c_void_p, C.POINTER(ChainGroup), C.c_void_p, C.c_int]
L.freesasa_structure_n.argtypes = [C.c_void_p]
L.freesasa_structure_coord_array.restype = C.POINTER(C.c_double)
L.freesasa_structure_coord_array.argtypes = [C.c_void_p]
L.freesasa_structure_radius.restype = C.POINTER(C.c_double)
L.freesasa_structure_radius.argtypes = [C.c_void_p]


def xyz_r(s):
    n = L.freesasa_structure_n(s)
    return (np.ctypeslib.as_array(L.freesasa_structure_coord_array(s), (3 * n,)).copy(),
            np.ctypeslib.as_array(L.freesasa_structure_radius(s), (n,)).copy())


def totals(s):
    x, r = xyz_r(s)
    return {"atoms": int(r.size),
            "lr20": ref.calc_coord(x, r, oracle.LEE_RICHARDS, 1.4, n_slices=20)[1],
            "sr100": ref.calc_coord(x, r, oracle.SHRAKE_RUPLEY, 1.4, n_points=100)[1]}


def main():
    out = []
    for name, spec in CASES:
        path = os.path.join(PDB, name).encode()
        fh = libc.fopen(path, b"r")
        whole = L.freesasa_structure_from_pdb(fh, None, 0)
        libc.fclose(fh)
        case = {"file": name, "spec": spec, "complex": totals(whole), "groups": []}
        if spec is not None:
            for grp in spec.split("+"):
                arr = (C.c_char_p * len(grp))(*[c.encode() for c in grp])
                cg = ChainGroup(arr, len(grp))
                s = L.freesasa_structure_get_chains_lcl(whole, C.byref(cg), None, 0)
                case["groups"].append(totals(s))
        else:
            fh = libc.fopen(path, b"r")
            n = C.c_int(0)
            arr = L.freesasa_structure_array(fh, C.byref(n), None, 1 << 4)   # FREESASA_SEPARATE_CHAINS
            libc.fclose(fh)
            case["groups"] = [totals(arr[k]) for k in range(n.value)]
        out.append(case)
    with open(os.path.join(OUT, "chain_groups.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
