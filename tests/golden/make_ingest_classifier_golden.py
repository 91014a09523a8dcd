#!/usr/bin/env python3
"""Mint the loader vectors under user classifiers: what the REFERENCE LIBRARY (oracle/_ref/libfreesasa_ref.so) holds after
freesasa_structure_from_pdb() / _from_cif() with freesasa_classifier_from_file(<config>) for the ingestion fixtures, under
the option sets of make_ingest_golden.py.  Runs only in the build container (like make_ingest_golden.py).  Output:
  tests/golden/classifiers/syn_any.pdb, syn_any.cif   inputs of this project's making: atoms only ANY rows resolve,
                                                      unknown residues, an mmCIF auth_comp_id longer than 3 characters
  tests/golden/ingest_classifiers.json                per config, file and option set: atom / residue counts and the
                                                      first 16 hex digits of the sha256 of the coordinate, radius, class
                                                      and residue-boundary arrays ({"fail": true} / {"crash": true} as in
                                                      ingest.json); "totals": L&R-20 and S&R-100 totals of a few entries
                                                      under the NACCESS radii (probe 1.4, one thread)
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_ingest_golden as G  # noqa: E402  (sets up the reference library's prototypes)
import oracle  # noqa: E402

lib, libc, from_cif = G.lib, G.libc, G.from_cif
lib.freesasa_classifier_from_file.restype = C.c_void_p
lib.freesasa_classifier_from_file.argtypes = [C.c_void_p]
lib.freesasa_classifier_free.argtypes = [C.c_void_p]
lib.freesasa_calc_structure.restype = C.POINTER(oracle.Result)
lib.freesasa_calc_structure.argtypes = [C.c_void_p, C.POINTER(oracle.Parameters)]
lib.freesasa_result_free.argtypes = [C.c_void_p]

CFG = os.path.join(HERE, "classifiers")
CONFIGS = ["protor", "naccess", "oons", "synthetic"]  # (the reference rejects its own dssp.config: classes 'backbone' / 'sidechain')
TOTAL_FILES = ["1ubq.pdb", "1a0q.pdb", "3bkr.pdb"]


def pdb_path(name):
    if name.startswith("syn_any"):
        return os.path.join(CFG, name)
    return os.path.join(HERE, "cif" if name.endswith(".cif") else "pdb", name)


def inputs():
    """(name, option sets) of every file the vectors cover"""
    pdb = [n for n in G.synthetic_files()] + G.FILES + ["syn_any.pdb"]
    cif = G.CIF_FILES + [n for n in G.synthetic_cifs()] + ["syn_any.cif"]
    return [(n, G.OPTION_SETS) for n in pdb] + [(n, G.CIF_OPTION_SETS) for n in cif]


def synthetic_any():
    L = G.atom_line
    pdb = "\n".join([
        L(1, " N  ", "LIG", "A", 1, "   1.000   2.000   3.000", tail="  1.00  0.00           N  "),   # ANY N only
        L(2, " CA ", "LIG", "A", 1, "   2.000   2.000   3.000"),                                      # ANY CA
        L(3, " C1 ", "LIG", "A", 1, "   3.000   2.000   3.000"),                                      # LIG's own row (synthetic)
        L(4, " CB ", "ALA", "A", 2, "   4.000   2.000   3.000"),                                      # ALA lists CB
        L(5, " SG ", "CYS", "A", 3, "   5.000   2.000   3.000", tail="  1.00  0.00           S  "),   # ANY SG (synthetic)
        L(6, " CA ", "XYZ", "A", 4, "   6.000   2.000   3.000"),                                      # unknown residue, ANY CA
        L(7, " QQ ", "XYZ", "A", 4, "   7.000   2.000   3.000", tail="  1.00  0.00           Q  "),   # unknown everywhere
        L(8, " CA ", "GLY", "A", 5, "   8.000   2.000   3.000"),                                      # GLY CA before ANY CA
        L(9, " SD ", "MET", "A", 6, "   9.000   2.000   3.000", tail="  1.00  0.00           S  "),
        L(10, " P  ", " DA", "B", 1, "  10.000   2.000   3.000", tail="  1.00  0.00           P  "),
        L(11, " O5'", " DA", "B", 1, "  11.000   2.000   3.000", tail="  1.00  0.00           O  "),
        L(12, "FE  ", "FE ", "C", 1, "  12.000   2.000   3.000", tail="  1.00  0.00          FE  ", rec="HETATM"),
        L(13, " O  ", "HOH", "C", 2, "  13.000   2.000   3.000", tail="  1.00  0.00           O  ", rec="HETATM"),
    ]) + "\n"

    def row(i, sym, name, comp, seq, xyz, group="ATOM"):
        return f"{group} {i} {sym} {name} . {comp} A 1 {seq} ? {xyz} 1.00 10.00 ? {seq} {comp} A {name} 1"
    cif = G.cif_loop([
        row(1, "N", "N", "LIGAND", 1, "1.000 2.000 3.000"),       # auth_comp_id longer than 3: cut to LIG
        row(2, "C", "CA", "LIGAND", 1, "2.000 2.000 3.000"),
        row(3, "C", "C1", "LIG01", 1, "3.000 2.000 3.000"),
        row(4, "C", "CB", "ALANINE", 2, "4.000 2.000 3.000"),     # cut to ALA
        row(5, "C", "CA", "XYZW", 3, "5.000 2.000 3.000"),        # unknown residue, ANY CA
        row(6, "S", "SG", "CYS", 4, "6.000 2.000 3.000"),
        row(7, "Q", "QQ", "XYZ", 5, "7.000 2.000 3.000"),
        row(8, "C", "CA", "GLY", 6, "8.000 2.000 3.000"),
        row(9, "O", "O", "HOH", 7, "9.000 2.000 3.000", group="HETATM"),
    ])
    return {"syn_any.pdb": pdb, "syn_any.cif": cif}


def short(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def view_unsafe(path, options, cfg):
    fc = libc.fopen(cfg.encode(), b"r")
    cls = lib.freesasa_classifier_from_file(fc)
    libc.fclose(fc)
    assert cls, cfg
    fp = libc.fopen(path.encode(), b"r")
    s = from_cif(fp, cls, options) if path.endswith(".cif") else lib.freesasa_structure_from_pdb(fp, cls, options)
    libc.fclose(fp)
    if not s:
        return {"fail": True}
    n, nr = lib.freesasa_structure_n(s), lib.freesasa_structure_n_residues(s)
    if n == 0:
        return {"fail": True}
    xyz = np.ctypeslib.as_array(lib.freesasa_structure_coord_array(s), shape=(3 * n,)).copy()
    rad = np.ctypeslib.as_array(lib.freesasa_structure_radius(s), shape=(n,)).copy()
    cl = np.array([lib.freesasa_structure_atom_class(s, i) for i in range(n)], dtype=np.uint8)
    first = []
    a, b = C.c_int(), C.c_int()
    for r in range(nr):
        lib.freesasa_structure_residue_atoms(s, r, C.byref(a), C.byref(b))
        first.append(a.value)
    out = {"n_atoms": n, "n_residues": nr, "xyz": short(xyz), "radii": short(rad), "classes": short(cl),
           "res_first": short(np.array(first + [n], dtype=np.int64))}
    if options == 0 and os.path.basename(path) in TOTAL_FILES and cfg.endswith("naccess.config"):
        for key, alg in (("lr20", 0), ("sr100", 1)):
            p = oracle.Parameters(alg, 1.4, 100, 20, 1)
            res = lib.freesasa_calc_structure(s, C.byref(p))
            out[key] = res.contents.total
            lib.freesasa_result_free(res)
    lib.freesasa_structure_free(s)
    return out


def view(path, options, cfg):
    """view_unsafe in a forked child (a few inputs make the reference abort: make_ingest_golden.reference_view)"""
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        os.close(r)
        try:
            os.write(w, json.dumps(view_unsafe(path, options, cfg)).encode())
        finally:
            os._exit(0)
    os.close(w)
    data = b""
    while True:
        chunk = os.read(r, 65536)
        if not chunk:
            break
        data += chunk
    os.close(r)
    _, status = os.waitpid(pid, 0)
    if status != 0 or not data:
        return {"crash": True}
    return json.loads(data)


def main():
    for name, text in synthetic_any().items():
        with open(os.path.join(CFG, name), "w", newline="") as fh:
            fh.write(text)
    out = {"vectors": {}, "totals": {}}
    for cfg in CONFIGS:
        path_cfg = os.path.join(CFG, cfg + ".config")
        per = {}
        for name, option_sets in inputs():
            per[name] = {str(o): view(pdb_path(name), o, path_cfg) for o in option_sets}
            for key in ("lr20", "sr100"):
                if key in per[name]["0"]:
                    out["totals"].setdefault(name, {})[key] = per[name]["0"].pop(key)
        out["vectors"][cfg] = per
    with open(os.path.join(HERE, "ingest_classifiers.json"), "w") as fh:
        fh.write("{\"totals\": " + json.dumps(out["totals"], sort_keys=True) + ",\n \"vectors\": {\n")
        cfgs = []
        for cfg in CONFIGS:
            lines = [f"   {json.dumps(n)}: {json.dumps(v, sort_keys=True)}" for n, v in out["vectors"][cfg].items()]
            cfgs.append(f"  {json.dumps(cfg)}: {{\n" + ",\n".join(lines) + "\n  }")
        fh.write(",\n".join(cfgs) + "\n }\n}\n")
    print(out["totals"])


if __name__ == "__main__":
    main()
