#!/usr/bin/env python3
"""Mint the vectors of the GENERATED parser inputs (tests/parse_gen.py): what the REFERENCE LIBRARY holds after
freesasa_structure_from_pdb() / freesasa_structure_from_cif() for every generated file under the family's option sets.
Same library and same handling of a crashing reference as make_ingest_golden.py (whose bindings this recipe uses);
like it, it runs only where oracle/_ref is built.  Output:
  tests/golden/parse_gen.json   per family: "options" (the option sets, the columns), "entries" (every distinct entry once),
                                "rows" (every distinct row of entries over the option sets once, as indices), "files" (per
                                file, in the generator's order, its row) and "names" (a digest of the file names, so that
                                vectors of other generators are noticed); an entry being the 64-bit digest of
                                parse_gen.digest() (atom count, coordinates, radii, classes, residue boundaries, labels),
                                "fail" (no structure, or one without atoms), "crash" (the reference aborted: the case binds
                                nobody) or "-" (not an option set of that file).  parse_gen.expected() reads it.
The generated files themselves are not kept: parse_gen.py remakes them."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_ingest_golden as G  # noqa: E402  (the reference's bindings)
import parse_gen  # noqa: E402


def view(path, options):
    """digest / "fail" for one file under one option set (in the calling process)"""
    lib = G.lib
    fp = G.libc.fopen(path.encode(), b"r")
    s = G.from_cif(fp, None, options) if path.endswith(".cif") else lib.freesasa_structure_from_pdb(fp, None, options)
    G.libc.fclose(fp)
    if not s:
        return "fail"
    n, nr = lib.freesasa_structure_n(s), lib.freesasa_structure_n_residues(s)
    if n == 0:      # the mmCIF reader hands back an empty structure where the PDB reader fails
        return "fail"
    xyz = np.ctypeslib.as_array(lib.freesasa_structure_coord_array(s), shape=(3 * n,)).copy()
    rad = np.ctypeslib.as_array(lib.freesasa_structure_radius(s), shape=(n,)).copy()
    cls = np.array([lib.freesasa_structure_atom_class(s, i) for i in range(n)], dtype=np.uint8)
    first, labels = [], []
    a, b = C.c_int(), C.c_int()
    for r in range(nr):
        lib.freesasa_structure_residue_atoms(s, r, C.byref(a), C.byref(b))
        first.append(a.value)
        labels.append(lib.freesasa_structure_residue_name(s, r).decode("latin-1") + "|" + lib.freesasa_structure_residue_number(s, r).decode("latin-1")
                      + "|" + lib.freesasa_structure_residue_chain_lcl(s, r).decode("latin-1"))
    lib.freesasa_structure_free(s)
    return parse_gen.digest(n, xyz, rad, cls, first + [n], labels)


def in_child(fn):
    """fn() in a forked child (the reference aborts on a few inputs): its JSON-able result, or None if the child died"""
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        os.close(r)
        try:
            os.write(w, json.dumps(fn()).encode())
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
    return json.loads(data) if status == 0 and data else None


def mint(path, opts):
    """one child for all option sets of a file; if it dies, one child per option set"""
    got = in_child(lambda: [view(path, o) for o in opts])
    if got is not None:
        return got
    out = []
    for o in opts:
        one = in_child(lambda: view(path, o))
        out.append("crash" if one is None else one)
    return out


def wrapped(items, per_line):
    """a JSON list over several lines"""
    parts = [json.dumps(v, separators=(",", ":")) for v in items]
    return "[" + ",\n".join(",".join(parts[k:k + per_line]) for k in range(0, len(parts), per_line)) + "]"


def main():
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for fam in parse_gen.FAMILIES:
            files = parse_gen.family(fam)
            all_opts = sorted({o for n, _, _ in files for o in parse_gen.options_of(fam, n)})
            entries, rows, per_file, flat = {}, {}, [], []
            for name, data, _ in files:
                path = os.path.join(tmp, name)
                with open(path, "wb") as fh:
                    fh.write(data)
                opts = parse_gen.options_of(fam, name)
                got = dict(zip(opts, mint(path, opts)))
                os.unlink(path)
                row = tuple(entries.setdefault(got.get(o, "-"), len(entries)) for o in all_opts)    # "-": not an option set of this file
                per_file.append(rows.setdefault(row, len(rows)))
                flat += [got.get(o, "-") for o in all_opts]
            out.append(f'"{fam}":{{"names":"{parse_gen.names_digest(fam)}","options":{json.dumps(all_opts, separators=(",", ":"))},\n'
                       f'"entries":{wrapped(list(entries), 8)},\n"rows":{wrapped([list(r) for r in rows], 6)},\n"files":{wrapped(per_file, 50)}}}')
            print(fam, len(files), "files;", flat.count("fail"), "fail,", flat.count("crash"), "crash of", len(flat) - flat.count("-"),
                  "-", len(entries), "entries,", len(rows), "rows")
    with open(os.path.join(HERE, "parse_gen.json"), "w") as fh:
        fh.write("{" + ",\n".join(out) + "}\n")


if __name__ == "__main__":
    main()
