#!/usr/bin/env python3
"""tools/interfaces.py STRUCTURE... [--chain-groups SPEC | --separate-chains] -o OUT.tsv [--alg lr|sr] [--resolution N] [--probe P]
                       [--residues RES.tsv [--min-buried X]]

The interface areas between the chain groups of structure files (freesasa_amd.calc_interfaces): one line per pair of groups
that are in contact - file, the two groups' chain labels, the atoms of each side, and six areas in A^2: each side's isolated
area, its area in the pair taken on its own, and the difference, the area the partner buries.  Files are loaded with
freesasa_amd.ingest.load_files (PDB or mmCIF, the loader's default options) and cut with its chain_groups: --chain-groups takes
the reference's syntax ("AB+CD": two groups), --separate-chains (the default) makes every chain a group.  A file that does not
load, or lacks a requested chain, is reported on stderr and gets no lines.
--residues RES.tsv adds the interface-residue table (the per-residue table of calc_interfaces, made on the device): one line per
residue of a side that loses more than --min-buried (default 0) A^2 - file, the two groups' labels, the label of the side the
residue is on, its chain, name and number (with insertion code), the atoms of the residue in that group, and its isolated
area, its area in the pair and the difference.  OUT.tsv is the same with and without it."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADER = "file\tgroup_a\tgroup_b\tatoms_a\tatoms_b\tiso_a\tiso_b\tin_pair_a\tin_pair_b\tburied_a\tburied_b"


def format_rows(files, labels, atoms, pair_struct, pair_groups, pair_areas):
    """the records, one string per interface (no line ends).  files [n_structs]: names; labels [n_structs][n_groups]: the label
    of every group; atoms [n_structs][n_groups]: its atom count; the three arrays of calc_interfaces."""
    out = []
    for s, (g, h), a in zip(pair_struct, pair_groups, pair_areas):
        s, g, h = int(s), int(g), int(h)
        out.append("\t".join([files[s], labels[s][g], labels[s][h], str(int(atoms[s][g])), str(int(atoms[s][h]))] + ["%.3f" % float(v) for v in a]))
    return out


RESIDUE_HEADER = "file\tgroup_a\tgroup_b\tside\tchain\tres_name\tres_number\tatoms\tiso\tin_pair\tburied"


def format_residue_rows(files, labels, pair_struct, pair_groups, res_offsets, res_index, res_atoms, res_areas, res_chain, res_name, res_number):
    """the residue records, one string per row of the per-residue table (no line ends), in its order: pair by pair, side a
    before side b.  res_chain, res_name, res_number: the loader's labels of every residue of the batch."""
    out = []
    for p, (s, (g, h)) in enumerate(zip(pair_struct, pair_groups)):
        s, g, h = int(s), int(g), int(h)
        for side, k in ((0, g), (1, h)):
            for j in range(int(res_offsets[2 * p + side]), int(res_offsets[2 * p + side + 1])):
                r = int(res_index[j])
                out.append("\t".join([files[s], labels[s][g], labels[s][h], labels[s][k], str(res_chain[r]).strip() or "_", str(res_name[r]).strip(),
                                      str(res_number[r]).strip(), str(int(res_atoms[j]))] + ["%.3f" % float(v) for v in res_areas[j]]))
    return out


def group_labels(batch, group, n_groups):
    """per structure, per group: the chain labels of its atoms in order of appearance, joined"""
    import numpy as np
    chain = np.repeat(np.asarray(batch.res_chain, dtype=object), np.diff(batch.res_first))
    labels, atoms = [], []
    for s in range(batch.n_structs):
        b, e = int(batch.offsets[s]), int(batch.offsets[s + 1])
        ls, ns = [], []
        for g in range(int(n_groups[s])):
            sel = group[b:e] == g
            seen = []
            for c in chain[b:e][sel]:
                t = str(c).strip() or "_"
                if t not in seen:
                    seen.append(t)
            ls.append("".join(seen) if all(len(t) == 1 for t in seen) else "/".join(seen))
            ns.append(int(sel.sum()))
        labels.append(ls); atoms.append(ns)
    return labels, atoms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    ap.add_argument("structures", nargs="+")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--chain-groups", default=None)
    ap.add_argument("--separate-chains", action="store_true")
    ap.add_argument("--alg", choices=("lr", "sr"), default="lr")
    ap.add_argument("--resolution", type=int, default=None)
    ap.add_argument("--probe", type=float, default=1.4)
    ap.add_argument("--residues", default=None, metavar="RES.tsv")
    ap.add_argument("--min-buried", type=float, default=0.0)
    args = ap.parse_args(argv)
    if args.chain_groups and args.separate_chains:
        sys.exit("--chain-groups and --separate-chains exclude each other")
    import freesasa_amd as fa
    from freesasa_amd import ingest
    batch = ingest.load_files(args.structures)
    group, n_groups, status = batch.chain_groups(args.chain_groups, separate_chains=args.chain_groups is None)
    for s, path in enumerate(args.structures):
        if batch.status[s] != 0 or status[s] != 0:
            print(f"{path}: not loaded or without a requested chain (status {int(batch.status[s])}, {int(status[s])})", file=sys.stderr)
    if batch.n_atoms == 0:
        sys.exit("no atoms loaded")
    alg = fa.LEE_RICHARDS if args.alg == "lr" else fa.SHRAKE_RUPLEY
    res = args.resolution or (20 if args.alg == "lr" else 100)
    if args.residues:
        got = fa.calc_interfaces(batch.xyz, batch.radii, batch.offsets, group, n_groups, alg=alg, probe=args.probe, resolution=res,
                                 res_first=batch.res_first, min_buried=args.min_buried)
    else:
        got = fa.calc_interfaces(batch.xyz, batch.radii, batch.offsets, group, n_groups, alg=alg, probe=args.probe, resolution=res)
    labels, atoms = group_labels(batch, group, n_groups)
    with open(args.output, "w") as f:
        f.write(HEADER + "\n")
        for line in format_rows([os.path.basename(p) for p in args.structures], labels, atoms, got.pair_struct, got.pair_groups, got.pair_areas):
            f.write(line + "\n")
    print(f"{got.n_pairs} interfaces of {batch.n_structs} structures -> {args.output}")
    if args.residues:
        with open(args.residues, "w") as f:
            f.write(RESIDUE_HEADER + "\n")
            for line in format_residue_rows([os.path.basename(p) for p in args.structures], labels, got.pair_struct, got.pair_groups,
                                            got.res_offsets, got.res_index, got.res_atoms, got.res_areas, batch.res_chain, batch.res_name,
                                            batch.res_number):
                f.write(line + "\n")
        print(f"{got.n_res_rows} interface residues -> {args.residues}")


if __name__ == "__main__":
    main()
