#!/usr/bin/env python3
"""tools/interfaces.py STRUCTURE... [--chain-groups SPEC | --separate-chains] -o OUT.tsv [--alg lr|sr] [--resolution N] [--probe P]
                       [--residues RES.tsv [--min-buried X]] [--contacts ATOMS.tsv [--residue-contacts RES.tsv]] [--contact-map MAP.tsv]

The interface areas between the chain groups of structure files (freesasa_amd.calc_interfaces): one line per pair of groups
that are in contact - file, the two groups' chain labels, the atoms of each side, and six areas in A^2: each side's isolated
area, its area in the pair taken on its own, and the difference, the area the partner buries.  Files are loaded with
freesasa_amd.ingest.load_files (PDB or mmCIF, the loader's default options) and cut with its chain_groups: --chain-groups takes
the reference's syntax ("AB+CD": two groups), --separate-chains (the default) makes every chain a group.  A file that does not
load, or lacks a requested chain, is reported on stderr and gets no lines.
--residues RES.tsv adds the interface-residue table (the per-residue table of calc_interfaces, made on the device): one line per
residue of a side that loses more than --min-buried (default 0) A^2 - file, the two groups' labels, the label of the side the
residue is on, its chain, name and number (with insertion code), the atoms of the residue in that group, and its isolated
area, its area in the pair and the difference.  OUT.tsv is the same with and without it.
--contacts ATOMS.tsv (Shrake-Rupley only: with --alg lr it is refused) adds the atom-atom contact table (freesasa_amd.
calc_interface_contacts, made on the device): one line per row - file, the two groups' labels, then chain, residue name, residue
number and atom name of the buried atom and of the partner atom that buries it, the test points and the area in A^2.  The table is
directed: a -> b and b -> a are rows of their own.  --residue-contacts RES.tsv folds these rows per (pair, residue of the buried
atom, residue of the partner) here, with numpy: the points summed, the areas added in row order.
--contact-map MAP.tsv (Shrake-Rupley only, with or without --contacts) writes the residue-residue contact map folded on the device
(calc_interface_contacts with res_first): one line per unordered pair of residues of every interface - file, the two groups'
labels, chain, name and number of group a's residue and of group b's residue, then the contact rows folded, the test points and
the area in A^2 that b's residue buries of a's (a -> b), and the same three for b -> a, zeros where there is no such row.  Per
interface the lines are side a's folded rows in the table's order, each joined to its reverse row, then side b's rows that have
no reverse."""
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


CONTACT_HEADER = "file\tgroup_a\tgroup_b\tchain\tres_name\tres_number\tatom\tpartner_chain\tpartner_res_name\tpartner_res_number\tpartner_atom\tpoints\tarea"
RESIDUE_CONTACT_HEADER = "file\tgroup_a\tgroup_b\tchain\tres_name\tres_number\tpartner_chain\tpartner_res_name\tpartner_res_number\tpoints\tarea"


def contact_row_keys(side_offsets, pair_atom, contact_first, contact_partner):
    """per row of the contact table: (its pair p, the input atom of i, the input atom of j) as three int64 arrays"""
    import numpy as np
    rows_of = np.diff(np.asarray(contact_first, dtype=np.int64))
    i = np.repeat(np.arange(len(rows_of), dtype=np.int64), rows_of)
    p = (np.searchsorted(np.asarray(side_offsets, dtype=np.int64), i, side="right") - 1) // 2
    pair_atom = np.asarray(pair_atom, dtype=np.int64)
    return p, pair_atom[i], pair_atom[np.asarray(contact_partner, dtype=np.int64)]


def format_contact_rows(files, labels, pair_struct, pair_groups, row_pair, atom_i, atom_j, points, area, atom_res, atom_name, res_chain,
                        res_name, res_number):
    """the atom records, one string per row of the contact table (no line ends), in its order.  atom_res [n]: the residue of every
    input atom; atom_name [n], res_chain, res_name, res_number: the loader's labels."""
    out = []
    tag = lambda r: [str(res_chain[r]).strip() or "_", str(res_name[r]).strip(), str(res_number[r]).strip()]
    for p, i, j, n, a in zip(row_pair, atom_i, atom_j, points, area):
        s, (g, h) = int(pair_struct[p]), pair_groups[p]
        out.append("\t".join([files[s], labels[s][int(g)], labels[s][int(h)]] + tag(int(atom_res[i])) + [str(atom_name[i]).strip()] +
                             tag(int(atom_res[j])) + [str(atom_name[j]).strip(), str(int(n)), "%.3f" % float(a)]))
    return out


def fold_contact_rows(row_pair, res_i, res_j, points, area):
    """the rows folded per (pair, residue of i, residue of j), in order of first appearance: (pair, res_i, res_j, points, area) -
    points summed, areas added in row order"""
    import numpy as np
    key = np.stack([np.asarray(row_pair, np.int64), np.asarray(res_i, np.int64), np.asarray(res_j, np.int64)], axis=1)
    if len(key) == 0:
        return key[:, 0], key[:, 1], key[:, 2], np.zeros(0, np.int64), np.zeros(0)
    uniq, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")              # the folded rows in order of first appearance
    place = np.empty(len(uniq), np.int64); place[order] = np.arange(len(uniq))
    slot = place[np.asarray(inverse).reshape(-1)]
    pts, tot = np.zeros(len(uniq), np.int64), np.zeros(len(uniq))
    np.add.at(pts, slot, np.asarray(points, np.int64))
    np.add.at(tot, slot, np.asarray(area, np.float64))   # (unbuffered, element by element: row order)
    u = uniq[order]
    return u[:, 0], u[:, 1], u[:, 2], pts, tot


def format_residue_contact_rows(files, labels, pair_struct, pair_groups, fold, res_chain, res_name, res_number):
    out = []
    tag = lambda r: [str(res_chain[r]).strip() or "_", str(res_name[r]).strip(), str(res_number[r]).strip()]
    for p, ri, rj, n, a in zip(*fold):
        s, (g, h) = int(pair_struct[p]), pair_groups[p]
        out.append("\t".join([files[s], labels[s][int(g)], labels[s][int(h)]] + tag(int(ri)) + tag(int(rj)) + [str(int(n)), "%.3f" % float(a)]))
    return out


CONTACT_MAP_HEADER = ("file\tgroup_a\tgroup_b\tchain_a\tres_name_a\tres_number_a\tchain_b\tres_name_b\tres_number_b\t"
                      "rows_ab\tpoints_ab\tarea_ab\trows_ba\tpoints_ba\tarea_ba")


def format_contact_map_rows(files, labels, pair_struct, pair_groups, offsets, residues, counts, area, reverse, res_chain, res_name, res_number):
    """the contact map's records, one string per unordered residue pair (no line ends): per pair of groups side a's folded rows
    in their order, each with its reverse row, then side b's rows whose reverse is -1.  The five rescontact arrays of
    calc_interface_contacts(res_first=...) are taken as they are."""
    out = []
    tag = lambda r: [str(res_chain[r]).strip() or "_", str(res_name[r]).strip(), str(res_number[r]).strip()]
    three = lambda k: ["0", "0", "%.3f" % 0.0] if k < 0 else [str(int(counts[k][0])), str(int(counts[k][1])), "%.3f" % float(area[k])]
    for p, (s, (g, h)) in enumerate(zip(pair_struct, pair_groups)):
        head = [files[int(s)], labels[int(s)][int(g)], labels[int(s)][int(h)]]
        for k in range(int(offsets[2 * p]), int(offsets[2 * p + 1])):
            out.append("\t".join(head + tag(int(residues[k][0])) + tag(int(residues[k][1])) + three(k) + three(int(reverse[k]))))
        for k in range(int(offsets[2 * p + 1]), int(offsets[2 * p + 2])):
            if int(reverse[k]) < 0:
                out.append("\t".join(head + tag(int(residues[k][1])) + tag(int(residues[k][0])) + three(-1) + three(k)))
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
    ap.add_argument("--contacts", default=None, metavar="ATOMS.tsv")
    ap.add_argument("--residue-contacts", default=None, metavar="RES.tsv")
    ap.add_argument("--contact-map", default=None, metavar="MAP.tsv")
    args = ap.parse_args(argv)
    if args.chain_groups and args.separate_chains:
        sys.exit("--chain-groups and --separate-chains exclude each other")
    if args.residue_contacts and not args.contacts:
        sys.exit("--residue-contacts needs --contacts")
    if args.contacts and args.alg != "sr":
        sys.exit("--contacts is made of Shrake-Rupley test points: give --alg sr (Lee-Richards has no contact table)")
    if args.contact_map and args.alg != "sr":
        sys.exit("--contact-map is made of Shrake-Rupley test points: give --alg sr (Lee-Richards has no contact table)")
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
    if args.contacts or args.contact_map:
        ct = fa.calc_interface_contacts(batch.xyz, batch.radii, batch.offsets, group, n_groups, probe=args.probe, n_points=res,
                                        res_first=batch.res_first if args.contact_map else None)
        files = [os.path.basename(p) for p in args.structures]
    if args.contact_map:
        with open(args.contact_map, "w") as f:
            f.write(CONTACT_MAP_HEADER + "\n")
            lines = format_contact_map_rows(files, labels, ct.pair_struct, ct.pair_groups, ct.rescontact_offsets, ct.rescontact_residues,
                                            ct.rescontact_counts, ct.rescontact_area, ct.rescontact_reverse, batch.res_chain, batch.res_name,
                                            batch.res_number)
            for line in lines:
                f.write(line + "\n")
        print(f"{len(lines)} residue pairs in contact -> {args.contact_map}")
    if args.contacts:
        import numpy as np
        atom_res = np.repeat(np.arange(batch.n_residues, dtype=np.int64), np.diff(batch.res_first))
        atom_name = [v.decode() for v in batch.atom_name_raw.tolist()]
        row_pair, atom_i, atom_j = contact_row_keys(ct.side_offsets, ct.pair_atom, ct.contact_first, ct.contact_partner)
        with open(args.contacts, "w") as f:
            f.write(CONTACT_HEADER + "\n")
            for line in format_contact_rows(files, labels, ct.pair_struct, ct.pair_groups, row_pair, atom_i, atom_j, ct.contact_points,
                                            ct.contact_area, atom_res, atom_name, batch.res_chain, batch.res_name, batch.res_number):
                f.write(line + "\n")
        print(f"{ct.n_contacts} atom contacts -> {args.contacts}")
        if args.residue_contacts:
            fold = fold_contact_rows(row_pair, atom_res[atom_i], atom_res[atom_j], ct.contact_points, ct.contact_area)
            with open(args.residue_contacts, "w") as f:
                f.write(RESIDUE_CONTACT_HEADER + "\n")
                for line in format_residue_contact_rows(files, labels, ct.pair_struct, ct.pair_groups, fold, batch.res_chain, batch.res_name,
                                                        batch.res_number):
                    f.write(line + "\n")
            print(f"{len(fold[0])} residue contacts -> {args.residue_contacts}")


if __name__ == "__main__":
    main()
