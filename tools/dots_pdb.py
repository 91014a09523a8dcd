#!/usr/bin/env python3
"""tools/dots_pdb.py STRUCTURE -o DOTS.pdb [--points N] [--probe P]

The Connolly dots of one structure file as a PDB file of HETATM records - what `gmx sasa -q` gives: one record per exposed
Shrake-Rupley test point, at the point (freesasa_amd.calc_dots; up to 128 points per atom).  Atom and residue name DOT; the
residue-number column holds the owning atom's serial number modulo 10000 - its 1-based place among the atoms the loader kept
(freesasa_amd.ingest.load_files: PDB or mmCIF, the loader's default options; a loaded batch keeps no serial numbers of the file) - and the record's own serial number counts
the dots modulo 100000.  Load the file next to the structure in any viewer to look at the surface or to pick patches of it."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def format_dots(dots, dot_atom):
    """the records, one string per dot (no line ends): dots [D, 3], dot_atom [D] (0-based atoms)"""
    return ["HETATM%5d %-4s %3s %1s%4d    %8.3f%8.3f%8.3f%6.2f%6.2f" % ((k + 1) % 100000, " DOT", "DOT", " ", (int(a) + 1) % 10000,
                                                                    float(p[0]), float(p[1]), float(p[2]), 1.0, 0.0)
            for k, (p, a) in enumerate(zip(dots, dot_atom))]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    ap.add_argument("structure")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--probe", type=float, default=1.4)
    args = ap.parse_args(argv)
    import freesasa_amd as fa
    from freesasa_amd import ingest
    batch = ingest.load_files([args.structure])
    if batch.n_structs != 1 or batch.status[0] != 0 or batch.n_atoms == 0:
        sys.exit(f"{args.structure}: could not be loaded as one structure")
    sasa, counts, totals, dots, dot_offsets, dot_atom, dot_point = fa.calc_dots(batch.xyz, batch.radii, batch.offsets, probe=args.probe,
                                                                              n_points=args.points, with_index=True)
    with open(args.output, "w") as f:
        f.write("REMARK   surface dots of %s: %d atoms, %d dots, %d test points, probe %.3f, SASA %.3f\n"
                % (os.path.basename(args.structure), batch.n_atoms, len(dots), args.points, args.probe, totals[0]))
        for line in format_dots(dots, dot_atom):
            f.write(line + "\n")
        f.write("END\n")
    print(f"{len(dots)} dots of {batch.n_atoms} atoms -> {args.output}")


if __name__ == "__main__":
    main()
