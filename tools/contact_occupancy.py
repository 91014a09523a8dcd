#!/usr/bin/env python3
"""tools/contact_occupancy.py TOPOLOGY FRAMES... -o OUT.tsv [--chain-groups SPEC | --separate-chains] [--points N] [--probe P]
                              [--block-frames N]

The residue contact map of a run: in what fraction of the frames residue a of one chain group touches residue b of another, and
over how much area when it does (freesasa_amd.ContactOccupancy; include/freesasa_gpu.h has the definitions).  TOPOLOGY is a PDB
or mmCIF file of the solute (its first structure), loaded as tools/interface_occupancy.py loads it; FRAMES are raw frames of
exactly its atoms - .f32 / .f64 (x, y, z per atom, frame by frame) or .npy ([f, n, 3]) - taken one behind the other as one run
and read in blocks of --block-frames frames through a memory map.  Other containers (DCD, NetCDF, XTC, TRR) are for the caller's
own reader, which feeds ContactOccupancy.add: the device decoders have no memory form.  --chain-groups takes the reference's
syntax ("AB+CD": two groups), --separate-chains (the default) makes every chain a group; all pairs of groups in contact are
tabulated.  Shrake-Rupley with --points test points (up to 128).

OUT.tsv has one line per unordered pair of residues in contact, residue a in the lower group: both groups' labels; both residues
(chain, name, number); occupancy_either, the fraction of the frames in which either buries test points of the other; then for a
-> b (b buries points of a) and for b -> a the occupancy, the mean number of buried points and the mean area (A^2) over the
frames in which that direction is present.  The per-frame tables never leave the device."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADER = ("group_a\tgroup_b\tchain_a\tres_name_a\tres_number_a\tchain_b\tres_name_b\tres_number_b\toccupancy_either\t"
          "occupancy_ab\tmean_points_ab\tmean_area_ab\toccupancy_ba\tmean_points_ba\tmean_area_ba")


def format_rows(labels, n_frames, keys, frames, frames_either, counts, area, reverse, res_chain, res_name, res_number):
    """the records, one string per unordered residue pair (no line ends): pair by pair of groups, residue a (in group g) ascending,
    then residue b (in group h).  labels [G]: the label of every group; the arrays are a ContactOccupancyTable's."""
    n_frames = float(max(int(n_frames), 1))
    res = lambda r: [str(res_chain[r]).strip() or "_", str(res_name[r]).strip(), str(res_number[r]).strip()]

    def direction(k):
        if k < 0:
            return ["0.0000", "0.00", "0.000"]
        f = float(frames[k])
        return ["%.4f" % (f / n_frames), "%.2f" % (float(counts[k][1]) / f), "%.3f" % (float(area[k][0]) / f)]

    pairs = {}
    for k in range(len(frames)):
        g, h, side, a, b = (int(v) for v in keys[k])
        where = (g, h, a, b) if side == 0 else (g, h, b, a)
        pairs.setdefault(where, [-1, -1])[side] = k
    out = []
    for (g, h, a, b), (ab, ba) in sorted(pairs.items()):
        k = ab if ab >= 0 else ba
        assert ab < 0 or ba < 0 or (int(reverse[ab]) == ba and int(reverse[ba]) == ab)
        out.append("\t".join([labels[g], labels[h]] + res(a) + res(b) + ["%.4f" % (float(frames_either[k]) / n_frames)] + direction(ab) + direction(ba)))
    return out


def frame_blocks(path, n_atoms, block_frames):
    """the frames of a raw file, [f, n_atoms, 3] fp64 blocks of up to block_frames frames, read through a memory map"""
    import numpy as np
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path, mmap_mode="r")
        if a.ndim != 3 or a.shape[1:] != (n_atoms, 3):
            sys.exit(f"{path}: an array of shape {a.shape}, the topology wants [f, {n_atoms}, 3]")
    else:
        a = np.memmap(path, dtype=np.float32 if ext == ".f32" else np.float64, mode="r")
        if a.size % (3 * n_atoms):
            sys.exit(f"{path}: {a.size} numbers are no whole number of frames of {n_atoms} atoms")
        a = a.reshape(-1, n_atoms, 3)
    for f0 in range(0, a.shape[0], block_frames):
        yield np.ascontiguousarray(a[f0:f0 + block_frames], dtype=np.float64)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    ap.add_argument("topology")
    ap.add_argument("frames", nargs="+")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--chain-groups", default=None)
    ap.add_argument("--separate-chains", action="store_true")
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--probe", type=float, default=1.4)
    ap.add_argument("--block-frames", type=int, default=256)
    args = ap.parse_args(argv)
    if args.chain_groups and args.separate_chains:
        sys.exit("--chain-groups and --separate-chains exclude each other")
    if args.block_frames < 1:
        sys.exit("--block-frames must be at least 1")
    for path in args.frames:
        if os.path.splitext(path)[1].lower() not in (".f32", ".f64", ".npy"):
            sys.exit(f"{path}: raw frames (.f32, .f64) or .npy only - read other containers with a reader of your own and feed ContactOccupancy.add")
    import numpy as np
    import freesasa_amd as fa
    from freesasa_amd import ingest
    from tools.interfaces import group_labels
    batch = ingest.load_files([args.topology])
    ids, n_groups, status = batch.chain_groups(args.chain_groups, separate_chains=args.chain_groups is None)
    if batch.n_structs < 1 or batch.status[0] != 0 or status[0] != 0:
        sys.exit(f"{args.topology}: not loaded or without a requested chain")
    n, n_res = int(batch.offsets[1]), int(batch.res_offsets[1])
    ids, G = ids[:n], int(n_groups[0])
    with fa.ContactOccupancy(batch.radii[:n], ids, G, batch.res_first[:n_res + 1], probe=args.probe, n_points=args.points) as acc:
        for path in args.frames:
            for block in frame_blocks(path, n, args.block_frames):
                acc.add(block)
        t = acc.table()
    labels, _ = group_labels(batch, np.concatenate([ids, np.full(batch.n_atoms - n, -1, np.int32)]), n_groups)
    lines = format_rows(labels[0], t.n_frames, t.keys, t.frames, t.frames_either, t.counts, t.area, t.reverse, batch.res_chain, batch.res_name,
                        batch.res_number)
    with open(args.output, "w") as f:
        f.write(HEADER + "\n")
        for line in lines:
            f.write(line + "\n")
    print(f"{len(lines)} residue pairs ({t.n_rows} directed rows) over {t.n_frames} frames -> {args.output}")


if __name__ == "__main__":
    main()
