#!/usr/bin/env python3
"""tools/interface_occupancy.py TOPOLOGY FRAMES... -o OUT.tsv [--chain-groups SPEC | --separate-chains] [--pairs all|A:B,...]
                                [--min-buried X] [--alg lr|sr] [--resolution N] [--probe P] [--frames-per-batch N] [--devices 0,1]
                                [--pbc [--triclinic]]

Which residues make up the interfaces between the chain groups of a system over a trajectory, how much each buries on average
and in what fraction of the frames it is in the interface at all (freesasa_amd.trajectory_file_topology with interface_pairs and
the statistics "pair_residues").  TOPOLOGY is a PDB or mmCIF file of the solute (its first structure); FRAMES are trajectory files
of it, taken one behind the other as one run: .dcd, .nc, .xtc, .trr, or raw frames (.f32 / .f64: x, y, z per atom, frame by
frame).  A file whose frames hold more atoms than the topology has the topology's atoms first.  --chain-groups takes the
reference's syntax ("AB+CD": two groups), --separate-chains (the default) makes every chain a group; --pairs names the pairs of
groups by number ("0:1,0:2"), default every pair.

OUT.tsv has one line per SEGMENT - the atoms of one side of a pair that lie in one residue: the two groups' chain labels and
the label of the side the residue is on; its chain, name and number; its atoms in that group; mean, standard deviation, minimum
and maximum over the frames of the area it buries in the pair (A^2); its mean isolated area; and its occupancy, the fraction of
the frames in which it buries more than --min-buried (default 0; with Lee-Richards give a threshold above rounding noise, e.g.
1).  It is made from the run statistics alone: the per-frame tables never leave the device.

--pbc: every frame, every group and every pair structure among the periodic images of the frame's own cell
(freesasa_amd.trajectory_file_groups_periodic with interface_pairs): for a wrapped trajectory, whose partners may lie in different
images of the box.  FRAMES must then be containers that carry a cell (.dcd with unit-cell records, .nc, .xtc, .trr); --triclinic
reads the cell as a triclinic one."""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADER = "group_a\tgroup_b\tside\tchain\tres_name\tres_number\tatoms\tburied_mean\tburied_std\tburied_min\tburied_max\tiso_mean\toccupancy"
FORMATS = {".dcd": "dcd", ".nc": "netcdf", ".ncdf": "netcdf", ".xtc": "xtc", ".trr": "trr", ".f32": "f32", ".f64": "f64"}


def format_rows(labels, pairs, seg_offsets, seg_res, seg_atoms, res_chain, res_name, res_number, stats):
    """the records, one string per segment (no line ends), in the table's order: pair by pair, side a before side b.  labels
    [G]: the label of every group; stats [4, S, 4]: mean, std, min, max of (iso_res, in_pair_res, buried_res, in_interface)."""
    out = []
    for k, (g, h) in enumerate(pairs):
        g, h = int(g), int(h)
        for side, x in ((0, g), (1, h)):
            for s in range(int(seg_offsets[2 * k + side]), int(seg_offsets[2 * k + side + 1])):
                r = int(seg_res[s])
                out.append("\t".join([labels[g], labels[h], labels[x], str(res_chain[r]).strip() or "_", str(res_name[r]).strip(),
                                      str(res_number[r]).strip(), str(int(seg_atoms[s]))] +
                                     ["%.3f" % float(stats[q, s, 2]) for q in range(4)] + ["%.3f" % float(stats[0, s, 0]), "%.4f" % float(stats[0, s, 3])]))
    return out


def parse_pairs(text, n_groups):
    if text == "all":
        return "all"
    try:
        return [tuple(int(v) for v in item.split(":")) for item in text.split(",")]
    except ValueError:
        sys.exit('--pairs is "all" or a list like 0:1,0:2 of group numbers below %d' % n_groups)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    ap.add_argument("topology")
    ap.add_argument("frames", nargs="+")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--chain-groups", default=None)
    ap.add_argument("--separate-chains", action="store_true")
    ap.add_argument("--pairs", default="all")
    ap.add_argument("--min-buried", type=float, default=0.0)
    ap.add_argument("--alg", choices=("lr", "sr"), default="lr")
    ap.add_argument("--resolution", type=int, default=None)
    ap.add_argument("--probe", type=float, default=1.4)
    ap.add_argument("--frames-per-batch", type=int, default=0)
    ap.add_argument("--devices", default="0")
    ap.add_argument("--pbc", action="store_true", help="among the periodic images of every frame's own cell (containers that carry a cell)")
    ap.add_argument("--triclinic", action="store_true", help="with --pbc: the cells read as triclinic cells")
    args = ap.parse_args(argv)
    if args.chain_groups and args.separate_chains:
        sys.exit("--chain-groups and --separate-chains exclude each other")
    if args.triclinic and not args.pbc:
        sys.exit("--triclinic goes with --pbc")
    for path in args.frames:
        if os.path.splitext(path)[1].lower() not in FORMATS:
            sys.exit(f"{path}: unknown trajectory format (one of {', '.join(sorted(FORMATS))})")
        if args.pbc and FORMATS[os.path.splitext(path)[1].lower()] in ("f32", "f64"):
            sys.exit(f"{path}: raw frame files carry no cell: --pbc needs .dcd, .nc, .xtc or .trr")
    import numpy as np
    import freesasa_amd as fa
    from freesasa_amd import ingest
    from tools.interfaces import group_labels
    batch = ingest.load_files([args.topology])
    ids, n_groups, status = batch.chain_groups(args.chain_groups, separate_chains=args.chain_groups is None)
    if batch.n_structs < 1 or batch.status[0] != 0 or status[0] != 0:
        sys.exit(f"{args.topology}: not loaded or without a requested chain")
    n = int(batch.offsets[1])
    ids, G = ids[:n], int(n_groups[0])
    pairs = fa._interface_pairs(parse_pairs(args.pairs, G), ids, G)
    seg_offsets, seg_res, seg_atoms = fa.traj_pair_segments(batch, ids, G, pairs)
    K, S = pairs.shape[0], seg_res.size
    n_iso = int((ids >= 0).sum())
    n_pair = int(sum((ids == g).sum() + (ids == h).sum() for g, h in pairs))
    alg = fa.LEE_RICHARDS if args.alg == "lr" else fa.SHRAKE_RUPLEY
    res = args.resolution or (20 if args.alg == "lr" else 100)
    devices = [int(d) for d in args.devices.split(",")]
    parts, frames = [], []
    with tempfile.TemporaryDirectory(prefix="interface_occupancy_") as tmp:
        for k, path in enumerate(args.frames):
            kind = FORMATS[os.path.splitext(path)[1].lower()]
            kw = {kind: True} if kind in ("dcd", "netcdf", "xtc", "trr") else {"f32": kind == "f32"}
            info = {"dcd": fa.dcd_info, "netcdf": fa.nc_info, "xtc": fa.xtc_info, "trr": fa.trr_info}.get(kind)
            frame_atoms = info(path).n_atoms if info else n
            if frame_atoms < n:
                sys.exit(f"{path}: its frames have {frame_atoms} atoms, the topology {n}")
            # (the shard length is given, so that the frames of every partial are known: the driver's own default)
            fpb = args.frames_per_batch or 1250000 // max(frame_atoms, n + n_iso + n_pair) + 1
            p = lambda name: os.path.join(tmp, "%d.%s" % (k, name))
            if args.pbc:
                kw["triclinic"] = args.triclinic
            run = fa.trajectory_file_groups_periodic if args.pbc else fa.trajectory_file_topology
            done, n_frames, _ = run(path, batch, p("totals"), frame_atoms=frame_atoms,
                                    atom_index=None if frame_atoms == n else np.arange(n, dtype=np.int32),
                                    alg=alg, probe=args.probe, resolution=res, frames_per_batch=fpb, devices=devices,
                                    group=ids, n_groups=G, interface_pairs=pairs, min_buried=args.min_buried,
                                    stats=("pair_residues",), stats_path=p("stats"), partials_path=p("parts"), **kw)
            assert done
            fpb = min(fpb, n_frames)
            parts.append(np.fromfile(p("parts"), dtype=np.float64).reshape(-1, 4, 4 * S))
            frames.append(np.array([min(fpb, n_frames - f0) for f0 in range(0, n_frames, fpb)], dtype=np.int64))
    stats = fa.traj_stats_merge(np.concatenate(parts), np.concatenate(frames)).reshape(4, S, 4)
    labels, _ = group_labels(batch, np.concatenate([ids, np.full(batch.n_atoms - n, -1, np.int32)]), n_groups)
    with open(args.output, "w") as f:
        f.write(HEADER + "\n")
        for line in format_rows(labels[0], pairs, seg_offsets, seg_res, seg_atoms, batch.res_chain, batch.res_name, batch.res_number, stats):
            f.write(line + "\n")
    print(f"{S} segments of {K} pairs over {int(np.concatenate(frames).sum())} frames -> {args.output}")


if __name__ == "__main__":
    main()
