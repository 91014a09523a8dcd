#!/usr/bin/env python3
"""Whole-directory sweep: PDB files -> batched ingestion on host threads -> SASA on the GPU ->
per-structure totals (BASELINE configs[3] in miniature; SURVEY §8f N1 + the batch entry point).

    python tools/sweep.py [--replicate N] [--threads T] [--batch-atoms A] [--devices 0,1,...] [--done FILE] [--cache FILE]
                          [--residues OUT.tsv] [--select CMD ... --select-out OUT.tsv]
                          [--chain-groups SPEC | --separate-chains, --groups-out OUT.tsv]
                          [--chain-groups SPEC | --separate-chains, --interfaces-out OUT.tsv [--interface-residues RES.tsv] [--min-buried X]]
                          [paths ...]

Without paths it sweeps the PDB fixtures under tests/golden/pdb, replicated N times.  Loading of
batch k+1 runs on host threads while the GPU computes batch k.  Prints one JSON line with the
end-to-end rate, the loader-only rate and (if oracle/_ref is present) the reference reader's
single-thread rate on the same files.  --devices: the GPUs that share the batches (freesasa_gpu_sweep_files_devices;
default: every visible device; entries may repeat); --done: a done-list, so that an interrupted sweep resumes — on any
device list; --cache FILE: sweep the binary cache FILE instead (written first from the files if it does not exist);
--residues OUT.tsv: the per-residue table of all files (freesasa_gpu_sweep_files_residues): file, chain, number, name, the
five absolute areas (total, main chain, side chain, polar, apolar) and the five relative ones, N/A where there is none;
--select CMD (repeatable, up to 64) with --select-out OUT.tsv: the reference's --select for all files
(freesasa_gpu_sweep_files_select): file, then one area column per selection name;
--chain-groups SPEC ("AB+C") or --separate-chains with --groups-out OUT.tsv: the reference's chain groups for all files
(freesasa_gpu_sweep_files_groups): file, group index, label, atoms, isolated, complex and buried area per line;
--interfaces-out OUT.tsv (with --chain-groups or --separate-chains; --groups-out may ride along): the interfaces between the
groups of all files (freesasa_gpu_sweep_files_interfaces): the lines of tools/interfaces.py -o for the same files, column for
column (a group's label is the group table's: with a spec, the first chain it names for the group), then per side the buried
area split as apolar, polar, unknown; --interface-residues RES.tsv: the lines of tools/interfaces.py --residues, a row per
residue of a side that loses more than --min-buried (default 0) A^2."""
import argparse
import glob
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_residues(path, paths, table):
    """one line per residue; NaN (no reference areas for the residue) is written N/A, as the reference's RSA files do"""
    name, number, chain = table.res_name, table.res_number, table.res_chain
    with open(path, "w") as fh:
        fh.write("file\tchain\tnumber\tname\tabs_total\tabs_main\tabs_side\tabs_polar\tabs_apolar\trel_total\trel_main\trel_side\trel_polar\trel_apolar\n")
        for k, p in enumerate(paths):
            for r in range(int(table.res_offsets[k]), int(table.res_offsets[k + 1])):
                cols = [p, chain[r], number[r].strip(), name[r].strip()] + [f"{v:.2f}" for v in table.abs[r, :5]] + \
                       ["N/A" if np.isnan(v) else f"{v:.1f}" for v in table.rel[r]]
                fh.write("\t".join(cols) + "\n")


def write_selections(path, paths, names, areas):
    """one line per file: its path, then the area of every selection"""
    with open(path, "w") as fh:
        fh.write("\t".join(["file"] + list(names)) + "\n")
        for k, p in enumerate(paths):
            fh.write("\t".join([p] + [f"{v:.2f}" for v in areas[k]]) + "\n")


def write_groups(path, paths, table):
    """one line per group: its file, its index in the file, label, atoms, isolated, complex and buried area"""
    chain = table.chain
    with open(path, "w") as fh:
        fh.write("file\tgroup\tlabel\tatoms\tisolated\tcomplex\tburied\n")
        for k, p in enumerate(paths):
            s = table.file(k)
            for g in range(s.start, s.stop):
                fh.write("\t".join([p, str(g - s.start), chain[g], str(int(table.group_atoms[g]))] + [f"{v:.2f}" for v in table.areas[g]]) + "\n")


def write_interfaces(path, res_path, paths, gtable, table):
    """tools/interfaces.py's lines from the sweep's tables: per pair the file, the two groups' labels and atoms and the six areas,
    then buried apolar / polar / unknown of side a and of side b; per residue row that tool's --residues line"""
    import interfaces as fmt
    files = [os.path.basename(p) for p in paths]
    chain = [c.strip() or "_" for c in gtable.chain]
    labels = [chain[gtable.file(k)] for k in range(len(paths))]
    atoms = [gtable.group_atoms[gtable.file(k)] for k in range(len(paths))]
    pair_struct = np.repeat(np.arange(len(paths)), np.diff(table.pair_offsets))
    with open(path, "w") as fh:
        fh.write(fmt.HEADER + "\tburied_apolar_a\tburied_polar_a\tburied_unknown_a\tburied_apolar_b\tburied_polar_b\tburied_unknown_b\n")
        for line, cls in zip(fmt.format_rows(files, labels, atoms, pair_struct, table.pair_groups, table.pair_areas), table.pair_class_buried):
            fh.write(line + "\t" + "\t".join("%.3f" % float(v) for v in cls.reshape(-1)) + "\n")
    if res_path:
        rows = np.arange(table.n_res_rows)      # (the rows carry their own labels: the formatter's residue r is row r)
        with open(res_path, "w") as fh:
            fh.write(fmt.RESIDUE_HEADER + "\n")
            for line in fmt.format_residue_rows(files, labels, pair_struct, table.pair_groups, table.res_offsets, rows, table.res_atoms, table.res_areas,
                                                table.res_chain, table.res_name, table.res_number):
                fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--replicate", type=int, default=200)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--batch-atoms", type=int, default=0, help="atoms per batch (0: the driver's default: 5e5 with the parser on the device, 1e6 with the host parser)")
    ap.add_argument("--host-parser", action="store_true", help="parse the files with the host loader (default: ON THE DEVICE, csrc/gpu_parse.hip; files it refuses go to the host parser anyway)")
    ap.add_argument("--slices", type=int, default=20)
    ap.add_argument("--no-gpu", action="store_true", help="time the loader only")
    ap.add_argument("--devices", default="", help="comma-separated device list (default: all visible devices)")
    ap.add_argument("--done", default=None, help="done-list file: resume an interrupted sweep")
    ap.add_argument("--cache", default=None, help="binary cache file to sweep (created from the files when missing)")
    ap.add_argument("--residues", default=None, metavar="OUT.tsv", help="write the per-residue table of all files (not with --done or --cache)")
    ap.add_argument("--select", action="append", default=[], metavar="CMD", help='a selection in the reference\'s language ("name, resn ala+arg and not chain B"); repeatable, up to 64')
    ap.add_argument("--select-out", default=None, metavar="OUT.tsv", help="write the selections' areas of all files (not with --done, --cache or --no-gpu)")
    ap.add_argument("--chain-groups", default=None, metavar="SPEC", help='the reference\'s --chain-groups for every file ("AB+C": chains A and B as one group, C as another)')
    ap.add_argument("--separate-chains", action="store_true", help="the reference's --separate-chains for every file: one group per chain")
    ap.add_argument("--groups-out", default=None, metavar="OUT.tsv", help="write the groups' areas of all files (not with --select, --residues, --done, --cache or --no-gpu)")
    ap.add_argument("--interfaces-out", default=None, metavar="OUT.tsv", help="write the interfaces between the groups of all files (with --chain-groups or --separate-chains)")
    ap.add_argument("--interface-residues", default=None, metavar="RES.tsv", help="... and their per-residue rows (with --interfaces-out)")
    ap.add_argument("--min-buried", type=float, default=0.0, help="a residue row for a buried area above this (A^2)")
    ap.add_argument("--engine", choices=["python", "c"], default="c",
                    help="c: freesasa_gpu_sweep_files (loader thread || GPU inside the library); "
                         "python: the same pipeline written with the two-step Python API")
    args = ap.parse_args()
    if args.residues and (args.done or args.cache or args.no_gpu or args.engine != "c"):
        ap.error("--residues goes with the C engine's plain file sweep only (no --done, --cache, --no-gpu, --engine python)")
    if bool(args.select) != bool(args.select_out):
        ap.error("--select and --select-out go together")
    if args.select and (args.done or args.cache or args.no_gpu or args.residues or args.engine != "c"):
        ap.error("--select goes with the C engine's plain file sweep only (no --done, --cache, --no-gpu, --residues, --engine python)")
    want_groups = args.chain_groups is not None or args.separate_chains
    if args.chain_groups is not None and args.separate_chains:
        ap.error("--chain-groups and --separate-chains can't be combined")
    if want_groups != bool(args.groups_out or args.interfaces_out):
        ap.error("--chain-groups / --separate-chains and --groups-out / --interfaces-out go together")
    if args.interface_residues and not args.interfaces_out:
        ap.error("--interface-residues needs --interfaces-out")
    if want_groups and (args.select or args.done or args.cache or args.no_gpu or args.residues or args.engine != "c"):
        ap.error("chain groups go with the C engine's plain file sweep only (no --select, --residues, --done, --cache, --no-gpu, --engine python)")
    import freesasa_amd as fa
    from freesasa_amd import ingest
    selection = None
    if args.select:
        try:
            selection = ingest.Selection(args.select)
        except ValueError as e:
            ap.error(str(e))

    paths = args.paths or [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pdb", "*.pdb")))
                           if os.path.getsize(p) > 10_000]
    paths = paths * args.replicate
    sizes = np.array([os.path.getsize(p) for p in paths])
    # batches of roughly equal atom count (~81 bytes per ATOM line)
    per_batch = max(1, int(args.batch_atoms * 81 / max(1.0, sizes.mean())))
    chunks = [paths[i:i + per_batch] for i in range(0, len(paths), per_batch)]

    t0 = time.perf_counter()
    probe = ingest.load_pdb_files(chunks[0], n_threads=args.threads)
    t_load1 = time.perf_counter() - t0
    out = {"files": len(paths), "batches": len(chunks), "threads": args.threads or os.cpu_count(),
           "loader_atoms_per_s": probe.n_atoms / t_load1, "loader_MB_per_s": sum(os.path.getsize(p) for p in chunks[0]) / t_load1 / 1e6}

    devices = [int(d) for d in args.devices.split(",") if d != ""] or list(range(max(1, fa.device_count())))
    out["devices"] = devices
    if not args.no_gpu and args.cache:
        if not os.path.exists(args.cache):
            t0 = time.perf_counter()
            ingest.load_pdb_files(paths, n_threads=args.threads).save(args.cache)
            out["cache_build_seconds"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        totals, _, atoms, status = fa.sweep_cache(args.cache, fa.LEE_RICHARDS, resolution=args.slices, batch_atoms=args.batch_atoms, devices=devices)
        dt = time.perf_counter() - t0
        ok = status == 0
        out.update({"engine": "freesasa_gpu_sweep_cache_devices", "atoms": int(atoms.sum()), "structures": int(ok.sum()),
                    "failed_inputs": int((~ok).sum()), "seconds": dt, "end_to_end_atoms_per_s": float(atoms.sum()) / dt,
                    "structures_per_s": float(ok.sum()) / dt, "mean_total_A2": float(totals[ok].mean())})
    elif not args.no_gpu and args.engine == "c":
        popt = 0 if args.host_parser else ingest.PARSE_ON_DEVICE
        fa.sweep_files(chunks[0][:20], fa.LEE_RICHARDS, resolution=args.slices, ingest_options=popt)                      # warm-up
        fa.sweep_parse_stats()
        t0 = time.perf_counter()
        if args.done:
            complete, totals, _, atoms, status = fa.sweep_files_resumable(paths, args.done, fa.LEE_RICHARDS, resolution=args.slices, n_threads=args.threads,
                                                                         batch_atoms=args.batch_atoms, devices=devices, ingest_options=popt)
            out["complete"] = bool(complete)
        elif args.residues:
            totals, _, atoms, status, table = fa.sweep_files_residues(paths, fa.LEE_RICHARDS, resolution=args.slices, n_threads=args.threads,
                                                                      batch_atoms=args.batch_atoms, devices=devices, ingest_options=popt)
            write_residues(args.residues, paths, table)
            out["residues"] = int(table.n_residues)
        elif selection is not None:
            totals, _, atoms, status, areas, counts = fa.sweep_files_select(paths, selection, fa.LEE_RICHARDS, resolution=args.slices, n_threads=args.threads,
                                                                            batch_atoms=args.batch_atoms, devices=devices, ingest_options=popt)
            write_selections(args.select_out, paths, selection.names, areas)
            out["selections"] = len(selection)
            out["selected_atoms"] = int(counts.sum())
        elif args.interfaces_out:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            totals, _, atoms, status, gstatus, istatus, gtable, itable = fa.sweep_files_interfaces(
                paths, args.chain_groups, separate_chains=args.separate_chains, alg=fa.LEE_RICHARDS, resolution=args.slices, n_threads=args.threads,
                batch_atoms=args.batch_atoms, devices=devices, ingest_options=popt, residues=bool(args.interface_residues), min_buried=args.min_buried)
            if args.groups_out:
                write_groups(args.groups_out, paths, gtable)
            write_interfaces(args.interfaces_out, args.interface_residues, paths, gtable, itable)
            out["groups"] = int(gtable.n_groups)
            out["interfaces"] = int(itable.n_pairs)
            out["interface_residues"] = int(itable.n_res_rows)
            out["files_without_interface_rows"] = int(((istatus != 0) & (status == 0)).sum())
        elif want_groups:
            totals, _, atoms, status, gstatus, gtable = fa.sweep_files_groups(paths, args.chain_groups, separate_chains=args.separate_chains, alg=fa.LEE_RICHARDS,
                                                                              resolution=args.slices, n_threads=args.threads, batch_atoms=args.batch_atoms,
                                                                              devices=devices, ingest_options=popt)
            write_groups(args.groups_out, paths, gtable)
            out["groups"] = int(gtable.n_groups)
            out["files_without_their_groups"] = int(((gstatus != 0) & (status == 0)).sum())
        else:
            totals, _, atoms, status = fa.sweep_files(paths, fa.LEE_RICHARDS, resolution=args.slices, n_threads=args.threads,
                                                      batch_atoms=args.batch_atoms, class_sums=True, devices=devices, ingest_options=popt)
        dt = time.perf_counter() - t0
        ok = status == 0
        on_dev, on_host = fa.sweep_parse_stats()
        out.update({"engine": "freesasa_gpu_sweep_files_devices", "parser": "host" if args.host_parser else "device",
                    "files_parsed_on_device": on_dev, "files_left_to_the_host_parser": on_host, "atoms": int(atoms.sum()), "structures": int(ok.sum()),
                    "failed_inputs": int((~ok).sum()), "seconds": dt, "end_to_end_atoms_per_s": float(atoms.sum()) / dt,
                    "structures_per_s": float(ok.sum()) / dt, "mean_total_A2": float(totals[ok].mean())})
    elif not args.no_gpu:
        totals, n_atoms, n_bad = [], 0, 0
        fa.calc_batch(probe.xyz[:3000], probe.radii[:3000], [0, 3000], fa.LEE_RICHARDS, resolution=args.slices)  # warm-up
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=1) as pool:              # the C loader brings its own threads
            fut = pool.submit(ingest.load_pdb_files, chunks[0], 0, args.threads)
            for k in range(len(chunks)):
                b = fut.result()
                if k + 1 < len(chunks):
                    fut = pool.submit(ingest.load_pdb_files, chunks[k + 1], 0, args.threads)
                ok = b.status == 0
                n_bad += int((~ok).sum())
                # empty structures are legal batch members only for the loader; drop them here
                keep = np.nonzero(ok)[0]
                offs = np.concatenate([[0], np.cumsum(np.diff(b.offsets)[keep])]).astype(np.int64)
                _, _, tot = fa.calc_batch(b.xyz, b.radii, offs, fa.LEE_RICHARDS, resolution=args.slices)
                totals.append(tot)
                n_atoms += b.n_atoms
        dt = time.perf_counter() - t0
        totals = np.concatenate(totals)
        out.update({"atoms": n_atoms, "structures": int(len(totals)), "failed_inputs": n_bad, "seconds": dt,
                    "end_to_end_atoms_per_s": n_atoms / dt, "structures_per_s": len(totals) / dt,
                    "mean_total_A2": float(totals.mean())})

    try:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import make_ingest_golden as mg                                # needs oracle/_ref (build container)
        sample = paths[:min(len(paths), 40)]
        t0 = time.perf_counter()
        n = sum(mg.reference_view_unsafe(p, 0).get("n_atoms", 0) for p in sample)
        out["reference_reader_atoms_per_s_1thread"] = n / (time.perf_counter() - t0)
    except Exception as e:                                             # noqa: BLE001 - optional comparison
        out["reference_reader"] = f"not available here ({type(e).__name__})"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
