#!/usr/bin/env python3
"""Chain groups of a directory of complexes, two ways:

  a  sweep_files_groups (parser on the device, separate chains, L&R-20): one call
  b  the only route before it: sweep_files for the plain results, then load_files -> chain_groups -> calc_groups for the groups
  c  sweep_files alone on the same files (the plain sweep, to compare with the same measurement on another commit)

The multi-chain fixtures are replicated to about --atoms atoms.  The runs are interleaved (a b c a b c ...), each timed by
wall clock and by the process's CPU time; the median of --repeats is reported, with the spread.  One JSON line per way goes
to stdout and, with --out, is appended to that file.  --only a|b|c runs one way once (for a kernel trace, or to alternate
processes of two libraries: FREESASA_AMD_LIB names the other one, --tag labels its lines)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MULTI = ["1a0q.pdb", "2jo4.pdb", "3gnn.pdb", "5dx9.pdb", "3bzd_trimmed.pdb", "alt_model_twochain.pdb"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=float, default=1e6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default=None, help="a label for the lines (e.g. which library FREESASA_AMD_LIB names)")
    args = ap.parse_args()
    import freesasa_amd as fa
    from freesasa_amd import ingest
    base = [os.path.join(ROOT, "tests", "golden", "pdb", n) for n in MULTI]
    per = int(ingest.load_files(base).n_atoms)
    paths = base * max(1, int(round(args.atoms / per)))
    DEV = ingest.PARSE_ON_DEVICE

    def way_a():
        r = fa.sweep_files_groups(paths, separate_chains=True, ingest_options=DEV, n_threads=args.threads)
        return int(r[2].sum()), int(r[5].n_groups)

    def way_b():
        r = fa.sweep_files(paths, ingest_options=DEV, n_threads=args.threads)
        b = ingest.load_files(paths, n_threads=args.threads)
        g, n, st = b.chain_groups(separate_chains=True)
        out = fa.calc_groups(b.xyz, b.radii, b.offsets, g, n)
        return int(r[2].sum()), int(out[3].shape[0])

    def way_c():
        r = fa.sweep_files(paths, ingest_options=DEV, n_threads=args.threads)
        return int(r[2].sum()), 0

    ways = {"a": ("sweep_files_groups", way_a), "b": ("sweep_files + load_files + chain_groups + calc_groups", way_b), "c": ("sweep_files", way_c)}
    if args.only:
        ways = {args.only: ways[args.only]}
    for _, f in ways.values():      # warm-up: contexts, page-locked staging, the launch hints
        f()
    wall, cpu, res = {k: [] for k in ways}, {k: [] for k in ways}, {}
    for _ in range(1 if args.only else args.repeats):
        for k, (_, f) in ways.items():
            t0, c0 = time.perf_counter(), time.process_time()
            res[k] = f()
            wall[k].append(time.perf_counter() - t0)
            cpu[k].append(time.process_time() - c0)
    for k, (name, _) in ways.items():
        atoms, groups = res[k]
        w, c = np.array(wall[k]), np.array(cpu[k])
        line = {"way": k, "what": name, "files": len(paths), "atoms": atoms, "groups": groups, "repeats": len(w),
                "seconds_median": float(np.median(w)), "seconds_min": float(w.min()), "seconds_max": float(w.max()),
                "atoms_per_s": atoms / float(np.median(w)), "host_cpu_ns_per_atom": 1e9 * float(np.median(c)) / max(atoms, 1)}
        if args.tag:
            line["tag"] = args.tag
        print(json.dumps(line))
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
