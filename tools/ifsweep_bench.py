#!/usr/bin/env python3
"""tools/ifsweep_bench.py [--replicate N] [--repeats K] [--out FILE.md]

What the interfaces cost in the file sweep, and what the sweep form gains over the long way it replaces.  Workload: the PDB
fixtures tools/sweep.py --replicate sweeps, separate chains, parser on the device, one device; Lee-Richards 20 slices and
Shrake-Rupley 100 points.  Three forms, alternated, K times each after a warm-up of every form, host clock around calls that
return after their last device synchronize; medians and the spread (min .. max) are printed:

  interfaces   freesasa_amd.sweep_files_interfaces(residues=True)
  groups       freesasa_amd.sweep_files_groups on the same files: the difference is the added cost
  long way     ingest.load_files + chain_groups + calc_interfaces(res_first=...), as tools/interfaces.py --residues runs it

The outputs of the first and the third form are compared (pairs, rows and every area, bit for bit) before anything is timed.
--trace-only: one sweep_files_interfaces call per algorithm and nothing else - the program a kernel trace is taken of."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def long_way(fa, ingest, paths, alg, res):
    b = ingest.load_files(paths)
    g, n, st = b.chain_groups(None, separate_chains=True)
    return b, fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg=alg, resolution=res, res_first=b.res_first, device=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicate", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import freesasa_amd as fa
    from freesasa_amd import ingest
    if fa.device_count() <= 0:
        sys.exit("no GPU: nothing is measured without one")
    base = [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pdb", "*.pdb"))) if os.path.getsize(p) > 10_000]
    paths = base * args.replicate
    kw = dict(separate_chains=True, ingest_options=ingest.PARSE_ON_DEVICE, devices=[0])
    lines = []
    for name, alg, res in (("L&R-20", fa.LEE_RICHARDS, 20), ("S&R-100", fa.SHRAKE_RUPLEY, 100)):
        forms = {
            "interfaces": lambda: fa.sweep_files_interfaces(paths, alg=alg, resolution=res, residues=True, **kw),
            "groups": lambda: fa.sweep_files_groups(paths, alg=alg, resolution=res, **kw),
            "long way": lambda: long_way(fa, ingest, paths, alg, res),
        }
        if args.trace_only:
            forms["interfaces"]()
            forms["interfaces"]()
            continue
        got = {k: f() for k, f in forms.items()}                   # warm-up of every form, and the outputs that are compared
        t, (b, lw) = got["interfaces"][7], got["long way"]
        same = (t.n_pairs == lw.n_pairs and t.n_res_rows == lw.n_res_rows and t.pair_areas.tobytes() == lw.pair_areas.tobytes() and
                t.res_areas.tobytes() == lw.res_areas.tobytes() and np.array_equal(t.pair_groups, lw.pair_groups))
        if not same:
            sys.exit(name + ": the sweep and the long way differ")
        atoms = int(got["interfaces"][2].sum())
        times = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, f in forms.items():                             # alternated: what else runs on the host hits every form alike
                t0 = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        row = dict(workload=name, files=len(paths), atoms=atoms, pairs=int(t.n_pairs), residue_rows=int(t.n_res_rows),
                   seconds={k: dict(median=med[k], min=min(v), max=max(v)) for k, v in times.items()},
                   long_way_over_interfaces=med["long way"] / med["interfaces"], added_over_groups_s=med["interfaces"] - med["groups"],
                   interfaces_over_groups=med["interfaces"] / med["groups"], interfaces_atoms_per_s=atoms / med["interfaces"])
        print(json.dumps(row))
        lines.append(row)
    if args.out and lines:
        with open(args.out, "w") as fh:
            fh.write("| workload | files | atoms | pairs | residue rows | interfaces s (min .. max) | groups s (min .. max) | long way s (min .. max) | long way / interfaces | interfaces - groups s | interfaces / groups |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in lines:
                s = r["seconds"]
                cell = lambda k: "%.4f (%.4f .. %.4f)" % (s[k]["median"], s[k]["min"], s[k]["max"])
                fh.write("| %s | %d | %d | %d | %d | %s | %s | %s | %.2f | %.4f | %.2f |\n" % (
                    r["workload"], r["files"], r["atoms"], r["pairs"], r["residue_rows"], cell("interfaces"), cell("groups"), cell("long way"),
                    r["long_way_over_interfaces"], r["added_over_groups_s"], r["interfaces_over_groups"]))


if __name__ == "__main__":
    main()
