#!/usr/bin/env python3
"""File sweep with and without a user classifier (freesasa_gpu_sweep_files_classified): atoms/s on bench.py's file mix
(the reference's 7 PDB entries + 4 mmCIF fixtures, copied until >= 3e6 atoms, the list taken four times), host parser and
device parser, ProtOr (classifier=None) against the NACCESS radii of tests/golden/classifiers/naccess.config.  The runs
alternate (ProtOr, NACCESS, ProtOr, ...) so that drift shows as spread.  One JSON line per (parser, classifier) on stdout.

    python tools/classifier_sweep_bench.py [--reps 3] [--scratch DIR]

For the kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/classifier_sweep_bench.py --reps 1`:
kp_parse_lines<false> is the ProtOr build, kp_parse_lines<true> the one with an uploaded table."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import freesasa_amd as fa  # noqa: E402
from freesasa_amd import ingest  # noqa: E402

PDB_NAMES = ["1a0q", "3gnn", "5dx9", "2jo4", "3bkr", "1d3z", "1ubq"]   # (bench.py's list)


def file_mix(scratch):
    pdb_dir, cif_dir = os.path.join(ROOT, "tests", "golden", "pdb"), os.path.join(ROOT, "tests", "golden", "cif")
    srcs = [os.path.join(pdb_dir, nm + ".pdb") for nm in PDB_NAMES] + \
        sorted(os.path.join(cif_dir, f) for f in os.listdir(cif_dir) if f.endswith(".cif"))[:4]
    one = ingest.load_pdb_files(srcs)
    reps = max(1, -(-3_000_000 // int(one.n_atoms)))
    paths = []
    for k in range(reps):
        for sp in srcs:
            dst = os.path.join(scratch, f"{k:04d}_{os.path.basename(sp)}")
            if not os.path.exists(dst):
                shutil.copyfile(sp, dst)
            paths.append(dst)
    return paths * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scratch", default=None)
    args = ap.parse_args()
    scratch = args.scratch or tempfile.mkdtemp(prefix="classifier_bench_")
    try:
        paths = file_mix(scratch)
        nac = ingest.Classifier(path=os.path.join(ROOT, "tests", "golden", "classifiers", "naccess.config"))
        runs = {}
        for parser, opt in (("host", 0), ("device", ingest.PARSE_ON_DEVICE)):
            for cname, c in (("protor", None), ("naccess", nac)):
                fa.sweep_files(paths[:44], ingest_options=opt, classifier=c)             # warm-up: contexts, staging, tables
            for _ in range(args.reps):
                for cname, c in (("protor", None), ("naccess", nac)):
                    fa.sweep_parse_stats()
                    t0 = time.perf_counter()
                    _, _, atoms, status = fa.sweep_files(paths, ingest_options=opt, classifier=c)
                    dt = time.perf_counter() - t0
                    dev, host = fa.sweep_parse_stats()
                    r = runs.setdefault((parser, cname), {"atoms": int(atoms.sum()), "files": len(paths), "atoms_per_s": [],
                                                         "device_files": dev, "host_files": host})
                    r["atoms_per_s"].append(int(atoms.sum()) / dt)
        for (parser, cname), r in runs.items():
            v = sorted(r["atoms_per_s"])
            print(json.dumps({"parser": parser, "classifier": cname, "median_atoms_per_s": v[len(v) // 2], "runs": v,
                              "atoms": r["atoms"], "files": r["files"], "device_files": r["device_files"],
                              "host_files": r["host_files"]}))
    finally:
        if not args.scratch:
            shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
