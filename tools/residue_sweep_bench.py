#!/usr/bin/env python3
"""What the per-residue table costs the file sweep (freesasa_gpu_sweep_files_residues), on bench.py's file mix (the reference's
7 PDB entries + 4 mmCIF fixtures, copied until >= 3e6 atoms, the list taken four times: >= 1e7 atoms), parser on the device,
page cache warm.  Arms, each run in a process of its own (the library is chosen when it is loaded), alternating a, b, e, c, a, ...:

    a   sweep_files on the PARENT commit's library (--parent-lib; left out without one)
    b   sweep_files on this tree's library
    c   sweep_files_residues on this tree's library
    d   the long way round on this tree's library: ingest.load_files -> calc_batch -> GpuContext.residue_areas (--long-way N runs)
    e   sweep_files_residues on the PARENT commit's library (with --parent-lib: c against e is the table's regression check)

b against a is the regression check (the medians must agree within the min-max spread of a's own runs), c against b is the
price of the table, c against d is what the table buys.  One JSON line per arm on stdout (and into --out).

    python tools/residue_sweep_bench.py [--reps 5] [--parent-lib PATH] [--parser device|host] [--long-way 3] [--out profiles/residue_sweep_bench.jsonl]

--parser host runs arms a, b, c with the host parser (ingest_options=0) instead.

For the kernel times: `rocprofv3 --kernel-trace --stats -- python tools/residue_sweep_bench.py --child c --scratch DIR`
(kp_res_keys / kp_res_count / kp_res_build / k_residue_areas are the table's kernels)."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PDB_NAMES = ["1a0q", "3gnn", "5dx9", "2jo4", "3bkr", "1d3z", "1ubq"]   # (bench.py's list)


def file_mix(scratch):
    from freesasa_amd import ingest
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


def child(arm, scratch, parser):
    """one warm-up over the whole list (contexts, staging, page cache), one timed run: a JSON line"""
    import freesasa_amd as fa
    from freesasa_amd import ingest
    paths = file_mix(scratch)
    out = {"arm": arm, "parser": parser, "files": len(paths)}
    options = ingest.PARSE_ON_DEVICE if parser == "device" else 0
    if arm in ("a", "b"):
        run = lambda: fa.sweep_files(paths, ingest_options=options)
    elif arm in ("c", "e"):
        run = lambda: fa.sweep_files_residues(paths, ingest_options=options)
    else:
        import torch
        dev = torch.device("cuda:0")
        table = ingest.residue_reference_table()

        def run():
            b = ingest.load_files(paths)
            sasa, _, tot = fa.calc_batch(b.xyz, b.radii, b.offsets)
            d_sasa = torch.from_numpy(sasa).to(dev)
            d_cls, d_bb = torch.from_numpy(b.atom_class).to(dev), torch.from_numpy(b.atom_backbone).to(dev)
            d_abs = torch.empty(6 * b.n_residues, dtype=torch.float64, device=dev)
            d_rel = torch.empty(5 * b.n_residues, dtype=torch.float64, device=dev)
            ctx = fa.GpuContext(0)
            ctx.residue_areas(d_sasa.data_ptr(), d_cls.data_ptr(), d_bb.data_ptr(), b.res_first, d_abs.data_ptr(),
                              res_ref=b.res_ref, ref_table=table, d_rel=d_rel.data_ptr())
            ctx.close()
            A, R = d_abs.cpu().numpy(), d_rel.cpu().numpy()
            return tot, None, np.diff(b.offsets), b.status, A, R
    run()
    fa.sweep_parse_stats()
    t0 = time.perf_counter()
    res = run()
    dt = time.perf_counter() - t0
    atoms = int(res[2].sum())
    out.update({"atoms": atoms, "seconds": dt, "atoms_per_s": atoms / dt})
    if arm in ("a", "b", "c", "e"):
        out["device_files"], out["host_files"] = fa.sweep_parse_stats()
    if arm in ("c", "e"):
        out["residues"] = int(res[4].n_residues)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long-way", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libfreesasa_amd.so built from the parent commit (arm a)")
    ap.add_argument("--parser", choices=("device", "host"), default="device", help="who parses in arms a, b, c")
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    scratch = args.scratch or tempfile.mkdtemp(prefix="residue_bench_")
    if args.child:
        child(args.child, scratch, args.parser)
        return
    try:
        runs = {}

        def one(arm):
            env = dict(os.environ)
            if arm in ("a", "e"):
                env["FREESASA_AMD_LIB"] = os.path.abspath(args.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm, "--scratch", scratch, "--parser", args.parser], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode:                                            # (a faulted arm ends the bench: nothing more is started)
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"arm {arm} failed with status {p.returncode}")
            runs.setdefault(arm, []).append(json.loads(p.stdout.strip().splitlines()[-1]))
        arms = ["a", "b", "e", "c"] if args.parent_lib else ["b", "c"]
        for _ in range(args.reps):
            for arm in arms:
                one(arm)
        for _ in range(args.long_way):
            one("d")
        lines = []
        for arm, rs in runs.items():
            v = sorted(r["atoms_per_s"] for r in rs)
            line = {"arm": arm, "parser": args.parser, "what": {"a": "sweep_files, parent library", "b": "sweep_files", "c": "sweep_files_residues",
                                         "d": "load_files -> calc_batch -> residue_areas", "e": "sweep_files_residues, parent library"}[arm],
                    "median_atoms_per_s": v[len(v) // 2], "min_atoms_per_s": v[0], "max_atoms_per_s": v[-1], "runs": v,
                    "atoms": rs[0]["atoms"], "files": rs[0]["files"]}
            for k in ("device_files", "host_files", "residues"):
                if k in rs[0]:
                    line[k] = rs[0][k]
            lines.append(json.dumps(line))
        print("\n".join(lines))
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    finally:
        if not args.scratch:
            shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
