#!/usr/bin/env python3
"""What selection areas cost the file sweep (freesasa_gpu_sweep_files_select), on bench.py's file mix (the reference's 7 PDB
entries + 4 mmCIF fixtures, copied until >= 3e6 atoms, the list taken four times: >= 1e7 atoms), parser on the device, page
cache warm.  Arms, each run in a process of its own (the library is chosen when it is loaded), alternating a, b, c1, c8, c64, a, ...:

    a     sweep_files on the PARENT commit's library (--parent-lib; left out without one)
    b     sweep_files on this tree's library
    c1, c8, c64   sweep_files_select with 1, 8 and 64 selections
    d     the long way round for 8 selections: ingest.load_files -> calc_batch -> Batch.select per structure and command ->
          GpuContext.class_sums with the mask as class (--long-way N runs)

b against a is the regression check (the plain sweep launches nothing new: the medians must agree within the min-max spread
of a's own runs), c against b is the price of the selections, c8 against d is what the device-side selection buys.  One JSON
line per arm on stdout (and into --out).

    python tools/select_sweep_bench.py [--reps 5] [--parent-lib PATH] [--parser device|host] [--long-way 2] [--out profiles/select_sweep_bench.jsonl]

For the kernel times: `rocprofv3 --kernel-trace --stats -- python tools/select_sweep_bench.py --child c8 --scratch DIR`
(kp_atom_keys / k_sel_mask / k_sel_sums are the selections' kernels; kp_res_keys / kp_res_count / kp_res_build run for them too)."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from residue_sweep_bench import file_mix   # noqa: E402 - bench.py's file mix x 4

EIGHT = ["bb, name n+ca+c+o", "hyd, resn ala+val+leu+ile+met+phe+trp+pro", "r, resi 10-20+30 and not symbol c",
         "open, resi -5 or resi 60-", "ch, chain A-B and not chain A", "ic, resi 52A", "het, symbol fe+zn+se+s", "w, name abcde"]
WHAT = {"a": "sweep_files, parent library", "b": "sweep_files", "c1": "sweep_files_select, 1 selection", "c8": "sweep_files_select, 8 selections",
        "c64": "sweep_files_select, 64 selections", "d": "load_files -> calc_batch -> Batch.select -> class_sums, 8 selections"}


def commands(n):
    return [f"s{k}_{EIGHT[k % 8]}" for k in range(n)]


def child(arm, scratch, parser):
    """one warm-up over the whole list (contexts, staging, page cache), one timed run: a JSON line"""
    import freesasa_amd as fa
    from freesasa_amd import ingest
    paths = file_mix(scratch)
    out = {"arm": arm, "parser": parser, "files": len(paths)}
    options = ingest.PARSE_ON_DEVICE if parser == "device" else 0
    if arm in ("a", "b"):
        run = lambda: fa.sweep_files(paths, ingest_options=options)
    elif arm.startswith("c"):
        sel = ingest.Selection(commands(int(arm[1:])))
        run = lambda: fa.sweep_files_select(paths, sel, ingest_options=options)
    else:
        import torch
        dev = torch.device("cuda:0")

        def run():
            b = ingest.load_files(paths)
            sasa, _, tot = fa.calc_batch(b.xyz, b.radii, b.offsets)
            d_sasa = torch.from_numpy(sasa).to(dev)
            d_out = torch.empty(3 * b.n_structs, dtype=torch.float64, device=dev)
            ctx = fa.GpuContext(0)
            areas = np.zeros((b.n_structs, 8))
            for q, cmd in enumerate(EIGHT):
                mask = np.concatenate([b.select(k, cmd)[1] for k in range(b.n_structs)])   # one tree walk per structure and command
                ctx.class_sums(d_sasa.data_ptr(), torch.from_numpy(mask).to(dev).data_ptr(), b.offsets, d_out.data_ptr())
                areas[:, q] = d_out.cpu().numpy().reshape(-1, 3)[:, 1]
            ctx.close()
            return tot, None, np.diff(b.offsets), b.status, areas
    run()
    fa.sweep_parse_stats()
    t0 = time.perf_counter()
    res = run()
    dt = time.perf_counter() - t0
    atoms = int(res[2].sum())
    out.update({"atoms": atoms, "seconds": dt, "atoms_per_s": atoms / dt})
    if arm != "d":
        out["device_files"], out["host_files"] = fa.sweep_parse_stats()
    if arm.startswith("c"):
        out["selected_atoms"] = int(res[5].sum())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long-way", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libfreesasa_amd.so built from the parent commit (arm a)")
    ap.add_argument("--parser", choices=("device", "host"), default="device", help="who parses in arms a, b, c")
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    scratch = args.scratch or tempfile.mkdtemp(prefix="select_bench_")
    if args.child:
        child(args.child, scratch, args.parser)
        return
    try:
        runs = {}

        def one(arm):
            env = dict(os.environ)
            if arm == "a":
                env["FREESASA_AMD_LIB"] = os.path.abspath(args.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm, "--scratch", scratch, "--parser", args.parser], env=env,
                               capture_output=True, text=True, timeout=900)
            if p.returncode:                                            # (a faulted arm ends the bench: nothing more is started)
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"arm {arm} failed with status {p.returncode}")
            runs.setdefault(arm, []).append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"# {arm}: {runs[arm][-1]['atoms_per_s']:.4g} atoms/s", file=sys.stderr, flush=True)
        arms = (["a"] if args.parent_lib else []) + ["b", "c1", "c8", "c64"]
        for _ in range(args.reps):
            for arm in arms:
                one(arm)
        for _ in range(args.long_way):
            one("d")
        lines = []
        for arm, rs in runs.items():
            v = sorted(r["atoms_per_s"] for r in rs)
            line = {"arm": arm, "parser": args.parser, "what": WHAT[arm], "median_atoms_per_s": v[len(v) // 2], "min_atoms_per_s": v[0],
                    "max_atoms_per_s": v[-1], "runs": v, "atoms": rs[0]["atoms"], "files": rs[0]["files"]}
            for k in ("device_files", "host_files", "selected_atoms"):
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
