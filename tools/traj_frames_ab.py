#!/usr/bin/env python3
"""The trajectory file driver of this commit against its parent commit's, run for run on one device: the same bytes, and the
same speed?  (profiles/traj_frames_refactor_ab.md is its output for the change that put the frame source, gpu_frames.hip,
behind the driver's input formats.)

One RUN is one fresh process (--worker) that loads one library - this commit's, or with FREESASA_AMD_LIB the parent's - and
    times  bench.py's trajectory_file key as bench.driver_workloads measures it (1000 frames x 100 000 atoms from a raw frame
           file: f64, f64_out_f32, f32 - warm-up on 104 frames, the better of two calls - and totals_only, one call), and the
           container arms of tools/traj_topology_bench.py on the files its --dcd --netcdf, --xtc and --trr modes make (one
           warm-up call, one timed call each); all values atom-frames/s, counted in the atoms of a frame as it comes in
    hashes the totals file and the per-atom file (SHA-256) of one file of each kind: raw fp64, raw fp32, DCD, NetCDF, a DCD file
           with a truncated octahedron's cell among periodic images (--pbc --triclinic), XTC, TRR single and double
The arms alternate - parent, this, parent, ... - and the files are made once, before the first run.  The rule of the speed
comparison: this commit's median does not lie below the lowest of the parent's own runs.  A run that fails ends the session.

    python tools/traj_frames_ab.py --parent-lib PATH [--runs 6] [--frames 240] [--scratch DIR] [--out FILE.md]"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BENCH_ATOMS, BENCH_FRAMES = 100_000, 1000


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 24), b""):
            h.update(piece)
    return h.hexdigest()


def prepare(scratch, frames):
    """every input file, by the tool's own writers and bench.py's recipe"""
    import tools
    from tools import traj_topology_bench as tb
    dirs = {k: os.path.join(scratch, k) for k in ("strided", "pbc", "xtc", "trr4", "trr8", "bench")}
    for d in dirs.values():
        os.makedirs(d)
    _, xyz = tb.solute()
    tb.make_frames(dirs["strided"], xyz, frames, True, True)
    tb.make_pbc_frames(dirs["pbc"], xyz, frames, True, False)
    mode = dict(frames=frames, reps=1, xtc_distinct=24, xtc_fpb=0, double=False, trr_arms="raw,trr")
    tb.xtc_mode(types.SimpleNamespace(**mode), dirs["xtc"])
    tb.trr_mode(types.SimpleNamespace(**mode), dirs["trr4"])
    tb.trr_mode(types.SimpleNamespace(**dict(mode, double=True)), dirs["trr8"])
    base, _ = tools.globule(BENCH_ATOMS, 5)
    with open(os.path.join(dirs["bench"], "frames.f64"), "wb") as a, open(os.path.join(dirs["bench"], "frames.f32"), "wb") as c:
        for f in range(BENCH_FRAMES):
            fr = tools.jitter(base, 100 + f, 0.5)
            fr.tofile(a)
            fr.astype(np.float32).tofile(c)


def worker(scratch, frames):
    import freesasa_amd as fa
    import tools
    from tools import traj_topology_bench as tb
    q = lambda *k: os.path.join(scratch, *k)
    out = tempfile.mkdtemp(prefix="run_", dir=scratch)
    o = lambda k: os.path.join(out, k)
    rates, hashes = {}, {}

    def keep(name, tp, sp):
        hashes[name + " totals"], hashes[name + " per-atom"] = sha(tp), sha(sp)
        os.unlink(sp)

    _, r = tools.globule(BENCH_ATOMS, 5)
    f64, f32 = q("bench", "frames.f64"), q("bench", "frames.f32")
    for tag, path, is32, o32 in (("f64", f64, False, False), ("f64_out_f32", f64, False, True), ("f32", f32, True, False)):
        tp, sp = o("tot_" + tag), o("sasa_" + tag)
        fa.trajectory_file(path, r, tp, sp, f32=is32, out_f32=o32, n_frames=104)
        dt = 1e9
        for _ in range(2):
            for old in (tp, sp):
                if os.path.exists(old):
                    os.unlink(old)
            t0 = time.perf_counter()
            done, got = fa.trajectory_file(path, r, tp, sp, f32=is32, out_f32=o32)
            dt = min(dt, time.perf_counter() - t0)
            assert done and got == BENCH_FRAMES
        rates["bench " + tag] = BENCH_ATOMS * BENCH_FRAMES / dt
        keep("raw " + tag, tp, sp)
    t0 = time.perf_counter()
    fa.trajectory_file(f64, r, o("tot_only"))
    rates["bench totals_only"] = BENCH_ATOMS * BENCH_FRAMES / (time.perf_counter() - t0)

    b, _ = tb.solute()
    index = np.arange(tb.N_SOLUTE, dtype=np.int32)
    n = tb.N_SOLUTE
    water = np.tile([1.1, 1.52, 1.1], n // 3 + 1)[:n].astype(np.float64)
    topo = lambda path, **kw: (lambda tp, sp=None: fa.trajectory_file_topology(path, b, tp, atom_index=index, sasa_path=sp, **kw))
    plain = lambda path, radii, **kw: (lambda tp, sp=None: fa.trajectory_file(path, radii, tp, sp, **kw))
    kinds = {"dcd": (topo(q("strided", "solvated.dcd"), dcd=True), tb.N_FRAME), "netcdf": (topo(q("strided", "solvated.nc"), netcdf=True), tb.N_FRAME),
             "xtc": (plain(q("xtc", "water.xtc"), water, xtc=True), n), "trr": (plain(q("trr4", "water.trr"), water, trr=True), n),
             "trr double": (plain(q("trr8", "water.trr"), water, trr=True), n),
             "dcd pbc triclinic": (plain(q("pbc", "octa_pbc.dcd"), b.radii, dcd=True, pbc=True, triclinic=True), n)}
    for name, (call, frame_atoms) in kinds.items():
        if name in ("dcd", "netcdf", "xtc", "trr"):      # the tool's arms: totals only
            call(o("warm"))
            t0 = time.perf_counter()
            res = call(o("timed"))
            rates["tool " + name] = frame_atoms * frames / (time.perf_counter() - t0)
            assert res[0] and res[1] == frames
        call(o("tot"), o("sasa"))
        keep(name, o("tot"), o("sasa"))
    shutil.rmtree(out)
    print(json.dumps({"rates": rates, "hashes": hashes}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--scratch")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args.scratch, args.frames)
    scratch = tempfile.mkdtemp(prefix="traj_frames_ab_", dir=args.scratch)
    try:
        prepare(scratch, args.frames)
        runs = {"parent": [], "this": []}
        for k in range(args.runs):
            for arm in runs:
                env = dict(os.environ)
                env.pop("FREESASA_AMD_LIB", None)
                if arm == "parent":
                    env["FREESASA_AMD_LIB"] = os.path.abspath(args.parent_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--scratch", scratch, "--frames", str(args.frames)],
                                   env=env, capture_output=True, text=True, timeout=400)
                if p.returncode != 0:
                    sys.exit(f"{arm} run {k + 1} failed ({p.returncode}): nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
                runs[arm].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(arm, k + 1, json.dumps(runs[arm][-1]["rates"]), flush=True)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    keys = list(runs["this"][0]["rates"])
    med = lambda v: float(np.median(v))
    text = ["| run | " + " | ".join(keys) + " |", "|---|" + "---|" * len(keys)]
    for k in range(args.runs):
        for arm in runs:
            text.append(f"| {arm} {k + 1} | " + " | ".join("%.4g" % runs[arm][k]["rates"][key] for key in keys) + " |")
    for arm in runs:
        text.append(f"| {arm} median | " + " | ".join("%.4g" % med([x["rates"][key] for x in runs[arm]]) for key in keys) + " |")
    text.append("")
    for key in keys:
        pv, tv = [x["rates"][key] for x in runs["parent"]], [x["rates"][key] for x in runs["this"]]
        text.append(f"- {key}: parent {min(pv):.4g} .. {max(pv):.4g} (median {med(pv):.4g}), this commit's median {med(tv):.4g}: "
                    + ("holds" if med(tv) >= min(pv) else "MISSES the rule"))
    text += ["", "SHA-256 of the result files, per arm (the same in every run of the arm unless said otherwise):", "",
             "| file | parent | this commit | |", "|---|---|---|---|"]
    for name in runs["this"][0]["hashes"]:
        hp, ht = {x["hashes"][name] for x in runs["parent"]}, {x["hashes"][name] for x in runs["this"]}
        text.append(f"| {name} | {' '.join(sorted(hp))} | {' '.join(sorted(ht))} | {'identical' if hp == ht and len(hp) == 1 else 'DIFFERENT'} |")
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
