"""One run of one arm of an A/B of the host-batch chunk path (csrc/gpu_hostbatch.hip): bench.py's end_to_end line (page-locked
and pageable host arrays) and its sweep_cache line, through whichever library FREESASA_AMD_LIB names; one JSON line appended
to OUT.jsonl, with digests of the results so that the arms can be compared.
    python tools/hostbatch_ab.py ARM OUT.jsonl [setup]      (setup: only write the cache file and the coil batch to /tmp)
Run the arms in turns, each run a process of its own: FREESASA_AMD_LIB=<parent's libfreesasa_amd.so> ... parent out.jsonl, then
... refactor out.jsonl, and so on."""
import hashlib, json, os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
import tools
import freesasa_amd as fa
from freesasa_amd import ingest

arm, out_path = sys.argv[1], sys.argv[2]
setup = len(sys.argv) > 3
scratch = "/tmp/hostbatch_ab"
os.makedirs(scratch, exist_ok=True)
cache = os.path.join(scratch, "sweep.fsab")
if setup or not os.path.exists(cache):
    pdb_dir, cif_dir = os.path.join(ROOT, "tests", "golden", "pdb"), os.path.join(ROOT, "tests", "golden", "cif")
    srcs = [os.path.join(pdb_dir, nm + ".pdb") for nm in bench.PDB_NAMES] + sorted(os.path.join(cif_dir, f) for f in os.listdir(cif_dir) if f.endswith(".cif"))[:4]
    one = ingest.load_pdb_files(srcs)
    reps = max(1, -(-3_000_000 // int(one.n_atoms)))
    b4 = ingest.load_pdb_files([p for _ in range(reps) for p in srcs] * 4)
    b4.save(cache)
    print("setup: cache of", int(b4.n_atoms), "atoms", flush=True)
    del b4
xyz, r, offs = tools.coil_batch(1000, 10000, seed0=1000, cache_dir="/tmp")
if setup:
    sys.exit(0)
args = types.SimpleNamespace(slices=20)
res = {"arm": arm, "lib": os.environ.get("FREESASA_AMD_LIB", "tree")}
# (bench.py compares the areas with its resident run's; here a digest of them, to compare the arms by)
e2e = bench.end_to_end(fa, torch, xyz, r, offs, args, 0, np.zeros(0))
got = fa.calc_batch_pipelined(xyz, r, offs, probe=1.4, resolution=20, device=0)
res["end_to_end_pinned"] = e2e["value"]
res["end_to_end_pageable"] = e2e["pageable_host_memory"]["value"]
res["e2e_sha"] = hashlib.sha256(got[0].tobytes() + got[2].tobytes()).hexdigest()[:16]
fa.sweep_cache(cache, device=0)
t0 = time.perf_counter(); ctot, ccls, catoms, cstatus = fa.sweep_cache(cache, device=0); dt = time.perf_counter() - t0
n4 = int(catoms.sum())
res["sweep_cache"] = n4 / dt
res["sweep_atoms"] = n4
res["sweep_sha"] = hashlib.sha256(ctot.tobytes() + ccls.tobytes()).hexdigest()[:16]
with open(out_path, "a") as f:
    f.write(json.dumps(res) + "\n")
print(json.dumps(res), flush=True)
