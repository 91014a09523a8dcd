#!/usr/bin/env python3
"""tools/dots_bench.py [--workload coil|pdb] [--points 100] [--repeats 3]
   tools/dots_bench.py --plain TREE

What the exposure masks and the surface dots cost on one device, device-resident, timed as bench.py times its coil_sr100 and
real_pdb_sr100 keys (3 warm-up calls, then 10 calls between two synchronisations, `--repeats` times): the plain Shrake-Rupley
launch (GpuContext.shrake_rupley), the mask launch (GpuContext.masks), and on the masks it left the scan
(GpuContext.dots_count) and the expansion (GpuContext.dots_expand, with and without the index arrays) with the bytes they
write per second - next to a plain hipMemsetAsync of the expansion's bytes in the same process.  One JSON line.
--plain TREE: only the plain Shrake-Rupley launch, on both workloads, of the package found in TREE (a checkout of any commit, built
there with `make`; `.` for this tree) - what shows whether a change costs the existing launches anything: run it from the parent's
checkout and from this tree in turn, a process each.
profiles/dots_bench.md holds the numbers of the MI355X."""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plain(tree, repeats):
    """the plain S&R-100 launch of the package in `tree` on the coil batch and the PDB entries: one JSON line"""
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import torch

    import bench
    import freesasa_amd as fa
    import tools
    assert os.path.abspath(fa.__file__).startswith(tree + os.sep), (fa.__file__, tree)
    dev = torch.device("cuda:0")
    res = {"tree": tree, "lib": fa.LIB_PATH}
    px, pr, poffs, per, reps = bench.real_pdb_batch()
    for name, (xyz, r, offs) in (("coil_sr100", tools.coil_batch(1000, 10000, seed0=1000)), ("real_pdb_sr100", (px, pr, poffs))):
        n = int(offs[-1])
        d_xyz, d_r = torch.from_numpy(np.ascontiguousarray(xyz).reshape(-1)).to(dev), torch.from_numpy(np.ascontiguousarray(r)).to(dev)
        d_sasa, d_cnt = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        ctx = fa.GpuContext(0)
        res[name] = timed(torch, lambda: ctx.shrake_rupley(d_xyz.data_ptr(), d_r.data_ptr(), offs, d_sasa.data_ptr(), d_cnt.data_ptr(), 0, probe=1.4, n_points=100), repeats)
        ctx.close()
    print(json.dumps(res))


def timed(torch, call, repeats, steps=10):
    """ms per call: 3 warm-up calls, then `steps` calls between two synchronisations, `repeats` times"""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    out = []
    gc.collect(); gc.disable()
    try:
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / steps)
    finally:
        gc.enable()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("coil", "pdb"), default="coil")
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--structs", type=int, default=1000, help="coils of the coil batch")
    ap.add_argument("--atoms", type=int, default=10000, help="atoms per coil")
    ap.add_argument("--plain", metavar="TREE", help="only the plain S&R launch of the package in TREE, on both workloads")
    args = ap.parse_args(argv)
    if args.plain:
        return plain(args.plain, args.repeats)
    import torch

    import bench
    import freesasa_amd as fa
    import tools
    if args.workload == "coil":
        xyz, r, offs = tools.coil_batch(args.structs, args.atoms, seed0=1000)
        wl = f"{args.structs} coils x {args.atoms} atoms"
    else:
        xyz, r, offs, per, reps = bench.real_pdb_batch()
        wl = f"{reps} x the PDB entries {', '.join(bench.PDB_NAMES)}"
    dev = torch.device("cuda:0")
    n, N = int(offs[-1]), args.points
    d_xyz, d_r = torch.from_numpy(np.ascontiguousarray(xyz).reshape(-1)).to(dev), torch.from_numpy(np.ascontiguousarray(r)).to(dev)
    d_sasa = torch.empty(n, dtype=torch.float64, device=dev)
    d_cnt = torch.empty(n, dtype=torch.int32, device=dev)
    d_masks = torch.empty((n, 4), dtype=torch.int32, device=dev)
    d_first = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ctx = fa.GpuContext(0)
    res = {"workload": wl, "atoms": n, "points": N}
    res["sr_ms"] = timed(torch, lambda: ctx.shrake_rupley(d_xyz.data_ptr(), d_r.data_ptr(), offs, d_sasa.data_ptr(), d_cnt.data_ptr(), 0, probe=1.4, n_points=N), args.repeats)
    res["masks_ms"] = timed(torch, lambda: ctx.masks(d_xyz.data_ptr(), d_r.data_ptr(), offs, d_sasa.data_ptr(), d_masks.data_ptr(), d_cnt.data_ptr(), probe=1.4, n_points=N), args.repeats)
    res["masks_over_sr"] = float(np.mean(res["masks_ms"]) / np.mean(res["sr_ms"]))
    D = ctx.dots_count(d_masks.data_ptr(), n, d_first.data_ptr(), n_points=N)
    assert D == int(d_cnt.sum(dtype=torch.int64).item())
    res["dots"] = D
    res["scan_ms"] = timed(torch, lambda: ctx.dots_count(d_masks.data_ptr(), n, d_first.data_ptr(), n_points=N), args.repeats)
    res["scan_read_bytes"], res["scan_written_bytes"] = 2 * 16 * n, 8 * (n + 1)
    d_dx = torch.empty((D, 3), dtype=torch.float64, device=dev)
    d_da, d_dp = torch.empty(D, dtype=torch.int32, device=dev), torch.empty(D, dtype=torch.int32, device=dev)
    expand = lambda a, p: ctx.dots_expand(d_xyz.data_ptr(), d_r.data_ptr(), n, d_masks.data_ptr(), d_first.data_ptr(), D, d_dx.data_ptr(), a, p, probe=1.4, n_points=N)
    res["expand_ms"] = timed(torch, lambda: expand(0, 0), args.repeats)
    res["expand_indexed_ms"] = timed(torch, lambda: expand(d_da.data_ptr(), d_dp.data_ptr()), args.repeats)
    res["expand_written_bytes"], res["expand_indexed_written_bytes"] = 24 * D, 32 * D
    res["expand_TB_per_s"] = 24 * D / (1e-3 * float(np.mean(res["expand_ms"]))) / 1e12
    res["expand_indexed_TB_per_s"] = 32 * D / (1e-3 * float(np.mean(res["expand_indexed_ms"]))) / 1e12
    # the yardstick of this machine, this session: a plain hipMemsetAsync of the same bytes, synchronised per call as the entries are
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipDeviceSynchronize.argtypes = []

    def memset(ptr, nbytes):
        assert hip.hipMemsetAsync(ptr, 0, nbytes, None) == 0 and hip.hipDeviceSynchronize() == 0

    res["memset_24D_ms"] = timed(torch, lambda: memset(d_dx.data_ptr(), 24 * D), args.repeats)
    res["memset_TB_per_s"] = 24 * D / (1e-3 * float(np.mean(res["memset_24D_ms"]))) / 1e12
    res["expand_over_memset_rate"] = res["expand_TB_per_s"] / res["memset_TB_per_s"]
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
