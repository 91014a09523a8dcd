#!/usr/bin/env python3
"""Chain groups: freesasa_gpu_groups_dev against what a caller would do without it (docs: DESIGN.md, chain groups).

1000 docking-like complexes of two 2 500-atom globules in contact, random orientations; Lee-Richards 20 slices and
Shrake-Rupley 100 points; warm contexts; HIP events around synchronous calls, three ways taken in turn per repetition:
  groups  one freesasa_gpu_groups_dev call (complex areas, isolated areas, totals, group totals)
  plain   two plain batch calls: the complex batch, then the pre-extracted batch of the isolated groups
  host    the round trip without the entry: download the coordinates, cut the groups out with numpy, upload them,
          a second call (the complex call included)
Prints one JSON line per algorithm (median ms of each way, groups / plain, host / groups).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import freesasa_amd as fa  # noqa: E402
import tools  # noqa: E402


def docking_batch(n_complex, n_each, seed):
    rng = np.random.default_rng(seed)
    xs, rs = [], []
    for k in range(n_complex):
        pair = []
        for h in range(2):
            x, r = tools.globule(n_each, 20_000 + 2 * k + h)
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            pair.append(((x - x.mean(axis=0)) @ q, r))
        (ax, ar), (bx, br) = pair
        bx = bx + np.array([ax[:, 0].max() - bx[:, 0].min() - 8.0, 0.0, 0.0])
        xs += [ax, bx]; rs += [ar, br]
    xyz, r = np.concatenate(xs), np.concatenate(rs)
    offs = np.arange(n_complex + 1, dtype=np.int64) * 2 * n_each
    group = np.tile(np.repeat(np.array([0, 1], np.int32), n_each), n_complex)
    return xyz, r, offs, group, np.full(n_complex, 2, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complexes", type=int, default=1000)
    ap.add_argument("--atoms", type=int, default=2500, help="atoms per partner")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--algs", default="lr,sr")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    xyz, r, offs, group, ng = docking_batch(args.complexes, args.atoms, 3)
    n, ns, G = len(r), len(offs) - 1, int(ng.sum())
    # the isolated batch, extracted once for the "plain" way (structure-major, atoms in order)
    order = np.concatenate([offs[s] + np.nonzero(group[offs[s]:offs[s + 1]] == g)[0] for s in range(ns) for g in range(ng[s])])
    ioffs = np.concatenate([[0], np.cumsum([np.count_nonzero(group[offs[s]:offs[s + 1]] == g) for s in range(ns) for g in range(ng[s])])]).astype(np.int64)
    d_x, d_r, d_g = (torch.from_numpy(a).to(dev) for a in (xyz.reshape(-1), r, group))
    d_ix, d_ir = torch.from_numpy(xyz[order].reshape(-1)).to(dev), torch.from_numpy(r[order]).to(dev)
    d_s, d_i, d_t, d_gt = (torch.empty(k, dtype=torch.float64, device=dev) for k in (n, n, ns, 3 * G))
    d_is, d_it = torch.empty(len(order), dtype=torch.float64, device=dev), torch.empty(G, dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0, stream=torch.cuda.current_stream().cuda_stream)
    tp = {}

    def plain(alg, res, dx, dr, o, ds, dt):
        if alg == fa.LEE_RICHARDS:
            ctx.lee_richards(dx.data_ptr(), dr.data_ptr(), o, ds.data_ptr(), dt.data_ptr(), n_slices=res)
        else:
            ctx.shrake_rupley(dx.data_ptr(), dr.data_ptr(), o, ds.data_ptr(), 0, dt.data_ptr(), n_points=res)

    for name in args.algs.split(","):
        alg, res = (fa.LEE_RICHARDS, 20) if name == "lr" else (fa.SHRAKE_RUPLEY, 100)

        def way_groups():
            ctx.groups(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, d_s.data_ptr(), d_i.data_ptr(),
                       d_t.data_ptr(), d_gt.data_ptr(), alg=alg, resolution=res)

        def way_plain():
            plain(alg, res, d_x, d_r, offs, d_s, d_t)
            plain(alg, res, d_ix, d_ir, ioffs, d_is, d_it)

        def way_host():
            plain(alg, res, d_x, d_r, offs, d_s, d_t)
            hx, hg = d_x.cpu().numpy().reshape(-1, 3), d_g.cpu().numpy()
            hr = d_r.cpu().numpy()
            sel = np.concatenate([offs[s] + np.nonzero(hg[offs[s]:offs[s + 1]] == g)[0] for s in range(ns) for g in range(ng[s])])
            o2 = np.concatenate([[0], np.cumsum([np.count_nonzero(hg[offs[s]:offs[s + 1]] == g) for s in range(ns) for g in range(ng[s])])]).astype(np.int64)
            ux, ur = torch.from_numpy(np.ascontiguousarray(hx[sel]).reshape(-1)).to(dev), torch.from_numpy(hr[sel]).to(dev)
            plain(alg, res, ux, ur, o2, d_is, d_it)

        ways = {"groups": way_groups, "plain": way_plain, "host": way_host}
        for f in ways.values():      # warm: workspaces sized, launch shapes learnt
            f(); f()
        times = {k: [] for k in ways}
        for _ in range(args.reps):
            for k, f in ways.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(json.dumps({"alg": name, "resolution": res, "complexes": ns, "atoms": n, "groups": G,
                          "ms_groups": med["groups"], "ms_plain_two_calls": med["plain"], "ms_host_round_trip": med["host"],
                          "groups_over_plain": med["groups"] / med["plain"], "host_over_groups": med["host"] / med["groups"],
                          "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
