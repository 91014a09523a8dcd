#!/usr/bin/env python3
"""Interfaces between chain groups: freesasa_gpu_interfaces_dev against the way to the same numbers without it (docs: DESIGN.md
section 10, interfaces).

Two workloads, Lee-Richards 20 slices and Shrake-Rupley 100 points, warm contexts:
  ring      N copies (default 40) of a 2 000-atom globule on a ring, each touching its two neighbours: N groups, N (N - 1) / 2
            pairs to test, N of them in contact
  tetramer  tests/golden/pdb/2jo4.pdb (four chains) x 250 structures: six pairs each, every one tested exactly
A host clock around synchronous calls (each ends in a stream synchronization), the ways taken in turn per repetition, medians:
  groups      GpuContext.groups: what every way below begins with
  pairs       GpuContext.interface_pairs: groups + the screen (boxes, candidates, exact contact, the flags back);
              screen = pairs - groups
  engine      the plain entry over the pair structures, cut beforehand: the engine run the whole call makes over them
  interfaces  GpuContext.interfaces, the whole call; rest = interfaces - pairs - engine: the gather, the sides' sums, the finish
              and the deliveries
  baseline    the parent's way: ALL G (G - 1) / 2 pairs of every structure and the isolated groups cut on the host with numpy
              (timed) and pushed through calc_batch (host arrays, upload and download included, as that entry is)
  host        freesasa_amd.calc_interfaces on host arrays (its sizing call included): what the baseline compares with like for like
Prints one JSON line per workload and algorithm.

--residues: the per-residue tables instead (freesasa_gpu_interface_residues_dev; docs: DESIGN.md section 10, residues).  The same
two workloads - the tetramer with the loader's residues, the ring in residues of 8 consecutive atoms, which a globule of
generated atoms does not have - and two ways taken in turn:
  interfaces  GpuContext.interfaces, as above
  residues    GpuContext.interface_residues with min_buried = 0: the same call and behind it heads, scans, segments and rows, R
              back to the host, the table delivered; added = residues - interfaces
and the bytes each delivers per structure: the table (res_offsets, and res_index, res_atoms, res_areas of R rows) against the
per-atom arrays a caller reduces himself (pair_atom and pair_buried of M atoms)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import freesasa_amd as fa  # noqa: E402
import tools  # noqa: E402


def ring(n_copies, n_atoms, seed):
    rng = np.random.default_rng(seed)
    x0, r0 = tools.globule(n_atoms, 30_000 + seed)
    x0 = x0 - x0.mean(axis=0)
    d = float(np.ptp(x0, axis=0).mean())
    R = (d - 1.0) / (2.0 * np.sin(np.pi / n_copies))
    xs = []
    for k in range(n_copies):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = 2.0 * np.pi * k / n_copies
        xs.append(x0 @ q + np.array([R * np.cos(a), R * np.sin(a), 0.0]))
    return (np.concatenate(xs), np.tile(r0, n_copies), np.array([0, n_copies * n_atoms], np.int64),
            np.repeat(np.arange(n_copies, dtype=np.int32), n_atoms), np.array([n_copies], np.int32))


def tetramers(copies):
    from freesasa_amd import ingest
    b = ingest.load_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    g, n, st = b.chain_groups(None, separate_chains=True)
    assert st[0] == 0
    return (np.tile(b.xyz, (copies, 1)), np.tile(b.radii, copies), np.arange(copies + 1, dtype=np.int64) * b.n_atoms, np.tile(g, copies),
            np.tile(n, copies))


def tetramer_residues(copies):
    from freesasa_amd import ingest
    b = ingest.load_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    first = np.asarray(b.res_first, np.int64)
    return np.concatenate([first[:-1] + k * b.n_atoms for k in range(copies)] + [[copies * b.n_atoms]]).astype(np.int64)


def run_residues(name, batch, res_first, alg, reps):
    import torch
    dev = torch.device("cuda:0")
    xyz, r, offs, group, ng = batch
    res = 20 if alg == fa.LEE_RICHARDS else 100
    n, ns, G = len(r), len(offs) - 1, int(ng.sum())
    ctx = fa.GpuContext(0)
    d_x, d_r, d_g = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz.reshape(-1), r, group))
    d_s, d_i, d_t, d_gt = (torch.empty(max(k, 1), dtype=torch.float64, device=dev) for k in (n, n, ns, 3 * G))
    P, M, T, C = ctx.interface_pairs(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, alg=alg, resolution=res)
    d_ar, d_so, d_ro = (torch.empty(k, dtype=t, device=dev) for k, t in ((6 * P, torch.float64), (2 * P + 1, torch.int64), (2 * P + 1, torch.int64)))
    d_ps, d_pg, d_pa, d_ri, d_ra = (torch.empty(max(k, 1), dtype=torch.int32, device=dev) for k in (P, 2 * P, M, M, M))
    d_pb, d_rar = torch.empty(max(M, 1), dtype=torch.float64, device=dev), torch.empty(3 * max(M, 1), dtype=torch.float64, device=dev)
    rows = {}

    def whole():
        ctx.interfaces(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, d_s.data_ptr(), d_i.data_ptr(), P, d_ar.data_ptr(), d_ps.data_ptr(),
                       d_pg.data_ptr(), atom_capacity=M, d_side_offsets=d_so.data_ptr(), d_pair_atom=d_pa.data_ptr(), d_pair_buried=d_pb.data_ptr(),
                       d_totals=d_t.data_ptr(), d_group_totals=d_gt.data_ptr(), alg=alg, resolution=res)

    def residues():
        rows["R"] = ctx.interface_residues(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, res_first, d_s.data_ptr(), d_i.data_ptr(), P,
                                           d_ar.data_ptr(), M, d_rar.data_ptr(), d_res_offsets=d_ro.data_ptr(), d_res_index=d_ri.data_ptr(),
                                           d_res_atoms=d_ra.data_ptr(), d_pair_struct=d_ps.data_ptr(), d_pair_groups=d_pg.data_ptr(),
                                           atom_capacity=M, d_side_offsets=d_so.data_ptr(), d_pair_atom=d_pa.data_ptr(),
                                           d_pair_buried=d_pb.data_ptr(), d_totals=d_t.data_ptr(), d_group_totals=d_gt.data_ptr(), alg=alg,
                                           resolution=res)[2]

    ways = dict(interfaces=whole, residues=residues)
    for f in ways.values():
        f()
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, f in ways.items():             # taken in turn
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    R = rows["R"]
    med = {k: float(np.median(v)) for k, v in times.items()}
    table_bytes, atom_bytes = 8 * (2 * P + 1) + 32 * R, 12 * M
    print(json.dumps(dict(workload=name, mode="residues", alg="lr20" if alg == fa.LEE_RICHARDS else "sr100", atoms=n, structures=ns, groups=G,
                          residues=int(len(res_first) - 1), contacts=P, pair_atoms=M, res_rows=R, reps=reps,
                          ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(float(np.min(v)), 3) for k, v in times.items()},
                          ms_max={k: round(float(np.max(v)), 3) for k, v in times.items()},
                          ms_added=round(med["residues"] - med["interfaces"], 3),
                          added_over_interfaces=round((med["residues"] - med["interfaces"]) / med["interfaces"], 4),
                          table_bytes_per_structure=round(table_bytes / ns, 1), per_atom_bytes_per_structure=round(atom_bytes / ns, 1))), flush=True)


def all_pairs_on_the_host(xyz, r, offs, group, ng):
    """the baseline's cut: every pair (g < h) of every structure, then every group, as one batch"""
    idx, sizes = [], []
    for s in range(len(ng)):
        mem = [offs[s] + np.nonzero(group[offs[s]:offs[s + 1]] == g)[0] for g in range(ng[s])]
        for g in range(ng[s]):
            for h in range(g + 1, ng[s]):
                idx += [mem[g], mem[h]]; sizes.append(len(mem[g]) + len(mem[h]))
        idx += mem; sizes += [len(m) for m in mem]
    idx = np.concatenate(idx)
    return xyz[idx], r[idx], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def run(name, batch, alg, reps):
    import torch
    dev = torch.device("cuda:0")
    xyz, r, offs, group, ng = batch
    res = 20 if alg == fa.LEE_RICHARDS else 100
    n, ns, G = len(r), len(offs) - 1, int(ng.sum())
    ctx = fa.GpuContext(0)
    d_x, d_r, d_g = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz.reshape(-1), r, group))
    d_s, d_i, d_t, d_gt = (torch.empty(max(k, 1), dtype=torch.float64, device=dev) for k in (n, n, ns, 3 * G))
    P, M, T, C = ctx.interface_pairs(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, alg=alg, resolution=res)
    ps, pg = np.empty(P, np.int32), np.empty((P, 2), np.int32)
    d_ar, d_so = torch.empty(6 * P, dtype=torch.float64, device=dev), torch.empty(2 * P + 1, dtype=torch.int64, device=dev)
    d_ps, d_pg, d_pa = (torch.empty(k, dtype=torch.int32, device=dev) for k in (P, 2 * P, M))
    d_pb = torch.empty(M, dtype=torch.float64, device=dev)

    def groups():
        ctx.groups(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, d_s.data_ptr(), d_i.data_ptr(), d_t.data_ptr(), d_gt.data_ptr(),
                   alg=alg, resolution=res)

    def pairs():
        ctx.interface_pairs(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, P, ps, pg, d_s.data_ptr(), d_i.data_ptr(), d_t.data_ptr(),
                            d_gt.data_ptr(), alg=alg, resolution=res)

    def whole():
        ctx.interfaces(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, d_s.data_ptr(), d_i.data_ptr(), P, d_ar.data_ptr(), d_ps.data_ptr(),
                       d_pg.data_ptr(), atom_capacity=M, d_side_offsets=d_so.data_ptr(), d_pair_atom=d_pa.data_ptr(), d_pair_buried=d_pb.data_ptr(),
                       d_totals=d_t.data_ptr(), d_group_totals=d_gt.data_ptr(), alg=alg, resolution=res)

    whole()
    pa, so = d_pa.cpu().numpy(), d_so.cpu().numpy()
    d_px, d_pr = torch.from_numpy(xyz[pa].reshape(-1)).to(dev), torch.from_numpy(r[pa]).to(dev)
    d_psasa, poffs = torch.empty(M, dtype=torch.float64, device=dev), so[::2].copy()

    def engine():
        if alg == fa.LEE_RICHARDS:
            ctx.lee_richards(d_px.data_ptr(), d_pr.data_ptr(), poffs, d_psasa.data_ptr(), n_slices=res)
        else:
            ctx.shrake_rupley(d_px.data_ptr(), d_pr.data_ptr(), poffs, d_psasa.data_ptr(), n_points=res)

    out = {}

    def baseline():
        bx, br, boffs = all_pairs_on_the_host(xyz, r, offs, group, ng)
        out["baseline_atoms"] = int(len(br))
        out["baseline_structures"] = int(len(boffs) - 1)
        fa.calc_batch(bx, br, boffs, alg=alg, resolution=res)

    def host():
        fa.calc_interfaces(xyz, r, offs, group, ng, alg=alg, resolution=res, per_atom=True)

    ways = dict(groups=groups, pairs=pairs, engine=engine, interfaces=whole, baseline=baseline, host=host)
    for f in ways.values():
        f()                                   # warm: code objects, workspaces, pooled contexts
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, f in ways.items():             # taken in turn
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    out.update(workload=name, alg="lr20" if alg == fa.LEE_RICHARDS else "sr100", atoms=n, structures=ns, groups=G, tests=T, candidates=C,
               contacts=P, contacts_per_candidate=round(P / max(C, 1), 4), pair_atoms=M, reps=reps,
               ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(float(np.min(v)), 3) for k, v in times.items()},
               ms_max={k: round(float(np.max(v)), 3) for k, v in times.items()},
               ms_screen=round(med["pairs"] - med["groups"], 3), ms_rest=round(med["interfaces"] - med["pairs"] - med["engine"], 3),
               baseline_over_host=round(med["baseline"] / med["host"], 2))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--copies", type=int, default=40, help="globules on the ring (24 to 60)")
    ap.add_argument("--atoms", type=int, default=2000)
    ap.add_argument("--tetramers", type=int, default=250)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--algs", default="lr,sr")
    ap.add_argument("--residues", action="store_true", help="time the per-residue tables against the interface entry")
    args = ap.parse_args()
    if fa.device_count() <= 0:
        sys.exit("no HIP device: this benchmark measures nothing without one")
    for a in args.algs.split(","):
        alg = fa.LEE_RICHARDS if a == "lr" else fa.SHRAKE_RUPLEY
        if args.residues:
            n = args.copies * args.atoms
            run_residues("ring-%dx%d" % (args.copies, args.atoms), ring(args.copies, args.atoms, 1), np.arange(0, n + 8, 8, dtype=np.int64).clip(max=n),
                         alg, args.reps)
            run_residues("2jo4x%d" % args.tetramers, tetramers(args.tetramers), tetramer_residues(args.tetramers), alg, args.reps)
            continue
        run("ring-%dx%d" % (args.copies, args.atoms), ring(args.copies, args.atoms, 1), alg, args.reps)
        run("2jo4x%d" % args.tetramers, tetramers(args.tetramers), alg, args.reps)


if __name__ == "__main__":
    main()
