#!/usr/bin/env python3
"""Atom-atom contact tables of the interfaces: freesasa_gpu_interface_contacts_dev against the interface entry it runs behind
(docs: DESIGN.md section 10, contacts).

The two workloads of tools/interfaces_bench.py (the ring of globules, the 2jo4 tetramers), Shrake-Rupley at 100 points, a warm
context.  A host clock around synchronous calls (each ends in a stream synchronization), the ways taken in turn per repetition,
medians:
  interfaces  GpuContext.interfaces: the call the new entry begins with
  masks       GpuContext.masks twice over the M pair-structure atoms, cut beforehand: as the P pair structures and as the 2 P
              sides - the two engine runs the stage adds
  contacts    GpuContext.interface_contacts, the whole new call with every array delivered; added = contacts - interfaces,
              rest = added - masks: the buried masks, the dots' scan and expansion, the partners, the rows, two synchronizations
              and the deliveries
and D_b (the buried test points), C (the rows) and the bytes the table takes.  Prints one JSON line per workload; a batch that
the entry refuses (the mask request's limits: include/freesasa_gpu.h) gets a line with the message instead of times.  The share
of the stage's own kernels is read from a kernel trace of this program (k_contact_masks, k_contact_attribute, k_contact_rows_*
against everything else): profiles/interface_contacts_bench.md says how."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import freesasa_amd as fa  # noqa: E402
from tools.interfaces_bench import ring, tetramers  # noqa: E402


def run(name, batch, n_points, reps):
    import torch
    dev = torch.device("cuda:0")
    xyz, r, offs, group, ng = batch
    n, ns, G = len(r), len(offs) - 1, int(ng.sum())
    ctx = fa.GpuContext(0)
    d_x, d_r, d_g = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz.reshape(-1), r, group))
    d_s, d_i, d_t, d_gt = (torch.empty(max(k, 1), dtype=torch.float64, device=dev) for k in (n, n, ns, 3 * G))
    P, M, T, Cand = ctx.interface_pairs(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, alg=fa.SHRAKE_RUPLEY, resolution=n_points)
    d_ar, d_so = torch.empty(6 * P, dtype=torch.float64, device=dev), torch.empty(2 * P + 1, dtype=torch.int64, device=dev)
    d_ps, d_pg, d_pa = (torch.empty(max(k, 1), dtype=torch.int32, device=dev) for k in (P, 2 * P, M))
    d_pb = torch.empty(max(M, 1), dtype=torch.float64, device=dev)
    common = dict(d_pair_struct=d_ps.data_ptr(), d_pair_groups=d_pg.data_ptr(), atom_capacity=M, d_side_offsets=d_so.data_ptr(),
                  d_pair_atom=d_pa.data_ptr(), d_pair_buried=d_pb.data_ptr(), d_totals=d_t.data_ptr(), d_group_totals=d_gt.data_ptr())

    def whole():
        ctx.interfaces(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, d_s.data_ptr(), d_i.data_ptr(), P, d_ar.data_ptr(),
                       alg=fa.SHRAKE_RUPLEY, resolution=n_points, **common)

    whole()
    pa, so = d_pa.cpu().numpy(), d_so.cpu().numpy()
    d_px, d_pr = torch.from_numpy(xyz[pa].reshape(-1)).to(dev), torch.from_numpy(r[pa]).to(dev)
    d_area, d_mask = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(4 * M, dtype=torch.int32, device=dev)
    poffs = so[::2].copy()

    def masks():
        ctx.masks(d_px.data_ptr(), d_pr.data_ptr(), poffs, d_area.data_ptr(), d_mask.data_ptr(), n_points=n_points)
        ctx.masks(d_px.data_ptr(), d_pr.data_ptr(), so, d_area.data_ptr(), d_mask.data_ptr(), n_points=n_points)

    # the counts first, then arrays that hold them
    try:
        _, _, Cn, D = ctx.interface_contacts(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, d_s.data_ptr(), d_i.data_ptr(), P,
                                             d_ar.data_ptr(), n_points=n_points, **common)
    except RuntimeError as e:                 # (a batch the mask request refuses: said, not timed)
        ctx.close()
        print(json.dumps(dict(workload=name, alg="sr%d" % n_points, atoms=n, structures=ns, groups=G, pairs=P, pair_atoms=M, refused=str(e))), flush=True)
        return
    d_cf, d_bm = torch.empty(M + 1, dtype=torch.int64, device=dev), torch.empty(4 * M, dtype=torch.int32, device=dev)
    d_cp, d_cn, d_dp = (torch.empty(max(k, 1), dtype=torch.int32, device=dev) for k in (Cn, Cn, D))
    d_ca = torch.empty(max(Cn, 1), dtype=torch.float64, device=dev)

    def contacts():
        ctx.interface_contacts(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, d_s.data_ptr(), d_i.data_ptr(), P, d_ar.data_ptr(),
                               contact_capacity=Cn, d_contact_first=d_cf.data_ptr(), d_contact_partner=d_cp.data_ptr(),
                               d_contact_points=d_cn.data_ptr(), d_contact_area=d_ca.data_ptr(), d_buried_masks=d_bm.data_ptr(), dot_capacity=D,
                               d_dot_partner=d_dp.data_ptr(), n_points=n_points, **common)

    ways = dict(interfaces=whole, masks=masks, contacts=contacts)
    for f in ways.values():
        f()                                   # warm: code objects, workspaces
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, f in ways.items():             # taken in turn
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    added = med["contacts"] - med["interfaces"]
    print(json.dumps(dict(workload=name, alg="sr%d" % n_points, atoms=n, structures=ns, groups=G, pairs=P, pair_atoms=M, buried_dots=D, rows=Cn,
                          reps=reps, ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(float(np.min(v)), 3) for k, v in times.items()},
                          ms_max={k: round(float(np.max(v)), 3) for k, v in times.items()}, ms_added=round(added, 3),
                          ms_rest=round(added - med["masks"], 3), added_over_interfaces=round(added / med["interfaces"], 4),
                          masks_share_of_added=round(med["masks"] / added, 4), dots_per_pair_atom=round(D / max(M, 1), 3),
                          table_bytes=8 * (M + 1) + 16 * Cn)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--copies", type=int, default=40, help="globules on the ring (24 to 60)")
    ap.add_argument("--atoms", type=int, default=2000)
    ap.add_argument("--tetramers", type=int, default=250)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if fa.device_count() <= 0:
        sys.exit("no HIP device: this benchmark measures nothing without one")
    run("ring-%dx%d" % (args.copies, args.atoms), ring(args.copies, args.atoms, 1), args.points, args.reps)
    run("2jo4x%d" % args.tetramers, tetramers(args.tetramers), args.points, args.reps)


if __name__ == "__main__":
    main()
