#!/usr/bin/env python3
"""Residue-residue contact tables of the interfaces: freesasa_gpu_interface_residue_contacts_dev against the contact entry it runs
behind (docs: DESIGN.md section 10, residue contacts).

The two workloads of tools/interface_contacts_bench.py (the ring of globules in residues of 8 atoms, the 2jo4 tetramers with their
own residues), Shrake-Rupley at 100 points, a warm context.  A host clock around synchronous calls (each ends in a stream
synchronization); the two entries taken in turn per repetition, the one that goes first changing with every repetition; the host
fold, tens of milliseconds of host work during which the device idles, in repetitions of its own behind them, so that it does not
sit in front of one of the two; medians:
  contacts     GpuContext.interface_contacts with every array delivered: the call the new entry begins with
  rescontacts  GpuContext.interface_residue_contacts, the whole new call with every array delivered; added = rescontacts -
               contacts: the segments, the fold, the reverse rows, one synchronization and five deliveries
  host_fold    for information: the contact call, its rows downloaded and folded by tools/interfaces.py fold_contact_rows - what a
               caller did before the device fold existed (it gives no reverse rows and no offsets)
and C (the contact rows), Q (the folded rows) and the bytes the folded table takes.  Prints one JSON line per workload; a
batch that the contact entry refuses (the mask request's limits: include/freesasa_gpu.h) gets a line with the message instead of
times.  The fold stage's kernel times are read from a kernel trace of this program (k_rc_fold_count, k_rc_fold_write, k_rc_reverse
and the reused k_iface_res_head / _first / _scan_*): profiles/interface_residue_contacts_bench.md says how."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import freesasa_amd as fa  # noqa: E402
from tools.interfaces import contact_row_keys, fold_contact_rows  # noqa: E402
from tools.interfaces_bench import ring, tetramer_residues, tetramers  # noqa: E402


def run(name, batch, res_first, n_points, reps):
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
    head = (d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng)
    # the counts first, then arrays that hold them
    try:
        _, _, Cn, D = ctx.interface_contacts(*head, d_s.data_ptr(), d_i.data_ptr(), P, d_ar.data_ptr(), n_points=n_points, **common)
    except RuntimeError as e:                 # (a batch the mask request refuses: said, not timed)
        ctx.close()
        print(json.dumps(dict(workload=name, alg="sr%d" % n_points, atoms=n, structures=ns, groups=G, pairs=P, pair_atoms=M, refused=str(e))), flush=True)
        return
    d_cf, d_bm = torch.empty(M + 1, dtype=torch.int64, device=dev), torch.empty(4 * M, dtype=torch.int32, device=dev)
    d_cp, d_cn, d_dp = (torch.empty(max(k, 1), dtype=torch.int32, device=dev) for k in (Cn, Cn, D))
    d_ca = torch.empty(max(Cn, 1), dtype=torch.float64, device=dev)
    table = dict(contact_capacity=Cn, d_contact_first=d_cf.data_ptr(), d_contact_partner=d_cp.data_ptr(), d_contact_points=d_cn.data_ptr(),
                 d_contact_area=d_ca.data_ptr(), d_buried_masks=d_bm.data_ptr(), dot_capacity=D, d_dot_partner=d_dp.data_ptr())
    d_qo = torch.empty(2 * P + 1, dtype=torch.int64, device=dev)
    d_qr, d_qc, d_qv = (torch.empty(max(k, 1), dtype=torch.int32, device=dev) for k in (2 * Cn, 2 * Cn, Cn))
    d_qa = torch.empty(max(Cn, 1), dtype=torch.float64, device=dev)
    atom_res = np.repeat(np.arange(len(res_first) - 1, dtype=np.int64), np.diff(res_first))
    rows = {}

    def contacts():
        ctx.interface_contacts(*head, d_s.data_ptr(), d_i.data_ptr(), P, d_ar.data_ptr(), n_points=n_points, **table, **common)

    def rescontacts():
        rows["Q"] = ctx.interface_residue_contacts(*head, res_first, d_s.data_ptr(), d_i.data_ptr(), P, d_ar.data_ptr(), Cn, d_qa.data_ptr(),
                                                   d_rescontact_offsets=d_qo.data_ptr(), d_rescontact_residues=d_qr.data_ptr(),
                                                   d_rescontact_counts=d_qc.data_ptr(), d_rescontact_reverse=d_qv.data_ptr(), n_points=n_points,
                                                   **table, **common)[4]

    def host_fold():
        contacts()
        so, pa, cf, cp, cn, ca = (t.cpu().numpy() for t in (d_so, d_pa, d_cf, d_cp, d_cn, d_ca))
        row_pair, ai, aj = contact_row_keys(so, pa[:M], cf, cp[:Cn])
        rows["host"] = len(fold_contact_rows(row_pair, atom_res[ai], atom_res[aj], cn[:Cn], ca[:Cn])[0])

    ways = dict(contacts=contacts, rescontacts=rescontacts, host_fold=host_fold)
    for f in ways.values():
        f()                                   # warm: code objects, workspaces
    times = {k: [] for k in ways}

    def timed(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ways[k]()
        times[k].append(1e3 * (time.perf_counter() - t0))

    for i in range(reps):
        for k in (("contacts", "rescontacts") if i % 2 == 0 else ("rescontacts", "contacts")):      # taken in turn
            timed(k)
    for _ in range(reps):
        timed("host_fold")
    ctx.close()
    assert rows["host"] == rows["Q"], (rows["host"], rows["Q"])      # the two folds have the same rows
    med = {k: float(np.median(v)) for k, v in times.items()}
    added = med["rescontacts"] - med["contacts"]
    print(json.dumps(dict(workload=name, alg="sr%d" % n_points, atoms=n, structures=ns, groups=G, residues=int(len(res_first) - 1), pairs=P, pair_atoms=M,
                          buried_dots=D, rows=Cn, folded_rows=rows["Q"], reps=reps, ms={k: round(v, 3) for k, v in med.items()},
                          ms_min={k: round(float(np.min(v)), 3) for k, v in times.items()},
                          ms_max={k: round(float(np.max(v)), 3) for k, v in times.items()}, ms_added=round(added, 3),
                          added_over_contacts=round(added / med["contacts"], 4), ms_host_fold_added=round(med["host_fold"] - med["contacts"], 3),
                          folded_table_bytes=8 * (2 * P + 1) + 28 * rows["Q"])), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--copies", type=int, default=40, help="globules on the ring (24 to 60)")
    ap.add_argument("--atoms", type=int, default=2000)
    ap.add_argument("--tetramers", type=int, default=250)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    if fa.device_count() <= 0:
        sys.exit("no HIP device: this benchmark measures nothing without one")
    n_ring = args.copies * args.atoms
    ring_res = np.unique(np.concatenate([np.arange(0, n_ring, 8), np.arange(0, n_ring + 1, args.atoms)])).astype(np.int64)
    run("ring-%dx%d" % (args.copies, args.atoms), ring(args.copies, args.atoms, 1), ring_res, args.points, args.reps)
    run("2jo4x%d" % args.tetramers, tetramers(args.tetramers), tetramer_residues(args.tetramers), args.points, args.reps)


if __name__ == "__main__":
    main()
