#!/usr/bin/env python3
"""The residue contact occupancy map of a run: freesasa_amd.contact_occupancy against the path a caller had before it - the same
frames, in the same chunks, through calc_interface_contacts(res_first=) with every table copied to the host (docs: DESIGN.md
section 10, contact occupancy; profiles/contact_occupancy_bench.md).

The system: two chains of --atoms / 2 atoms each, jittered lattices at a protein's density (22 A^3 an atom, radii 1.5 .. 1.9) in
residues of 8 atoms, face to face; --frames frames in which every atom jitters and chain B slides along the face.  Shrake-Rupley at
--points points.  A host clock around synchronous calls (each ends in a stream synchronization), one warm pass of both ways over
the first chunk, then the two ways taken in turn per repetition, the one that goes first changing; medians:
  occupancy   contact_occupancy(frames, ...): open, add_frames over all frames, table, close
  batches     per chunk of the same frames_per_batch frames calc_interface_contacts(..., res_first=): its three calls (pairs,
              counts, arrays) and every table on the host; the merge of the tables, which the caller then has to do in Python,
              is NOT in this time
and once, untimed, the batches' rows re-keyed and reduced by tests/contact_occupancy_ref.py against the table (--check).
--only occupancy: that way alone, for a kernel trace of its own.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import freesasa_amd as fa  # noqa: E402


def system(n_atoms, n_frames, seed=20261023):
    """(frames [F, n, 3], radii, group, n_groups, res_first)"""
    rng = np.random.default_rng(seed)
    half = n_atoms // 2
    side = int(round((half / 10.0) ** 0.5))
    half = side * side * 10
    grid = np.array([[x, y, z] for x in range(10) for y in range(side) for z in range(side)], float) * 2.8
    a = grid + rng.normal(0, 0.3, grid.shape)
    b = grid + rng.normal(0, 0.3, grid.shape) + np.array([10 * 2.8 + 3.0, 0.0, 0.0])
    radii = rng.uniform(1.5, 1.9, 2 * half)
    group = np.repeat(np.arange(2, dtype=np.int32), half)
    res_first = np.unique(np.concatenate([np.arange(0, 2 * half, 8), [half, 2 * half]])).astype(np.int64)
    frames = np.empty((n_frames, 2 * half, 3))
    for f in range(n_frames):
        slide = np.array([0.5 * np.sin(f / 40.0), 6.0 * f / max(n_frames - 1, 1), 0.0])
        frames[f] = np.concatenate([a, b + slide]) + rng.normal(0, 0.25, (2 * half, 3))
    return frames, radii, group, 2, res_first


def batches(frames, radii, group, n_groups, res_first, n_points, fpb):
    """the parent's path: the folded tables of every chunk on the host (a list of InterfaceContacts)"""
    n, out = radii.size, []
    for f0 in range(0, len(frames), fpb):
        x = frames[f0:f0 + fpb]
        F = len(x)
        brf = np.concatenate([res_first[:-1] + f * n for f in range(F)] + [[F * n]]).astype(np.int64)
        out.append(fa.calc_interface_contacts(x.reshape(-1, 3), np.tile(radii, F), np.arange(F + 1, dtype=np.int64) * n, np.tile(group, F),
                                              np.full(F, n_groups, np.int32), n_points=n_points, res_first=brf))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--atoms", type=int, default=2880)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--frames-per-batch", type=int, default=0, help="0: the accumulator's default, 1250000 / (3 atoms) + 1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("occupancy",), default=None)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if fa.device_count() <= 0:
        sys.exit("no HIP device: this benchmark measures nothing without one")
    frames, radii, group, G, res_first = system(args.atoms, args.frames)
    n = radii.size
    fpb = args.frames_per_batch or 1250000 // (3 * n) + 1
    ways = dict(occupancy=lambda x: fa.contact_occupancy(x, radii, group, G, res_first, n_points=args.points, frames_per_batch=fpb),
                batches=lambda x: batches(x, radii, group, G, res_first, args.points, fpb))
    if args.only:
        ways = {args.only: ways[args.only]}
    for f in ways.values():
        f(frames[:fpb])                         # warm: code objects, workspaces
    times, last = {k: [] for k in ways}, {}
    for i in range(args.reps):
        for k in (list(ways) if i % 2 == 0 else list(ways)[::-1]):
            t0 = time.perf_counter()
            last[k] = ways[k](frames)
            times[k].append(1e3 * (time.perf_counter() - t0))
    t = last["occupancy"]
    out = dict(atoms=n, residues=int(res_first.size - 1), frames=len(frames), frames_per_batch=fpb, alg="sr%d" % args.points, reps=args.reps,
               table_rows=t.n_rows, table_bytes=96 * t.n_rows, ms={k: round(float(np.median(v)), 2) for k, v in times.items()},
               ms_min={k: round(float(np.min(v)), 2) for k, v in times.items()}, ms_max={k: round(float(np.max(v)), 2) for k, v in times.items()})
    if "batches" in last:
        out["folded_rows"] = int(sum(b.n_rescontacts for b in last["batches"]))
        out["batch_table_bytes"] = int(sum(sum(a.nbytes for a in (b.pair_struct, b.pair_groups, b.pair_areas, b.side_offsets, b.pair_atom, b.pair_buried,
                                                                   b.contact_first, b.contact_partner, b.contact_points, b.contact_area, b.buried_masks,
                                                                   b.rescontact_offsets, b.rescontact_residues, b.rescontact_counts, b.rescontact_area,
                                                                   b.rescontact_reverse)) for b in last["batches"]))
        out["occupancy_over_batches"] = round(out["ms"]["occupancy"] / out["ms"]["batches"], 4)
    if args.check and "batches" in last:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import contact_occupancy_ref as occ
        rows, n_res = [], res_first.size - 1
        for k, b in enumerate(last["batches"]):
            F = min(fpb, len(frames) - k * fpb)
            rows += occ.frames_of_batch(F, n_res, b.pair_struct, b.pair_groups, b.rescontact_offsets, b.rescontact_residues, b.rescontact_counts,
                                        b.rescontact_area)
        want = occ.reduce(rows)
        out["equals_the_python_reduction"] = bool(all(getattr(t, c).tobytes() == want[c].tobytes() for c in occ.COLUMNS))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
