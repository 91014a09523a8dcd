#!/usr/bin/env python3
"""What a topology costs the trajectory file driver (freesasa_gpu_trajectory_file_topology): frames of a 100 000-atom solvated
system (fp32, page cache warm) whose solute is a 10 000-atom poly-alanine globule at the front of every frame, the other
90 000 atoms solvent that the gather drops on the device.  Arms, alternating, each run after one warm-up pass:

    plain     trajectory_file on frames of the 10 000 solute atoms alone, totals only (what a caller who strips the
              solvent on the host would run; the stripping itself is not timed)
    totals    trajectory_file_topology on the full frames, totals only
    all       ... with class sums, per-residue areas (2000 residues) and 8 selections
    groups    ... totals and the chain groups' areas (isolated, complex, buried per frame): the solute cut into two groups of
              5 000 atoms, group areas only - against `totals` this is what the groups cost
    longway   the same numbers without the driver's groups: per shard-sized run of frames the host reads the full frames,
              strips the solvent, widens to fp64 and calls calc_groups with the ids repeated per frame (per-atom areas come back)

With --dcd the arms are instead
    raw       `totals` above: the raw fp32 file
    dcd       the same call on a little-endian DCD file with a unit-cell record that holds the same fp32 values (12 N + 80 bytes
              per frame against 12 N; de-planarized, gathered and widened by one kernel on the device)
timed in one process, interleaved; the totals files must be identical.
With --netcdf (alone or beside --dcd) one arm more, interleaved with the others:
    netcdf    the same call on an AMBER NetCDF file (64-bit offset, written here) whose records hold the time, the same fp32 values
              big-endian and the cell: 12 N + 52 bytes per frame; byte-swapped, gathered and widened by one kernel on the device

With --pbc the arms are the periodic images of the DCD drivers (FREESASA_GPU_FRAMES_PBC) against the same call without the bit,
on two DCD files with a unit-cell record:
    solvated      the 100 000-atom frames above moved into the cell [0, 2 half)^3, the solute mid-box and further than c from
                  every face (almost no images: the cost of the stage itself), trajectory_file_topology, totals only
    solvated-pbc  the same call with pbc=True
    filled        frames of the 10 000 solute atoms alone in a cell one lattice spacing wider than their extent: the kept atoms
                  fill the box (the expansion factor decides the cost, about ((L + 2 c) / L)^3), trajectory_file, totals only
    filled-pbc    the same call with pbc=True
each line with images_per_atom (calc_periodic on frame 0; null where the library has no periodic entry).  --pbc-arms off runs the
two arms without the bit alone and passes no pbc keyword: the form an older library's wrapper takes, for a baseline.
With --triclinic beside --pbc (FREESASA_GPU_FRAMES_TRICLINIC) three arms more, interleaved with the others:
    solvated-tri  solvated-pbc with triclinic=True: the same right-angled records through the general geometry (the totals file
    filled-tri    must be that of the arm without the bit, byte for byte) - its price at an equal image count
    octa-tri      the frames of `filled` in a truncated octahedron of the same volume as filled's cell (box vectors of length d
                  at GROMACS's angles, the record's angles as cosines 1/3, -1/3, 1/3), pbc=True, triclinic=True; images_per_atom
                  from calc_periodic_triclinic on frame 0.  The globule was not built for that cell: where its corners wrap onto
                  its faces atoms overlap, which a cost measurement can live with.

With --groups beside --pbc three arms more, all on the filled box's frames and cells through the topology entries, the solute cut
into two groups of 5 000 atoms, totals and group areas only:
    filled-topo-pbc    freesasa_gpu_trajectory_file_topology with pbc=True: the plain periodic run
    filled-groups      the chain groups' run without the bit: isolated, complex, buried of a system that is not periodic
    filled-groups-pbc  freesasa_gpu_trajectory_file_groups_periodic: chain groups among periodic images - its totals file must be
                       filled-topo-pbc's, byte for byte
each line with real_atoms, group_atoms and image_atoms (the images of the complex and of its groups in frame 0): the atoms per
frame in the engine.  With --interfaces beside --pbc --groups two arms more (and with --interface-residues a third), the one pair of the two groups:
    filled-interfaces              freesasa_gpu_trajectory_file_interfaces without the bit
    filled-interfaces-pbc          freesasa_gpu_trajectory_file_interfaces_periodic: its totals and group areas must be filled-groups-pbc's
    filled-interface-residues-pbc  freesasa_gpu_trajectory_file_interface_residues_periodic, min_buried = 0
each line with pair_atoms and, in image_atoms, the pair structure's images as well.  engine_atoms_per_frame is the sum of the four: the
atoms per frame the engine sees.
With --netcdf beside --pbc two arms more: `solvated` and `solvated-pbc` on an AMBER NetCDF file of the same frames and cell
(solvated-nc, solvated-nc-pbc); their totals files must be those of the DCD arms, byte for byte.

With --xtc the system is instead 10 000 atoms of water-like runs (3333 groups of an oxygen and two hydrogens within 0.1 nm of it,
and one atom more), no topology, and the arms are three files of the same decoded frames, interleaved:
    raw       trajectory_file on the raw fp32 file
    netcdf    ... on an AMBER NetCDF file of them
    xtc       ... on a GROMACS XTC file: --xtc-distinct frames encoded by tests/xtc_codec.py (precision 1000) and repeated up to
              --frames, since frames are independent; scanned and unpacked on the device
each line with the host CPU time of the process per atom-frame; the totals files must be identical.  --xtc-fpb sets
frames_per_batch for all three arms (0: the driver's default).

With --trr the system is the same water-like 10 000 atoms and the arms are two files of the same frames, interleaved:
    raw       trajectory_file on the raw frame file a TRR file of that precision stands in for: fp32 (Angstrom, rounded once more)
              for a single-precision TRR, fp64 (float64(x_nm) * 10.0, the very numbers) with --double
    trr       ... on a GROMACS TRR file written by tests/trr_codec.py (box and coordinates per record), single precision or, with
              --double, double: --xtc-distinct frames repeated up to --frames; gathered, byte-swapped and scaled on the device
each line with the host CPU time of the process per atom-frame; with --double the totals files must be identical, in single
precision equal to fp32 rounding.  --trr-arms raw times the raw arm alone (a library without TRR input); --xtc-fpb as above.

With --stats the frames are those of the 10 000 solute atoms alone (fp32, no solvent, the topology the whole frame) and the arms are
what a caller who wants the averages over the run can do, interleaved:
    totals    trajectory_file_topology, totals only (the floor: nothing per atom leaves the device)
    stream    ... with the per-atom file (fp64 [F, n]): the stream-out a host-side reduction needs (the reduction itself is not timed)
    stats     ... with stats=("atoms", "residues") and no per-atom file: mean, std, min, max per atom and per residue column, reduced on
              the device shard by shard (k_traj_stats), 4 W doubles per shard down
each line with the bytes of results per frame; the stats arm's per-atom means must be those of the stream arm's file to rounding.

With --groups (without --pbc) the solute is the same globule labelled as four chains A, B, C, D of 500 residues (2 500 atoms), in the
same solvated frames, and the arms are, interleaved, totals and the named outputs only:
    groups      trajectory_file_topology with separate_chains=True: isolated, complex, buried of the four chains per frame
    interfaces  (with --interfaces beside it) the same with interface_pairs="all": the six pairs' rows per frame as well
each line with frames_per_batch, the shards of the run and the median time per shard, and engine_atoms_per_frame: the atoms of a
frame, of its isolated groups and of its pair structures that go through the engine (n + n_iso + n_pair).  --kernel-stats FILE: a
`rocprofv3 --kernel-trace --stats` kernel-stats CSV of a run of this mode; the share of the kernels the pairs add (k_traj_pair_*
and k_totals, which sums the sides) in the kernel time of the whole trace goes into the interfaces line as new_kernels_share.
    interface-residues        (with --interface-residues beside --interfaces) the same with pair_residues_path and min_buried = 0: the dense
                              per-residue table [F, S, 4] as well (one kernel more, k_traj_pair_res, and 4 S doubles per frame down)
    interface-residues-stats  (with --stats beside those) stats=("pairs", "pair_residues") and neither pair file: mean, std, min, max of
                              the 6 K + 4 S columns - the occupancy among them - from the statistics alone; its means must be those of
                              the interface-residues arm's files to rounding
the share of k_traj_pair_res alone goes into those two lines as pair_res_kernel_share.

One JSON line per arm: atom-frames/s counted in SOLUTE atoms and in frame atoms, the median and the spread of --reps runs.

    python tools/traj_topology_bench.py [--frames 240] [--reps 5] [--arms plain,totals,all,groups,longway] [--scratch DIR] [--out FILE] [--dcd] [--netcdf] [--pbc [--pbc-arms all|off] [--triclinic] [--groups [--interfaces [--interface-residues]]]] [--xtc [--xtc-distinct 24] [--xtc-fpb 0]] [--trr [--double] [--trr-arms raw,trr]] [--stats] [--groups [--interfaces [--interface-residues [--stats]]] [--kernel-stats FILE]]

For the kernel times: `rocprofv3 --kernel-trace --stats -- python tools/traj_topology_bench.py --reps 1 --arms all`
(k_traj_gather / k_traj_residues / k_traj_class / k_traj_sel are the topology's kernels, k_traj_group_* the groups')."""
import argparse
import json
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import freesasa_amd as fa          # noqa: E402
import tools                       # noqa: E402
from freesasa_amd import ingest    # noqa: E402

N_SOLUTE, N_FRAME = 10_000, 100_000
EIGHT = ["bb, name n+ca+c+o", "cb, name cb", "r, resi 10-200 and not symbol c", "open, resi -50 or resi 1900-", "ch, chain A",
         "o, symbol o", "n, symbol n and resi 500-1500", "none, resn gly"]


def solute(n_chains=1):
    """a poly-alanine of 2000 residues on the positions of tools.globule: (batch of one structure, xyz [n, 3]); n_chains: the
    residues labelled as that many chains A, B, ... of equal length"""
    xyz, _ = tools.globule(N_SOLUTE, 11)
    xyz = xyz - xyz.mean(0)
    names = [(" N  ", "N"), (" CA ", "C"), (" C  ", "C"), (" O  ", "O"), (" CB ", "C")]
    lines = []
    for i, (x, y, z) in enumerate(xyz):
        nm, el = names[i % 5]
        lines.append("ATOM  %5d %s ALA %s%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s" % ((i + 1) % 100000, nm, "ABCDEFGH"[i * n_chains // N_SOLUTE], i // 5 + 1,
                                                                                          x, y, z, el))
    b = ingest.load_pdb_texts(["\n".join(lines) + "\nEND\n"])
    assert b.status[0] == 0 and b.n_atoms == N_SOLUTE and b.n_residues == N_SOLUTE // 5
    return b, b.xyz.copy()


def dcd_header(n_atoms, n_frames):
    """a little-endian CHARMM-style DCD header: a unit cell per frame, no 4th dimension, one title line"""
    rec = lambda body: struct.pack("<i", len(body)) + body + struct.pack("<i", len(body))
    icntrl = [0] * 20
    icntrl[0], icntrl[1], icntrl[2], icntrl[3], icntrl[10], icntrl[19] = n_frames, 1, 1, n_frames, 1, 24
    return rec(b"CORD" + struct.pack("<20i", *icntrl)) + rec(struct.pack("<i", 1) + b"REMARKS traj_topology_bench".ljust(80)) + rec(struct.pack("<i", n_atoms))


def nc_header(n_atoms, n_frames):
    """a NetCDF classic header (64-bit offset) in the AMBER trajectory convention: a record holds time (fp32), coordinates (fp32),
    cell_lengths and cell_angles (fp64), all big-endian"""
    name = lambda t: struct.pack(">i", len(t)) + t.encode() + b"\0" * (-len(t) % 4)
    text = lambda k, v: name(k) + struct.pack(">ii", 2, len(v)) + v.encode() + b"\0" * (-len(v) % 4)
    dims = [("frame", 0), ("spatial", 3), ("atom", n_atoms), ("cell_spatial", 3), ("cell_angular", 3)]
    gatts = [("Conventions", "AMBER"), ("ConventionVersion", "1.0"), ("program", "traj_topology_bench")]
    variables = [("time", (0,), 5, 4), ("coordinates", (0, 2, 1), 5, 12 * n_atoms), ("cell_lengths", (0, 3), 6, 24), ("cell_angles", (0, 4), 6, 24)]
    head = b"CDF\x02" + struct.pack(">iii", n_frames, 0x0A, len(dims)) + b"".join(name(d) + struct.pack(">i", n) for d, n in dims)
    head += struct.pack(">ii", 0x0C, len(gatts)) + b"".join(text(k, v) for k, v in gatts) + struct.pack(">ii", 0x0B, len(variables))
    metas = [name(v) + struct.pack(">i", len(d)) + b"".join(struct.pack(">i", k) for k in d) + b"\0" * 8 + struct.pack(">ii", t, size)
             for v, d, t, size in variables]
    begin = len(head) + sum(len(m) + 8 for m in metas)
    for m, v in zip(metas, variables):
        head += m + struct.pack(">q", begin)
        begin += v[3]
    return head


def nc_record(f, frame, cell):
    return struct.pack(">f", f) + frame.astype(">f4").tobytes() + np.array(list(cell) + [90.0] * 3).astype(">f8").tobytes()


def make_frames(scratch, xyz, n_frames, dcd=False, nc=False):
    full, bare, as_dcd = os.path.join(scratch, "solvated.f32"), os.path.join(scratch, "solute.f32"), os.path.join(scratch, "solvated.dcd")
    as_nc = os.path.join(scratch, "solvated.nc")
    rng = np.random.default_rng(5)
    half = 1.3 * np.abs(xyz).max()
    plane = struct.pack("<i", 4 * N_FRAME)
    cell = struct.pack("<i", 48) + np.array([2 * half, 0, 2 * half, 0, 0, 2 * half]).astype("<f8").tobytes() + struct.pack("<i", 48)
    with open(full, "wb") as f_full, open(bare, "wb") as f_bare, open(as_dcd if dcd else os.devnull, "wb") as f_dcd, \
            open(as_nc if nc else os.devnull, "wb") as f_nc:
        f_dcd.write(dcd_header(N_FRAME, n_frames))
        f_nc.write(nc_header(N_FRAME, n_frames))
        for f in range(n_frames):
            s = (xyz + rng.uniform(-0.25, 0.25, xyz.shape)).astype(np.float32)
            w = rng.uniform(-half, half, (N_FRAME - N_SOLUTE, 3)).astype(np.float32)
            s.tofile(f_bare)
            frame = np.concatenate([s, w])
            frame.tofile(f_full)
            if dcd:
                f_dcd.write(cell + b"".join(plane + np.ascontiguousarray(frame[:, k]).tobytes() + plane for k in range(3)))
            if nc:
                f_nc.write(nc_record(f, frame, [2 * half] * 3))
    return full, bare, as_dcd, as_nc


def make_pbc_frames(scratch, xyz, n_frames, octa=False, nc=False):
    """the two DCD files of --pbc -> (solvated path, its cell, filled path, its cell); coordinates as make_frames draws them,
    moved so that the cell begins at 0.  octa: behind them the path of a third file - filled's frames with the record of a
    truncated octahedron of filled's volume - and that record.  nc: beside the solvated file an AMBER NetCDF file of the same frames
    and cell, solvated_pbc.nc"""
    rng = np.random.default_rng(5)
    half = 1.3 * np.abs(xyz).max()
    lo = xyz.min(0) - 0.5 * 2.6 - 0.25
    edge = (xyz.max(0) - xyz.min(0)) + 2.6 + 0.5
    out = []
    for name, n, shift, cell in (("solvated_pbc.dcd", N_FRAME, half, np.full(3, 2 * half)), ("filled_pbc.dcd", N_SOLUTE, -lo, edge)):
        path = os.path.join(scratch, name)
        plane = struct.pack("<i", 4 * n)
        rec = struct.pack("<i", 48) + np.array([cell[0], 0, cell[1], 0, 0, cell[2]]).astype("<f8").tobytes() + struct.pack("<i", 48)
        with open(path, "wb") as fh, open(os.path.join(scratch, "solvated_pbc.nc") if nc and n > N_SOLUTE else os.devnull, "wb") as f_nc:
            fh.write(dcd_header(n, n_frames))
            f_nc.write(nc_header(n, n_frames))
            for f in range(n_frames):
                frame = (xyz + rng.uniform(-0.25, 0.25, xyz.shape) + shift).astype(np.float32)
                if n > N_SOLUTE:
                    frame = np.concatenate([frame, rng.uniform(0, 2 * half, (n - N_SOLUTE, 3)).astype(np.float32)])
                fh.write(rec + b"".join(plane + np.ascontiguousarray(frame[:, k]).tobytes() + plane for k in range(3)))
                if nc and n > N_SOLUTE:
                    f_nc.write(nc_record(f, frame, cell))
        out += [path, cell]
    if octa:
        d = float(np.prod(out[3]) / (4.0 * np.sqrt(3.0) / 9.0)) ** (1.0 / 3.0)     # the volume of GROMACS's cell of vector length d is 4 sqrt(3) / 9 d^3
        record = np.array([d, 1.0 / 3.0, d, -1.0 / 3.0, 1.0 / 3.0, d])
        data = bytearray(open(out[2], "rb").read())
        info = fa.dcd_info(out[2])
        for f in range(n_frames):
            struct.pack_into("<6d", data, info.first_frame + f * info.frame_bytes + 4, *record)
        path = os.path.join(scratch, "octa_pbc.dcd")
        with open(path, "wb") as fh:
            fh.write(bytes(data))
        out += [path, record]
    return out


def first_frame(path, n):
    """the first n atoms of frame 0 of a little-endian DCD file with a cell record, widened"""
    info = fa.dcd_info(path)
    raw = np.fromfile(path, dtype=np.uint8, count=info.frame_bytes, offset=info.first_frame)
    return np.stack([raw[info.x_off + k * info.plane_bytes:][:4 * n].view("<f4") for k in range(3)], axis=1).astype(np.float64)


def long_way(full, b, ids, n_frames, out_path):
    """group areas of every frame through calc_groups on host-tiled batches of the driver's default shard length"""
    fpb = 1250000 // N_FRAME + 1
    areas = np.empty((n_frames, 2, 3))
    frames = np.memmap(full, dtype=np.float32, mode="r", shape=(n_frames, N_FRAME, 3))
    for f0 in range(0, n_frames, fpb):
        nf = min(fpb, n_frames - f0)
        xyz = np.ascontiguousarray(frames[f0:f0 + nf, :N_SOLUTE], dtype=np.float64).reshape(-1, 3)
        offs = np.arange(nf + 1, dtype=np.int64) * N_SOLUTE
        _, _, _, gt = fa.calc_groups(xyz, np.tile(b.radii, nf), offs, np.tile(ids, nf), np.full(nf, 2, np.int32))
        areas[f0:f0 + nf] = gt.reshape(nf, 2, 3)
    areas.tofile(out_path)
    return True, n_frames


def xtc_mode(args, scratch):
    """the three arms of --xtc -> the JSON lines"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import xtc_codec as xc
    n, mol = N_SOLUTE, N_SOLUTE // 3
    rng = np.random.default_rng(9)
    plan = [(2, 0)] * mol + [(0, 0)] * (n - 3 * mol)
    box = np.diag([4.64, 4.64, 4.64])
    coded, decoded = [], []
    for f in range(args.xtc_distinct):
        big = rng.integers(0, 4640, (mol + n - 3 * mol, 3))
        h1 = big[:mol] + rng.integers(-100, 101, (mol, 3))
        h2 = h1 + rng.integers(-160, 161, (mol, 3))
        ints = np.concatenate([np.stack([h1, big[:mol], h2], axis=1).reshape(-1, 3), big[mol:]])        # (output order: small, big, small)
        coded.append(xc.encode(ints, 1000.0, box=box, plan=plan, smallidx=33, step=f, time=float(f)))      # (magicints[33] / 2 = 1024 > 160)
        decoded.append(xc.to_angstrom(ints, 1000.0))
    p = lambda k: os.path.join(scratch, k)
    half = 23.2
    with open(p("water.xtc"), "wb") as f_xtc, open(p("water.f32"), "wb") as f_raw, open(p("water.nc"), "wb") as f_nc:
        f_nc.write(nc_header(n, args.frames))
        for f in range(args.frames):
            f_xtc.write(coded[f % len(coded)])
            decoded[f % len(decoded)].tofile(f_raw)
            f_nc.write(nc_record(f, decoded[f % len(decoded)], [2 * half] * 3))
    info = fa.xtc_info(p("water.xtc"))
    assert info.n_frames == args.frames and info.n_atoms == n
    radii = np.tile([1.1, 1.52, 1.1], mol + 1)[:n].astype(np.float64)
    kw = dict(frames_per_batch=args.xtc_fpb)
    arms = {"raw": lambda: fa.trajectory_file(p("water.f32"), radii, p("x0"), f32=True, **kw),
            "netcdf": lambda: fa.trajectory_file(p("water.nc"), radii, p("x1"), netcdf=True, **kw),
            "xtc": lambda: fa.trajectory_file(p("water.xtc"), radii, p("x2"), xtc=True, **kw)}
    runs, cpu = {a: [] for a in arms}, {a: [] for a in arms}
    for a in arms:
        arms[a]()                                                        # warm-up: contexts, staging, page cache
    for _ in range(args.reps):
        for a in arms:
            t0, c0 = time.perf_counter(), time.process_time()
            res = arms[a]()
            runs[a].append(time.perf_counter() - t0)
            cpu[a].append(time.process_time() - c0)
            assert res[0] and res[1] == args.frames
    totals = [np.fromfile(p(k)) for k in ("x0", "x1", "x2")]
    assert all(np.array_equal(t, totals[0]) for t in totals) and np.all(totals[0] > 0)
    lines = []
    for a in arms:
        v, c = sorted(runs[a]), sorted(cpu[a])
        med = v[len(v) // 2]
        lines.append(json.dumps({"arm": a, "frames": args.frames, "frame_atoms": n, "frames_per_batch": args.xtc_fpb, "file_bytes_per_frame":
                                 os.path.getsize(p({"raw": "water.f32", "netcdf": "water.nc", "xtc": "water.xtc"}[a])) / args.frames,
                                 "median_seconds": med, "min_seconds": v[0], "max_seconds": v[-1], "atom_frames_per_s": n * args.frames / med,
                                 "host_cpu_ns_per_atom_frame": 1e9 * c[len(c) // 2] / (n * args.frames), "runs": len(v)}))
    return lines


def trr_mode(args, scratch):
    """the arms of --trr -> the JSON lines"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import trr_codec as tc
    n, mol = N_SOLUTE, N_SOLUTE // 3
    rng = np.random.default_rng(9)
    box = np.diag([4.64, 4.64, 4.64])
    real = np.float64 if args.double else np.float32
    coded, raw = [], []
    for f in range(args.xtc_distinct):
        big = rng.integers(0, 4640, (mol + n - 3 * mol, 3))
        h1 = big[:mol] + rng.integers(-100, 101, (mol, 3))
        h2 = h1 + rng.integers(-160, 161, (mol, 3))
        x_nm = np.concatenate([np.stack([h1, big[:mol], h2], axis=1).reshape(-1, 3), big[mol:]]) / 1000.0
        coded.append(tc.record_bytes(n, double=args.double, x=x_nm, box=box, step=f, t=float(f)))
        raw.append((x_nm.astype(real).astype(np.float64) * 10.0).astype(real))                           # (--double: what the TRR run computes on)
    p = lambda k: os.path.join(scratch, k)
    with open(p("water.trr"), "wb") as f_trr, open(p("water.raw"), "wb") as f_raw:
        for f in range(args.frames):
            f_trr.write(coded[f % len(coded)])
            raw[f % len(raw)].tofile(f_raw)
    radii = np.tile([1.1, 1.52, 1.1], mol + 1)[:n].astype(np.float64)
    kw = dict(frames_per_batch=args.xtc_fpb)
    arms = {"raw": lambda: fa.trajectory_file(p("water.raw"), radii, p("x0"), f32=not args.double, **kw),
            "trr": lambda: fa.trajectory_file(p("water.trr"), radii, p("x1"), trr=True, **kw)}
    arms = {a: arms[a] for a in args.trr_arms.split(",")}
    if "trr" in arms:
        info = fa.trr_info(p("water.trr"))
        assert info.n_frames == args.frames and info.n_atoms == n and info.real_bytes == (8 if args.double else 4)
    runs, cpu = {a: [] for a in arms}, {a: [] for a in arms}
    for a in arms:
        arms[a]()                                                        # warm-up: contexts, staging, page cache
    for _ in range(args.reps):
        for a in arms:
            t0, c0 = time.perf_counter(), time.process_time()
            res = arms[a]()
            runs[a].append(time.perf_counter() - t0)
            cpu[a].append(time.process_time() - c0)
            assert res[0] and res[1] == args.frames
    if len(arms) == 2:
        t_raw, t_trr = np.fromfile(p("x0")), np.fromfile(p("x1"))
        assert np.all(t_raw > 0) and (np.array_equal(t_raw, t_trr) if args.double else np.allclose(t_raw, t_trr, rtol=1e-5, atol=0))
    lines = []
    for a in arms:
        v, c = sorted(runs[a]), sorted(cpu[a])
        med = v[len(v) // 2]
        lines.append(json.dumps({"arm": a + ("-f64" if args.double else "-f32"), "frames": args.frames, "frame_atoms": n, "frames_per_batch": args.xtc_fpb,
                                 "file_bytes_per_frame": os.path.getsize(p({"raw": "water.raw", "trr": "water.trr"}[a])) / args.frames,
                                 "median_seconds": med, "min_seconds": v[0], "max_seconds": v[-1], "atom_frames_per_s": n * args.frames / med,
                                 "host_cpu_ns_per_atom_frame": 1e9 * c[len(c) // 2] / (n * args.frames), "runs": len(v)}))
    return lines


def stats_mode(args, scratch):
    """the three arms of --stats -> the JSON lines"""
    b, xyz = solute()
    p = lambda k: os.path.join(scratch, k)
    rng = np.random.default_rng(5)
    with open(p("solute.f32"), "wb") as fh:
        for f in range(args.frames):
            (xyz + rng.uniform(-0.25, 0.25, xyz.shape)).astype(np.float32).tofile(fh)
    R = b.n_residues
    arms = {"totals": lambda: fa.trajectory_file_topology(p("solute.f32"), b, p("t0"), f32=True),
            "stream": lambda: fa.trajectory_file_topology(p("solute.f32"), b, p("t1"), f32=True, sasa_path=p("a1")),
            "stats": lambda: fa.trajectory_file_topology(p("solute.f32"), b, p("t2"), f32=True, stats=("atoms", "residues"),
                                                         stats_path=p("s2"), partials_path=p("p2"))}
    runs = {a: [] for a in arms}
    for a in arms:
        arms[a]()                                                        # warm-up: contexts, staging, page cache
    for _ in range(args.reps):
        for a in arms:
            t0 = time.perf_counter()
            res = arms[a]()
            runs[a].append(time.perf_counter() - t0)
            assert res[0] and res[1] == args.frames
    totals = [np.fromfile(p(k)) for k in ("t0", "t1", "t2")]
    assert all(np.array_equal(t, totals[0]) for t in totals) and np.all(totals[0] > 0)
    got = fa.traj_stats_read(p("s2"), ("atoms", "residues"), N_SOLUTE, R)
    areas = np.memmap(p("a1"), dtype=np.float64, mode="r", shape=(args.frames, N_SOLUTE))
    assert np.allclose(got["atoms"][0], areas.mean(0), rtol=1e-12, atol=1e-12) and np.array_equal(got["atoms"][3], areas.max(0))
    out_bytes = {"totals": 8, "stream": 8 + 8 * N_SOLUTE, "stats": 8 + os.path.getsize(p("p2")) / args.frames}
    lines = []
    for a in arms:
        v = sorted(runs[a])
        med = v[len(v) // 2]
        lines.append(json.dumps({"arm": a, "frames": args.frames, "frame_atoms": N_SOLUTE, "result_bytes_per_frame": out_bytes[a],
                                 "median_seconds": med, "min_seconds": v[0], "max_seconds": v[-1],
                                 "atom_frames_per_s": N_SOLUTE * args.frames / med, "runs": len(v)}))
    return lines


def new_kernels_share(path, only=None):
    """the share of k_traj_pair_* and k_totals (only: of that kernel alone, or of a tuple of kernels) in the kernel time of a rocprofv3 kernel-stats CSV
    (columns Name, ..., TotalDurationNs)"""
    import csv
    new = total = 0.0
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            ns = float(row["TotalDurationNs"])
            total += ns
            name = row["Name"].split("(")[0]
            if (name in only if isinstance(only, tuple) else name == only) if only else name.startswith("k_traj_pair_") or name == "k_totals":
                new += ns
    return new / total if total else None


def groups_mode(args, scratch):
    """the arms of --groups [--interfaces] -> the JSON lines"""
    b, xyz = solute(4)
    full = make_frames(scratch, xyz, args.frames)[0]
    index = np.arange(N_SOLUTE, dtype=np.int32)
    p = lambda k: os.path.join(scratch, k)
    kw = dict(atom_index=index, frame_atoms=N_FRAME, f32=True, separate_chains=True)
    arms = {"groups": lambda: fa.trajectory_file_topology(full, b, p("t0"), group_areas_path=p("g0"), **kw)}
    if args.interfaces:
        arms["interfaces"] = lambda: fa.trajectory_file_topology(full, b, p("t1"), group_areas_path=p("g1"), interface_pairs="all",
                                                                 pair_areas_path=p("p1"), **kw)
    ids, ng, _ = b.chain_groups(separate_chains=True)
    G = int(ng[0])
    assert G == 4 and np.array_equal(np.bincount(ids), [N_SOLUTE // 4] * 4)
    K, n_pair = G * (G - 1) // 2, (G - 1) * N_SOLUTE
    S = 0
    if args.interface_residues:
        S = fa.traj_pair_segments(b, ids, G, [(g, h) for g in range(G) for h in range(g + 1, G)])[1].size
        assert S == (G - 1) * b.n_residues
        arms["interface-residues"] = lambda: fa.trajectory_file_topology(full, b, p("t2"), group_areas_path=p("g2"), interface_pairs="all",
                                                                         pair_areas_path=p("p2"), pair_residues_path=p("r2"), min_buried=0.0, **kw)
        if args.stats:
            arms["interface-residues-stats"] = lambda: fa.trajectory_file_topology(full, b, p("t3"), group_areas_path=p("g3"), interface_pairs="all",
                                                                                   min_buried=0.0, stats=("pairs", "pair_residues"),
                                                                                   stats_path=p("s3"), partials_path=p("q3"), **kw)
    runs = {a: [] for a in arms}
    for a in arms:
        arms[a]()                                                        # warm-up: contexts, staging, page cache
    for _ in range(args.reps):
        for a in arms:
            t0 = time.perf_counter()
            res = arms[a]()
            runs[a].append(time.perf_counter() - t0)
            assert res[0] and res[1] == args.frames
    if args.interfaces:
        assert np.array_equal(np.fromfile(p("t1")), np.fromfile(p("t0"))) and np.array_equal(np.fromfile(p("g1")), np.fromfile(p("g0")))
        rows, areas = np.fromfile(p("p1")).reshape(args.frames, K, 6), np.fromfile(p("g0")).reshape(args.frames, G, 3)
        assert np.array_equal(rows[:, 0, 0], areas[:, 0, 0]) and np.array_equal(rows[:, K - 1, 1], areas[:, G - 1, 0]) and np.all(rows[:, :, 4:] >= -1e-6)
    if args.interface_residues:
        assert np.array_equal(np.fromfile(p("t2")), np.fromfile(p("t0"))) and np.array_equal(np.fromfile(p("p2")), np.fromfile(p("p1")))
        table = np.fromfile(p("r2")).reshape(args.frames, S, 4)
        assert np.all(table[:, :, 2] == table[:, :, 0] - table[:, :, 1]) and np.array_equal(table[:, :, 3], (table[:, :, 2] > 0.0).astype(np.float64))
        if args.stats:
            got = fa.traj_stats_read(p("s3"), ("pairs", "pair_residues"), N_SOLUTE, b.n_residues, 0, G, n_pairs=K, n_segments=S)
            assert np.allclose(got["pair_residues"][0], table.mean(0), rtol=1e-12, atol=1e-12) and np.array_equal(got["pair_residues"][3], table.max(0))
            assert np.allclose(got["pairs"][0], np.fromfile(p("p2")).reshape(args.frames, K, 6).mean(0), rtol=1e-12, atol=1e-12)
    lines = []
    for a in arms:
        v = sorted(runs[a])
        med = v[len(v) // 2]
        engine = 2 * N_SOLUTE + (n_pair if a != "groups" else 0)
        fpb = 1250000 // max(N_FRAME, engine) + 1                        # (the driver's default: include/freesasa_gpu.h)
        shards = -(-args.frames // fpb)
        line = {"arm": a, "frames": args.frames, "frame_atoms": N_FRAME, "solute_atoms": N_SOLUTE, "groups": G, "pairs": K if a != "groups" else 0,
                "segments": S if a.startswith("interface-residues") else 0,
                "result_bytes_per_frame": 8 + 24 * G + (48 * K if a in ("interfaces", "interface-residues") else 0) + (32 * S if a == "interface-residues" else 0)
                + (os.path.getsize(p("q3")) / args.frames if a == "interface-residues-stats" else 0),
                "frames_per_batch": fpb, "shards": shards, "engine_atoms_per_frame": engine, "median_seconds": med, "min_seconds": v[0],
                "max_seconds": v[-1], "median_ms_per_shard": 1e3 * med / shards, "solute_atom_frames_per_s": N_SOLUTE * args.frames / med,
                "engine_atom_frames_per_s": engine * args.frames / med, "runs": len(v)}
        if a == "interfaces" and args.kernel_stats:
            line["new_kernels_share"] = new_kernels_share(args.kernel_stats)
        if a.startswith("interface-residues") and args.kernel_stats:
            line["pair_res_kernel_share"] = new_kernels_share(args.kernel_stats, "k_traj_pair_res")
        lines.append(json.dumps(line))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--arms", default="plain,totals,all,groups,longway")
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dcd", action="store_true", help="time the raw fp32 file against a DCD file of the same frames")
    ap.add_argument("--netcdf", action="store_true", help="time the raw fp32 file (and with --dcd the DCD file) against an AMBER NetCDF file of the same "
                                                          "frames; with --pbc: the solvated arms on a NetCDF file as well")
    ap.add_argument("--pbc", action="store_true", help="time the DCD drivers with and without periodic images")
    ap.add_argument("--pbc-arms", default="all", choices=["all", "off"])
    ap.add_argument("--triclinic", action="store_true", help="with --pbc: the arms of the triclinic bit beside the others")
    ap.add_argument("--groups", action="store_true", help="with --pbc: chain groups among periodic images against the plain periodic run and the non-periodic groups' run; "
                                                          "without: the solute as four chains, a group each")
    ap.add_argument("--interfaces", action="store_true", help="with --groups: the interfaces between all pairs of the four chains beside the groups' run; "
                                                             "with --pbc --groups: the interfaces between the two groups without and among periodic images")
    ap.add_argument("--interface-residues", action="store_true", help="with --groups --interfaces: the per-residue interface tables beside them; with --stats as well: "
                                                                      "the statistics of both pair outputs with neither delivered")
    ap.add_argument("--kernel-stats", default=None, help="with --groups --interfaces: a rocprofv3 kernel-stats CSV; the share of the pairs' kernels in it is reported "
                                                           "(with --pbc: of k_gpbc_cells and k_gpbc_finish, the phases that carry the pair part)")
    ap.add_argument("--xtc", action="store_true", help="time a GROMACS XTC file against the raw fp32 file and an AMBER NetCDF file of the same decoded frames")
    ap.add_argument("--xtc-distinct", type=int, default=24, help="with --xtc: distinct frames that are encoded and then repeated")
    ap.add_argument("--xtc-fpb", type=int, default=0, help="with --xtc: frames_per_batch of all three arms (0: the driver's default)")
    ap.add_argument("--trr", action="store_true", help="time a GROMACS TRR file against the raw frame file of the same frames")
    ap.add_argument("--double", action="store_true", help="with --trr: a double-precision TRR file against the raw fp64 file (default: single against raw fp32)")
    ap.add_argument("--trr-arms", default="raw,trr", help="with --trr: the arms that run")
    ap.add_argument("--stats", action="store_true", help="time the run statistics against the per-atom stream-out and against totals only")
    args = ap.parse_args()
    scratch = args.scratch or tempfile.mkdtemp(prefix="traj_topology_bench_")
    try:
        if args.interfaces and not args.groups:
            ap.error("--interfaces goes with --groups")
        if args.interface_residues and not args.interfaces:
            ap.error("--interface-residues goes with --groups --interfaces")
        if args.xtc or args.stats or args.trr or (args.groups and not args.pbc):
            lines = groups_mode(args, scratch) if args.interface_residues and not args.pbc else stats_mode(args, scratch) if args.stats else trr_mode(args, scratch) if args.trr else xtc_mode(args, scratch) if args.xtc \
                else groups_mode(args, scratch)
            print("\n".join(lines))
            if args.out:
                with open(args.out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")
            return
        b, xyz = solute()
        full, bare, as_dcd, as_nc = make_frames(scratch, xyz, args.frames, args.dcd, args.netcdf) if not args.pbc else (None, None, None, None)
        sel = ingest.Selection(EIGHT)
        index = np.arange(N_SOLUTE, dtype=np.int32)
        ids = (np.arange(N_SOLUTE) >= N_SOLUTE // 2).astype(np.int32)
        p = lambda k: os.path.join(scratch, k)
        arms = {
            "plain": lambda: fa.trajectory_file(bare, b.radii, p("t0"), f32=True),
            "totals": lambda: fa.trajectory_file_topology(full, b, p("t1"), atom_index=index, frame_atoms=N_FRAME, f32=True),
            "all": lambda: fa.trajectory_file_topology(full, b, p("t2"), atom_index=index, frame_atoms=N_FRAME, f32=True, selection=sel,
                                                       class_sums_path=p("c2"), residues_path=p("r2"), selections_path=p("s2")),
            "groups": lambda: fa.trajectory_file_topology(full, b, p("t3"), atom_index=index, frame_atoms=N_FRAME, f32=True, group=ids, n_groups=2,
                                                          group_areas_path=p("g3")),
            "longway": lambda: long_way(full, b, ids, args.frames, p("g4")),
        }
        if args.dcd:
            arms = {"raw": arms["totals"],
                    "dcd": lambda: fa.trajectory_file_topology(as_dcd, b, p("t5"), atom_index=index, dcd=True)}
            assert fa.dcd_info(as_dcd).n_frames == args.frames and os.path.getsize(as_dcd) - os.path.getsize(full) == 80 * args.frames + 196
        if args.netcdf and not args.pbc:
            arms = {"raw": arms["raw" if args.dcd else "totals"], **({"dcd": arms["dcd"]} if args.dcd else {}),
                    "netcdf": lambda: fa.trajectory_file_topology(as_nc, b, p("t13"), atom_index=index, netcdf=True)}
            info = fa.nc_info(as_nc)
            assert info.n_frames == args.frames and info.record_bytes == 12 * N_FRAME + 52 and info.has_cell
        images = {}
        if args.pbc:
            tri = args.triclinic and args.pbc_arms == "all"
            solv, solv_cell, fill, fill_cell, *octa = make_pbc_frames(scratch, xyz, args.frames, tri, args.netcdf)
            solv_nc = os.path.join(scratch, "solvated_pbc.nc")
            arms = {"solvated": lambda: fa.trajectory_file_topology(solv, b, p("t6"), atom_index=index, dcd=True),
                    "filled": lambda: fa.trajectory_file(fill, b.radii, p("t8"), dcd=True)}
            if args.pbc_arms == "all":
                arms = {"solvated": arms["solvated"],
                        "solvated-pbc": lambda: fa.trajectory_file_topology(solv, b, p("t7"), atom_index=index, dcd=True, pbc=True),
                        "filled": arms["filled"],
                        "filled-pbc": lambda: fa.trajectory_file(fill, b.radii, p("t9"), dcd=True, pbc=True)}
            if tri:
                arms.update({"solvated-tri": lambda: fa.trajectory_file_topology(solv, b, p("t10"), atom_index=index, dcd=True, pbc=True, triclinic=True),
                             "filled-tri": lambda: fa.trajectory_file(fill, b.radii, p("t11"), dcd=True, pbc=True, triclinic=True),
                             "octa-tri": lambda: fa.trajectory_file(octa[0], b.radii, p("t12"), dcd=True, pbc=True, triclinic=True)})
            if args.groups and args.pbc_arms == "all":
                arms.update({"filled-topo-pbc": lambda: fa.trajectory_file_topology(fill, b, p("t16"), dcd=True, pbc=True),
                             "filled-groups": lambda: fa.trajectory_file_topology(fill, b, p("t17"), dcd=True, group=ids, n_groups=2,
                                                                                  group_areas_path=p("g17")),
                             "filled-groups-pbc": lambda: fa.trajectory_file_groups_periodic(fill, b, p("t18"), dcd=True, group=ids, n_groups=2,
                                                                                             group_areas_path=p("g18"))})
            if args.groups and args.interfaces and args.pbc_arms == "all":
                arms.update({"filled-interfaces": lambda: fa.trajectory_file_topology(fill, b, p("t19"), dcd=True, group=ids, n_groups=2, group_areas_path=p("g19"),
                                                                                      interface_pairs="all", pair_areas_path=p("p19")),
                             "filled-interfaces-pbc": lambda: fa.trajectory_file_groups_periodic(fill, b, p("t20"), dcd=True, group=ids, n_groups=2,
                                                                                                 group_areas_path=p("g20"), interface_pairs="all",
                                                                                                 pair_areas_path=p("p20"))})
                if args.interface_residues:
                    arms["filled-interface-residues-pbc"] = lambda: fa.trajectory_file_groups_periodic(
                        fill, b, p("t21"), dcd=True, group=ids, n_groups=2, group_areas_path=p("g21"), interface_pairs="all", pair_areas_path=p("p21"),
                        pair_residues_path=p("r21"), min_buried=0.0)
            if args.netcdf:
                arms["solvated-nc"] = lambda: fa.trajectory_file_topology(solv_nc, b, p("t14"), atom_index=index, netcdf=True)
                if args.pbc_arms == "all":
                    arms["solvated-nc-pbc"] = lambda: fa.trajectory_file_topology(solv_nc, b, p("t15"), atom_index=index, netcdf=True, pbc=True)
        names = list(arms) if args.dcd or args.netcdf or args.pbc else [a for a in args.arms.split(",") if a in arms]
        runs = {a: [] for a in names}
        for a in names:
            arms[a]()                                                    # warm-up: contexts, staging, page cache
        for _ in range(args.reps):
            for a in names:
                t0 = time.perf_counter()
                res = arms[a]()
                runs[a].append(time.perf_counter() - t0)
                assert res[0] and res[1] == args.frames
        if args.pbc and hasattr(fa, "calc_periodic"):    # (behind the timed runs: a batch of another shape leaves its launch history in a pooled context)
            for a, path, cell in (("solvated", solv, solv_cell), ("filled", fill, fill_cell)):
                k = fa.calc_periodic(first_frame(path, N_SOLUTE), b.radii, [0, N_SOLUTE], [cell])[2]
                images[a] = images[a + "-pbc"] = images[a + "-tri"] = images[a + "-nc"] = images[a + "-nc-pbc"] = float(k[0]) / N_SOLUTE
            if tri:
                k = fa.calc_periodic_triclinic(first_frame(octa[0], N_SOLUTE), b.radii, [0, N_SOLUTE], [fa.cell_from_dcd(octa[1])])[2]
                images["octa-tri"] = float(k[0]) / N_SOLUTE
        atoms = {}
        if "filled-groups-pbc" in names:  # the atoms per frame the engine sees in each of the three arms (frame 0)
            x0 = first_frame(fill, N_SOLUTE)
            k_c = int(fa.calc_periodic(x0, b.radii, [0, N_SOLUTE], [fill_cell])[2][0])
            k_g = int(fa.calc_periodic(np.concatenate([x0[ids == 0], x0[ids == 1]]), np.concatenate([b.radii[ids == 0], b.radii[ids == 1]]),
                                       [0, N_SOLUTE // 2, N_SOLUTE], [fill_cell, fill_cell])[2].sum())
            atoms = {"filled-topo-pbc": (N_SOLUTE, 0, k_c), "filled-groups": (N_SOLUTE, N_SOLUTE, 0), "filled-groups-pbc": (N_SOLUTE, N_SOLUTE, k_c + k_g)}
            assert np.array_equal(np.fromfile(p("t18")), np.fromfile(p("t16"))) and np.array_equal(np.fromfile(p("t18")), np.fromfile(p("t9")))
            assert not np.array_equal(np.fromfile(p("g18")), np.fromfile(p("g17")))
            images["filled-topo-pbc"] = images["filled-groups-pbc"] = images["filled-pbc"]
        if "filled-interfaces-pbc" in names:  # ... and with the one pair of the two groups: its pair structure holds the complex's atoms, group by group
            r, gi, ti = atoms["filled-groups-pbc"]
            atoms = {a: v + (0,) for a, v in atoms.items()}
            atoms["filled-interfaces"] = (r, gi, 0, N_SOLUTE)
            x0 = first_frame(fill, N_SOLUTE)
            order = np.concatenate([np.flatnonzero(ids == 0), np.flatnonzero(ids == 1)])
            k_p = int(fa.calc_periodic(x0[order], b.radii[order], [0, N_SOLUTE], [fill_cell])[2][0])
            atoms["filled-interfaces-pbc"] = atoms["filled-interface-residues-pbc"] = (r, gi, ti + k_p, N_SOLUTE)
            images["filled-interfaces-pbc"] = images["filled-interface-residues-pbc"] = images["filled-pbc"]
            # the outputs shared with the groups' periodic run are its bytes; the pairs' rows are those of the definition's columns
            assert np.array_equal(np.fromfile(p("t20")), np.fromfile(p("t18"))) and np.array_equal(np.fromfile(p("g20")), np.fromfile(p("g18")))
            rows, areas = np.fromfile(p("p20")).reshape(args.frames, 1, 6), np.fromfile(p("g20")).reshape(args.frames, 2, 3)
            assert np.array_equal(rows[:, 0, :2], areas[:, :, 0]) and np.array_equal(rows[:, 0, 4:], rows[:, 0, :2] - rows[:, 0, 2:4])
            assert not np.array_equal(rows, np.fromfile(p("p19")).reshape(args.frames, 1, 6))
            if "filled-interface-residues-pbc" in names:
                assert np.array_equal(np.fromfile(p("p21")), np.fromfile(p("p20")))
                table = np.fromfile(p("r21")).reshape(args.frames, -1, 4)
                assert np.all(table[:, :, 2] == table[:, :, 0] - table[:, :, 1]) and np.array_equal(table[:, :, 3], (table[:, :, 2] > 0.0).astype(np.float64))
        totals = [np.fromfile(p(k)) for a, k in (("plain", "t0"), ("totals", "t1"), ("all", "t2"), ("groups", "t3"), ("raw", "t1"), ("dcd", "t5"), ("netcdf", "t13")) if a in names]
        assert all(np.array_equal(t, totals[0]) for t in totals)
        if "solvated-pbc" in names:      # no atom of the solute within c of a face: the bit changes nothing; a filled box: it must
            assert images["solvated"] > 0 or np.array_equal(np.fromfile(p("t6")), np.fromfile(p("t7")))
            assert np.all(np.fromfile(p("t9")) < np.fromfile(p("t8")))
        if "solvated-nc" in names:       # the NetCDF arms: the files of the DCD arms
            assert np.array_equal(np.fromfile(p("t14")), np.fromfile(p("t6")))
            assert "solvated-nc-pbc" not in names or np.array_equal(np.fromfile(p("t15")), np.fromfile(p("t7")))
        if "filled-tri" in names:        # right-angled records through the general geometry: the files of the arms without bit 4
            assert np.array_equal(np.fromfile(p("t10")), np.fromfile(p("t7"))) and np.array_equal(np.fromfile(p("t11")), np.fromfile(p("t9")))
        assert not ("groups" in names and "longway" in names) or np.array_equal(np.fromfile(p("g3")), np.fromfile(p("g4")))
        lines = []
        for a in names:
            v = sorted(runs[a])
            med = v[len(v) // 2]
            frame_atoms = N_SOLUTE if a == "plain" or a.startswith("filled") or a.startswith("octa") else N_FRAME
            line = {"arm": a, "frames": args.frames, "frame_atoms": frame_atoms, "solute_atoms": N_SOLUTE,
                    "median_seconds": med, "min_seconds": v[0], "max_seconds": v[-1],
                    "solute_atom_frames_per_s": N_SOLUTE * args.frames / med,
                    "frame_atom_frames_per_s": frame_atoms * args.frames / med, "runs": len(v)}
            if args.pbc:
                line["images_per_atom"] = images.get(a)
            if a in atoms:
                line["real_atoms"], line["group_atoms"], line["image_atoms"] = atoms[a][:3]
                if len(atoms[a]) > 3:
                    line["pair_atoms"] = atoms[a][3]
                line["engine_atoms_per_frame"] = int(sum(atoms[a]))
            if a.startswith("filled-interface") and a.endswith("-pbc") and args.kernel_stats:
                line["new_kernels_share"] = new_kernels_share(args.kernel_stats, ("k_gpbc_cells", "k_gpbc_finish"))
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
