"""TESTS ONLY: chain groups among periodic images as include/freesasa_gpu.h (freesasa_gpu_groups_periodic_dev) defines them,
restated in numpy from the restatements of its two parents - tests/pbc_ref.py / tests/pbc_tri_ref.py (the expansion of one
structure in one cell) and a host cut of the groups - and the seeded batches of tests/test_groups_pbc.py and
tests/test_groups_pbc_gpu.py.

    combined   the complexes as they are, then every group (s, g) in structure-major order as a structure of its own: the
               atoms of s with id g, in input order, radii unchanged
    cells      every combined structure has the cell of its complex
    expanded   every combined structure expanded on its own by the periodic restatement - so the cutoff c = 2 (max radius +
               probe) of a group structure is that of ITS atoms - wrapped atoms first, then the images in the documented order
    sasa[i]    the area of atom i of its complex's expanded structure
    iso[i]     the area of i's place in its group's expanded structure; an atom with id -1: sasa[i]
    cgath      the complex area of every combined atom: what the groups' complex totals are summed from
"""
import os

import numpy as np

import pbc_ref
import pbc_tri_ref

PROBE = 1.4


def cut(offsets, group, n_groups):
    """the host cut -> (comb [ns + G + 1] the combined batch's offsets, src [n_iso] the input atom of every isolated atom,
    gbase [ns + 1] the first group of every structure, cplx [ns + G] the complex of every combined structure)"""
    offsets, group = np.asarray(offsets, dtype=np.int64), np.asarray(group, dtype=np.int32)
    n_groups = np.asarray(n_groups, dtype=np.int64)
    ns = offsets.size - 1
    gbase = np.concatenate([[0], np.cumsum(n_groups)]).astype(np.int64)
    comb, src, cplx = list(offsets), [], list(range(ns))
    for s in range(ns):
        a, b = int(offsets[s]), int(offsets[s + 1])
        ids = group[a:b]
        if ids.size and (ids.min() < -1 or ids.max() >= n_groups[s]):
            raise ValueError("group ids are -1 .. n_groups[s] - 1")
        for g in range(int(n_groups[s])):
            members = a + np.flatnonzero(ids == g)                 # (ascending: input order)
            src.extend(int(i) for i in members)
            comb.append(comb[-1] + members.size)
            cplx.append(s)
    return np.array(comb, dtype=np.int64), np.array(src, dtype=np.int32), gbase, np.array(cplx, dtype=np.int64)


def combined(xyz, radii, offsets, group, n_groups):
    """-> (cxyz [N, 3], cradii [N], comb, src, gbase, cplx)"""
    xyz, radii = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(radii, dtype=np.float64)
    comb, src, gbase, cplx = cut(offsets, group, n_groups)
    return np.vstack([xyz, xyz[src]]), np.concatenate([radii, radii[src]]), comb, src, gbase, cplx


def expanded(xyz, radii, offsets, group, n_groups, cells, probe=PROBE):
    """for every complex and every group the expanded structure -> (exyz, eradii, eoff [ns + G + 1], images [ns + G], comb, src,
    gbase, cplx).  cells [ns, 3]: orthorhombic; [ns, 6]: triclinic."""
    cells = np.asarray(cells, dtype=np.float64)
    one = pbc_ref.expand if cells.shape[1] == 3 else pbc_tri_ref.expand
    cxyz, cradii, comb, src, gbase, cplx = combined(xyz, radii, offsets, group, n_groups)
    ex, er, eo, ni = [np.zeros((0, 3))], [np.zeros(0)], [0], []
    for k in range(comb.size - 1):
        a, b = int(comb[k]), int(comb[k + 1])
        x, r, m = one(cxyz[a:b], cradii[a:b], cells[cplx[k]], probe)
        ex.append(np.asarray(x).reshape(-1, 3)); er.append(r); ni.append(m); eo.append(eo[-1] + (b - a) + m)
    return np.vstack(ex), np.concatenate(er), np.array(eo, dtype=np.int64), np.array(ni, dtype=np.int64), comb, src, gbase, cplx


def slots(offsets, group, comb, eoff, src):
    """which expanded atom each real atom's two areas come from -> (slot of sasa [n], slot of iso [n])"""
    offsets, group = np.asarray(offsets, dtype=np.int64), np.asarray(group, dtype=np.int32)
    ns, n = offsets.size - 1, int(offsets[-1])
    s_of = np.searchsorted(offsets, np.arange(n), side="right") - 1 if n else np.zeros(0, dtype=np.int64)
    # (searchsorted on offsets with empty structures: "right" - 1 gives the LAST s with offsets[s] <= i, the one that holds i)
    slot_sasa = eoff[s_of] + (np.arange(n) - offsets[s_of])
    slot_iso = slot_sasa.copy()
    for k in range(ns, comb.size - 1):
        a, b = int(comb[k]), int(comb[k + 1])
        slot_iso[src[a - n:b - n]] = eoff[k] + np.arange(b - a)
    assert np.all(slot_iso[group < 0] == slot_sasa[group < 0])
    return slot_sasa, slot_iso


def finish(esasa, offsets, group, comb, eoff, src):
    """-> (sasa [n], iso [n], carea [N] the compact combined areas, cgath [N] the complex area of every combined atom)"""
    esasa = np.asarray(esasa, dtype=np.float64)
    n = int(offsets[-1])
    slot_sasa, slot_iso = slots(offsets, group, comb, eoff, src)
    sasa, iso = esasa[slot_sasa], esasa[slot_iso]
    carea = np.concatenate([esasa[eoff[k]:eoff[k] + comb[k + 1] - comb[k]] for k in range(comb.size - 1)] + [np.zeros(0)])
    return sasa, iso, carea, np.concatenate([sasa, sasa[src]])


def group_structures(xyz, radii, offsets, group, n_groups, cells):
    """the groups cut out on the host as a batch of their own, each with its complex's cell -> (xyz, radii, offsets [G + 1],
    cells [G, W], src)"""
    cxyz, cradii, comb, src, gbase, cplx = combined(xyz, radii, offsets, group, n_groups)
    ns, n = len(offsets) - 1, int(offsets[-1])
    return cxyz[n:], cradii[n:], comb[ns:] - n, np.asarray(cells, dtype=np.float64)[cplx[ns:]], src


# ---------------------------------------------------------------- the batch of the CPU tests

SMALL_CELL = (7.0, 7.5, 8.0)           # every edge in [c, 2 c) for c = 6.8: an atom mid-cell admits all 26 images


def _ids(rng, n, sizes, free):
    """n ids in a shuffled order: sizes[g] atoms of group g, `free` atoms with -1"""
    ids = np.concatenate([np.full(k, g, dtype=np.int32) for g, k in enumerate(sizes)] + [np.full(free, -1, dtype=np.int32)])
    assert ids.size == n
    rng.shuffle(ids)
    return ids


def batch(seed=20261019):
    """-> (xyz, radii, offsets, group, n_groups, cells [5, 3]).  Five structures:
      0   20 atoms, 0 groups (every id -1)                                       cell (30, 9, 50)
      1   300 atoms: groups of 257 (one more than PBC_B: its image scan crosses a step), 0, 1 and 30 atoms, 12 atoms with -1,
          the ids shuffled (a stable cut is not a copy)                          cell (12, 14, 16): Lx < 2 c
      2   no atoms, but one (empty) group: an empty structure between full ones  (its cell is never read: NaN)
      3   5 atoms in SMALL_CELL, the first of radius 2.0 mid-cell, one cell away, a group of its own: 26 images in the complex
          AND on its own; the others the second group
      4   40 atoms, two groups of 20, half of the atoms outside the cell         cell (30, 9, 50)"""
    rng = np.random.default_rng(seed)
    sizes = (20, 300, 0, 5, 40)
    cells = np.array([(30.0, 9.0, 50.0), (12.0, 14.0, 16.0), (np.nan,) * 3, SMALL_CELL, (30.0, 9.0, 50.0)])
    parts = [pbc_ref.structure(n, c if n else (1.0, 1.0, 1.0), seed + k) for k, (n, c) in enumerate(zip(sizes, cells))]
    xyz, radii = np.vstack([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    radii[offsets[1]] = 2.0                                        # (c = 6.8 for the 300)
    radii[offsets[3]] = 2.0
    xyz[offsets[3]] = (3.5 + 7.0, 3.75 - 7.5, 4.0)
    group = np.concatenate([np.full(20, -1, dtype=np.int32), _ids(rng, 300, (257, 0, 1, 30), 12), np.zeros(0, dtype=np.int32),
                            np.array([0, 1, 1, 1, 1], dtype=np.int32), _ids(rng, 40, (20, 20), 0)])
    return xyz, radii, offsets, group, np.array([0, 4, 1, 2, 2], dtype=np.int32), cells


def triclinic_cells(cells):
    """the batch's cells as six numbers, right-angled - but structure 1's: the skewed cell of tests/pbc_tri_ref.py (widths 8.2,
    10.9, 15 against c = 6.8)"""
    cells = np.asarray(cells, dtype=np.float64)
    out = np.zeros((cells.shape[0], 6))
    out[:, 0], out[:, 2], out[:, 5] = cells[:, 0], cells[:, 1], cells[:, 2]
    out[1] = pbc_tri_ref.SKEWED
    return out


# ---------------------------------------------------------------- the batch of the GPU tests

PDB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdb")


def dimer():
    """chains A and B of 2jo4 (129 atoms each), centred on the origin -> (xyz [258, 3], radii, ids)"""
    from freesasa_amd import ingest
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    ids = np.asarray(b.chain_groups(separate_chains=True)[0], dtype=np.int32)
    keep = np.flatnonzero(ids < 2)
    xyz = np.asarray(b.xyz, dtype=np.float64).reshape(-1, 3)[keep]
    return xyz - np.round(xyz.mean(0)), np.asarray(b.radii, dtype=np.float64)[keep], ids[keep]


def blob(n, extent, seed):
    """n atoms with radii 1.2 .. 2.0 spread over a box of `extent` centred on the origin - astride the faces at 0 of any cell, at
    a protein's density where extent holds about 40 A^3 per atom: a system with a surface"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.0, (n, 3)) - 0.5) * np.asarray(extent, dtype=np.float64), rng.uniform(1.2, 2.0, n)


def gpu_batch(seed=20261019):
    """-> (xyz, radii, offsets, group, n_groups, cells [6, 3]).  Four structures of 300 to 600 atoms, an empty one and a tiny one:
      0   2jo4 (516 atoms), its four chains a group each, astride the faces at 0 of a cell 3 A wider than its extent
      1   400 atoms, 0 groups                                                    cell (30, 28, 34) around a blob of (24, 24, 30)
      2   no atoms, one (empty) group
      3   300 atoms, a blob of (11, 24, 24) in (13.2, 30, 30) - Lx in [c, 2 c) for c = 6.8: atoms with both shifts on x -, groups
          of 257, 0, 1 and 30 atoms, 12 with -1, shuffled; the group of one has radius 2.0
      4   600 atoms, three groups of 200                                          cell (38, 30, 33) around a blob of (34, 26, 30)
      5   tests/groups_pbc_ref.batch's five atoms in SMALL_CELL (every edge in [c, 2 c)): the first, of radius 2.0, mid-cell and a
          group of its own - 26 images in the complex and on its own"""
    from freesasa_amd import ingest
    rng = np.random.default_rng(seed)
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    x0 = np.asarray(b.xyz, dtype=np.float64).reshape(-1, 3)
    g0 = np.asarray(b.chain_groups(separate_chains=True)[0], dtype=np.int32)
    sizes = (516, 400, 0, 300, 600, 5)
    cells = np.array([tuple(np.ceil(x0.max(0) - x0.min(0)) + 3.0), (30.0, 28.0, 34.0), (np.nan,) * 3, (13.2, 30.0, 30.0), (38.0, 30.0, 33.0),
                      SMALL_CELL])
    parts = [(x0, np.asarray(b.radii, dtype=np.float64)), blob(400, (24.0, 24.0, 30.0), seed + 1), blob(0, (1.0, 1.0, 1.0), seed + 2),
             blob(300, (11.0, 24.0, 24.0), seed + 3), blob(600, (34.0, 26.0, 30.0), seed + 4), pbc_ref.structure(5, SMALL_CELL, seed + 5)]
    xyz, radii = np.vstack([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g3 = _ids(rng, 300, (257, 0, 1, 30), 12)
    radii[int(offsets[3] + np.flatnonzero(g3 == 2)[0])] = 2.0
    radii[offsets[5]] = 2.0
    xyz[offsets[5]] = (3.5 + 7.0, 3.75 - 7.5, 4.0)
    group = np.concatenate([g0, np.full(400, -1, dtype=np.int32), g3, _ids(rng, 600, (200, 200, 200), 0), np.array([0, 1, 1, 1, 1], dtype=np.int32)])
    return xyz, radii, offsets, group, np.array([4, 0, 1, 4, 3, 2], dtype=np.int32), cells
