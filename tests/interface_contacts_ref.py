"""A numpy restatement of the atom-atom contact tables of the interfaces between chain groups (include/freesasa_gpu.h,
freesasa_gpu_interface_contacts_dev): the two sets of exposure masks, the buried masks, the partner of every buried test point and
the rows - and the CONTACT EDGE BATCH the tests of tests/test_interface_contacts.py and tests/test_interface_contacts_gpu.py run on,
with what it has to hold (coverage()).  Fed only from tests/volume_ref.py (exposed_mask), tests/dots_ref.py and
tests/interfaces_ref.py (table, pair_structures); never from the entry under test.  Every operation is numpy's, rounded on its own.

    side_mask_i    atom i's exposed points with its side a structure of its own;  pair_mask_i: in the pair structure
    buried_mask_i  side_mask_i & ~pair_mask_i
    test point     t = u_k * R_i; t += x_i                                 (dots_ref.dots)
    cover          dx * dx + dy * dy + dz * dz <= R_j * R_j, dx = t_x - x_j   (volume_ref.exposed_mask), j of the other side
    partner        the covering j with the smallest w = (dx * dx + dy * dy + dz * dz) - R_j * R_j, the lowest j among equals
    rows           per (i, j) with n >= 1 points, i ascending, then j ascending: area = (4.0 * pi * R_i * R_i * n) / N
"""
import functools
import math

import numpy as np

import dots_ref as dr
import interfaces_ref as ir
import volume_ref as vr

PROBE = 1.4
WORKGROUP = 256       # CT_B (csrc/contact_kernels.h): dots per workgroup and atoms per LDS tile of contact_attribute
N_POINTS = (1, 31, 32, 33, 100, 128)
COVERAGE_N = 100      # the point count the grazing cover is made for and coverage() looks at


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def unit_points(n_points):
    import freesasa_amd as fa
    return np.asarray(fa.test_points(n_points), dtype=np.float64).reshape(-1, 3)


def masks(pxyz, pradii, side_offsets, probe, unit):
    """(side_mask, pair_mask) [M, N] bool of the pair batch: its atoms as 2 P structures and as P"""
    pxyz, R = np.asarray(pxyz, np.float64).reshape(-1, 3), np.asarray(pradii, np.float64) + probe
    M = len(R)
    side, pair = np.zeros((M, len(unit)), bool), np.zeros((M, len(unit)), bool)
    for q in range(len(side_offsets) - 1):
        b, e = side_offsets[q], side_offsets[q + 1]
        side[b:e] = vr.exposed_mask(pxyz[b:e], R[b:e], unit)
    for p in range((len(side_offsets) - 1) // 2):
        b, e = side_offsets[2 * p], side_offsets[2 * p + 2]
        pair[b:e] = vr.exposed_mask(pxyz[b:e], R[b:e], unit)
    return side, pair


def contacts(pxyz, pradii, side_offsets, probe, unit, side_mask, pair_mask):
    """the table of the pair batch: a dict of buried_masks [M, 4] uint32, dot_first [M + 1], dot_atom, dot_point, dot_partner [D_b],
    contact_first [M + 1] int64, contact_partner, contact_points [C] int32, contact_area [C] fp64, tie_dots (the dots whose
    smallest w two atoms share) and cover_counts [D_b]"""
    pxyz, R = np.asarray(pxyz, np.float64).reshape(-1, 3), np.asarray(pradii, np.float64) + probe
    M, N = len(R), len(unit)
    assert not (pair_mask & ~side_mask).any()          # a point exposed in the pair structure is exposed in the side alone
    buried = dr.masks_of(side_mask & ~pair_mask)
    first = dr.dot_first(buried, N)
    t, atom, point = dr.dots(pxyz, pradii, probe, unit, buried)
    partner = np.full(len(atom), -1, np.int32)
    ties, covers = [], np.zeros(len(atom), np.int64)
    R2 = R * R
    for q in range(len(side_offsets) - 1):
        d0, d1 = first[side_offsets[q]], first[side_offsets[q + 1]]
        if d0 == d1:
            continue
        o0, o1 = side_offsets[q ^ 1], side_offsets[(q ^ 1) + 1]
        dx = t[d0:d1, 0][:, None] - pxyz[o0:o1, 0][None, :]
        dy = t[d0:d1, 1][:, None] - pxyz[o0:o1, 1][None, :]
        dz = t[d0:d1, 2][:, None] - pxyz[o0:o1, 2][None, :]
        s = dx * dx + dy * dy
        s = s + dz * dz
        cov = s <= R2[o0:o1][None, :]
        assert cov.any(axis=1).all(), "a buried point without a cover on the other side"
        w = np.where(cov, s - R2[o0:o1][None, :], np.inf)
        best = np.argmin(w, axis=1)                    # (the first of equal minima: the lowest j)
        partner[d0:d1] = o0 + best
        covers[d0:d1] = cov.sum(axis=1)
        ties.extend(d0 + np.nonzero((w == w.min(axis=1)[:, None]).sum(axis=1) > 1)[0])
    cf, cp, cn, ca = [0], [], [], []
    for i in range(M):
        js, ns = np.unique(partner[first[i]:first[i + 1]], return_counts=True)
        for j, n in zip(js, ns):
            cp.append(int(j)); cn.append(int(n))
            ca.append((4.0 * math.pi * float(R[i]) * float(R[i]) * int(n)) / N)
        cf.append(len(cp))
    return dict(buried_masks=buried, dot_first=first, dot_atom=atom, dot_point=point, dot_partner=partner,
                contact_first=np.array(cf, np.int64), contact_partner=np.array(cp, np.int32), contact_points=np.array(cn, np.int32),
                contact_area=np.array(ca, np.float64), tie_dots=np.array(ties, np.int64), cover_counts=covers)


def _cloud(rng, count, corner, per_atom=40.0):
    edge = np.cbrt(per_atom * max(count, 1))
    return np.asarray(corner, float) + rng.uniform(0, edge, (count, 3)), rng.uniform(1.0, 2.0, count)


@functools.lru_cache(maxsize=None)
def contacts_edge_batch():
    """(xyz [n, 3], radii [n], offsets, group [n] int32, n_groups int32, names: the structures' kinds)"""
    rng = np.random.default_rng(20261020)
    structs, names = [], []

    def add(name, x, r, g, ng):
        structs.append((np.asarray(x, float).reshape(-1, 3), np.asarray(r, float), np.asarray(g, np.int32), ng)); names.append(name)

    # sides of one atom; the two lie along y, so at N = 1 (the point (1, 0, 0) R) the pair is in contact and buries no point
    add("one-atom-sides", [[0, 0, 0], [0, 3.0, 0]], [1.5, 1.5], [0, 1], 2)
    # a small atom wholly inside a large partner atom: all its points buried, one row
    add("inside", [[0, 0, 0], [2.0, 0, 0]], [8.0, 0.1], [0, 1], 2)
    # an atom with six partners around it
    x = [[0, 0, 0]] + [list(3.4 * np.eye(3)[k] * s) for k in range(3) for s in (1, -1)]
    add("six-partners", x, [2.0] + [1.2] * 6, [0] + [1] * 6, 2)
    # an exact tie: two partner atoms with identical coordinates and radius
    add("tie", [[0, 0, 0], [3.0, 0.5, 0], [3.0, 0.5, 0]], [1.6, 1.7, 1.7], [0, 1, 1], 2)
    # a group that is in three pairs, and a fifth group in none
    parts = [_cloud(rng, 30, (0, 0, 0)), _cloud(rng, 20, (9, 0, 0)), _cloud(rng, 20, (0, 9, 0)), _cloud(rng, 20, (0, 0, 9)), _cloud(rng, 10, (80, 80, 80))]
    add("three-pairs", np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
        np.concatenate([np.full(len(p[1]), k) for k, p in enumerate(parts)]), 5)
    # a structure with no pair
    add("no-pair", [[0, 0, 0], [50.0, 0, 0]], [1.5, 1.5], [0, 1], 2)
    # a side with many more than 256 buried dots: two groups interleaved in one cloud
    x, r = _cloud(rng, 120, (0, 0, 0), 60.0)
    add("big-sides", x, r, np.arange(120) % 2, 2)
    # ten tiny pairs (dimers far from each other) whose dots share a workgroup
    x = np.array([[30.0 * k, 0, 0] if s == 0 else [30.0 * k, 4.9, 0] for k in range(10) for s in (0, 1)])
    add("tiny-pairs", x, np.full(20, 1.5), np.arange(20), 20)
    # another side of 620 atoms whose only cover is its last atom, in the third LDS tile
    far, rf = _cloud(rng, 619, (40, 40, 40))
    add("last-tile", np.concatenate([[[0, 0, 0]], far, [[3.1, 0, 0]]]), np.concatenate([[1.5], rf, [1.5]]), [0] + [1] * 620, 2)
    # a cover whose sphere reaches one test point of its partner (and so the box of its dots) by 5e-7 A, at COVERAGE_N points
    u = unit_points(COVERAGE_N)[37]
    Ra, Rb = 1.5 + PROBE, 1.8 + PROBE
    t = u * Ra
    add("grazing", [[0, 0, 0], list(t + u * (Rb - 5e-7))], [1.5, 1.8], [0, 1], 2)

    xyz = np.concatenate([t[0] for t in structs]); radii = np.concatenate([t[1] for t in structs])
    group = np.concatenate([t[2] for t in structs]); n_groups = np.array([t[3] for t in structs], np.int32)
    for a in (xyz, radii, group, n_groups):
        a.setflags(write=False)
    return xyz, radii, _offsets([len(t[1]) for t in structs]), group, n_groups, tuple(names)


@functools.lru_cache(maxsize=None)
def edge_table():
    """the edge batch's pair table (interfaces_ref.table): pair_struct, pair_groups, side_offsets, pair_atom"""
    xyz, radii, offsets, group, n_groups, _ = contacts_edge_batch()
    t = ir.table(xyz, radii, offsets, group, n_groups)
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def edge_contacts(n_points):
    """the edge batch's masks and table at n_points: (side_mask, pair_mask, contacts(...)); computed once, read-only"""
    xyz, radii, offsets, group, n_groups, _ = contacts_edge_batch()
    _, _, so, pa = edge_table()
    px, pr, _ = ir.pair_structures(xyz, radii, so, pa)
    unit = unit_points(n_points)
    side, pair = masks(px, pr, so, PROBE, unit)
    c = contacts(px, pr, so, PROBE, unit, side, pair)
    for a in (side, pair) + tuple(c.values()):
        a.setflags(write=False)
    return side, pair, c


def coverage():
    """what the edge batch holds, decided on this restatement alone: {kind: bool}"""
    xyz, radii, offsets, group, n_groups, names = contacts_edge_batch()
    ps, pg, so, pa = edge_table()
    side, pair, c = edge_contacts(COVERAGE_N)
    first, cf = c["dot_first"], c["contact_first"]
    P, M = len(ps), len(pa)
    pair_of = lambda name: [p for p in range(P) if ps[p] == names.index(name)]
    sizes = np.diff(so)
    rows_of = np.diff(cf)
    out = {}
    p = pair_of("one-atom-sides")
    out["sides of one atom"] = bool(len(p) == 1 and sizes[2 * p[0]] == 1 and sizes[2 * p[0] + 1] == 1 and first[so[2 * p[0] + 2]] > first[so[2 * p[0]]])
    p = pair_of("inside")[0]
    small = so[2 * p + 1]
    out["a small atom wholly inside its partner"] = bool(first[small + 1] - first[small] == COVERAGE_N and rows_of[small] == 1)
    side128, pair128, c128 = edge_contacts(128)
    out["... 128 buried points, one row"] = bool(c128["dot_first"][small + 1] - c128["dot_first"][small] == 128 and np.diff(c128["contact_first"])[small] == 1)
    out["an atom with at least 4 partners"] = bool(rows_of.max() >= 4)
    p = pair_of("tie")[0]
    tied = c["tie_dots"]
    out["an exact tie, the lower index wins"] = bool(len(tied) > 0 and np.all(c["dot_partner"][tied] == so[2 * p + 1]) and
                                                     np.all((tied >= first[so[2 * p]]) & (tied < first[so[2 * p + 1]])))
    _, _, c1 = edge_contacts(1)
    p = pair_of("one-atom-sides")[0]
    out["a pair in contact that buries no point at N = 1"] = bool(c1["dot_first"][so[2 * p + 2]] == c1["dot_first"][so[2 * p]])
    s = names.index("three-pairs")
    in_pairs = np.bincount(pg[ps == s].reshape(-1), minlength=5)
    out["a group in three pairs"] = bool(in_pairs.max() >= 3)
    out["a structure with no pair"] = bool(not (ps == names.index("no-pair")).any() and n_groups[names.index("no-pair")] == 2)
    dots_of_side = first[so[1:]] - first[so[:-1]]
    dot_side = np.searchsorted(so, c["dot_atom"], side="right") - 1
    edges = np.arange(WORKGROUP, first[M], WORKGROUP)
    out["a side with more than 256 buried dots"] = bool(dots_of_side.max() > WORKGROUP)
    out["a workgroup boundary inside a side and inside an atom's run"] = bool(
        np.any((dot_side[edges - 1] == dot_side[edges]) & (c["dot_atom"][edges - 1] == c["dot_atom"][edges])))
    blocks = np.arange(first[M]) // WORKGROUP
    out["six tiny pairs in one workgroup"] = bool(max(len(set(dot_side[blocks == b] // 2)) for b in range(blocks.max() + 1)) >= 6)
    p = pair_of("last-tile")[0]
    a0 = so[2 * p]
    partners = c["contact_partner"][cf[a0]:cf[a0 + 1]]
    out["more than 600 atoms, the only cover in the last tile"] = bool(
        sizes[2 * p + 1] > 600 and len(partners) == 1 and partners[0] == so[2 * p + 2] - 1 and
        (partners[0] - so[2 * p + 1]) // WORKGROUP == (sizes[2 * p + 1] - 1) // WORKGROUP >= 2)
    p = pair_of("grazing")[0]
    a0, b0 = so[2 * p], so[2 * p + 1]
    px, pr, _ = ir.pair_structures(xyz, radii, so, pa)
    dots = dr.dots(px, pr, PROBE, unit_points(COVERAGE_N), c["buried_masks"])[0][first[a0]:first[a0 + 1]]
    if len(dots):
        lo, hi = dots.min(axis=0), dots.max(axis=0)
        gap = np.maximum(np.maximum(lo - px[b0], px[b0] - hi), 0.0)
        reach = (pr[b0] + PROBE) - float(np.sqrt((gap * gap).sum()))
        out["a cover that reaches the dots' box by less than 1e-6"] = bool(0.0 < reach < 1e-6)
    else:
        out["a cover that reaches the dots' box by less than 1e-6"] = False
    return out
