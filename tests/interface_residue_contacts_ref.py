"""A numpy restatement of the residue-residue contact tables of the interfaces between chain groups (include/freesasa_gpu.h,
freesasa_gpu_interface_residue_contacts_dev): the segments of the pair table's sides, the fold of the atom-atom contact rows per
partner residue with every sum an explicit sequential loop over Python numbers, rescontact_offsets and the reverse rows - and
the BATCH the tests of tests/test_interface_residue_contacts.py and tests/test_interface_residue_contacts_gpu.py run on: the
contact edge batch of tests/interface_contacts_ref.py with one structure appended (many-partners) and residue boundaries chosen
to give the cases coverage() lists.  Fed only from tests/interface_contacts_ref.py, tests/interfaces_ref.py and
tests/interface_residues_ref.py; never from the entry under test.

    segment       a maximal run of one side's pair-structure atoms whose input atoms lie in one residue (interface_residues_ref)
    folded rows   segment a with atoms b .. e-1 has the contact rows contact_first[b] .. contact_first[e] - 1; one folded row per
                  distinct residue of pair_atom[contact_partner[t]], ascending: n_rows, n_points = the sum of contact_points,
                  area = the sum of contact_area in row order, one addition at a time from 0
    reverse       the folded row of the partner segment whose partner is the source segment, or -1
"""
import functools

import numpy as np

import interface_contacts_ref as cr
import interface_residues_ref as rr
import interfaces_ref as ir

PROBE = cr.PROBE
N_POINTS = cr.N_POINTS
WAVE = 64
COVERAGE_N = (100, 128)   # the point counts at which coverage() asks for the large segments


def fold(side_offsets, pair_atom, res_first, contact_first, contact_partner, contact_points, contact_area):
    """the folded table: a dict of rescontact_offsets [2P + 1] int64, rescontact_residues [Q, 2] int32, rescontact_counts [Q, 2]
    int32, rescontact_area [Q] fp64, rescontact_reverse [Q] int32 - and, for the tests, seg_first [K + 1], row_seg [Q] (the source
    segment of every folded row), row_partner_seg [Q] and seg_rows [K] (the contact rows of every segment)"""
    side_offsets, cf = np.asarray(side_offsets, np.int64), np.asarray(contact_first, np.int64)
    heads, first, seg_res, seg_side = rr.segments(side_offsets, pair_atom, res_first)
    atom_seg = np.cumsum(heads) - 1
    K, n_sides = len(seg_res), len(side_offsets) - 1
    cp, cn, ca = [int(v) for v in contact_partner], [int(v) for v in contact_points], [float(v) for v in contact_area]
    res, cnt, area, row_seg, row_pseg, per_side = [], [], [], [], [], np.zeros(n_sides, np.int64)
    for a in range(K):
        r0, r1 = int(cf[first[a]]), int(cf[first[a + 1]])
        keys = [int(atom_seg[cp[t]]) for t in range(r0, r1)]
        for s in sorted(set(keys)):
            n_rows, n_points, total = 0, 0, 0.0
            for t, k in zip(range(r0, r1), keys):
                if k == s:
                    n_rows += 1
                    n_points += cn[t]
                    total += ca[t]
            res.append((int(seg_res[a]), int(seg_res[s]))); cnt.append((n_rows, n_points)); area.append(total)
            row_seg.append(a); row_pseg.append(s)
            per_side[seg_side[a]] += 1
    where = {(a, s): k for k, (a, s) in enumerate(zip(row_seg, row_pseg))}
    rev = [where.get((s, a), -1) for a, s in zip(row_seg, row_pseg)]
    return dict(rescontact_offsets=np.concatenate([[0], np.cumsum(per_side)]).astype(np.int64),
                rescontact_residues=np.array(res, np.int32).reshape(-1, 2), rescontact_counts=np.array(cnt, np.int32).reshape(-1, 2),
                rescontact_area=np.array(area, np.float64), rescontact_reverse=np.array(rev, np.int32),
                seg_first=first, row_seg=np.array(row_seg, np.int64), row_partner_seg=np.array(row_pseg, np.int64),
                seg_rows=cf[first[1:]] - cf[first[:-1]], seg_side=seg_side)


KEYS = ("rescontact_offsets", "rescontact_residues", "rescontact_counts", "rescontact_area", "rescontact_reverse")


@functools.lru_cache(maxsize=None)
def rescontacts_batch():
    """(xyz [n, 3], radii [n], offsets, group [n] int32, n_groups int32, names, res_first): the contact edge batch, the structure
    many-partners behind it, and the residue cut"""
    xyz, radii, offsets, group, n_groups, names = cr.contacts_edge_batch()
    # three big atoms far from each other (group 0) and around each a shell of 128 small atoms (group 1) that sit in the big
    # atom's probe shell: shell atom k of every centre lies in the direction of unit point k
    centres = np.array([[0.0, 0, 0], [40.0, 0, 0], [0, 40.0, 0]])
    u = cr.unit_points(128)
    shell = np.array([c + u[k] * (7.4 + 0.2) for k in range(128) for c in centres])
    xyz = np.concatenate([xyz, centres, shell]); radii = np.concatenate([radii, np.full(3, 6.0), np.full(384, 0.3)])
    group = np.concatenate([group, np.zeros(3, np.int32), np.ones(384, np.int32)]).astype(np.int32)
    n_groups = np.concatenate([n_groups, [2]]).astype(np.int32)
    offsets = np.concatenate([offsets, [offsets[-1] + 387]]).astype(np.int64)
    names = names + ("many-partners",)
    cut = {"six-partners": [1, 1, 2, 3], "three-pairs": [7] * 14 + [2], "big-sides": [80] + [2] * 20, "last-tile": [1, 620],
           "many-partners": [3] + [3] * 128}
    sizes = []
    for s, name in enumerate(names):
        n = int(offsets[s + 1] - offsets[s])
        part = cut.get(name, [1] * n)
        assert sum(part) == n, name
        sizes += part
    res_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for a in (xyz, radii, group, n_groups, offsets, res_first):
        a.setflags(write=False)
    return xyz, radii, offsets, group, n_groups, names, res_first


@functools.lru_cache(maxsize=None)
def batch_table():
    """the batch's pair table (interfaces_ref.table): pair_struct, pair_groups, side_offsets, pair_atom"""
    t = ir.table(*rescontacts_batch()[:5])
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def batch_contacts(n_points):
    """the batch's atom-atom contact table at n_points (interface_contacts_ref.contacts); computed once, read-only"""
    xyz, radii = rescontacts_batch()[:2]
    _, _, so, pa = batch_table()
    px, pr, _ = ir.pair_structures(xyz, radii, so, pa)
    unit = cr.unit_points(n_points)
    side, pair = cr.masks(px, pr, so, PROBE, unit)
    c = cr.contacts(px, pr, so, PROBE, unit, side, pair)
    for a in c.values():
        a.setflags(write=False)
    return c


def fold_of(c, res_first, so=None, pa=None):
    if so is None:
        _, _, so, pa = batch_table()
    return fold(so, pa, res_first, c["contact_first"], c["contact_partner"], c["contact_points"], c["contact_area"])


@functools.lru_cache(maxsize=None)
def batch_fold(n_points):
    """the batch's folded table at n_points; computed once, read-only"""
    f = fold_of(batch_contacts(n_points), rescontacts_batch()[6])
    for a in f.values():
        a.setflags(write=False)
    return f


def coverage(stage):
    """what the batch holds, decided on this restatement alone: {kind: bool}.  stage: the rows of a segment whose keys the fold
    kernels keep in LDS (RC_STAGE, csrc/rescontact_kernels.h), the size at which they change path"""
    _, _, so, pa = batch_table()
    res_first = rescontacts_batch()[6]
    out = {}
    f = batch_fold(100)
    c = batch_contacts(100)
    rows, K = f["seg_rows"], len(f["seg_rows"])
    out["a segment without rows"] = bool((rows == 0).any())
    # a folded row of several contact rows that are not adjacent: some row between two of them has another key
    heads = np.zeros(len(pa), bool); heads[f["seg_first"][:-1]] = True
    atom_seg = np.cumsum(heads) - 1
    keys = atom_seg[c["contact_partner"]]
    cf = c["contact_first"]
    split = False
    for k in np.nonzero(f["rescontact_counts"][:, 0] > 1)[0]:
        a = f["row_seg"][k]
        seg_keys = keys[cf[f["seg_first"][a]]:cf[f["seg_first"][a + 1]]]
        at = np.nonzero(seg_keys == f["row_partner_seg"][k])[0]
        split = split or bool(np.any(np.diff(at) > 1))
    out["a folded row of several non-adjacent contact rows"] = split
    res = f["rescontact_residues"]
    out["a residue in contact with itself across a pair"] = bool(np.any((res[:, 0] == res[:, 1]) & (f["row_seg"] != f["row_partner_seg"])))
    out["a row without a reverse and one with"] = bool((f["rescontact_reverse"] == -1).any() and (f["rescontact_reverse"] >= 0).any())
    out["three segments with more than 64 rows"] = bool((rows > WAVE).sum() >= 3)
    below = above = False
    for n in COVERAGE_N:
        fn = batch_fold(n)
        partners = np.bincount(fn["row_seg"], minlength=len(fn["seg_rows"]))
        big = (fn["seg_rows"] > 256) & (partners > WAVE)
        out[f"N = {n}: a segment with more than 256 rows and more than 64 partner residues"] = bool(big.any())
        below = below or bool(((fn["seg_rows"] > 0) & (fn["seg_rows"] <= stage)).any())
        above = above or bool((fn["seg_rows"] > stage).any())
    out["a whole number of waves of rows in a large segment"] = bool(np.any((batch_fold(128)["seg_rows"] > 256) & (batch_fold(128)["seg_rows"] % WAVE == 0)))
    out["segments on either side of the staging cap"] = below and above
    out["segments within a side ascend with their residues"] = bool(all(
        np.all(np.diff(rr.segments(so, pa, res_first)[2][(f["seg_side"] == q)]) > 0) for q in range(len(so) - 1)))
    return out
