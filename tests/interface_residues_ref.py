"""A numpy restatement of the per-residue tables of the interfaces between chain groups (include/freesasa_gpu.h,
freesasa_gpu_interface_residues_dev): the segments of the pair table's sides, their three sums as explicit sequential loops over
Python floats, the rows and res_offsets - and the RESIDUE EDGE BATCH the tests of tests/test_interface_residues.py and
tests/test_interface_residues_gpu.py run on: the edge batch of tests/interfaces_ref.py with residue boundaries chosen to give
the cases coverage() lists.  Nothing here asks the code under test."""
import functools

import numpy as np

import interfaces_ref as ir

WORKGROUP = 256   # IF_B (csrc/iface_kernels.h): threads of a workgroup, elements of a block of the scan
WAVE = 64


def residue_of(res_first, atoms):
    """the residue of every input atom: the last r < n_res with res_first[r] <= atom (empty residues are never found)"""
    res_first = np.asarray(res_first, np.int64)
    return (np.searchsorted(res_first[:-1], np.asarray(atoms, np.int64), side="right") - 1).astype(np.int32)


def segments(side_offsets, pair_atom, res_first):
    """(heads [M] bool, seg_first [K + 1], seg_res [K], seg_side [K]): a segment is a maximal run of consecutive atoms of one
    side whose input atoms lie in one residue"""
    side_offsets, pair_atom = np.asarray(side_offsets, np.int64), np.asarray(pair_atom, np.int64)
    M = len(pair_atom)
    res = residue_of(res_first, pair_atom)
    heads = np.zeros(M, bool)
    if M:
        heads[1:] = res[1:] != res[:-1]
        heads[side_offsets[:-1]] = True
    first = np.nonzero(heads)[0].astype(np.int64)
    side = (np.searchsorted(side_offsets, first, side="right") - 1).astype(np.int64)
    return heads, np.concatenate([first, [M]]).astype(np.int64), res[first], side


def rows(iso, pair_area, side_offsets, pair_atom, res_first, min_buried):
    """(res_offsets [2P + 1] int64, res_index [R] int32, res_atoms [R] int32, res_areas [R, 3]) from the isolated areas of the
    input atoms (iso [n]) and the areas of the pair-structure atoms (pair_area [M]): every sum one addition at a time in atom
    order, buried = iso - in_pair, a row iff buried > min_buried"""
    _, first, seg_res, seg_side = segments(side_offsets, pair_atom, res_first)
    n_sides = len(side_offsets) - 1
    index, atoms, areas, per_side = [], [], [], np.zeros(n_sides, np.int64)
    iso_l, pa_l, atom_l = [float(v) for v in iso], [float(v) for v in pair_area], [int(v) for v in pair_atom]
    for k in range(len(seg_res)):
        a = b = 0.0
        for m in range(int(first[k]), int(first[k + 1])):
            a += iso_l[atom_l[m]]
            b += pa_l[m]
        buried = a - b
        if buried > min_buried:
            index.append(int(seg_res[k])); atoms.append(int(first[k + 1] - first[k])); areas.append((a, b, buried))
            per_side[seg_side[k]] += 1
    offs = np.concatenate([[0], np.cumsum(per_side)]).astype(np.int64)
    return offs, np.array(index, np.int32), np.array(atoms, np.int32), np.array(areas, np.float64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def edge_table():
    """ir.table() of the edge batch (brute force: made once)"""
    return ir.table(*ir.edge_batch()[:5])


@functools.lru_cache(maxsize=None)
def residue_edge_batch():
    """(xyz, radii, offsets, group, n_groups, names, res_first): ir.edge_batch() and its residue boundaries.
    In the edge batch atoms in no group lie only behind a structure's groups, so the residue that holds atoms of a group and
    atoms in no group is one that begins in the last group and ends among the no-group atoms behind it."""
    xyz, radii, offsets, group, n_groups, names = ir.edge_batch()
    n = int(offsets[-1])
    cuts = set(int(o) for o in offsets)

    def every(s, step, lo=None, hi=None):
        lo = int(offsets[s]) if lo is None else lo
        hi = int(offsets[s + 1]) if hi is None else hi
        cuts.update(range(lo, hi, step))
        cuts.add(hi)

    s = names.index("sizes")                        # groups of 0, 1, 63, 64, 65, 256, 257 atoms one behind the other, then 40 in no group
    assert offsets[s] == 0
    every(s, 1, 0, 1)                               # a one-atom residue
    every(s, 7, 1, 64)                              # the 63-atom group in residues of 7
    cuts.update((64, 128, 193))                     # the 64-atom group and the 65-atom group: a residue each
    every(s, 10, 193, 449)                          # the 256-atom group in residues of 10 (the last of 6)
    cuts.update((449, 449 + 257 + 5))               # the 257-atom group and the first 5 no-group atoms: ONE residue
    cuts.update((730, 746))                         # two residues of no-group atoms only
    every(names.index("interleaved"), 3)            # every residue split over three groups, every segment one atom
    every(names.index("one-group"), 8)
    every(names.index("no-groups"), 10)
    every(names.index("strict"), 1)
    every(names.index("diagonal"), 9)
    every(names.index("late-hit"), 11)
    every(names.index("lds-overflow-hit"), 12)
    every(names.index("lds-overflow-miss"), 15)
    # a segment that starts on the last pair atom before a multiple of 256 and ends behind it: three consecutive input atoms of
    # one side in the late-hit structure, made a residue of their own
    _, _, so, pa = edge_table()
    s = names.index("late-hit")
    for m in range(WORKGROUP - 1, len(pa) - 2, WORKGROUP):
        a = int(pa[m])
        q = int(np.searchsorted(so, m, side="right") - 1)
        if offsets[s] <= a and a + 3 <= offsets[s + 1] and m + 2 < so[q + 1] and pa[m + 1] == a + 1 and pa[m + 2] == a + 2:
            cuts.difference_update((a + 1, a + 2))
            cuts.update((a, a + 3))
            break
    first = sorted(cuts)
    # empty residues at the start, in the middle (inside a structure and on a structure's boundary) and at the end
    first = [0, 0] + first[1:]
    for at in (64, int(offsets[1]), int(offsets[5]) + 9):
        k = first.index(at)
        first.insert(k, at)
    first += [n, n]
    res_first = np.array(first, np.int64)
    res_first.setflags(write=False)
    return xyz, radii, offsets, group, n_groups, names, res_first


def coverage():
    """what the residue edge batch holds, decided on this restatement alone: {kind: bool}"""
    xyz, radii, offsets, group, n_groups, names, res_first = residue_edge_batch()
    ps, pg, so, pa = edge_table()
    heads, first, seg_res, seg_side = segments(so, pa, res_first)
    length = np.diff(first)
    n_res = len(res_first) - 1
    size = np.diff(res_first)
    res_struct = np.searchsorted(offsets, res_first[:-1], side="right") - 1
    out = {"well-formed": bool(res_first[0] == 0 and res_first[-1] == offsets[-1] and np.all(size >= 0) and
                               all(size[r] == 0 or res_first[r + 1] <= offsets[res_struct[r] + 1] for r in range(n_res))),
           "segments stay within a side": bool(np.all(np.searchsorted(so, first[1:] - 1, side="right") - 1 == seg_side)),
           "one-atom residues": bool(np.any(size[seg_res] == 1))}
    s = names.index("interleaved")
    in_s = (pa[first[:-1]] >= offsets[s]) & (pa[first[:-1]] < offsets[s + 1])
    rs = np.nonzero((res_first[:-1] >= offsets[s]) & (res_first[:-1] < offsets[s + 1]) & (size > 0))[0]
    out["interleaved: 3-atom residues over three groups, one-atom segments"] = bool(
        in_s.any() and np.all(length[in_s] == 1) and np.all(size[rs] == 3) and
        all(len(set(group[res_first[r]:res_first[r + 1]].tolist())) == 3 for r in rs))
    out["a segment longer than a workgroup"] = bool(np.any(length == WORKGROUP + 1))
    out["a 64-atom and a 65-atom residue"] = bool(np.any((length == WAVE) & (size[seg_res] == WAVE)) and
                                                   np.any((length == WAVE + 1) & (size[seg_res] == WAVE + 1)))
    out["a segment from the last atom before a multiple of 256 to behind it"] = bool(
        np.any((first[:-1] % WORKGROUP == WORKGROUP - 1) & (length >= 2)))
    empty = np.nonzero(size == 0)[0]
    out["empty residues at the start, in the middle and at the end"] = bool(
        size[0] == 0 and size[-1] == 0 and np.any((res_first[empty] > 0) & (res_first[empty] < offsets[-1])))
    out["no empty residue in a segment"] = bool(np.all(size[seg_res] > 0))
    out["a residue of no-group atoms only"] = bool(any(
        size[r] > 0 and n_groups[res_struct[r]] > 0 and np.all(group[res_first[r]:res_first[r + 1]] < 0) for r in range(n_res)))
    mixed = [r for r in range(n_res) if size[r] > 0 and (group[res_first[r]:res_first[r + 1]] < 0).any() and
             (group[res_first[r]:res_first[r + 1]] >= 0).any()]
    out["a residue of group atoms and no-group atoms: shorter segment"] = bool(any(
        np.any((seg_res == r) & (length < size[r])) for r in mixed))
    out["several blocks of the scan"] = bool(len(pa) > 2 * WORKGROUP and len(seg_res) > 2 * WORKGROUP)
    # the strict structure gives pairs of one-atom sides; the diagonal structure gives no pair at all
    out["strict: one-atom sides"] = bool(np.any((ps == names.index("strict")) & (np.diff(so)[::2] == 1) & (np.diff(so)[1::2] == 1)))
    out["diagonal: no pair"] = bool(not np.any(ps == names.index("diagonal")))
    return out
