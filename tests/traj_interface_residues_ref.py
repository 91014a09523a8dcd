"""A numpy / plain Python restatement of the per-residue interface tables per frame of a trajectory (include/freesasa_gpu.h,
freesasa_gpu_trajectory_interface_residues): the segments - interface_residues_ref.segments on the cut of
traj_interfaces_ref.cut - a frame's dense [S, 4] table as explicit loops over Python floats, and the SYNTHETIC TOPOLOGY the
tests of tests/test_traj_interface_residues.py run on, with a coverage() that decides on this restatement alone that it holds
every case.  Nothing here asks the code under test."""
import numpy as np

import interface_residues_ref as rr
import traj_interfaces_ref as tr


def sides(group, n_groups, pairs):
    """pside [2 K + 1]: where every side begins within a frame's pair part (side g of pair k, then side h)"""
    group = np.asarray(group)
    counts = np.bincount(group[group >= 0], minlength=n_groups)
    sizes = [int(counts[x]) for g, h in pairs for x in (g, h)]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def segments(group, n_groups, pairs, res_first):
    """(seg_first [S + 1], seg_res [S], seg_side [S], pside [2 K + 1], psrc [n_pair]) of a topology of one structure"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    _, psrc = tr.cut(np.asarray(group), pairs)
    pside = sides(group, n_groups, pairs)
    assert pside[-1] == len(psrc)
    # (empty sides at the very end begin at n_pair, where rr.segments would put a head behind its last atom: they own no
    # segment and are left off; the numbers of the sides in front of them do not change)
    last = int(np.nonzero(np.diff(pside) > 0)[0][-1]) if len(psrc) else -1
    _, first, seg_res, seg_side = rr.segments(pside[:last + 2], psrc, res_first)
    return first, seg_res.astype(np.int32), seg_side.astype(np.int32), pside, psrc


def side_offsets(seg_side, n_pairs):
    """[2 K + 1]: the prefix of the segments per side"""
    return np.concatenate([[0], np.cumsum(np.bincount(seg_side, minlength=2 * n_pairs))]).astype(np.int64)


def frame_table(iso_atoms, pair_area, seg_first, psrc, min_buried):
    """[S, 4] of one frame.  iso_atoms [n]: every topology atom's area in its isolated group (the run's `isolated` output of
    the frame); pair_area [n_pair]: the areas of the frame's pair-structure atoms.  Both sums one addition at a time in atom
    order from 0.0, buried = iso - in_pair, in_interface = 1.0 iff buried > min_buried."""
    iso_l, pa_l, src_l = [float(v) for v in iso_atoms], [float(v) for v in pair_area], [int(v) for v in psrc]
    S = len(seg_first) - 1
    out = np.empty((S, 4))
    for s in range(S):
        a = b = 0.0
        for m in range(int(seg_first[s]), int(seg_first[s + 1])):
            a += iso_l[src_l[m]]
            b += pa_l[m]
        buried = a - b
        out[s] = (a, b, buried, 1.0 if buried > float(min_buried) else 0.0)
    return out


def combined_table(csasa, nf, n, group, n_groups, pairs, res_first, min_buried):
    """[nf, S, 4] from the areas of a shard's COMBINED batch (csasa [nf (n + n_iso + n_pair)]: the frames, behind them every
    frame's isolated groups - group-major, input order within a group - behind those every frame's pair part)"""
    group = np.asarray(group)
    first, _, _, pside, psrc = segments(group, n_groups, pairs, res_first)
    src = np.concatenate([np.nonzero(group == g)[0] for g in range(n_groups)]).astype(np.int64)
    n_iso, n_pair = len(src), len(psrc)
    csasa = np.asarray(csasa, np.float64)
    assert csasa.size == nf * (n + n_iso + n_pair)
    out = []
    for f in range(nf):
        iso_atoms = np.full(n, np.nan)
        iso_atoms[src] = csasa[nf * n + f * n_iso:nf * n + (f + 1) * n_iso]
        at = nf * (n + n_iso) + f * n_pair
        out.append(frame_table(iso_atoms, csasa[at:at + n_pair], first, psrc, min_buried))
    return np.stack(out)


N_SYNTH = 516       # the atoms of tests/golden/pdb/2jo4.pdb, whose coordinates and radii the synthetic topology borrows
LONG = 257          # the long segment: more than a workgroup of the other per-segment kernels, 32 loads-ahead of 8 and one more


def synthetic():
    """(group [516] int32, G, pairs [4, 2], res_first [R + 1] int64) - one structure:
      atoms 0 - 9 group 0, 10 - 16 group 1, 17 - 24 in no group, 25 - 27 group 2, 28 - 284 group 3, from 285 on residues of 7
      atoms that go to groups 0, 1, 2 and to no group in turn; group 4 is empty.
      residues: [0, 4) [4, 8) | [8, 14): split over groups 0 and 1 | [14, 20): group 1 and no-group atoms | [20, 25): no-group atoms
      only | 25, 26, 27: one atom each | [28, 285): 257 atoms | sevens | empty ones at the start, at 25 and at the end.
      pairs: group 0 in three of them, the empty group 4 in one."""
    n = N_SYNTH
    group = np.full(n, -1, np.int32)
    group[0:10], group[10:17], group[25:28], group[28:28 + LONG] = 0, 1, 2, 3
    for j, at in enumerate(range(28 + LONG, n, 7)):
        group[at:at + 7] = (0, 1, 2, -1)[j % 4]
    cuts = [0, 4, 8, 14, 20, 25, 26, 27, 28] + list(range(28 + LONG, n, 7)) + [n]
    first = [0] + cuts                                  # an empty residue at the start
    first.insert(first.index(25), 25)                   # ... in the middle
    first += [n]                                        # ... and at the end
    pairs = np.array([(0, 1), (0, 2), (0, 3), (1, 4)], np.int32)
    res_first = np.array(first, np.int64)
    res_first.setflags(write=False)
    return group, 5, pairs, res_first


def coverage():
    """what the synthetic topology holds, decided on this restatement alone: {kind: bool}"""
    group, G, pairs, res_first = synthetic()
    first, seg_res, seg_side, pside, psrc = segments(group, G, pairs, res_first)
    length, size = np.diff(first), np.diff(res_first)
    R = len(size)
    res_groups = [set(group[res_first[r]:res_first[r + 1]].tolist()) for r in range(R)]
    side_group = pairs.reshape(-1)
    out = {"well-formed": bool(res_first[0] == 0 and res_first[-1] == len(group) and np.all(size >= 0) and R <= len(group)),
           "segments stay within a side": bool(np.all(np.searchsorted(pside, first[1:] - 1, side="right") - 1 == seg_side)),
           "segments cover the pair part": bool(length.sum() == len(psrc) and np.all(length >= 1)),
           "no empty residue in a segment": bool(np.all(size[seg_res] > 0))}
    split = [r for r in range(R) if len(res_groups[r] - {-1}) >= 2]
    out["a residue split over two groups: a segment on each side"] = bool(any(
        all(np.any((seg_res == r) & (side_group[seg_side] == g)) for g in res_groups[r] - {-1}) for r in split))
    mixed = [r for r in range(R) if -1 in res_groups[r] and len(res_groups[r]) >= 2]
    out["a residue of group atoms and no-group atoms: shorter segment"] = bool(any(
        np.any((seg_res == r) & (length < size[r])) for r in mixed))
    only = [r for r in range(R) if res_groups[r] == {-1}]
    out["a residue of no-group atoms only: in no segment"] = bool(only and not np.isin(seg_res, only).any())
    empty = np.nonzero(size == 0)[0]
    out["empty residues at the start, in the middle and at the end"] = bool(
        size[0] == 0 and size[-1] == 0 and np.any((res_first[empty] > 0) & (res_first[empty] < len(group))))
    out["one-atom residues"] = bool(np.any((length == 1) & (size[seg_res] == 1)))
    out["a segment of 257 atoms"] = bool(np.any(length == LONG))
    counts = np.bincount(group[group >= 0], minlength=G)
    out["an empty group named in a pair: a side without a segment"] = bool(
        any(counts[g] == 0 and not np.any(seg_side == j) for j, g in enumerate(side_group)))
    out["one group named in three pairs: its residues once per pair"] = bool(any(
        np.sum(side_group == g) == 3 and len({tuple(seg_res[seg_side == j]) for j in np.nonzero(side_group == g)[0]}) == 1 and
        np.sum(side_group[seg_side] == g) == 3 * np.sum(seg_side == np.nonzero(side_group == g)[0][0]) > 0 for g in range(G)))
    return out
