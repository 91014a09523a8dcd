"""A numpy / plain Python restatement of the interfaces between chain groups in the trajectory drivers (include/freesasa_gpu.h,
freesasa_gpu_trajectory_interfaces): the pairs of "all", the cut of a frame's pair structures, the order in which the
per-structure totals kernel adds a segment, and the six columns of a row.  Every addition is one Python float addition."""
import numpy as np

import interfaces_ref as ir

TOT_B = 256     # SASA_TOT_B (csrc/sasa_kernels.h): threads of the totals kernel's workgroup


def all_pairs(n_groups):
    """every g < h in the order of interfaces_ref.table: g-major"""
    return np.array([(g, h) for g in range(n_groups) for h in range(g + 1, n_groups)], np.int32).reshape(-1, 2)


def cut(group, pairs):
    """(pfirst [K + 1], psrc [n_pair]) of one structure: pair k is interfaces_ref.members of g, then of h"""
    offsets = np.array([0, len(group)], np.int64)
    sides = [ir.members(offsets, group, 0, k) for g, h in pairs for k in (g, h)]
    sizes = [len(sides[2 * k]) + len(sides[2 * k + 1]) for k in range(len(pairs))]
    psrc = np.concatenate(sides).astype(np.int32) if sides else np.zeros(0, np.int32)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), psrc


def k_totals_sum(v, b=TOT_B):
    """v summed as totals_phase0 / totals_phase1 add a segment: b contiguous runs of ceil(len / b) values, each added in order
    from 0.0, then the runs added in order from 0.0"""
    n = len(v)
    per = -(-n // b)
    total = 0.0
    for t in range(b):
        run = 0.0
        for i in range(t * per, min(t * per + per, n)):
            run += float(v[i])
        total += run
    return total


def rows(iso, in_pair, pairs):
    """[K, 6] of one frame: iso [G] the groups' isolated totals, in_pair [K, 2] the sides' sums"""
    out = np.empty((len(pairs), 6))
    for k, (g, h) in enumerate(pairs):
        out[k] = (iso[g], iso[h], in_pair[k, 0], in_pair[k, 1], iso[g] - in_pair[k, 0], iso[h] - in_pair[k, 1])
    return out


def frame_rows(group, pairs, iso, areas):
    """[K, 6] of one frame from `areas`: the areas of the frame's pair structures, one behind the other (side g, then side h)"""
    counts = np.bincount(group[group >= 0], minlength=len(iso))
    in_pair, at = np.empty((len(pairs), 2)), 0
    for k, (g, h) in enumerate(pairs):
        for q, side in enumerate((g, h)):
            in_pair[k, q] = k_totals_sum(areas[at:at + counts[side]])
            at += counts[side]
    assert at == len(areas)
    return rows(iso, in_pair, pairs)
