"""TESTS ONLY: what the file sweep's two interface kernels (freesasa_amd/csrc/ifsweep_kernels.h) compute, restated in numpy from
their definitions in include/freesasa_gpu.h - no binary search, no threads: searchsorted over the whole tables and plain loops."""
import numpy as np

TOT_B = 256     # SASA_TOT_B: the class-sum kernel's threads per structure (csrc/sasa_kernels.h)


def side_class(pair_atom, cls):
    """the class of every pair-structure atom"""
    return np.asarray(cls, np.uint8)[np.asarray(pair_atom, np.int64)]


def class_sums(values, cls, offsets):
    """freesasa_gpu_class_sums_dev's sums in ITS order: per structure 256 contiguous chunks in atom order, each summed left to
    right per class, the 256 partials added left to right -> [n, 3]"""
    values, cls, offsets = np.asarray(values, np.float64), np.asarray(cls, np.uint8), np.asarray(offsets, np.int64)
    out = np.zeros((offsets.size - 1, 3))
    for s in range(offsets.size - 1):
        b, e = int(offsets[s]), int(offsets[s + 1])
        per = (e - b + TOT_B - 1) // TOT_B
        tot = [0.0, 0.0, 0.0]
        for t in range(TOT_B):
            lo, hi = b + t * per, min(b + t * per + per, e)
            part = [0.0, 0.0, 0.0]
            for i in range(lo, hi):
                c = min(int(cls[i]), 2)
                part[c] = part[c] + float(values[i])
            for c in range(3):
                tot[c] = tot[c] + part[c]
        out[s] = tot
    return out


def res_rows(res_off, pair_struct, offsets, res_first, n_res_dev, res_index, lab_d, lab_h):
    """per residue row: its place among the residues of its structure, and its label bytes (names [R, 4], chains [R, 4], numbers [R, 6], uint8).
    lab_d / lab_h: (names, chains, numbers) of the device parser's first n_res_dev residues / of the host parser's behind them."""
    res_off, pair_struct = np.asarray(res_off, np.int64), np.asarray(pair_struct, np.int64)
    offsets, res_first, res_index = np.asarray(offsets, np.int64), np.asarray(res_first, np.int64), np.asarray(res_index, np.int64)
    R = int(res_off[-1])
    rows_per_side = np.diff(res_off)
    side = np.repeat(np.arange(rows_per_side.size), rows_per_side)          # (a side without a row is repeated 0 times)
    assert side.size == R
    s = pair_struct[side // 2]
    # a structure's first residue: the residues before it are those that begin before its first atom
    first = np.array([int((res_first[:-1] < offsets[k]).sum()) for k in s], np.int64)
    local = (res_index - first).astype(np.int32)
    assert len(lab_d[0]) == n_res_dev
    name, chain, number = (np.concatenate([np.asarray(d, np.uint8).reshape(-1, w), np.asarray(h, np.uint8).reshape(-1, w)])[res_index]
                           for d, h, w in zip(lab_d, lab_h, (4, 4, 6)))
    return local, name, chain, number
