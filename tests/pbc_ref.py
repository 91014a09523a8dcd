"""TESTS ONLY: periodic images as include/freesasa_gpu.h (freesasa_gpu_calc_periodic) defines them, restated in numpy - the
yardstick of tests/test_pbc.py and tests/test_pbc_gpu.py, checked itself against the explicit 27-replica system in
tests/test_pbc.py - and the seeded batch both files use.

    c         2 (max radius + probe)
    wrap      w = x - L * floor(x / L), fp64 (numpy rounds every operation: no fma)
    images    axis a admits shift 0 always, +1 when w < c, -1 when w > L - c; every admitted (sx, sy, sz) != (0, 0, 0)
    order     the wrapped atoms, then the images by atom and within an atom by 9 (sx + 1) + 3 (sy + 1) + (sz + 1)
"""
import numpy as np


def cutoff(radii, probe=1.4):
    radii = np.asarray(radii, dtype=np.float64)
    return 2.0 * ((float(radii.max()) if radii.size else 0.0) + probe)


def wrap(xyz, cell):
    xyz, cell = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(cell, dtype=np.float64)
    return xyz - cell * np.floor(xyz / cell)


def expand(xyz, radii, cell, probe=1.4):
    """-> (expanded xyz [N, 3], expanded radii [N], image count N - n)"""
    radii, cell = np.asarray(radii, dtype=np.float64), np.asarray(cell, dtype=np.float64)
    c = cutoff(radii, probe)
    if not (np.all(np.isfinite(cell)) and np.all(cell >= c)) and radii.size:
        raise ValueError("the cell must be finite and every edge >= c")
    w = wrap(xyz, cell)
    img_xyz, img_r = [], []
    for i in range(radii.size):
        admit = [[s for s in (-1, 0, 1) if s == 0 or (s == 1 and w[i, a] < c) or (s == -1 and w[i, a] > cell[a] - c)] for a in range(3)]
        for sx in admit[0]:                       # (ascending shifts, x slowest: ascending code)
            for sy in admit[1]:
                for sz in admit[2]:
                    if (sx, sy, sz) != (0, 0, 0):
                        img_xyz.append(w[i] + np.array([sx, sy, sz], dtype=np.float64) * cell)
                        img_r.append(radii[i])
    if img_r:
        return np.vstack([w, np.array(img_xyz)]), np.concatenate([radii, np.array(img_r)]), len(img_r)
    return w, radii.copy(), 0


def replicas(xyz, radii, cell):
    """the explicit 27-replica system of the WRAPPED atoms: the central cell first -> (xyz [27 n, 3], radii [27 n])"""
    w, cell = wrap(xyz, cell), np.asarray(cell, dtype=np.float64)
    shifts = [(0, 0, 0)] + [(sx, sy, sz) for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1) if (sx, sy, sz) != (0, 0, 0)]
    return np.vstack([w + np.array(s, dtype=np.float64) * cell for s in shifts]), np.tile(np.asarray(radii, dtype=np.float64), 27)


# ---------------------------------------------------------------- the batch of the tests

SIZES = (0, 1, 2, 60, 516)        # 516: three steps of 256 of the count kernel, the last one short
CELLS = ((30.0, 9.0, 50.0), (7.0, 7.5, 8.0), (30.0, 9.0, 50.0), (12.0, 14.0, 16.0), (30.0, 9.0, 50.0))


def structure(n, cell, seed, outside=True):
    """n atoms with radii 1.2 .. 2.0 spread over the cell; with `outside` a quarter of them up to 1.5 box lengths outside it, on
    both sides"""
    rng = np.random.default_rng(seed)
    cell = np.asarray(cell, dtype=np.float64)
    xyz = rng.uniform(0.0, 1.0, (n, 3)) * cell
    if outside and n:
        out = rng.random(n) < 0.25
        out[0] = True
        xyz[out] += rng.choice([-1.0, 1.0], (int(out.sum()), 3)) * rng.uniform(0.0, 1.5, (int(out.sum()), 3)) * cell
    return xyz, rng.uniform(1.2, 2.0, n)


def batch(seed=20261018):
    """five structures of SIZES atoms, each with its own cell of CELLS -> (xyz [n, 3], radii [n], offsets [6], cells [5, 3]).
    (12, 14, 16) with radii up to 2.0 and probe 1.4: c = 6.8 > Lx / 2 - atoms with both shifts on the x axis (up to 11 images).
    The one-atom structure sits mid-cell, one cell away, in a cell barely larger than c: both shifts on every axis, 26 images."""
    parts = [structure(n, cell, seed + k) for k, (n, cell) in enumerate(zip(SIZES, CELLS))]
    xyz = np.vstack([p[0] for p in parts])
    radii = np.concatenate([p[1] for p in parts])
    radii[SIZES[0]] = 2.0                                         # (the one-atom structure: c = 6.8 <= 7.0)
    xyz[SIZES[0]] = (3.5 + 7.0, 3.0 - 7.5, 4.0)
    radii[sum(SIZES[:3])] = 2.0                                   # (the 60 atoms: c = 6.8, Lx = 12 < 2 c)
    return xyz, radii, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64), np.array(CELLS, dtype=np.float64)


def expand_batch(xyz, radii, offsets, cells, probe=1.4):
    """-> (expanded xyz, expanded radii, expanded offsets, image counts)"""
    ex, er, eo, ni = [], [], [0], []
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        x, r, k = expand(xyz[a:b], radii[a:b], cells[s], probe)
        ex.append(x.reshape(-1, 3)); er.append(r); ni.append(k); eo.append(eo[-1] + (b - a) + k)
    return np.vstack(ex), np.concatenate(er), np.array(eo, dtype=np.int64), np.array(ni, dtype=np.int64)
