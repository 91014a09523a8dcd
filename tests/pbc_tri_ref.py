"""TESTS ONLY: periodic images in a triclinic cell as include/freesasa_gpu.h (freesasa_gpu_calc_periodic_triclinic) defines them,
restated in numpy - the yardstick of tests/test_pbc_tri.py and tests/test_pbc_tri_gpu.py, checked itself against the explicit
5 x 5 x 5 replica system in tests/test_pbc_tri.py - and the seeded batch both files use.

    cell      h = (ax, bx, by, cx, cy, cz): rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz) of the box matrix
    c         2 (max radius + probe)
    widths    d_c = cz;  d_b = by * (cz / sqrt(cy*cy + cz*cz));  t = bx*cy - by*cx;
              d_a = ax * ((by*cz) / sqrt(((by*cz)*(by*cz) + (bx*cz)*(bx*cz)) + t*t))
    frac      fc = z / cz;  fb = (y - fc*cy) / by;  fa = ((x - fc*cx) - fb*bx) / ax
    wrap      n = floor(frac(p)):  w_x = ((x - nc*cx) - nb*bx) - na*ax;  w_y = (y - nc*cy) - nb*by;  w_z = z - nc*cz
    images    g = frac(w); axis k admits 0 always, +1 when g_k * d_k < c, -1 when (1.0 - g_k) * d_k < c; every admitted
              (sa, sb, sc) != (0, 0, 0) at x = ((w_x + sc*cx) + sb*bx) + sa*ax;  y = (w_y + sc*cy) + sb*by;  z = w_z + sc*cz
    order     the wrapped atoms, then the images by atom and within an atom by 9 (sa + 1) + 3 (sb + 1) + (sc + 1)
numpy rounds every operation on its own (no fma); the expressions below are written in exactly that order.
"""
import math

import numpy as np

S2, S3, S6 = math.sqrt(2.0), math.sqrt(3.0), math.sqrt(6.0)
HEXAGONAL = (14.0, -7.0, 7.0 * S3, 0.0, 0.0, 16.0)
OCTAHEDRAL = (18.0, 6.0, 12.0 * S2, -6.0, 6.0 * S2, 6.0 * S6)      # GROMACS's truncated octahedron, d = 18
SKEWED = (13.0, 9.0, 12.0, -11.0, 7.0, 15.0)                       # not reduced
FLAT = (30.0, 4.0, 9.0, -7.0, 2.0, 50.0)
SMALL_HEXAGONAL = (7.9, -3.95, 3.95 * S3, 0.0, 0.0, 7.0)           # widths 6.84, 6.84, 7.0 against c = 6.8


def cutoff(radii, probe=1.4):
    radii = np.asarray(radii, dtype=np.float64)
    return 2.0 * ((float(radii.max()) if radii.size else 0.0) + probe)


def widths(h):
    ax, bx, by, cx, cy, cz = (np.float64(v) for v in h)
    t = bx * cy - by * cx
    d_b = by * (cz / np.sqrt(cy * cy + cz * cz))
    d_a = ax * ((by * cz) / np.sqrt(((by * cz) * (by * cz) + (bx * cz) * (bx * cz)) + t * t))
    return np.array([d_a, d_b, cz], dtype=np.float64)


def cell9(cells6):
    """[ns, 6] -> [ns, 9]: every cell with its widths behind it, as the device takes them"""
    cells6 = np.asarray(cells6, dtype=np.float64).reshape(-1, 6)
    return np.hstack([cells6, np.array([widths(h) for h in cells6]).reshape(-1, 3)])


def matrix(h):
    ax, bx, by, cx, cy, cz = h
    return np.array([[ax, 0.0, 0.0], [bx, by, 0.0], [cx, cy, cz]], dtype=np.float64)


def frac(p, h):
    """p [n, 3] -> the fractional coordinates (a, b, c) [n, 3]"""
    ax, bx, by, cx, cy, cz = (np.float64(v) for v in h)
    fc = p[:, 2] / cz
    fb = (p[:, 1] - fc * cy) / by
    fa = ((p[:, 0] - fc * cx) - fb * bx) / ax
    return np.stack([fa, fb, fc], axis=1)


def wrap(xyz, h):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    ax, bx, by, cx, cy, cz = (np.float64(v) for v in h)
    n = np.floor(frac(xyz, h))
    na, nb, nc = n[:, 0], n[:, 1], n[:, 2]
    return np.stack([((xyz[:, 0] - nc * cx) - nb * bx) - na * ax, (xyz[:, 1] - nc * cy) - nb * by, xyz[:, 2] - nc * cz], axis=1)


def shifted(w, h, sa, sb, sc):
    ax, bx, by, cx, cy, cz = (np.float64(v) for v in h)
    sa, sb, sc = np.float64(sa), np.float64(sb), np.float64(sc)
    return np.stack([((w[..., 0] + sc * cx) + sb * bx) + sa * ax, (w[..., 1] + sc * cy) + sb * by, w[..., 2] + sc * cz], axis=-1)


def expand(xyz, radii, h, probe=1.4):
    """-> (expanded xyz [N, 3], expanded radii [N], image count N - n)"""
    radii, h = np.asarray(radii, dtype=np.float64), np.asarray(h, dtype=np.float64)
    c = cutoff(radii, probe)
    if radii.size and not (np.all(np.isfinite(h)) and h[0] > 0 and h[2] > 0 and h[5] > 0 and np.all(widths(h) >= c)):
        raise ValueError("the cell must be finite with ax, by, cz > 0 and every width >= c")
    w = wrap(xyz, h)
    if not radii.size:
        return w, radii.copy(), 0
    d, g = widths(h), frac(w, h)
    plus, minus = g * d < c, (1.0 - g) * d < c
    img_xyz, img_r = [], []
    for i in range(radii.size):
        admit = [[s for s in (-1, 0, 1) if s == 0 or (s == 1 and plus[i, k]) or (s == -1 and minus[i, k])] for k in range(3)]
        for sa in admit[0]:                       # (ascending shifts, a slowest: ascending code)
            for sb in admit[1]:
                for sc in admit[2]:
                    if (sa, sb, sc) != (0, 0, 0):
                        img_xyz.append(shifted(w[i], h, sa, sb, sc))
                        img_r.append(radii[i])
    if img_r:
        return np.vstack([w, np.array(img_xyz)]), np.concatenate([radii, np.array(img_r)]), len(img_r)
    return w, radii.copy(), 0


def replicas(xyz, radii, h, shell=2):
    """the explicit (2 shell + 1)^3 replica system of the WRAPPED atoms, the central cell first -> (xyz, radii)"""
    w = wrap(xyz, h)
    rng = range(-shell, shell + 1)
    shifts = [(0, 0, 0)] + [(sa, sb, sc) for sa in rng for sb in rng for sc in rng if (sa, sb, sc) != (0, 0, 0)]
    return np.vstack([shifted(w, h, *s) for s in shifts]), np.tile(np.asarray(radii, dtype=np.float64), len(shifts))


def expand_batch(xyz, radii, offsets, cells6, probe=1.4):
    """-> (expanded xyz, expanded radii, expanded offsets, image counts)"""
    ex, er, eo, ni = [], [], [0], []
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        x, r, k = expand(xyz[a:b], radii[a:b], cells6[s], probe)
        ex.append(x.reshape(-1, 3)); er.append(r); ni.append(k); eo.append(eo[-1] + (b - a) + k)
    return np.vstack(ex), np.concatenate(er), np.array(eo, dtype=np.int64), np.array(ni, dtype=np.int64)


def cell_from_cosines(A, cg, B, cb, ca, C):
    """include/freesasa_gpu.h, freesasa_gpu_cell_from_dcd, on cosines, in its order of operations"""
    A, cg, B, cb, ca, C = (np.float64(v) for v in (A, cg, B, cb, ca, C))
    bx, by, cx = B * cg, B * np.sqrt(1.0 - cg * cg), C * cb
    cy = C * ((ca - cb * cg) / np.sqrt(1.0 - cg * cg))
    return np.array([A, bx, by, cx, cy, np.sqrt((C * C - cx * cx) - cy * cy)], dtype=np.float64)


# ---------------------------------------------------------------- the batch of the tests

SIZES = (0, 1, 2, 60, 516)        # 516: three steps of 256 of the count kernel, the last one short
CELLS = (FLAT, SMALL_HEXAGONAL, OCTAHEDRAL, SKEWED, FLAT)
SEED = 20261018


def structure(n, h, seed, outside=True):
    """n atoms with radii 1.2 .. 2.0 spread over the cell; with `outside` a quarter of them up to 1.5 cells outside it in
    fractional coordinates, on both sides"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, 1.0, (n, 3))
    if outside and n:
        out = rng.random(n) < 0.25
        out[0] = True
        q[out] += rng.choice([-1.0, 1.0], (int(out.sum()), 3)) * rng.uniform(0.0, 1.5, (int(out.sum()), 3))
    return q @ matrix(h), rng.uniform(1.2, 2.0, n)


def sixty(h, seed=SEED + 3):
    """the 60 atoms of the yardstick and invariance tests in the cell h: one radius 2.0, so c = 6.8"""
    xyz, radii = structure(60, h, seed)
    radii[0] = 2.0
    return xyz, radii


def batch(seed=SEED):
    """five structures of SIZES atoms, each with its own cell of CELLS -> (xyz [n, 3], radii [n], offsets [6], cells6 [5, 6]).
    The one atom (radius 2.0, c = 6.8) sits mid-cell, one cell away along a and b, in a hexagonal cell whose widths 6.84, 6.84,
    7.0 barely reach c: both shifts on every axis, 26 images.  The 60 atoms: one radius 2.0 in the skewed cell, whose widths
    (8.2, 10.9, 15) are below 2 c - atoms with both shifts on an axis."""
    parts = [structure(n, h, seed + k) for k, (n, h) in enumerate(zip(SIZES, CELLS))]
    xyz = np.vstack([p[0] for p in parts])
    radii = np.concatenate([p[1] for p in parts])
    radii[SIZES[0]] = 2.0
    xyz[SIZES[0]] = np.array([0.5 + 1.0, 0.5 - 1.0, 0.5]) @ matrix(SMALL_HEXAGONAL)
    radii[sum(SIZES[:3])] = 2.0
    return xyz, radii, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64), np.array(CELLS, dtype=np.float64)
