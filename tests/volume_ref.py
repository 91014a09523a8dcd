"""The definition of the molecular volume (include/freesasa_gpu.h, freesasa_amd/csrc/vol_kernels.h) restated in numpy: the
yardstick of tests/test_volume.py and tests/test_volume_gpu.py.  fp64; numpy rounds every elementwise operation on its own, as
the build does with -ffp-contract=off; every sum whose order the definition fixes is a Python loop in that order.

    V = (1/3) sum_i a_i ( (x_i - o) . E_i + R_i n_i ),   E_i = sum over atom i's exposed points of u_k,  a_i = 4 pi R_i^2 / N
"""
import math

import numpy as np

TOT_B = 256          # SASA_TOT_B: threads of a workgroup of the totals kernels
BOUNDS_CHUNK = 4096  # SASA_BOUNDS_CHUNK: atoms of a structure one workgroup of the totals kernels sums


def exposed_mask(xyz, r_ext, unit):
    """[n, N] bool: point k of atom i is covered iff for some other atom j  dx^2 + dy^2 + dz^2 <= R_j * R_j, with the test
    point made in two rounded steps, t = u_k * R_i; t += x_i (oracle/sasa_oracle.c:211-227)"""
    xyz, r_ext, unit = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(r_ext, dtype=np.float64), np.asarray(unit, dtype=np.float64).reshape(-1, 3)
    n = len(r_ext)
    r2 = r_ext * r_ext
    out = np.empty((n, len(unit)), dtype=bool)
    for i in range(n):
        t = unit * r_ext[i]
        t = t + xyz[i]
        d = t[:, None, :] - xyz[None, :, :]
        dx2, dy2, dz2 = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]
        s = dx2 + dy2
        s = s + dz2
        cov = s <= r2[None, :]
        cov[:, i] = False
        out[i] = ~cov.any(axis=1)
    return out


def evec_of(mask, unit):
    """E_i: from (0, 0, 0), the exposed points' unit vectors added in ascending point order, component by component"""
    unit = np.asarray(unit, dtype=np.float64).reshape(-1, 3)
    E = np.zeros((mask.shape[0], 3))
    for k in range(mask.shape[1]):
        rows = mask[:, k]
        E[rows] = E[rows] + unit[k]
    return E


def origin_of(xyz):
    """per axis (min + max) * 0.5; a structure without atoms: (0, 0, 0)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros(3)
    return (xyz.min(axis=0) + xyz.max(axis=0)) * 0.5


def atom_terms(xyz, r_ext, counts, E, o, n_points):
    """v_i = (a * (t + R_i * n_i)) / 3.0 with a = (4.0 * PI * R_i * R_i) / N, d = x_i - o, t = d_x E_x + d_y E_y + d_z E_z left to right"""
    xyz, r_ext = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(r_ext, dtype=np.float64)
    a = 4.0 * math.pi * r_ext
    a = a * r_ext
    a = a / float(n_points)
    d = xyz - o
    t = d[:, 0] * E[:, 0]
    t = t + d[:, 1] * E[:, 1]
    t = t + d[:, 2] * E[:, 2]
    inner = t + r_ext * np.asarray(counts, dtype=np.float64)
    return (a * inner) / 3.0


def totals_of(v):
    """the engine's totals of one structure (kl_totals): per chunk of BOUNDS_CHUNK atoms, thread tid of TOT_B adds atoms tid,
    tid + TOT_B, ... in order from 0.0 (totals_chunk_phase0), thread 0 adds the TOT_B partials in order from 0.0
    (totals_chunk_phase1); then the chunks are added in order from 0.0 (totals_struct)"""
    v = np.asarray(v, dtype=np.float64)
    total = 0.0
    for b in range(0, len(v), BOUNDS_CHUNK):
        c = v[b:b + BOUNDS_CHUNK]
        part = np.zeros(TOT_B)
        for j in range(0, len(c), TOT_B):          # round j: every thread's next atom
            seg = c[j:j + TOT_B]
            part[:len(seg)] = part[:len(seg)] + seg
        t = 0.0
        for k in range(TOT_B):
            t = t + part[k]
        total = total + t
    return float(total)


def volume_batch(xyz, radii, offsets, probe, unit, shared_radii=False):
    """the whole definition on a batch -> dict(counts [n] int32, evec [n, 3], vol [n], volumes [n_structs], origin [n_structs, 3])"""
    xyz, radii = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(radii, dtype=np.float64)
    unit = np.asarray(unit, dtype=np.float64).reshape(-1, 3)
    n, ns, N = len(xyz), len(offsets) - 1, len(unit)
    counts, evec, vol = np.zeros(n, dtype=np.int32), np.zeros((n, 3)), np.zeros(n)
    volumes, origin = np.zeros(ns), np.zeros((ns, 3))
    for s in range(ns):
        b, e = int(offsets[s]), int(offsets[s + 1])
        if e <= b:
            continue
        R = (radii[:e - b] if shared_radii else radii[b:e]) + probe
        mask = exposed_mask(xyz[b:e], R, unit)
        counts[b:e] = mask.sum(axis=1)
        evec[b:e] = evec_of(mask, unit)
        origin[s] = origin_of(xyz[b:e])
        vol[b:e] = atom_terms(xyz[b:e], R, counts[b:e], evec[b:e], origin[s], N)
        volumes[s] = totals_of(vol[b:e])
    return dict(counts=counts, evec=evec, vol=vol, volumes=volumes, origin=origin)


def volume_one(xyz, radii, probe, unit):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return float(volume_batch(xyz, radii, np.array([0, len(xyz)]), probe, unit)["volumes"][0])


def two_sphere_union(R, d):
    """analytic volume of the union of two spheres of radius R whose centres are d apart (0 <= d <= 2 R): two spheres minus the lens"""
    lens = math.pi * (4.0 * R + d) * (2.0 * R - d) ** 2 / 12.0
    return 2.0 * (4.0 / 3.0) * math.pi * R ** 3 - lens


SEED = 20261019
POINT_COUNTS = (1, 31, 32, 33, 100, 128)  # the mask-word edges and both ends of the domain
SHIFT = np.array([1000.0, -2000.0, 500.0])


def batch(seed=SEED):
    """The batch of the volume tests, seeded: seven structures - 1 atom; 2 atoms far apart (no neighbours); 2 overlapping atoms;
    3 atoms, one of them wholly inside another (n = 0, E = 0, v = 0); none; 70 atoms at protein density (more than one tile, no
    multiple of a tile's atoms); 400 atoms at protein density (several cells and tiles) -> (xyz [n, 3], radii [n], offsets [8]).
    The seed is one for which the restatement's counts equal oracle_shrake_rupley's on every atom at every one of POINT_COUNTS,
    and on the 400 atoms moved by SHIFT (tests/test_volume.py checks it)."""
    import tools
    rng = np.random.default_rng(seed)
    place = lambda: rng.uniform(-40.0, 40.0, 3)
    parts = []
    o = place()
    parts.append((o[None], np.array([1.7])))
    o = place()
    parts.append((np.array([o, o + [30.0, 5.0, -7.0]]), np.array([1.6, 2.0])))
    o = place()
    parts.append((np.array([o, o + rng.uniform(0.8, 1.2, 3)]), np.array([1.8, 1.5])))
    o = place()
    parts.append((np.array([o, o + [0.3, -0.2, 0.25], o + [3.1, 0.4, -0.6]]), np.array([2.5, 0.5, 1.7])))
    parts.append((np.zeros((0, 3)), np.zeros(0)))
    for n, k in ((70, 1), (400, 2)):
        x, r = tools.globule(n, seed + k)
        parts.append((x + place(), r))
    xyz = np.concatenate([p[0] for p in parts])
    radii = np.concatenate([p[1] for p in parts])
    offsets = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.int64)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(radii), offsets
