"""A numpy restatement of the interfaces between chain groups (include/freesasa_gpu.h, freesasa_gpu_interfaces_dev): the contact
between two groups by brute force with the reference's neighbour test (ref: src/nb.c:487-491), the candidates by the boxes, the
table's order, side_offsets, and the pair structures cut on the host - and the EDGE BATCH the tests of tests/test_interfaces.py
and tests/test_interfaces_gpu.py run on, with what it has to hold (coverage()).  Every operation is numpy's, rounded on its own."""
import functools

import numpy as np

PROBE = 1.4
LDS_ATOMS = 1024      # IF_LDS_ATOMS (csrc/iface_kernels.h): the survivors of a side the contact kernel keeps in LDS
WORKGROUP = 256       # IF_B


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _cloud(rng, count, corner, edge=None):
    """count atoms in a cube (about 15 A^3 an atom unless edge is given) at corner, radii 1 .. 2"""
    edge = np.cbrt(15.0 * max(count, 1)) if edge is None else edge
    return np.asarray(corner, float) + rng.uniform(0, edge, (count, 3)), rng.uniform(1.0, 2.0, count)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """(xyz [n, 3], radii [n], offsets, group [n] int32, n_groups int32, names: the structures' kinds)"""
    rng = np.random.default_rng(20261019)
    structs, names = [], []

    def add(name, parts, ng):
        x = np.concatenate([p[0] for p in parts]).reshape(-1, 3)
        r = np.concatenate([p[1] for p in parts])
        g = np.concatenate([np.full(len(p[1]), p[2], np.int32) if np.isscalar(p[2]) else np.asarray(p[2], np.int32) for p in parts])
        structs.append((x, r, g, ng)); names.append(name)

    # groups of 0, 1, 63, 64, 65, 256 and 257 atoms, some touching, and atoms in no group
    parts = []
    for g, count in enumerate((0, 1, 63, 64, 65, 256, 257)):
        parts.append(_cloud(rng, count, (15.0 * (g % 4), 15.0 * (g // 4), 0.0)) + (g,))
    parts.append(_cloud(rng, 40, (0.0, 0.0, 0.0), 40.0) + (-1,))
    add("sizes", parts, 7)
    # three groups interleaved atom by atom
    x, r = _cloud(rng, 600, (0.0, 0.0, 0.0))
    add("interleaved", [(x, r, np.arange(600) % 3)], 3)
    add("one-group", [_cloud(rng, 300, (0.0, 0.0, 0.0)) + (0,)], 1)
    add("no-groups", [_cloud(rng, 50, (0.0, 0.0, 0.0)) + (-1,)], 0)
    # strict <: two one-atom groups at exactly r_i + r_j + 2 probe (no contact), two at nextafter below it (contact)
    s = (1.5 + PROBE) + (1.5 + PROBE)
    x = np.array([[0.0, 0.0, 0.0], [s, 0.0, 0.0], [0.0, 100.0, 0.0], [np.nextafter(s, 0.0), 100.0, 0.0]])
    add("strict", [(x, np.full(4, 1.5), np.arange(4))], 4)
    # globules placed diagonally: the boxes make the pair a candidate, no atoms touch
    add("diagonal", [_cloud(rng, 100, (0.0, 0.0, 0.0), 12.0) + (0,), _cloud(rng, 100, (16.5, 16.5, 16.5), 12.0) + (1,)], 2)
    # the hit lies beyond the first 256 atoms of both sides
    add("late-hit", [_cloud(rng, 300, (0.0, 0.0, 0.0)) + (0,), _cloud(rng, 60, (60.0, 0.0, 0.0), 10.0) + (0,),
                     _cloud(rng, 300, (200.0, 0.0, 0.0)) + (1,), _cloud(rng, 60, (66.0, 0.0, 0.0), 10.0) + (1,)], 2)
    # more survivors than LDS holds, with a hit: two groups interleaved in one cloud
    m = 2 * (LDS_ATOMS + 80)
    x, r = _cloud(rng, m, (0.0, 0.0, 0.0), 45.0)
    add("lds-overflow-hit", [(x, r, np.arange(m) % 2)], 2)
    # ... and without one: a sparse grid around atoms at the centres of its cells (8.66 A from the corners, cut-off 5.8)
    gi = np.stack(np.meshgrid(np.arange(11), np.arange(11), np.arange(10), indexing="ij"), -1).reshape(-1, 3) * 10.0
    ci = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(9), indexing="ij"), -1).reshape(-1, 3) * 10.0 + 5.0
    add("lds-overflow-miss", [(gi, np.full(len(gi), 1.5), 1), (ci, np.full(len(ci), 1.5), 0)], 2)

    xyz = np.concatenate([t[0] for t in structs]); radii = np.concatenate([t[1] for t in structs])
    group = np.concatenate([t[2] for t in structs]); n_groups = np.array([t[3] for t in structs], np.int32)
    for a in (xyz, radii, group, n_groups):
        a.setflags(write=False)
    return xyz, radii, _offsets([len(t[1]) for t in structs]), group, n_groups, tuple(names)


def members(offsets, group, s, g):
    """the input atoms of group g of structure s, in input order"""
    return offsets[s] + np.nonzero(group[offsets[s]:offsets[s + 1]] == g)[0]


def contact_matrix(xyz, radii, ia, ja, probe=PROBE):
    """[len(ia), len(ja)] bool: the reference's neighbour test between atoms ia and ja, operand for operand"""
    ri, rj = radii[ia] + probe, radii[ja] + probe
    s = ri[:, None] + rj[None, :]
    cut2 = s * s
    dx = xyz[ja, 0][None, :] - xyz[ia, 0][:, None]
    dy = xyz[ja, 1][None, :] - xyz[ia, 1][:, None]
    dz = xyz[ja, 2][None, :] - xyz[ia, 2][:, None]
    return dx * dx + dy * dy + dz * dz < cut2


def box(xyz, radii, ia, probe=PROBE):
    if len(ia) == 0:
        return np.full(3, np.inf), np.full(3, -np.inf), 0.0
    return xyz[ia].min(axis=0), xyz[ia].max(axis=0), float((radii[ia] + probe).max())


def screen(xyz, radii, offsets, group, n_groups, probe=PROBE):
    """every test in the table's order: (tests [T, 3] = (s, g, h), candidate [T] bool, contact [T] bool)"""
    tests, cand, hit = [], [], []
    for s in range(len(offsets) - 1):
        mem = [members(offsets, group, s, g) for g in range(n_groups[s])]
        boxes = [box(xyz, radii, m, probe) for m in mem]
        for g in range(n_groups[s]):
            for h in range(g + 1, n_groups[s]):
                (lg, hg, rg), (lh, hh, rh) = boxes[g], boxes[h]
                c = rg + rh
                tests.append((s, g, h))
                cand.append(bool(np.all(lh - hg < c) and np.all(lg - hh < c)))
                hit.append(bool(len(mem[g]) and len(mem[h]) and contact_matrix(xyz, radii, mem[g], mem[h], probe).any()))
    return np.array(tests, np.int32).reshape(-1, 3), np.array(cand, bool), np.array(hit, bool)


def table(xyz, radii, offsets, group, n_groups, probe=PROBE):
    """(pair_struct [P], pair_groups [P, 2], side_offsets [2P + 1], pair_atom [M]) of the batch"""
    tests, _, hit = screen(xyz, radii, offsets, group, n_groups, probe)
    rows = tests[hit]
    sides = [members(offsets, group, s, k) for s, g, h in rows for k in (g, h)]
    pair_atom = np.concatenate(sides).astype(np.int32) if sides else np.zeros(0, np.int32)
    return rows[:, 0].copy(), rows[:, 1:].copy(), _offsets([len(x) for x in sides]), pair_atom


def pair_structures(xyz, radii, side_offsets, pair_atom):
    """the pair structures cut on the host: a batch (xyz, radii, offsets) of P structures"""
    return xyz[pair_atom], radii[pair_atom], side_offsets[::2].copy()


def coverage():
    """what the edge batch holds, decided on this restatement alone: {kind: bool}"""
    xyz, radii, offsets, group, n_groups, names = edge_batch()
    tests, cand, hit = screen(xyz, radii, offsets, group, n_groups)
    sizes = {int(len(members(offsets, group, s, g))) for s in range(len(n_groups)) for g in range(n_groups[s])}
    out = {"sizes": {0, 1, 63, 64, 65, 256, 257} <= sizes,
           "no-group atoms": bool((group < 0).any() and any((group[offsets[s]:offsets[s + 1]] < 0).any() and n_groups[s] > 0 for s in range(len(n_groups)))),
           "one group": bool((n_groups == 1).any()), "no groups": bool((n_groups == 0).any()),
           "local ids": bool(any(hit[k] and int(np.sum(n_groups[:tests[k, 0]])) > 0 for k in range(len(tests)))),
           "candidate without contact": bool((cand & ~hit).any()), "contact implies candidate": bool(np.all(cand[hit]))}
    s = names.index("interleaved")
    g = group[offsets[s]:offsets[s + 1]]
    out["interleaved"] = bool(np.all(g[1:] != g[:-1]))
    s = names.index("strict")
    k = {(int(a), int(b)): i for i, (t, a, b) in enumerate(tests) if t == s}
    ia, ib = members(offsets, group, s, 0), members(offsets, group, s, 1)
    d = xyz[ib[0], 0] - xyz[ia[0], 0]
    out["exact distance: no contact"] = bool(d == (radii[ia[0]] + PROBE) + (radii[ib[0]] + PROBE) and not hit[k[(0, 1)]])
    ic, idd = members(offsets, group, s, 2), members(offsets, group, s, 3)
    out["nextafter below: contact"] = bool(xyz[idd[0], 0] - xyz[ic[0], 0] == np.nextafter(d, 0.0) and hit[k[(2, 3)]])
    s = names.index("late-hit")
    cm = contact_matrix(xyz, radii, members(offsets, group, s, 0), members(offsets, group, s, 1))
    ii, jj = np.nonzero(cm)
    out["hit beyond the first 256 of both sides"] = bool(len(ii) and ii.min() >= WORKGROUP and jj.min() >= WORKGROUP)
    for name, want in (("lds-overflow-hit", True), ("lds-overflow-miss", False)):
        s = names.index(name)
        a, b = members(offsets, group, s, 0), members(offsets, group, s, 1)
        (la, ha, ra), (lb, hb, rb) = box(xyz, radii, a), box(xyz, radii, b)
        rb_i = radii[b] + PROBE
        surv = np.all((xyz[b] - ha < (rb_i + ra)[:, None]) & (la - xyz[b] < (rb_i + ra)[:, None]), axis=1)
        ra_i = radii[a] + PROBE
        surv_a = np.all((xyz[a] - hb < (ra_i + rb)[:, None]) & (lb - xyz[a] < (ra_i + rb)[:, None]), axis=1)
        t = [i for i, (u, _, _) in enumerate(tests) if u == s][0]
        out[name] = bool(surv.sum() > LDS_ATOMS and surv_a.any() and hit[t] == want and cand[t])
    return out
