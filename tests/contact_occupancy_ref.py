"""A plain-Python restatement of the residue contact occupancy map over a trajectory's interfaces (include/freesasa_gpu.h,
freesasa_gpu_contact_occupancy_open): the reduction of per-frame lists of folded rows into the run table - dicts, explicit loops,
Python floats - and the two fixtures the tests of tests/test_contact_occupancy.py and tests/test_contact_occupancy_gpu.py run on,
with what they have to hold (coverage()).  Fed only from tests/interface_residue_contacts_ref.py, tests/interface_contacts_ref.py
and tests/interfaces_ref.py; never from the entry under test.

    frame's rows   frame f as a batch of one structure has the folded rows of the residue-residue contact tables
    key            (g, h, side, res_a, res_b): the pair, 0 / 1 for a source segment in g / h, the source and the partner residue
                   within the system; a frame's keys ascend strictly; reversed: (g, h, 1 - side, res_b, res_a)
    run table      one row per distinct key, ascending: frames, frames_either (the key OR its reversed key has a row), the sums of
                   n_rows and n_points, area sum (in frame order, one addition at a time from 0.0) / min / max, first and last
                   frame, and the row of the reversed key or -1

A row of a frame is (key, n_rows, n_points, area).
"""
import functools

import numpy as np

import interface_contacts_ref as cr
import interface_residue_contacts_ref as qr
import interfaces_ref as ir

PROBE = cr.PROBE
TRAJ_POINTS = (100, 128)
COVERAGE_N = 100


def reversed_key(k):
    return (k[0], k[1], 1 - k[2], k[4], k[3])


def reduce(frames):
    """the run table of a list of frames (each a list of rows) as a dict of arrays: keys [U, 5] int32, frames [U] int64,
    frames_either [U] int64, counts [U, 2] int64, area [U, 3] fp64, span [U, 2] int64, reverse [U] int32 - and n_frames"""
    acc, either = {}, {}
    for f, rows in enumerate(frames):
        present = []
        for key, n_rows, n_points, area in rows:
            key, area = tuple(int(v) for v in key), float(area)
            present.append(key)
            a = acc.get(key)
            if a is None:
                acc[key] = [1, int(n_rows), int(n_points), 0.0 + area, area, area, f, f]
            else:
                a[0] += 1
                a[1] += int(n_rows)
                a[2] += int(n_points)
                a[3] = a[3] + area
                if area < a[4]:
                    a[4] = area
                if area > a[5]:
                    a[5] = area
                a[7] = f
        touched = set()
        for key in present:
            touched.add(key)
            touched.add(reversed_key(key))
        for key in touched:
            either[key] = either.get(key, 0) + 1
    keys = sorted(acc)
    where = {}
    for i, key in enumerate(keys):
        where[key] = i
    U = len(keys)
    out = dict(keys=np.zeros((U, 5), np.int32), frames=np.zeros(U, np.int64), frames_either=np.zeros(U, np.int64),
               counts=np.zeros((U, 2), np.int64), area=np.zeros((U, 3), np.float64), span=np.zeros((U, 2), np.int64),
               reverse=np.zeros(U, np.int32))
    for i, key in enumerate(keys):
        a = acc[key]
        out["keys"][i] = key
        out["frames"][i] = a[0]
        out["frames_either"][i] = either[key]
        out["counts"][i] = (a[1], a[2])
        out["area"][i] = (a[3], a[4], a[5])
        out["span"][i] = (a[6], a[7])
        out["reverse"][i] = where.get(reversed_key(key), -1)
    out["n_frames"] = len(frames)
    return out


COLUMNS = ("keys", "frames", "frames_either", "counts", "area", "span", "reverse")


def row_arrays(frames):
    """the frames as freesasa_gpu_contact_occupancy_add_rows takes them: frame_first [F + 1] int64, keys [q, 5] int32, counts
    [q, 2] int32, area [q] fp64"""
    first = np.zeros(len(frames) + 1, np.int64)
    keys, counts, area = [], [], []
    for f, rows in enumerate(frames):
        for key, n_rows, n_points, a in rows:
            keys.append(key); counts.append((n_rows, n_points)); area.append(a)
        first[f + 1] = len(keys)
    return (first, np.array(keys, np.int64).astype(np.int32).reshape(-1, 5), np.array(counts, np.int32).reshape(-1, 2),
            np.array(area, np.float64))


def frames_of_batch(n_frames, n_res, pair_struct, pair_groups, rescontact_offsets, residues, counts, area):
    """a batch of n_frames structures (every frame one) and its folded table, re-keyed: the rows of every frame"""
    frames = [[] for _ in range(n_frames)]
    for q in range(len(rescontact_offsets) - 1):
        p, side = q // 2, q % 2
        f = int(pair_struct[p])
        for t in range(int(rescontact_offsets[q]), int(rescontact_offsets[q + 1])):
            key = (int(pair_groups[p][0]), int(pair_groups[p][1]), side, int(residues[t][0]) - f * n_res, int(residues[t][1]) - f * n_res)
            frames[f].append((key, int(counts[t][0]), int(counts[t][1]), float(area[t])))
    return frames


def invariants(t, frame_counts=None):
    """the relations the issue states, on a table (a dict of COLUMNS): a list of the ones that do not hold"""
    bad = []
    keys = [tuple(int(v) for v in k) for k in t["keys"]]
    if any(not a < b for a, b in zip(keys, keys[1:])):
        bad.append("keys strictly ascending")
    rev, fr, ei = t["reverse"], t["frames"], t["frames_either"]
    for k in range(len(keys)):
        r = int(rev[k])
        if r >= 0:
            if int(rev[r]) != k or keys[r] != reversed_key(keys[k]):
                bad.append(f"reverse is an involution (row {k})")
            if ei[k] != ei[r] or not max(fr[k], fr[r]) <= ei[k] <= fr[k] + fr[r]:
                bad.append(f"frames_either of a row and its reverse (row {k})")
        elif ei[k] != fr[k] or reversed_key(keys[k]) in keys:
            bad.append(f"frames_either without a reverse (row {k})")
    if frame_counts is not None and int(fr.sum()) != int(np.asarray(frame_counts)[:, 1].sum()):
        bad.append("sum(frames) == sum(Q_f)")
    return bad


# ------------------------------------------------------------------ fixture LISTS: synthetic rows, no geometry

AREAS = (1e8, 1.0, -1e8, 0.1, 3.3e-7, 12345.678)


@functools.lru_cache(maxsize=None)
def lists_universe():
    """the keys the frames draw from, ascending: neighbours that differ only in the last component, only in side, residues up to
    2^31 - 1, groups up to 4095"""
    top = 2 ** 31 - 1
    keys = [(0, 1, s, a, b) for s in (0, 1) for a in range(20) for b in range(20)]
    keys += [(2, 3, s, top - a, top - b) for s in (0, 1) for a in range(10) for b in range(10)]
    keys += [(4094, 4095, s, a, b) for s in (0, 1) for a in range(15) for b in range(15)]
    return tuple(sorted(keys))


@functools.lru_cache(maxsize=None)
def lists_frames():
    """frames of 0, 1, 63, 64, 65, 256 and 257 rows and more - disjoint, identical, nested - over lists_universe()"""
    uni = lists_universe()
    n = len(uni)
    rng = np.random.default_rng(20261021)
    pick = lambda count: sorted(int(i) for i in rng.choice(n, count, replace=False))
    f64 = pick(64)
    f256 = [i for i in range(n) if i % 5 == 1][:256]
    tail = list(range(n - 450, n))
    plan = [[], [700], pick(63), f64, sorted(set(f64) | {3}), f256, sorted(set(f256) | {0}), f256, tail[::2], [], pick(300), pick(500),
            list(range(n)), [n - 1], [0, 1, 2]]
    frames = []
    for f, idx in enumerate(plan):
        rows = []
        for i in idx:
            n_rows = 1 + (i + f) % 5
            rows.append((uni[i], n_rows, n_rows + (i * f) % 100, AREAS[(f + 3 * i) % len(AREAS)]))
        frames.append(rows)
    return tuple(tuple(r) for r in frames)


# ------------------------------------------------------------------ fixture TRAJ: three groups, twelve frames

N_FRAMES = 12
SPACING = 1.9


@functools.lru_cache(maxsize=None)
def traj_system():
    """(radii [n], group [n] int32, n_groups, res_first [n_res + 1] int64): two 3 x 3 x 3 bodies A (group 0) and B (group 1), a cluster
    C of three atoms and a big atom (group 2), a small atom (group 0).  Residues of four atoms in input order: residue 6 holds three
    atoms of A and one of B; the big atom shares a residue with C; the small atom is a residue of its own."""
    n_body = 27
    radii = np.concatenate([1.2 + 0.1 * (np.arange(2 * n_body) % 7), [1.5, 1.6, 1.7], [6.0], [0.2]])
    group = np.concatenate([np.zeros(n_body), np.ones(n_body), np.full(4, 2), [0]]).astype(np.int32)
    n = len(radii)
    res_first = np.array(list(range(0, n - 1, 4)) + [n - 1, n], np.int64)
    for a in (radii, group, res_first):
        a.setflags(write=False)
    return radii, group, 3, res_first


def _body():
    """27 atoms on a grid, y slowest and x fastest: the last atom is a corner of the +x face, the first one of the -x face, and every
    residue has atoms on both"""
    return np.array([[ix, iy, iz] for iy in range(3) for iz in range(3) for ix in range(3)], float) * SPACING


@functools.lru_cache(maxsize=None)
def traj_frames():
    """xyz [F, n, 3]: B approaches A corner to corner, touches, slides down A's face and parts; C touches B in three frames (in frame 3 with
    keys of A's lower residues arriving too); the small
    atom sits inside the big one in the frames 1 .. 10; frames 5 and 6 are identical; frame 0 has no pair at all"""
    edge = 2 * SPACING
    far = 60.0
    #        gap     y / z offset of B     C at B?   small inside big?
    plan = [(30.0, (edge, edge), False, False),
            (4.6, (edge, edge), False, True),
            (3.6, (edge, edge), False, True),
            (3.0, (0.75 * edge, 0.75 * edge), True, True),
            (3.0, (0.5 * edge, 0.5 * edge), False, True),
            (3.0, (0.25 * edge, 0.5 * edge), False, True),
            (3.0, (0.25 * edge, 0.5 * edge), False, True),
            (2.8, (-0.5 * edge, -0.5 * edge), True, True),
            (2.8, (-1.0 * edge, -0.75 * edge), True, True),
            (4.4, (-1.0 * edge, -0.75 * edge), False, True),
            (9.0, (-1.0 * edge, -0.75 * edge), False, True),
            (30.0, (edge, edge), False, False)]
    assert len(plan) == N_FRAMES
    body = _body()
    big = np.array([0.0, -40.0, 0.0])
    frames = []
    for gap, (dy, dz), c_at_b, inside in plan:
        b = body + np.array([edge + gap, dy, dz])
        c = (b[[8, 17, 26]] + np.array([3.4, 0.0, 0.0])) if c_at_b else np.array([[far, far, far + 4.0 * k] for k in range(3)])
        small = big + np.array([2.0, 0.0, 0.0]) if inside else np.array([-far, far, 0.0])
        frames.append(np.concatenate([body, b, c, [big], [small]]))
    xyz = np.array(frames)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def traj_batch():
    """TRAJ's frames as ONE batch of F structures: (xyz [F n, 3], radii, offsets, group, n_groups [F], res_first)"""
    radii, group, n_groups, res_first = traj_system()
    xyz = traj_frames()
    F, n = xyz.shape[:2]
    brf = np.concatenate([res_first[:-1] + f * n for f in range(F)] + [[F * n]]).astype(np.int64)
    return xyz.reshape(-1, 3), np.tile(radii, F), np.arange(F + 1, dtype=np.int64) * n, np.tile(group, F), np.full(F, n_groups, np.int32), brf


@functools.lru_cache(maxsize=None)
def traj_folded(n_points):
    """the batch's pair table and folded table at n_points by the numpy restatements (interfaces_ref.table,
    interface_contacts_ref.masks / contacts, interface_residue_contacts_ref.fold): (pair_struct, pair_groups, fold dict)"""
    bx, br, offsets, bg, ng, brf = traj_batch()
    ps, pg, so, pa = ir.table(bx, br, offsets, bg, ng, PROBE)
    px, pr, _ = ir.pair_structures(bx, br, so, pa)
    unit = cr.unit_points(n_points)
    side, pair = cr.masks(px, pr, so, PROBE, unit)
    c = cr.contacts(px, pr, so, PROBE, unit, side, pair)
    return ps, pg, qr.fold(so, pa, brf, c["contact_first"], c["contact_partner"], c["contact_points"], c["contact_area"])


@functools.lru_cache(maxsize=None)
def traj_rows(n_points):
    """(frames, frame_counts [F, 2]) of TRAJ at n_points: the restated folded table, re-keyed"""
    F, n_res = N_FRAMES, len(traj_system()[3]) - 1
    ps, pg, f = traj_folded(n_points)
    counts = np.zeros((F, 2), np.int64)
    for s in ps:
        counts[s, 0] += 1
    frames = frames_of_batch(F, n_res, ps, pg, f["rescontact_offsets"], f["rescontact_residues"], f["rescontact_counts"], f["rescontact_area"])
    for k, rows in enumerate(frames):
        counts[k, 1] = len(rows)
    counts.setflags(write=False)
    return tuple(tuple(r) for r in frames), counts


def coverage():
    """what the fixtures hold, decided on this restatement alone: {kind: bool}"""
    out = {}
    frames, counts = traj_rows(COVERAGE_N)
    t = reduce(frames)
    keys = [tuple(int(v) for v in k) for k in t["keys"]]
    with_rows = int((counts[:, 1] > 0).sum())
    out["TRAJ: a frame with no pair at all"] = bool((counts[:, 0] == 0).any())
    out["TRAJ: a frame with two pairs"] = bool((counts[:, 0] == 2).any())
    out["TRAJ: a key present in one frame only"] = bool((t["frames"] == 1).any())
    # (a frame without a pair has no key, so "in all frames" is: in every frame that has a row)
    out["TRAJ: a key present in every frame that has rows"] = bool(with_rows >= 8 and (t["frames"] == with_rows).any())
    out["TRAJ: a key whose reverse never occurs"] = bool((t["reverse"] == -1).any())
    first = {k: int(s) for k, s in zip(keys, t["span"][:, 0])}
    out["TRAJ: a key that appears first in a later frame than its reverse"] = any(
        reversed_key(k) in first and first[reversed_key(k)] < first[k] for k in keys)
    out["TRAJ: two identical frames"] = any(frames[f] == frames[f + 1] and len(frames[f]) > 0 and
                                            np.array_equal(traj_frames()[f], traj_frames()[f + 1]) for f in range(len(frames) - 1))
    out["TRAJ: a residue split over two groups in contact with itself"] = any(k[3] == k[4] for k in keys)
    seen, mixed = set(), False
    for rows in frames:
        new = [r[0] for r in rows if r[0] not in seen]
        if seen and new:
            lo, hi = min(seen), max(seen)
            mixed = mixed or (min(new) < lo and max(new) > hi and any(lo < k < hi for k in new))
        seen.update(r[0] for r in rows)
    out["TRAJ: first occurrences of one frame before, among and behind the old rows"] = mixed
    out["TRAJ: about 12 frames of about 60 atoms, three groups"] = bool(traj_frames().shape == (N_FRAMES, 59, 3) and traj_system()[2] == 3)
    lf = lists_frames()
    sizes = [len(r) for r in lf]
    out["LISTS: frames of 0, 1, 63, 64, 65, 256 and 257 rows"] = {0, 1, 63, 64, 65, 256, 257} <= set(sizes)
    sets = [frozenset(r[0] for r in rows) for rows in lf]
    out["LISTS: disjoint, identical and nested frames"] = bool(
        any(a and b and not (a & b) for a in sets for b in sets) and any(sets[i] == sets[j] and sets[i] for i in range(len(sets)) for j in range(i))
        and any(a < b for a in sets for b in sets if a))
    sizes_u, seen = [], set()
    for s in sets:
        seen |= s
        sizes_u.append(len(seen))
    out["LISTS: U crosses 256 and 1024"] = bool(any(a < 256 < b for a, b in zip(sizes_u, sizes_u[1:])) and any(a < 1024 < b for a, b in zip(sizes_u, sizes_u[1:])))
    uni = lists_universe()
    out["LISTS: keys that differ only in the last component, only in side"] = bool(
        any(a[:4] == b[:4] and a[4] != b[4] for a, b in zip(uni, uni[1:])) and any(reversed_key(reversed_key(k)) == k and (k[0], k[1], 1 - k[2], k[3], k[4]) in uni for k in uni))
    out["LISTS: residues up to 2^31 - 1, groups up to 4095"] = bool(max(k[3] for k in uni) == 2 ** 31 - 1 and max(k[1] for k in uni) == 4095)
    # the order of addition shows: some key's areas, summed in another order, give another number
    tl = reduce(lf)
    shows = False
    for i, k in enumerate(tuple(int(v) for v in key) for key in tl["keys"]):
        xs = [r[3] for rows in lf for r in rows if r[0] == k]
        back = 0.0
        for x in reversed(xs):
            back = back + x
        shows = shows or back != tl["area"][i, 0]
    out["LISTS: the order of addition shows in the sum"] = shows
    return out
