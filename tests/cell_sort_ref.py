"""TESTS ONLY: what the cell sort must produce, in plain numpy, and the inputs that reach its edges.

The cell sort (freesasa_amd/csrc/sasa_kernels.h K1..K5, gpu_kernels.hip k_sort_struct) gives every structure of a batch the
reference's cell grid (src/nb.c:61-69: lower corner = min - d/2, d = 2 max(radius + probe), cells per axis = ceil((max + d/2 -
corner) / d)), every atom its cell (src/nb.c:74-83, 137-140: (int)((v - corner) / d), x fastest), and hands the tile kernels the
atoms in cell order with a table that says where every cell's atoms begin.  Everything it writes is an integer or a copied
double, and its few floating-point operations are single IEEE operations numpy repeats bit for bit: every comparison here is
exact.  No import of the library: Reference is the definition, check_sorted holds one pass's outputs (the test hook's, or the
emulation's) to it, and the case builders assert that they reach the edge they are named for."""
import numpy as np

import tools

SORT_ATOMS = 16128              # engine_internal.h: atoms of a structure k_sort_struct holds
SORT_CELLS = 1 << 18            # ... cells it holds in LDS at a time (a pass)
SORT_CELL_BITS = 26             # ... cells of a structure it numbers
PIPE_B = 256                    # sasa_kernels.h SASA_PIPE_B: the general pipeline's workgroup
SCAN_BLOCK = 256 * 16           # ... cells of one block of the chained scan
BOUNDS_CHUNK = 4096             # ... atoms of one bounds chunk
X0, X1, Y0, Y1, Z0, Z1 = 1, 2, 4, 8, 16, 32   # CELL_*: the faces of its structure's grid an atom's cell lies on
ERR_BAD_RADIUS, ERR_GRID_TOO_BIG, ERR_BAD_COORD = 1, 2, 3
ONES32 = np.int32(-1)
ONES64 = np.uint64(0xFFFFFFFFFFFFFFFF)
PROBE = 1.5                     # with radii 0.5: d = 4 exactly
# the records and status words of the test hook (include/freesasa_gpu.h, freesasa_gpu_cell_sort_dev)
STATUS_WORDS, ST_ERROR, ST_OCC_SUM, ST_OCC_N, ST_RETRY, ST_CELLS = 142, 0, 4, 5, 7, 140
GRID = np.dtype([("x0", "<f8"), ("y0", "<f8"), ("z0", "<f8"), ("d", "<f8"), ("nx", "<i4"), ("ny", "<i4"), ("nz", "<i4"), ("cell_base", "<i4")])
IDX = np.dtype([("cell", "<i8"), ("orig", "<i4"), ("strct", "<i4")])


def cell_pack_grid(nx, ny):
    return (nx << 6) | (ny << 19) if nx < 8192 and ny < 8192 else 0


def popcount32(v):
    v = np.asarray(v, dtype=np.uint64)
    v = v - ((v >> np.uint64(1)) & np.uint64(0x55555555))
    v = (v & np.uint64(0x33333333)) + ((v >> np.uint64(2)) & np.uint64(0x33333333))
    v = (v + (v >> np.uint64(4))) & np.uint64(0x0F0F0F0F)
    return ((v * np.uint64(0x01010101)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)


def compact_first_atom(cell_tbl, cell_first, x):
    """cell_first_atom / cell_rank of sasa_kernels.h over a compact table, for an array of batch-wide cells"""
    x = np.asarray(x, dtype=np.int64)
    w = cell_tbl[x >> 5]
    below = (w & np.uint64(0xFFFFFFFF)) & ((np.uint64(1) << (x & 31).astype(np.uint64)) - np.uint64(1))
    return cell_first[(w >> np.uint64(32)).astype(np.int64) + popcount32(below).astype(np.int64)]


def take_of(C, arrangement):
    """cells of the batch-wide numbering a structure of C cells takes"""
    return C if arrangement == 0 else C + 1 if arrangement == 1 else (C + 1 + 31) & ~31


class Reference:
    """grid, cells, flags and the dense definition of the table for one batch"""

    def __init__(self, xyz, radii, offsets, probe, shared_radii=False):
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.radii = np.ascontiguousarray(radii, dtype=np.float64)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.probe, self.shared = float(probe), bool(shared_radii)
        ns, n = self.offsets.size - 1, int(self.offsets[-1])
        self.ns, self.n = ns, n
        self.strct = np.repeat(np.arange(ns), np.diff(self.offsets))
        self.ridx = np.arange(n) - self.offsets[self.strct] if self.shared else np.arange(n)
        self.rp = self.radii[self.ridx] + self.probe                      # src/sasa_lr.c:136
        self.corner = np.zeros((ns, 3))
        self.d = np.ones(ns)
        self.dims = np.zeros((ns, 3), dtype=np.int64)
        self.cell = np.zeros(n, dtype=np.int64)                           # within the structure
        self.high = np.zeros(n, dtype=np.int64)                           # flags | cell_pack_grid
        self.sorted_cells = []                                            # per structure, ascending
        for s in range(ns):
            b, e = int(self.offsets[s]), int(self.offsets[s + 1])
            if e == b:
                self.sorted_cells.append(np.zeros(0, dtype=np.int64))
                continue
            p = self.xyz[b:e]
            d = 2 * max(0.0, float(self.rp[b:e].max()))                   # src/nb.c:543
            corner = p.min(axis=0) - d / 2.                               # src/nb.c:61-66
            dims = np.ceil((p.max(axis=0) + d / 2. - corner) / d).astype(np.int64)   # src/nb.c:67-69
            idx = ((p - corner) / d).astype(np.int64)                     # src/nb.c:137-140
            assert (idx >= 0).all() and (idx < dims).all()
            self.corner[s], self.d[s], self.dims[s] = corner, d, dims
            self.cell[b:e] = idx[:, 0] + dims[0] * (idx[:, 1] + dims[1] * idx[:, 2])   # src/nb.c:74-83
            fl = np.zeros(e - b, dtype=np.int64)
            for k, (f0, f1) in enumerate(((X0, X1), (Y0, Y1), (Z0, Z1))):
                fl |= np.where(idx[:, k] == 0, f0, 0) | np.where(idx[:, k] == dims[k] - 1, f1, 0)
            self.high[b:e] = fl | cell_pack_grid(int(dims[0]), int(dims[1]))
            self.sorted_cells.append(np.sort(self.cell[b:e]))
        self.C = self.dims.prod(axis=1)

    def first(self, s, x):
        """the dense definition: offsets[s] + the atoms of s in cells < x, x in [0, C]"""
        return self.offsets[s] + np.searchsorted(self.sorted_cells[s], np.asarray(x, dtype=np.int64), side="left")

    def occupied(self, s):
        return np.unique(self.sorted_cells[s])

    def total(self, arrangement):
        """the batch's cell total: k_sort_struct numbers the structures that hold atoms only"""
        if arrangement == 0:
            return int(self.C.sum())
        return int(sum(take_of(int(c), arrangement) for c, m in zip(self.C, np.diff(self.offsets)) if m > 0))

    def population(self):
        """per atom, the atoms in its cell"""
        key = self.strct.astype(np.int64) * (int(self.C.max()) + 1) + self.cell
        _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        return cnt[inv]

    def passes(self, s):
        return -(-int(self.C[s]) // SORT_CELLS)

    def pass_atoms(self, s):
        return np.bincount(self.sorted_cells[s] // SORT_CELLS, minlength=self.passes(s))

    def expected(self, arrangement, cells_cap=None, order=None, occ_stride=None):
        """outputs as a good pass leaves them, made from the definition alone (atoms inside a cell in the caller's order, the
        structures' runs in the order `order` of the structures that hold atoms): what check_sorted is itself checked with"""
        ns, n = self.ns, self.n
        total = self.total(arrangement)
        cap = total if cells_cap is None else cells_cap
        live = [s for s in range(ns) if self.offsets[s + 1] > self.offsets[s]]
        base = np.zeros(ns, dtype=np.int64)
        if arrangement == 0:
            base = np.concatenate([[0], np.cumsum(self.C)[:-1]])
        else:
            run = 0
            for s in (live if order is None else order):
                base[s] = run
                run += take_of(int(self.C[s]), arrangement)
        grid = np.zeros(ns, dtype=GRID)
        grid["x0"], grid["y0"], grid["z0"] = self.corner.T
        grid["d"], grid["cell_base"] = self.d, base
        grid["nx"], grid["ny"], grid["nz"] = self.dims.T
        perm = np.lexsort((np.arange(n), self.cell, self.strct))
        s_idx = np.zeros(n, dtype=IDX)
        s_idx["orig"], s_idx["strct"] = perm, self.strct[perm]
        s_idx["cell"] = ((base[self.strct[perm]] + self.cell[perm]).astype(np.uint64) | (self.high[perm].astype(np.uint64) << np.uint64(32))).view(np.int64)
        stride = occ_stride or (n // 256 if n >= 256 else 1)
        sample = np.arange(0, n, stride)
        status = np.zeros(STATUS_WORDS, dtype=np.int32)
        status[ST_OCC_SUM], status[ST_OCC_N] = self.population()[sample].sum(), sample.size
        status[ST_CELLS:ST_CELLS + 2] = np.array([total], dtype=np.int64).view(np.int32)
        out = {"status": status, "error": 0, "retry": 0, "occ_sum": int(status[ST_OCC_SUM]), "occ_n": int(status[ST_OCC_N]), "cells": total,
               "occ_stride": stride, "cells_cap": cap, "grid": grid, "ncells": self.C.copy(),
               "sq": np.column_stack([self.xyz[perm], self.rp[perm]]), "s_idx": s_idx}
        if arrangement < 2:
            cs = np.full(cap + 2, -1, dtype=np.int32) if arrangement else np.zeros(cap + 2, dtype=np.int32)
            for s in (range(ns) if arrangement == 0 else live):
                C = int(self.C[s])
                cs[base[s]:base[s] + C + 1] = self.first(s, np.arange(C + 1))
            out["cell_start"] = cs
        else:
            tbl = np.full((cap >> 5) + 2, ONES64, dtype=np.uint64)
            first = np.full(n + ns + 2, -1, dtype=np.int32)
            for s in live:
                bits, pre, occ = self.compact_words(s)
                tbl[base[s] >> 5:(base[s] >> 5) + bits.size] = bits | (pre << np.uint64(32))
                k0 = int(self.offsets[s]) + s
                first[k0:k0 + occ.size] = self.first(s, occ)
                first[k0 + occ.size] = self.offsets[s + 1]
            out["cell_tbl"], out["cell_first"] = tbl, first
        return out

    def compact_words(self, s):
        """per 32 cells of structure s (cells [0, C]): the occupancy bitmap, offsets[s] + s + the occupied cells before the
        word; and the occupied cells"""
        C, occ = int(self.C[s]), self.occupied(s)
        bits = np.zeros(-(-(C + 1) // 32), dtype=np.uint64)
        np.bitwise_or.at(bits, occ >> 5, np.uint64(1) << (occ & 31).astype(np.uint64))
        before = np.concatenate([[0], np.cumsum(popcount32(bits).astype(np.int64))[:-1]])
        return bits, (before + int(self.offsets[s]) + s).astype(np.uint64), occ


def check_sorted(out, xyz, radii, offsets, probe, arrangement, shared_radii=False, ref=None, sample_above=1 << 24):
    """everything a good pass must satisfy (ST_ERROR == 0 and ST_RETRY == 0); returns the per-atom cells within the structures,
    indexed by the caller's atom order: equal between arrangements where the cells hold the same sets of atoms"""
    R = ref if ref is not None else Reference(xyz, radii, offsets, probe, shared_radii)
    ns, n, offs = R.ns, R.n, R.offsets
    live = np.flatnonzero(np.diff(offs) > 0)
    assert out["error"] == 0 and out["retry"] == 0, (out["error"], out["retry"])
    # ---- grid
    g = out["grid"]
    for k, name in enumerate(("x0", "y0", "z0")):
        assert g[name].tobytes() == R.corner[:, k].copy().tobytes(), name
    assert g["d"].tobytes() == R.d.tobytes()
    assert np.array_equal(g["nx"], R.dims[:, 0]) and np.array_equal(g["ny"], R.dims[:, 1]) and np.array_equal(g["nz"], R.dims[:, 2])
    assert np.array_equal(out["ncells"], R.C)
    empty = np.diff(offs) == 0
    assert (R.C[empty] == 0).all() and (R.d[empty] == 1).all() and (R.dims[empty] == 0).all() and (R.corner[empty] == 0).all()
    # ---- cell bases and the total
    base = g["cell_base"].astype(np.int64)
    total = R.total(arrangement)
    assert out["cells"] == total, (out["cells"], total)
    assert total <= out["cells_cap"]
    if arrangement == 0:
        assert np.array_equal(base, np.concatenate([[0], np.cumsum(R.C)[:-1]]))
    else:
        take = np.array([take_of(int(c), arrangement) for c in R.C[live]], dtype=np.int64)
        o = np.argsort(base[live], kind="stable")
        b_sorted, t_sorted = base[live][o], take[o]
        assert b_sorted[0] == 0 and np.array_equal(b_sorted[1:], (b_sorted + t_sorted)[:-1]) and b_sorted[-1] + t_sorted[-1] == total
        if arrangement == 2:
            assert (base[live] % 32 == 0).all()
        assert (base[empty] == 0).all()                      # (a structure without atoms takes no run: as grid_struct leaves it)
    # ---- sorted records
    si, sq = out["s_idx"], out["sq"]
    assert np.array_equal(si["strct"], R.strct)
    orig = si["orig"].astype(np.int64)
    assert np.array_equal(np.sort(orig), np.arange(n)) and np.array_equal(R.strct[orig], R.strct)   # a permutation of every structure's range
    want_sq = np.column_stack([R.xyz[orig], R.rp[orig]])
    assert sq.tobytes() == want_sq.tobytes()
    low, high = si["cell"] & 0xFFFFFFFF, (si["cell"].view(np.uint64) >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(low, base[R.strct] + R.cell[orig])
    assert np.array_equal(high, R.high[orig])
    step = np.diff(low)
    assert (step[R.strct[1:] == R.strct[:-1]] >= 0).all()
    # ---- the table
    if arrangement < 2:
        cs = out["cell_start"]
        assert cs.size == out["cells_cap"] + 2
        for s in (range(ns) if arrangement == 0 else live):
            C = int(R.C[s])
            assert np.array_equal(cs[base[s]:base[s] + C + 1], R.first(s, np.arange(C + 1))), s
        if arrangement == 1:
            assert (cs[total:] == ONES32).all()              # (the runs tile [0, total): everything outside them)
    else:
        tbl, first = out["cell_tbl"], out["cell_first"]
        assert tbl.size == (out["cells_cap"] >> 5) + 2 and first.size == n + ns + 2
        rng = np.random.default_rng(5)
        own_word, own_first = np.zeros(tbl.size, dtype=bool), np.zeros(first.size, dtype=bool)
        for s in live:
            C = int(R.C[s])
            bits, pre, occ = R.compact_words(s)
            w = tbl[base[s] >> 5:(base[s] >> 5) + bits.size]
            assert np.array_equal(w & np.uint64(0xFFFFFFFF), bits), s      # (no bit at or beyond C: `bits` has none)
            assert np.array_equal(w >> np.uint64(32), pre), s
            k0, k1 = int(offs[s]) + s, int(offs[s + 1]) + s + 1
            assert np.array_equal(first[k0:k0 + occ.size], R.first(s, occ)), s
            assert first[k0 + occ.size] == offs[s + 1]
            assert (first[k0 + occ.size + 1:k1] == ONES32).all(), s
            assert not own_word[base[s] >> 5:(base[s] >> 5) + bits.size].any() and not own_first[k0:k0 + occ.size + 1].any(), s
            own_word[base[s] >> 5:(base[s] >> 5) + bits.size] = own_first[k0:k0 + occ.size + 1] = True
            if C + 1 <= sample_above:
                x = np.arange(C + 1)
            else:
                x = np.unique(np.clip(np.concatenate([occ - 1, occ, occ + 1, rng.integers(0, C + 1, 100_000), [0, C]]), 0, C))
            assert np.array_equal(compact_first_atom(tbl, first, base[s] + x), R.first(s, x)), s
        # everything else - table words that are no structure's, below the total or beyond it; the entries of cell_first behind a
        # structure's occupied cells, the slot of a structure without atoms, the two behind them all - is nobody's to write
        assert (tbl[~own_word] == ONES64).all() and (first[~own_first] == ONES32).all()
        assert own_word[:total >> 5].all()                   # (the structures' runs tile the numbering in 32s)
    # ---- density samples
    stride = out["occ_stride"]
    assert out["occ_n"] == -(-n // stride)
    assert out["occ_sum"] == int(R.population()[::stride].sum())
    loc = np.empty(n, dtype=np.int64)
    loc[orig] = low - base[R.strct]
    return loc


# ------------------------------------------------------------------------------------------------ inputs

def cells_of(dims, ijk):
    ijk = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    return ijk[:, 0] + dims[0] * (ijk[:, 1] + dims[1] * ijk[:, 2])


def lattice(dims, cells, seed=0, origin=(0.0, 0.0, 0.0), open_last=False):
    """One structure whose grid is dims by construction (radii 0.5, probe 1.5: d = 4): the atoms, in the order of `cells` (cells
    within the structure), at 4 (i, j, k) + a jitter within (-1.9, 1.9) clipped to the box [0, 4 (dims - 1)]; the first atom of
    cell 0 sits on the box's lower corner and - unless open_last, where the first atoms of the cells (nx-1, 0, 0), (0, ny-1, 0)
    and (0, 0, nz-1) span the box and the last cell may stay empty - the first atom of the last cell on its upper one."""
    dims = np.asarray(dims, dtype=np.int64)
    cells = np.asarray(cells, dtype=np.int64)
    C = int(dims.prod())
    assert cells.size and cells.min() >= 0 and cells.max() < C
    ijk = np.stack([cells % dims[0], cells // dims[0] % dims[1], cells // (dims[0] * dims[1])], axis=1)
    top = 4.0 * (dims - 1)
    p = np.clip(4.0 * ijk + np.random.default_rng(seed).uniform(-1.9, 1.9, ijk.shape), 0.0, top)
    pins = [(0, np.zeros(3))]
    if open_last:
        for k in range(3):
            v = np.zeros(3, dtype=np.int64)
            v[k] = dims[k] - 1
            pins.append((int(cells_of(dims, v)[0]), 4.0 * v))
    else:
        pins.append((C - 1, top))
    done = set()
    for c, where in pins:
        if c in done:
            continue
        done.add(c)
        at = np.flatnonzero(cells == c)
        assert at.size, "the cell sequence must hold cell %d" % c
        p[at[0]] = where if c else 0.0
    if open_last:                                            # every pin fixes one axis only; together they span the box
        assert (p.max(axis=0) == top).all() and (p.min(axis=0) == 0).all()
    return p + np.asarray(origin, dtype=np.float64), np.full(cells.size, 0.5)


def random_cells(dims, n, seed, distinct=False, keep=None, open_last=False):
    """n cells of the grid with cell 0 and the last cell (open_last: the three axis ends instead) among them, shuffled;
    keep: a predicate on cells the random ones satisfy"""
    dims = np.asarray(dims, dtype=np.int64)
    C = int(dims.prod())
    rng = np.random.default_rng(seed)
    ends = [0]
    if open_last:
        for k in range(3):
            v = np.zeros(3, dtype=np.int64)
            v[k] = dims[k] - 1
            ends.append(int(cells_of(dims, v)[0]))
    else:
        ends.append(C - 1)
    ends = list(dict.fromkeys(ends))[:max(n, 1)]
    if distinct:
        pool = np.setdiff1d(np.arange(C), ends)
        if keep is not None:
            pool = pool[keep(pool)]
        more = rng.choice(pool, n - len(ends), replace=False)
    else:
        more = rng.integers(0, C - 1 if open_last else C, 4 * n + 64)
        if keep is not None:
            more = more[keep(more)]
        more = more[:n - len(ends)]
        assert more.size == n - len(ends)
    cells = np.concatenate([np.array(ends, dtype=np.int64), more.astype(np.int64)])
    rng.shuffle(cells)
    return cells


class Case:
    """a batch and what it claims to reach: claims holds (name, predicate over the Reference) pairs.  parts: the structures
    as (xyz, radii) pairs, or a function that makes them - the batch is built when a test first asks for it, not when the
    test modules are collected"""

    def __init__(self, name, parts, claims=(), probe=PROBE, shared_radii=False, arrangements=(0, 1, 2), cells_cap=0, radii=None):
        self.name, self.probe, self.shared, self.arrangements, self.cells_cap = name, probe, shared_radii, tuple(arrangements), cells_cap
        self._parts, self._radii, self._batch = parts, radii, None
        self.claims = list(claims)
        self._ref = None

    def _built(self):
        if self._batch is None:
            parts = self._parts() if callable(self._parts) else self._parts
            radii = self._radii() if callable(self._radii) else self._radii
            xyz = np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1, 3) for p in parts])
            offsets = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
            self._batch = (xyz, offsets, np.concatenate([p[1] for p in parts]) if radii is None else np.asarray(radii, dtype=np.float64))
        return self._batch

    xyz = property(lambda self: self._built()[0])
    offsets = property(lambda self: self._built()[1])
    radii = property(lambda self: self._built()[2])

    @property
    def ref(self):
        if self._ref is None:
            self._ref = Reference(self.xyz, self.radii, self.offsets, self.probe, self.shared)
        return self._ref

    def cap(self, arrangement):
        """the cells_cap to run the case with: its own; else 0 (the engine's sizing of a first batch) where that holds the
        batch, and for the sparse lattices, which it does not hold, a little more than they need"""
        if self.cells_cap:
            return self.cells_cap
        total = self.ref.total(arrangement)
        return 0 if total <= 10 * self.ref.n + 256 * self.ref.ns else total + 7

    def check_claims(self):
        for what, holds in self.claims:
            assert holds(self.ref), (self.name, what)

    def __repr__(self):
        return self.name


def dims_are(*dims, s=0):
    return ("the grid is %s" % "x".join(map(str, dims)), lambda R: tuple(R.dims[s]) == dims)


def one(name, dims, n, seed=1, claims=(), **kw):
    """one lattice structure of n atoms in random cells"""
    opts = {k: kw.pop(k) for k in ("distinct", "keep", "open_last") if k in kw}
    return Case(name, lambda: [lattice(dims, random_cells(dims, n, seed, **opts), seed, open_last=opts.get("open_last", False))],
                [dims_are(*dims)] + list(claims), **kw)


def passes_are(k, held, s=0):
    return ("%d passes, atoms in %s" % (k, held), lambda R: R.passes(s) == k and list(R.pass_atoms(s) > 0) == list(held))


def small_batch(n_structs, seed, empties=(), sizes=(1, 40)):
    """structures of a few atoms in small grids at scattered origins, empty ones where asked"""
    rng = np.random.default_rng(seed)
    parts = []
    for s in range(n_structs):
        if s in empties:
            parts.append((np.zeros((0, 3)), np.zeros(0)))
            continue
        n = int(rng.integers(sizes[0], sizes[1] + 1))
        dims = (1, 1, 1) if n == 1 else tuple(int(v) for v in rng.integers(1, 6, 3))
        if n > 1 and dims == (1, 1, 1):
            dims = (2, 1, 1)
        parts.append(lattice(dims, random_cells(dims, n, seed * 1000 + s), seed * 1000 + s, origin=rng.uniform(-300, 300, 3).round(1)))
    return parts


def line(nx, n=None, seed=1):
    """a structure of nx x 1 x 1 cells"""
    return lattice((nx, 1, 1), random_cells((nx, 1, 1), n or max(2, min(nx, 24)), seed), seed)


def cells_total_is(t):
    return ("%d cells in all" % t, lambda R: int(R.C.sum()) == t)


def ordered(name, seq, claims, dims=(6, 1, 1)):
    return Case(name, lambda: [lattice(dims, np.asarray(seq), 3)], [dims_are(*dims)] + list(claims))


def global_cells(R):
    return np.concatenate([[0], np.cumsum(R.C)[:-1]])[R.strct] + R.cell


def cases_fused():
    """a. the shapes of k_sort_struct"""
    out = []
    for n in (1, 2, 3, 64, 65, 1023, 1024, 1025):
        out.append(one("%d atoms" % n, (1, 1, 1) if n == 1 else (5, 4, 3), n, seed=n))
    out.append(Case("SORT_ATOMS atoms in one cell", lambda: [(np.zeros((SORT_ATOMS, 3)) + 7.25, np.full(SORT_ATOMS, 0.5))],
                    [dims_are(1, 1, 1), ("every atom has all six flags", lambda R: (R.high & 63 == 63).all())]))
    out.append(one("SORT_ATOMS atoms, a cell each", (128, 126, 1), SORT_ATOMS, distinct=True,
                   claims=[("occ == n == C", lambda R: R.occupied(0).size == R.n == R.C[0] == SORT_ATOMS)]))
    for n, dims in ((7, (7, 1, 1)), (8, (4, 2, 1)), (1001, (11, 13, 7)), (2000, (20, 10, 10))):
        out.append(one("occ == n, n = %d" % n, dims, n, distinct=True, seed=n, claims=[("occ == n", lambda R: R.occupied(0).size == R.n)]))
    out.append(Case("one cell, three atoms", lambda: [(np.zeros((3, 3)) - 2.5, np.full(3, 0.5))],
                    [dims_are(1, 1, 1), ("every atom has all six flags", lambda R: (R.high & 63 == 63).all())]))
    for dims in ((31, 1, 1), (4, 4, 2), (8, 4, 1), (33, 1, 1)):
        C = int(np.prod(dims))
        out.append(one("%d cells (%s)" % (C, "x".join(map(str, dims))), dims, 40, seed=C + dims[0], claims=[("C % 32", lambda R, C=C: R.C[0] % 32 == C % 32)]))
    out.append(one("C % 32 == 0, last cell occupied", (8, 4, 3), 50, claims=[
        ("", lambda R: R.C[0] % 32 == 0 and R.sorted_cells[0][-1] == R.C[0] - 1)]))
    out.append(one("C % 32 == 0, last cell empty", (8, 4, 3), 50, open_last=True, claims=[
        ("", lambda R: R.C[0] % 32 == 0 and R.sorted_cells[0][-1] < R.C[0] - 1)]))
    for dims in ((1, 5, 4), (5, 1, 4), (5, 4, 1)):
        k = dims.index(1)
        out.append(one("a grid one cell wide (%s)" % "x".join(map(str, dims)), dims, 60, seed=k + 1, claims=[
            ("both flags of the axis on every atom", lambda R, k=k: ((R.high >> (2 * k)) & 3 == 3).all())]))
    for dims, packed in (((8191, 3, 1), True), ((8192, 2, 2), False), ((2, 8192, 2), False)):
        out.append(one("%s" % "x".join(map(str, dims)), dims, 50, seed=dims[0], claims=[
            ("cell_pack_grid", lambda R, packed=packed: ((R.high >> 6 != 0) == packed).all())]))
    edge = [SORT_CELLS - 1, SORT_CELLS]
    out.append(one("64x64x64: one pass, the sentinel word", (64, 64, 64), 300, claims=[
        passes_are(1, [True]), ("C == SORT_CELLS", lambda R: R.C[0] == SORT_CELLS)]))
    for dims in ((65, 64, 64), (64, 64, 65)):
        C = int(np.prod(dims))
        out.append(Case("%s: two passes" % "x".join(map(str, dims)), lambda dims=dims: [lattice(dims, np.concatenate([random_cells(dims, 300, 9), edge, edge]), 9)], [dims_are(*dims), passes_are(2, [True, True]), (
            "atoms on both sides of the pass boundary, a second pass of 4096 cells",
            lambda R, C=C: C - SORT_CELLS == 4096 and {SORT_CELLS - 1, SORT_CELLS} <= set(R.sorted_cells[0].tolist()))]))
    out.append(Case("65x64x64: the second pass holds the corner only", lambda: [lattice((65, 64, 64), random_cells((65, 64, 64), 300, 10, keep=lambda c: c < SORT_CELLS), 10)], [
        dims_are(65, 64, 64), ("", lambda R: R.pass_atoms(0)[1] == 1)]))
    five = (128, 128, 80)
    mid_empty = lambda c: (c < 2 * SORT_CELLS) | (c >= 3 * SORT_CELLS)
    out.append(one("five passes, none in the middle one", five, 400, keep=mid_empty, claims=[passes_are(5, [True, True, False, True, True])]))
    big = (512, 512, 256)
    out.append(one("512x512x256: 2^26 cells", big, 200, arrangements=(2,), cells_cap=(1 << 26) + 64, claims=[
        ("C == 2^26, 256 passes", lambda R: R.C[0] == 1 << SORT_CELL_BITS and R.passes(0) == 256)]))
    out.append(Case("600 structures of 1 to 40 atoms", lambda: small_batch(600, 4, empties=(0, 1, 17, 300, 301, 598, 599)), [
        ("empty ones at both ends and inside", lambda R: R.C[0] == 0 and R.C[-1] == 0 and (R.C[2:598] == 0).sum() == 3),
        ("1 to 40 atoms", lambda R: {1, 40} <= set(np.diff(R.offsets).tolist()))]))
    mixed = lambda: [lattice(five, random_cells(five, 400, 11, keep=mid_empty), 11), lattice((1, 1, 1), [0]), lattice((1, 1, 1), [0], origin=(9, 9, 9)),
             lattice((128, 126, 1), random_cells((128, 126, 1), SORT_ATOMS, 12, distinct=True), 12, origin=(-900, 0, 0)), lattice((1, 1, 1), [0], origin=(50, 0, 0))]
    out.append(Case("five passes, single atoms and SORT_ATOMS in one batch", mixed, [
        passes_are(5, [True, True, False, True, True]), ("", lambda R: np.diff(R.offsets).tolist() == [400, 1, 1, SORT_ATOMS, 1])]))
    def frames():
        base, rng = tools.coil(300, 21)[0], np.random.default_rng(8)
        return [(base + rng.normal(0, 0.4, base.shape) + rng.uniform(-50, 50, 3), None) for _ in range(12)]
    out.append(Case("shared radii: 12 structures of 300 atoms", frames, [
        ("unequal radii, 300 of them", lambda R: R.radii.size == 300 and np.unique(R.radii).size > 100)],
        probe=1.4, shared_radii=True, radii=lambda: np.random.default_rng(9).uniform(1.0, 2.0, 300)))
    diag = lambda: np.linspace(0.0, 600.0, 240)[:, None] * np.ones((1, 3)) + np.random.default_rng(1).uniform(-0.3, 0.3, (240, 3))
    out.append(Case("off the lattice: coils, a globule, the diagonal", lambda: [tools.coil(1500, 40), tools.coil(900, 77), tools.globule(1200, 3), (diag(), np.full(240, 1.8)),
                                                                       (np.zeros((0, 3)), np.zeros(0)), (np.array([[1.0, 2.0, 3.0]]), np.array([1.7]))],
                    [("the diagonal takes several passes", lambda R: R.passes(3) >= 3)], probe=1.4))
    return out


def cases_general():
    """b. the shapes of the general pipeline"""
    out = []
    for n in (4095, 4096, 4097, 8193, 65537):
        out.append(one("one structure of %d atoms" % n, (20, 20, 20), n, seed=n, arrangements=(0, 1, 2) if n <= SORT_ATOMS else (0,), claims=[
            ("bounds chunks", lambda R, n=n: -(-R.n // BOUNDS_CHUNK) == -(-n // BOUNDS_CHUNK))]))
    for ns in (17, 33, 257, 600):
        out.append(Case("%d structures" % ns, lambda ns=ns: small_batch(ns, ns, empties=(0, 5, ns // 2, ns - 1), sizes=(1, 12)), [
            ("empty ones among them", lambda R: (R.C == 0).sum() == 4)]))
    for total, nxs in ((4095, (2048, 2047)), (4096, (2048, 2048)), (4097, (2048, 2049)), (8192, (4096, 2048, 2048)), (8192 + 15, (4096, 4096, 15)),
                       (8192 + 16, (4096, 4096, 16))):
        out.append(Case("%d cells" % total, lambda nxs=nxs: [line(nx, seed=k) for k, nx in enumerate(nxs)], [cells_total_is(total)]))
    out.append(Case("about 3e5 cells", lambda: [lattice((40, 40, 38), random_cells((40, 40, 38), 500, k), k) for k in range(5)], [cells_total_is(304000)]))
    for k in (1, 2, 3):
        out.append(Case("cells_cap + 2 == %d modulo 4" % k, lambda: [line(37), line(22, seed=2)], [cells_total_is(59)], arrangements=(0,), cells_cap=60 + (k - 2) % 4 + 0))
    blockwise = lambda R: np.pad(global_cells(R), (0, -R.n % PIPE_B), constant_values=-1).reshape(-1, PIPE_B)
    seq = [1] * 256 + [0, 5, 2, 3]
    out.append(ordered("256 atoms of a workgroup in one cell", seq, [("", lambda R: (blockwise(R)[0] == 1).all())]))
    seq = [0, 5] + [2, 3] * 126 + [2] + [4] * 40 + [1] * 10
    out.append(ordered("a run from thread 255 into the next workgroup", seq, [
        ("", lambda R: global_cells(R)[254] != global_cells(R)[255] and (global_cells(R)[255:295] == 4).all())]))
    seq = [0, 5] + [1, 2] * 300
    out.append(ordered("strictly alternating cells", seq, [("", lambda R: (np.diff(global_cells(R)) != 0).all() and R.n > 2 * PIPE_B)]))
    seq = [0, 5] + [2, 3] * 254 + [2] + [4] * 78
    out.append(ordered("a run across the last workgroups, n not a multiple of 256", seq, [
        ("", lambda R: R.n % PIPE_B == 77 and global_cells(R)[510] != 4 and (global_cells(R)[511:] == 4).all())]))
    return out


def declined_513():
    """513x512x256: more cells than k_sort_struct numbers"""
    dims = (513, 512, 256)
    return Case("513x512x256", lambda: [lattice(dims, random_cells(dims, 100, 2), 2)], [dims_are(*dims), ("", lambda R: R.C[0] > 1 << SORT_CELL_BITS)])
