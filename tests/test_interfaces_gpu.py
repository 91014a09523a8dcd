"""Interfaces between chain groups on the device (include/freesasa_gpu.h: freesasa_gpu_interface_pairs_dev,
freesasa_gpu_interfaces_dev, freesasa_gpu_calc_interfaces) against the numpy restatement (tests/interfaces_ref.py), the plain
entries on the pair structures cut on the host, the chain-group entry, the golden PDB files, capacities and repeated calls.
L&R at 20 slices and S&R at 100 points.  Reads nothing outside the repository.

The area of a pair-structure atom is not an output of its own: it is held to the plain entry through pair_buried, which has to be
iso[pair_atom] minus the plain entry's area bit for bit, and through in_pair_*, the sum of those areas over a side.
Sums: in_pair_* is summed in another order than math.fsum or the chain-group entry's columns sum the same numbers; every such
sum of N <= 2300 areas is within N * 2^-53 of the exact one relative to the sum of the terms, far inside the 1e-9 relative the
chain-group tests (tests/test_groups_gpu.py) hold their totals to, which is the bar here."""
import math
import os

import numpy as np
import pytest

import interfaces_ref as ir
from conftest import GOLDEN
from test_groups_gpu import _docking_batch, run_groups, run_plain, LR, SR, RES, LR_TOL

pytestmark = pytest.mark.gpu

GUARD = 64  # elements behind every output array that no call may touch


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0, "no HIP device: the GPU tests cannot run"
    return freesasa_amd


@pytest.fixture(scope="module")
def edge():
    return tuple(np.array(a) for a in ir.edge_batch()[:5])      # (copies: the restatement's own arrays stay read-only)


@pytest.fixture(scope="module")
def edge_table(edge):
    return ir.table(*edge)


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(torch.device("cuda:0"))


def _guarded(n, dtype, fill):
    import torch
    return torch.full((max(n, 0) + GUARD,), fill, dtype=dtype, device=torch.device("cuda:0"))


class Run:
    """one freesasa_gpu_interfaces_dev call: the outputs as host arrays, the guards checked"""

    def __init__(self, ctx, alg, xyz, r, offs, group, n_groups, pcap, mcap, per_atom=True):
        import torch
        n, ns, G = len(r), len(offs) - 1, int(np.sum(n_groups))
        d_x, d_r, d_g = _dev(np.asarray(xyz).reshape(-1), np.float64), _dev(r, np.float64), _dev(group, np.int32)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        out = dict(sasa=_guarded(n, f64, -7.0), iso=_guarded(n, f64, -7.0), totals=_guarded(ns, f64, -7.0), gt=_guarded(3 * G, f64, -7.0),
                   ps=_guarded(pcap, i32, -7), pg=_guarded(2 * pcap, i32, -7), areas=_guarded(6 * pcap, f64, -7.0),
                   so=_guarded(2 * pcap + 1, i64, -7), pa=_guarded(mcap, i32, -7), pb=_guarded(mcap, f64, -7.0))
        sizes = dict(sasa=n, iso=n, totals=ns, gt=3 * G, ps=pcap, pg=2 * pcap, areas=6 * pcap, so=2 * pcap + 1, pa=mcap, pb=mcap)
        self.error = None
        try:
            self.P, self.M = ctx.interfaces(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), n_groups, out["sasa"].data_ptr(),
                                            out["iso"].data_ptr(), pcap, out["areas"].data_ptr(), out["ps"].data_ptr(), out["pg"].data_ptr(),
                                            atom_capacity=mcap, d_side_offsets=out["so"].data_ptr(),
                                            d_pair_atom=out["pa"].data_ptr() if per_atom else 0,
                                            d_pair_buried=out["pb"].data_ptr() if per_atom else 0, d_totals=out["totals"].data_ptr(),
                                            d_group_totals=out["gt"].data_ptr(), alg=alg, resolution=RES[alg])
        except RuntimeError as e:
            self.error = str(e)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        for k, v in host.items():
            assert np.all(v[sizes[k]:] == -7), f"the guard behind {k} was written"
        self.raw = {k: v[:sizes[k]] for k, v in host.items()}
        if self.error is None:
            P, M = self.P, self.M
            self.sasa, self.iso, self.totals, self.gt = host["sasa"][:n], host["iso"][:n], host["totals"][:ns], host["gt"][:3 * G].reshape(G, 3)
            self.ps, self.pg, self.areas = host["ps"][:P], host["pg"][:2 * P].reshape(P, 2), host["areas"][:6 * P].reshape(P, 6)
            self.so, self.pa, self.pb = host["so"][:2 * P + 1], host["pa"][:M], host["pb"][:M]
            for k, used in (("ps", P), ("pg", 2 * P), ("areas", 6 * P), ("so", 2 * P + 1), ("pa", M if per_atom else 0), ("pb", M if per_atom else 0)):
                assert np.all(self.raw[k][used:] == -7), f"{k} was written beyond its rows"

    def bytes(self):
        return b"".join(a.tobytes() for a in (self.sasa, self.iso, self.totals, self.gt, self.ps, self.pg, self.areas, self.so, self.pa, self.pb))


@pytest.mark.parametrize("alg", [LR, SR])
def test_pair_list_and_pair_areas_on_the_edge_batch(fa, edge, edge_table, alg):
    xyz, r, offs, group, ng = edge
    ps, pg, so, pa = edge_table
    P, M = len(ps), len(pa)
    ctx = fa.GpuContext(0)
    try:
        got_ps, got_pg = np.full(P, -7, np.int32), np.full((P, 2), -7, np.int32)
        d_x, d_r, d_g = _dev(xyz.reshape(-1)), _dev(r), _dev(group, np.int32)
        counts = ctx.interface_pairs(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, P, got_ps, got_pg, alg=alg, resolution=RES[alg])
        tests, cand, hit = ir.screen(*edge)
        assert counts == (P, M, len(tests), int(cand.sum()))
        assert np.array_equal(got_ps, ps) and np.array_equal(got_pg, pg)
        run = Run(ctx, alg, xyz, r, offs, group, ng, P, M)
        assert run.error is None, run.error
        assert (run.P, run.M) == (P, M)
        assert np.array_equal(run.ps, ps) and np.array_equal(run.pg, pg) and np.array_equal(run.so, so) and np.array_equal(run.pa, pa)
        px, pr, poffs = ir.pair_structures(xyz, r, so, pa)
        plain, _ = run_plain(ctx, alg, px, pr, poffs)
        assert np.array_equal(run.pb, run.iso[pa] - plain)
        gbase = np.concatenate([[0], np.cumsum(ng)])
        for p in range(P):
            for side in (0, 1):
                f = math.fsum(plain[so[2 * p + side]:so[2 * p + side + 1]])
                assert abs(run.areas[p, 2 + side] - f) <= 1e-9 * abs(f), (p, side, run.areas[p, 2 + side], f)
                assert run.areas[p, side] == run.gt[gbase[ps[p]] + pg[p, side], 0]
        assert np.array_equal(run.areas[:, 4:], run.areas[:, :2] - run.areas[:, 2:4])
    finally:
        ctx.close()


@pytest.mark.parametrize("alg", [LR, SR])
def test_groups_parity(fa, edge, edge_table, alg):
    xyz, r, offs, group, ng = edge
    ctx = fa.GpuContext(0)
    try:
        want = run_groups(ctx, alg, xyz, r, offs, group, ng)
        run = Run(ctx, alg, xyz, r, offs, group, ng, len(edge_table[0]), len(edge_table[3]))
        assert run.error is None, run.error
        for a, b in zip((run.sasa, run.iso, run.totals, run.gt), want):
            assert np.array_equal(a, b)
    finally:
        ctx.close()
    got = fa.calc_interfaces(xyz, r, offs, group, ng, alg=alg, resolution=RES[alg], per_atom=True)
    assert b"".join(a.tobytes() for a in (got.sasa, got.iso, got.totals, got.group_totals, got.pair_struct, got.pair_groups, got.pair_areas,
                                          got.side_offsets, got.pair_atom, got.pair_buried)) == run.bytes()
    pairs = fa.interface_pairs(xyz, r, offs, group, ng, alg=alg, resolution=RES[alg])
    assert np.array_equal(pairs.pair_struct, run.ps) and np.array_equal(pairs.pair_groups, run.pg) and pairs.n_pair_atoms == run.M


@pytest.mark.parametrize("alg", [LR, SR])
def test_two_group_structures(fa, alg):
    """20 complexes of two 800-atom globules in contact: one row each; the pair structure is the complex itself, atom for atom,
    so every atom's area in the pair is its complex area bit for bit (pair_buried == iso - sasa), and in_pair and buried are the
    chain-group entry's complex and buried columns, the same numbers summed in another order (the bar: the head of this file)"""
    xyz, r, offs, group, ng = _docking_batch(20, 800, 11)
    ctx = fa.GpuContext(0)
    try:
        run = Run(ctx, alg, xyz, r, offs, group, ng, 20, 20 * 1600)
        assert run.error is None, run.error
    finally:
        ctx.close()
    assert run.P == 20 and run.M == 20 * 1600
    assert np.array_equal(run.ps, np.arange(20)) and np.array_equal(run.pg, np.tile([0, 1], (20, 1)))
    assert np.array_equal(run.pa, np.arange(20 * 1600)) and np.array_equal(run.so, 800 * np.arange(41))
    assert np.array_equal(run.pb, run.iso - run.sasa)
    gt = run.gt.reshape(20, 2, 3)
    assert np.array_equal(run.areas[:, :2], gt[:, :, 0])
    assert np.all(np.abs(run.areas[:, 2:4] - gt[:, :, 1]) <= 1e-9 * gt[:, :, 1])
    assert np.all(np.abs(run.areas[:, 4:] - gt[:, :, 2]) <= 1e-9 * gt[:, :, 0])
    assert np.all(run.areas[:, 4:] > 0)


@pytest.mark.parametrize("alg", [LR, SR])
def test_omitted_pairs_bury_nothing(fa, edge, alg):
    """the candidates that are not contacts get no row: their pair structures, cut on the host, through the plain entry give
    every atom the area it has in its isolated group"""
    xyz, r, offs, group, ng = edge
    tests, cand, hit = ir.screen(*edge)
    omitted = tests[cand & ~hit]
    assert len(omitted) >= 2
    sides = [ir.members(offs, group, s, k) for s, g, h in omitted for k in (g, h)]
    idx = np.concatenate(sides)
    poffs = np.concatenate([[0], np.cumsum([len(x) for x in sides])]).astype(np.int64)
    ctx = fa.GpuContext(0)
    try:
        d_x, d_r = _dev(xyz[idx].reshape(-1)), _dev(r[idx])
        import torch
        d_s = torch.empty(len(idx), dtype=torch.float64, device="cuda:0")
        d_c = torch.zeros(len(idx), dtype=torch.int32, device="cuda:0")
        iso_counts = None
        both = []
        for o in (poffs[::2], poffs):                 # the pair structures, then every side on its own
            if alg == LR:
                ctx.lee_richards(d_x.data_ptr(), d_r.data_ptr(), o, d_s.data_ptr(), n_slices=RES[LR])
            else:
                ctx.shrake_rupley(d_x.data_ptr(), d_r.data_ptr(), o, d_s.data_ptr(), d_c.data_ptr(), n_points=RES[SR])
            both.append((d_s.cpu().numpy().copy(), d_c.cpu().numpy().copy()))
    finally:
        ctx.close()
    (pair, pair_counts), (iso, iso_counts) = both
    if alg == SR:
        assert np.array_equal(pair_counts, iso_counts) and np.array_equal(pair, iso)
    else:
        assert np.max(np.abs(pair - iso)) <= LR_TOL


def _golden(name, options=0):
    from freesasa_amd import ingest
    b = ingest.load_files([os.path.join(GOLDEN, "pdb", name)], options=options)
    g, n, st = b.chain_groups(None, separate_chains=True)
    assert st[0] == 0 and n[0] == 4
    chains = []
    for c in b.res_chain:
        if c not in chains:
            chains.append(c)
    return b, g, n, chains


@pytest.mark.parametrize("alg", [LR, SR])
@pytest.mark.parametrize("name,hydrogens", [("2jo4.pdb", False), ("2jo4.pdb", True), ("3gnn.pdb", False)])
def test_golden_pdb(fa, alg, name, hydrogens):
    """separate chains; for every row (X, Y) the pair is the isolated group of calc_groups' spec "XY" (chains lie in file order)"""
    from freesasa_amd import ingest
    opt = ingest.INCLUDE_HYDROGEN if hydrogens else 0
    b, g, n, chains = _golden(name, opt)
    if name == "2jo4.pdb":
        assert [int((g == k).sum()) for k in range(4)] == ([277] * 4 if hydrogens else [129] * 4)   # (a pair with hydrogens: 554 atoms)
    got = fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg=alg, resolution=RES[alg], per_atom=True)
    assert got.n_pairs >= 1
    for p in range(got.n_pairs):
        x, y = chains[got.pair_groups[p, 0]], chains[got.pair_groups[p, 1]]
        g2, n2, st2 = b.chain_groups(x + y)
        assert st2[0] == 0 and n2[0] == 1
        _, iso, _, gt = fa.calc_groups(b.xyz, b.radii, b.offsets, g2, n2, alg=alg, resolution=RES[alg])
        total = got.pair_areas[p, 2] + got.pair_areas[p, 3]
        assert abs(total - gt[0, 0]) <= 1e-9 * gt[0, 0], (x, y, total, gt[0, 0])
        atoms = got.pair_atom[got.side_offsets[2 * p]:got.side_offsets[2 * p + 2]]
        assert np.array_equal(atoms, np.nonzero(g2 == 0)[0])
        buried = got.pair_buried[got.side_offsets[2 * p]:got.side_offsets[2 * p + 2]]
        assert np.array_equal(buried, got.iso[atoms] - iso[atoms])


def test_capacities(fa, edge, edge_table):
    xyz, r, offs, group, ng = edge
    P, M = len(edge_table[0]), len(edge_table[3])
    ctx = fa.GpuContext(0)
    try:
        good = Run(ctx, LR, xyz, r, offs, group, ng, P, M)
        assert good.error is None
        for pcap, mcap, number, word in ((P - 1, M, P, "pair_capacity"), (P, M - 1, M, "atom_capacity"), (0, 0, P, "pair_capacity")):
            run = Run(ctx, LR, xyz, r, offs, group, ng, pcap, mcap)      # (Run checks the guards)
            assert run.error is not None and word in run.error and str(number) in run.error, run.error
            for k in ("ps", "pg", "areas", "so", "pa", "pb"):
                assert np.all(run.raw[k] == -7), k
        rows_only = Run(ctx, LR, xyz, r, offs, group, ng, P, 0, per_atom=False)     # no per-atom arrays: their capacity is not looked at
        assert rows_only.error is None and np.array_equal(rows_only.areas, good.areas)
        got_ps = np.full(P, -7, np.int32)
        d_x, d_r, d_g = _dev(xyz.reshape(-1)), _dev(r), _dev(group, np.int32)
        with pytest.raises(RuntimeError, match=f"pair_capacity.*{P} pairs"):
            ctx.interface_pairs(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, P - 1, got_ps, None)
        assert np.all(got_ps == -7)
        assert Run(ctx, LR, xyz, r, offs, group, ng, P, M).bytes() == good.bytes()
    finally:
        ctx.close()
    with pytest.raises(RuntimeError, match="group id"):
        fa.calc_interfaces(xyz, r, offs, np.full_like(group, 400), ng)


@pytest.mark.parametrize("alg", [LR, SR])
def test_repeated_calls_give_the_same_bytes(fa, edge, edge_table, alg):
    xyz, r, offs, group, ng = edge
    P, M = len(edge_table[0]), len(edge_table[3])
    ctx = fa.GpuContext(0)
    try:
        sx, sr, so, sg, sn = xyz[:offs[2]], r[:offs[2]], offs[:3], group[:offs[2]], ng[:2]     # the first two structures: a smaller batch
        sp, _, _, spa = ir.table(sx, sr, so, sg, sn)
        small = Run(ctx, alg, sx, sr, so, sg, sn, len(sp), len(spa))
        assert small.error is None and small.P == len(sp) > 0
        first = Run(ctx, alg, xyz, r, offs, group, ng, P, M)                                     # the buffers grow
        assert Run(ctx, alg, xyz, r, offs, group, ng, P, M).bytes() == first.bytes()
        assert Run(ctx, alg, sx, sr, so, sg, sn, len(sp), len(spa)).bytes() == small.bytes()
        assert Run(ctx, alg, xyz, r, offs, group, ng, P, M).bytes() == first.bytes()
    finally:
        ctx.close()
