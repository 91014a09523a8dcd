"""Per-residue tables of the interfaces between chain groups on the device (include/freesasa_gpu.h:
freesasa_gpu_interface_residues_dev, freesasa_gpu_calc_interface_residues) against the numpy restatement
(tests/interface_residues_ref.py) on the residue edge batch, a line of 70 000 one-atom residues and a golden PDB file; min_buried,
capacities, repeated calls and tools/interfaces.py --residues.  L&R at 20 slices and S&R at 100 points.  Reads nothing outside the
repository.

The restatement is never fed from the entry under test: the isolated areas come from freesasa_gpu_groups_dev, the areas of the
pair-structure atoms from the plain batch entry on the pair structures cut on the host, the pair table from
tests/interfaces_ref.py.  Rows are compared bit for bit.  One sum is taken in another order: a side's buried_res summed over its
rows against the pair row's buried_*, a difference of two sums of up to 129 areas each; it is held to the 1e-9 relative that
tests/test_interfaces_gpu.py states for such sums."""
import os

import numpy as np
import pytest

import interfaces_ref as ir
import interface_residues_ref as rr
from conftest import GOLDEN
from test_groups_gpu import run_groups, run_plain, LR, SR, RES
from test_interfaces_gpu import Run as PairRun, GUARD, _dev, _guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0, "no HIP device: the GPU tests cannot run"
    return freesasa_amd


@pytest.fixture(scope="module")
def edge():
    b = rr.residue_edge_batch()
    return tuple(np.array(a) for a in b[:5]) + (np.array(b[6]),)     # (copies: the restatement's own arrays stay read-only)


class Run:
    """one freesasa_gpu_interface_residues_dev call: the outputs as host arrays, the guards checked"""

    def __init__(self, ctx, alg, xyz, r, offs, group, n_groups, res_first, pcap, mcap, rcap, min_buried=0.0):
        import torch
        n, ns, G = len(r), len(offs) - 1, int(np.sum(n_groups))
        d_x, d_r, d_g = _dev(np.asarray(xyz).reshape(-1), np.float64), _dev(r, np.float64), _dev(group, np.int32)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        out = dict(sasa=_guarded(n, f64, -7.0), iso=_guarded(n, f64, -7.0), totals=_guarded(ns, f64, -7.0), gt=_guarded(3 * G, f64, -7.0),
                   ps=_guarded(pcap, i32, -7), pg=_guarded(2 * pcap, i32, -7), areas=_guarded(6 * pcap, f64, -7.0),
                   so=_guarded(2 * pcap + 1, i64, -7), pa=_guarded(mcap, i32, -7), pb=_guarded(mcap, f64, -7.0),
                   ro=_guarded(2 * pcap + 1, i64, -7), ri=_guarded(rcap, i32, -7), ra=_guarded(rcap, i32, -7), rar=_guarded(3 * rcap, f64, -7.0))
        sizes = dict(sasa=n, iso=n, totals=ns, gt=3 * G, ps=pcap, pg=2 * pcap, areas=6 * pcap, so=2 * pcap + 1, pa=mcap, pb=mcap,
                     ro=2 * pcap + 1, ri=rcap, ra=rcap, rar=3 * rcap)
        self.error = None
        try:
            self.P, self.M, self.R = ctx.interface_residues(
                d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), n_groups, res_first, out["sasa"].data_ptr(), out["iso"].data_ptr(), pcap,
                out["areas"].data_ptr(), rcap, out["rar"].data_ptr(), d_res_offsets=out["ro"].data_ptr(), d_res_index=out["ri"].data_ptr(),
                d_res_atoms=out["ra"].data_ptr(), d_pair_struct=out["ps"].data_ptr(), d_pair_groups=out["pg"].data_ptr(), atom_capacity=mcap,
                d_side_offsets=out["so"].data_ptr(), d_pair_atom=out["pa"].data_ptr(), d_pair_buried=out["pb"].data_ptr(),
                d_totals=out["totals"].data_ptr(), d_group_totals=out["gt"].data_ptr(), alg=alg, resolution=RES[alg], min_buried=min_buried)
        except RuntimeError as e:
            self.error = str(e)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        for k, v in host.items():
            assert len(v) == sizes[k] + GUARD and np.all(v[sizes[k]:] == -7), f"the guard behind {k} was written"
        self.raw = {k: v[:sizes[k]] for k, v in host.items()}
        if self.error is None:
            P, M, R = self.P, self.M, self.R
            self.sasa, self.iso, self.totals, self.gt = host["sasa"][:n], host["iso"][:n], host["totals"][:ns], host["gt"][:3 * G].reshape(G, 3)
            self.ps, self.pg, self.areas = host["ps"][:P], host["pg"][:2 * P].reshape(P, 2), host["areas"][:6 * P].reshape(P, 6)
            self.so, self.pa, self.pb = host["so"][:2 * P + 1], host["pa"][:M], host["pb"][:M]
            self.ro, self.ri, self.ra, self.rar = host["ro"][:2 * P + 1], host["ri"][:R], host["ra"][:R], host["rar"][:3 * R].reshape(R, 3)
            for k, used in (("ps", P), ("pg", 2 * P), ("areas", 6 * P), ("so", 2 * P + 1), ("pa", M), ("pb", M), ("ro", 2 * P + 1), ("ri", R),
                            ("ra", R), ("rar", 3 * R)):
                assert np.all(self.raw[k][used:] == -7), f"{k} was written beyond its rows"

    def pair_bytes(self):
        """what freesasa_gpu_interfaces_dev also gives, in the order of its Run.bytes()"""
        return b"".join(a.tobytes() for a in (self.sasa, self.iso, self.totals, self.gt, self.ps, self.pg, self.areas, self.so, self.pa, self.pb))

    def bytes(self):
        return self.pair_bytes() + b"".join(a.tobytes() for a in (self.ro, self.ri, self.ra, self.rar))


def _same_rows(run, want):
    off, index, atoms, areas = want
    assert run.R == len(index)
    assert np.array_equal(run.ro, off) and np.array_equal(run.ri, index) and np.array_equal(run.ra, atoms)
    assert run.rar.tobytes() == areas.tobytes()


_inputs = {}


def _restatement_inputs(fa, alg, edge):
    """(iso [n] from the chain-group entry, the pair-structure atoms' areas [M] from the plain entry): computed once per algorithm"""
    if alg not in _inputs:
        xyz, r, offs, group, ng, res_first = edge
        _, _, so, pa = rr.edge_table()
        ctx = fa.GpuContext(0)
        try:
            iso = run_groups(ctx, alg, xyz, r, offs, group, ng)[1].copy()
            px, pr, poffs = ir.pair_structures(xyz, r, so, pa)
            plain = run_plain(ctx, alg, px, pr, poffs)[0].copy()
        finally:
            ctx.close()
        iso.setflags(write=False); plain.setflags(write=False)
        _inputs[alg] = (iso, plain)
    return _inputs[alg]


@pytest.mark.parametrize("alg", [LR, SR])
def test_rows_on_the_residue_edge_batch(fa, edge, alg):
    xyz, r, offs, group, ng, res_first = edge
    ps, pg, so, pa = rr.edge_table()
    P, M = len(ps), len(pa)
    iso, plain = _restatement_inputs(fa, alg, edge)
    want = rr.rows(iso, plain, so, pa, res_first, 0.0)
    ctx = fa.GpuContext(0)
    try:
        old = PairRun(ctx, alg, xyz, r, offs, group, ng, P, M)
        run = Run(ctx, alg, xyz, r, offs, group, ng, res_first, P, M, M)
        assert old.error is None and run.error is None, (old.error, run.error)
        assert (run.P, run.M) == (P, M) and run.pair_bytes() == old.bytes()
        assert PairRun(ctx, alg, xyz, r, offs, group, ng, P, M).bytes() == old.bytes()     # ... and the old entry behind the new one
    finally:
        ctx.close()
    _same_rows(run, want)
    assert 0 < run.R < len(rr.segments(so, pa, res_first)[2])
    for q in range(2 * P):
        assert run.ra[run.ro[q]:run.ro[q + 1]].sum() <= so[q + 1] - so[q]
    if alg == SR:
        heads, first, seg_res, seg_side = rr.segments(so, pa, res_first)
        loses = np.array([np.any(run.pb[first[k]:first[k + 1]] != 0) for k in range(len(seg_res))])
        per_side = np.array([loses[seg_side == q].sum() for q in range(2 * P)])
        assert np.array_equal(np.diff(run.ro), per_side) and np.array_equal(run.ri, seg_res[loses])


@pytest.mark.parametrize("alg", [LR, SR])
def test_min_buried(fa, edge, alg):
    xyz, r, offs, group, ng, res_first = edge
    ps, pg, so, pa = rr.edge_table()
    P, M = len(ps), len(pa)
    iso, plain = _restatement_inputs(fa, alg, edge)
    off0, index0, atoms0, areas0 = rr.rows(iso, plain, so, pa, res_first, 0.0)
    k = len(index0) // 2
    cut = float(areas0[k, 2])
    assert cut > 0
    ctx = fa.GpuContext(0)
    try:
        at_cut = Run(ctx, alg, xyz, r, offs, group, ng, res_first, P, M, M, min_buried=cut)
        none = Run(ctx, alg, xyz, r, offs, group, ng, res_first, P, M, M, min_buried=1e300)
        zero = Run(ctx, alg, xyz, r, offs, group, ng, res_first, P, M, M)
    finally:
        ctx.close()
    assert at_cut.error is None and none.error is None and zero.error is None
    _same_rows(zero, (off0, index0, atoms0, areas0))
    _same_rows(at_cut, rr.rows(iso, plain, so, pa, res_first, cut))
    stay = areas0[:, 2] > cut                                          # strict: the row whose buried_res is the cut is gone
    assert not stay[k] and np.array_equal(at_cut.ri, index0[stay]) and at_cut.rar.tobytes() == areas0[stay].tobytes()
    assert at_cut.R == int(stay.sum()) <= len(index0) - 1
    assert none.R == 0 and np.array_equal(none.ro, np.zeros(2 * P + 1, np.int64))
    for key in ("ri", "ra", "rar"):
        assert np.all(none.raw[key] == -7), key
    assert none.pair_bytes() == zero.pair_bytes()


def test_capacities(fa, edge):
    xyz, r, offs, group, ng, res_first = edge
    ps, pg, so, pa = rr.edge_table()
    P, M = len(ps), len(pa)
    ctx = fa.GpuContext(0)
    try:
        good = Run(ctx, LR, xyz, r, offs, group, ng, res_first, P, M, M)
        assert good.error is None
        R = good.R
        for pcap, mcap, rcap, number, word in ((P, M, R - 1, R, "res_capacity"), (P - 1, M, R, P, "pair_capacity"), (P, M - 1, R, M, "atom_capacity"),
                                               (P, M, 0, R, "res_capacity")):
            run = Run(ctx, LR, xyz, r, offs, group, ng, res_first, pcap, mcap, rcap)      # (Run checks the guards)
            assert run.error is not None and word in run.error and str(number) in run.error, run.error
            for k in ("ps", "pg", "areas", "so", "pa", "pb", "ro", "ri", "ra", "rar"):
                assert np.all(run.raw[k] == -7), k
            assert Run(ctx, LR, xyz, r, offs, group, ng, res_first, P, M, R).bytes() == good.bytes()   # the call after a failed one
        short = Run(ctx, LR, xyz, r, offs, group, ng, res_first, P, M, R - 1)
        assert "residue rows" in short.error
    finally:
        ctx.close()


@pytest.mark.parametrize("alg", [LR, SR])
def test_many_segments(fa, alg):
    """70 000 atoms on a line, groups alternating, every atom a residue: P = 1, M = K = 70 000 - more blocks' sums (274) than the
    256 one workgroup of the scan holds, so the scan takes its third level"""
    n = 70_000
    xyz = np.zeros((n, 3)); xyz[:, 0] = np.arange(n) * 1.0
    r = np.full(n, 1.5)
    offs, group, ng = np.array([0, n], np.int64), (np.arange(n) % 2).astype(np.int32), np.array([2], np.int32)
    res_first = np.arange(n + 1, dtype=np.int64)
    so, pa = np.array([0, n // 2, n], np.int64), np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)]).astype(np.int32)
    ctx = fa.GpuContext(0)
    try:
        iso = run_groups(ctx, alg, xyz, r, offs, group, ng)[1]
        plain = run_plain(ctx, alg, xyz[pa], r[pa], np.array([0, n], np.int64))[0]
        run = Run(ctx, alg, xyz, r, offs, group, ng, res_first, 1, n, n)
        again = Run(ctx, alg, xyz, r, offs, group, ng, res_first, 1, n, n)
    finally:
        ctx.close()
    assert run.error is None and again.error is None, (run.error, again.error)
    assert (run.P, run.M) == (1, n) and np.array_equal(run.so, so) and np.array_equal(run.pa, pa)
    _same_rows(run, rr.rows(iso, plain, so, pa, res_first, 0.0))
    assert run.R > 65_536
    assert again.bytes() == run.bytes()


def _golden():
    from freesasa_amd import ingest
    b = ingest.load_files([os.path.join(GOLDEN, "pdb", "2jo4.pdb")])
    g, n, st = b.chain_groups(None, separate_chains=True)
    assert st[0] == 0 and n[0] == 4
    return b, g, n


@pytest.mark.parametrize("alg", [LR, SR])
def test_golden_pdb(fa, alg):
    b, g, n = _golden()
    got = fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg=alg, resolution=RES[alg], per_atom=True, res_first=b.res_first)
    plain_call = fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg=alg, resolution=RES[alg], per_atom=True)
    assert plain_call.res_offsets is None and plain_call.res_areas is None and plain_call.n_res_rows is None
    for name in ("sasa", "iso", "totals", "group_totals", "pair_struct", "pair_groups", "pair_areas", "side_offsets", "pair_atom", "pair_buried"):
        assert getattr(got, name).tobytes() == getattr(plain_call, name).tobytes(), name
    assert got.n_pairs >= 1 and got.n_res_rows == len(got.res_index) == len(got.res_atoms) == len(got.res_areas) > 0
    ctx = fa.GpuContext(0)
    try:
        iso = run_groups(ctx, alg, b.xyz, b.radii, b.offsets, g, n)[1]
        px, pr, poffs = ir.pair_structures(b.xyz, b.radii, got.side_offsets, got.pair_atom)
        plain = run_plain(ctx, alg, px, pr, poffs)[0]
    finally:
        ctx.close()
    off, index, atoms, areas = rr.rows(iso, plain, got.side_offsets, got.pair_atom, b.res_first, 0.0)
    assert np.array_equal(got.res_offsets, off) and np.array_equal(got.res_index, index) and np.array_equal(got.res_atoms, atoms)
    assert got.res_areas.tobytes() == areas.tobytes()
    chains = []
    for c in b.res_chain:
        if c not in chains:
            chains.append(c)
    for p in range(got.n_pairs):
        for side in (0, 1):
            rows = got.side_rows(p, side)
            assert rows.stop > rows.start
            assert all(b.res_chain[k] == chains[got.pair_groups[p, side]] for k in got.res_index[rows])
            if alg == SR:
                total = 0.0
                for v in got.res_areas[rows, 2]:
                    total += float(v)
                want = got.pair_areas[p, 4 + side]
                assert abs(total - want) <= 1e-9 * abs(want), (p, side, total, want)


def test_the_tool_writes_the_residue_table(fa, tmp_path):
    from tools import interfaces
    path = os.path.join(GOLDEN, "pdb", "2jo4.pdb")
    a, c, res = str(tmp_path / "a.tsv"), str(tmp_path / "c.tsv"), str(tmp_path / "res.tsv")
    interfaces.main([path, "-o", a, "--alg", "sr"])
    interfaces.main([path, "-o", c, "--alg", "sr", "--residues", res])
    assert open(a, "rb").read() == open(c, "rb").read()
    b, g, n = _golden()
    got = fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg=SR, resolution=RES[SR], res_first=b.res_first)
    lines = open(res).read().splitlines()
    assert lines[0] == interfaces.RESIDUE_HEADER and len(lines) == 1 + got.n_res_rows
    names, numbers = b.res_name, b.res_number
    for line, k, area in zip(lines[1:], got.res_index, got.res_areas):
        f = line.split("\t")
        assert len(f) == 11 and f[0] == "2jo4.pdb" and f[5] == names[k].strip() and f[6] == numbers[k].strip() and f[10] == "%.3f" % area[2]
    more = str(tmp_path / "more.tsv")
    interfaces.main([path, "-o", c, "--alg", "sr", "--residues", more, "--min-buried", "20"])
    assert len(open(more).read().splitlines()) == 1 + int((got.res_areas[:, 2] > 20.0).sum()) < len(lines)
