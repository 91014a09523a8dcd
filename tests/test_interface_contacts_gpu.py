"""Atom-atom contact tables of the interfaces between chain groups on the device (include/freesasa_gpu.h:
freesasa_gpu_interface_contacts_dev, freesasa_gpu_calc_interface_contacts) against the numpy restatement
(tests/interface_contacts_ref.py) on the contact edge batch at 1, 31, 32, 33, 100 and 128 test points and on a golden PDB file;
the integer and the area identity per atom, the untouched interface outputs, capacities, repeated calls and another tile shape,
the host form, the refusals and tools/interfaces.py --contacts.  Reads nothing outside the repository.

The restatement is never fed from the entry under test: its masks come from tests/volume_ref.py's exposed_mask on the pair
structures and the sides cut on the host by tests/interfaces_ref.py.  contact_first, contact_partner, contact_points, contact_area,
the buried masks and the dots' partners are compared bit for bit.

The area identity.  Per atom the sum of contact_area, added in row order, is held to pair_buried[i] within 256 * 2^-53 * A,
A = 4 pi R_i^2.  With u = 2^-53: pair_buried is the difference of two areas (4.0 * PI * R * R * n) / N, each at most A with 4
roundings (8 u A) and one more for the difference (u A); every contact_area has the same 4 roundings and they add up to at most A
(4 u A); a sum of at most 127 terms has at most 126 additions whose results are at most A (126 u A): 139 u A in all, below the
bound."""
import math
import os

import numpy as np
import pytest

import dots_ref as dr
import interfaces_ref as ir
import interface_contacts_ref as cr
from conftest import GOLDEN
from test_interfaces_gpu import GUARD, _dev, _guarded

pytestmark = pytest.mark.gpu
SR = 1


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0, "no HIP device: the GPU tests cannot run"
    return freesasa_amd


@pytest.fixture(scope="module")
def edge():
    return tuple(np.array(a) for a in cr.contacts_edge_batch()[:5])      # (copies: the restatement's own arrays stay read-only)


def with_cfg(cfg, fn):
    """fn() with the tuning aid FREESASA_AMD_CFG = "B,TA,records per atom,ds" set: the engine reads it batch by batch"""
    old = os.environ.get("FREESASA_AMD_CFG")
    os.environ["FREESASA_AMD_CFG"] = cfg
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("FREESASA_AMD_CFG", None)
        else:
            os.environ["FREESASA_AMD_CFG"] = old


class Run:
    """one freesasa_gpu_interface_contacts_dev call (contacts=False: freesasa_gpu_interfaces_dev with the same arrays): the outputs
    as host arrays, the guards checked"""

    def __init__(self, ctx, n_points, xyz, r, offs, group, n_groups, pcap, mcap, ccap, dcap, contacts=True, alg=SR, misalign=False):
        import torch
        n, ns, G = len(r), len(offs) - 1, int(np.sum(n_groups))
        d_x, d_r, d_g = _dev(np.asarray(xyz).reshape(-1), np.float64), _dev(r, np.float64), _dev(group, np.int32)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        out = dict(sasa=_guarded(n, f64, -7.0), iso=_guarded(n, f64, -7.0), totals=_guarded(ns, f64, -7.0), gt=_guarded(3 * G, f64, -7.0),
                   ps=_guarded(pcap, i32, -7), pg=_guarded(2 * pcap, i32, -7), areas=_guarded(6 * pcap, f64, -7.0),
                   so=_guarded(2 * pcap + 1, i64, -7), pa=_guarded(mcap, i32, -7), pb=_guarded(mcap, f64, -7.0),
                   cf=_guarded(mcap + 1, i64, -7), cp=_guarded(ccap, i32, -7), cn=_guarded(ccap, i32, -7), ca=_guarded(ccap, f64, -7.0),
                   bm=_guarded(4 * mcap, i32, -7), dp=_guarded(dcap, i32, -7))
        sizes = dict(sasa=n, iso=n, totals=ns, gt=3 * G, ps=pcap, pg=2 * pcap, areas=6 * pcap, so=2 * pcap + 1, pa=mcap, pb=mcap,
                     cf=mcap + 1, cp=ccap, cn=ccap, ca=ccap, bm=4 * mcap, dp=dcap)
        self.error = None
        p = {k: v.data_ptr() for k, v in out.items()}
        try:
            if contacts:
                self.P, self.M, self.C, self.D = ctx.interface_contacts(
                    d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), n_groups, p["sasa"], p["iso"], pcap, p["areas"], contact_capacity=ccap,
                    d_contact_first=p["cf"], d_contact_partner=p["cp"], d_contact_points=p["cn"], d_contact_area=p["ca"],
                    d_buried_masks=p["bm"] + (4 if misalign else 0), dot_capacity=dcap, d_dot_partner=p["dp"], d_pair_struct=p["ps"],
                    d_pair_groups=p["pg"], atom_capacity=mcap, d_side_offsets=p["so"], d_pair_atom=p["pa"], d_pair_buried=p["pb"],
                    d_totals=p["totals"], d_group_totals=p["gt"], alg=alg, n_points=n_points)
            else:
                self.P, self.M = ctx.interfaces(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), n_groups, p["sasa"], p["iso"], pcap,
                                                p["areas"], p["ps"], p["pg"], atom_capacity=mcap, d_side_offsets=p["so"], d_pair_atom=p["pa"],
                                                d_pair_buried=p["pb"], d_totals=p["totals"], d_group_totals=p["gt"], alg=alg, resolution=n_points)
                self.C = self.D = 0
        except RuntimeError as e:
            self.error = str(e)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        for k, v in host.items():
            assert len(v) == sizes[k] + GUARD and np.all(v[sizes[k]:] == -7), f"the guard behind {k} was written"
        self.raw = {k: v[:sizes[k]] for k, v in host.items()}
        if self.error is None:
            P, M, Cn, D = self.P, self.M, self.C, self.D
            self.sasa, self.iso, self.totals, self.gt = host["sasa"][:n], host["iso"][:n], host["totals"][:ns], host["gt"][:3 * G].reshape(G, 3)
            self.ps, self.pg, self.areas = host["ps"][:P], host["pg"][:2 * P].reshape(P, 2), host["areas"][:6 * P].reshape(P, 6)
            self.so, self.pa, self.pb = host["so"][:2 * P + 1], host["pa"][:M], host["pb"][:M]
            used = [("ps", P), ("pg", 2 * P), ("areas", 6 * P), ("so", 2 * P + 1), ("pa", M), ("pb", M)]
            if contacts:
                self.cf, self.cp, self.cn, self.ca = host["cf"][:M + 1 if P else 1], host["cp"][:Cn], host["cn"][:Cn], host["ca"][:Cn]
                self.bm, self.dp = host["bm"][:4 * M].view(np.uint32).reshape(M, 4), host["dp"][:D]
                used += [("cf", M + 1 if P else 1), ("cp", Cn), ("cn", Cn), ("ca", Cn), ("bm", 4 * M), ("dp", D)]
            for k, u in used:
                assert np.all(self.raw[k][u:] == -7), f"{k} was written beyond its rows"

    def pair_bytes(self):
        return b"".join(a.tobytes() for a in (self.sasa, self.iso, self.totals, self.gt, self.ps, self.pg, self.areas, self.so, self.pa, self.pb))

    def bytes(self):
        return self.pair_bytes() + b"".join(a.tobytes() for a in (self.cf, self.cp, self.cn, self.ca, self.bm, self.dp))


def _same_table(run, want):
    M = len(want["dot_first"]) - 1
    assert (run.C, run.D) == (len(want["contact_partner"]), len(want["dot_partner"]))
    assert np.array_equal(run.cf, want["contact_first"]) and np.array_equal(run.cp, want["contact_partner"])
    assert np.array_equal(run.cn, want["contact_points"]) and run.ca.tobytes() == want["contact_area"].tobytes()
    assert run.bm.shape == (M, 4) and run.bm.tobytes() == want["buried_masks"].tobytes()
    assert np.array_equal(run.dp, want["dot_partner"])


def _identities(fa, run, px, pr, so, n_points):
    """the integer identity (exact) and the area identity per atom; the counts from plain mask runs on the structures cut on the host"""
    M = len(pr)
    _, counts_pair, _, _ = fa.calc_masks(px, pr, so[::2].copy(), probe=cr.PROBE, n_points=n_points)
    _, counts_side, _, _ = fa.calc_masks(px, pr, so, probe=cr.PROBE, n_points=n_points)
    rows_atom = np.repeat(np.arange(M), np.diff(run.cf))
    points = np.bincount(rows_atom, weights=run.cn, minlength=M).astype(np.int64)
    assert np.array_equal(points, counts_side.astype(np.int64) - counts_pair)
    assert np.array_equal(dr.popcounts(run.bm, n_points), points) and not (run.bm & ~dr.full_words(n_points)).any()
    worst = 0.0
    for i in range(M):
        total = 0.0
        for v in run.ca[run.cf[i]:run.cf[i + 1]]:
            total += float(v)
        R = float(pr[i]) + cr.PROBE
        bound = 256.0 * 2.0 ** -53 * 4.0 * math.pi * R * R
        worst = max(worst, abs(total - float(run.pb[i])) / bound)
        assert abs(total - float(run.pb[i])) <= bound, (i, total, run.pb[i], bound)
    print(f"N = {n_points}: the area identity's worst atom is at {worst:.3f} of its bound")


@pytest.mark.parametrize("n_points", cr.N_POINTS)
def test_the_table_on_the_contact_edge_batch(fa, edge, n_points):
    xyz, r, offs, group, ng = edge
    ps, pg, so, pa = cr.edge_table()
    P, M = len(ps), len(pa)
    side, pair, want = cr.edge_contacts(n_points)
    Cn, D = len(want["contact_partner"]), len(want["dot_partner"])
    ctx = fa.GpuContext(0)
    try:
        old = Run(ctx, n_points, xyz, r, offs, group, ng, P, M, 0, 0, contacts=False)
        run = Run(ctx, n_points, xyz, r, offs, group, ng, P, M, Cn, D)
        again = Run(ctx, n_points, xyz, r, offs, group, ng, P, M, Cn + 5, D + 5)
        assert old.error is None and run.error is None and again.error is None, (old.error, run.error, again.error)
        assert (run.P, run.M) == (P, M) and np.array_equal(run.so, so) and np.array_equal(run.pa, pa)
        assert run.pair_bytes() == old.pair_bytes()                                                # the interface outputs: untouched
        assert Run(ctx, n_points, xyz, r, offs, group, ng, P, M, 0, 0, contacts=False).pair_bytes() == old.pair_bytes()   # ... and the old entry behind the new one
    finally:
        ctx.close()
    _same_table(run, want)
    assert again.bytes() == run.bytes()
    px, pr, _ = ir.pair_structures(xyz, r, so, pa)
    _identities(fa, run, px, pr, so, n_points)


def test_another_tile_shape_gives_the_same_bytes(fa, edge):
    xyz, r, offs, group, ng = edge
    ps, pg, so, pa = cr.edge_table()
    P, M = len(ps), len(pa)
    _, _, want = cr.edge_contacts(100)
    Cn, D = len(want["contact_partner"]), len(want["dot_partner"])

    def run():
        ctx = fa.GpuContext(0)
        try:
            return Run(ctx, 100, xyz, r, offs, group, ng, P, M, Cn, D)
        finally:
            ctx.close()

    base = run()
    assert base.error is None, base.error
    for cfg in ("64,3,48,0", "256,8,112,0"):
        other = with_cfg(cfg, run)
        assert other.error is None and other.bytes() == base.bytes(), (cfg, other.error)


def test_capacities(fa, edge):
    xyz, r, offs, group, ng = edge
    ps, pg, so, pa = cr.edge_table()
    P, M = len(ps), len(pa)
    _, _, want = cr.edge_contacts(33)
    Cn, D = len(want["contact_partner"]), len(want["dot_partner"])
    ctx = fa.GpuContext(0)
    try:
        good = Run(ctx, 33, xyz, r, offs, group, ng, P, M, Cn, D)
        assert good.error is None and (good.C, good.D) == (Cn, D)
        for pcap, mcap, ccap, dcap, number, word in ((P, M, Cn - 1, D, Cn, "contact_capacity"), (P, M, Cn, D - 1, D, "dot_capacity"),
                                                     (P - 1, M, Cn, D, P, "pair_capacity"), (P, M - 1, Cn, D, M, "atom_capacity"),
                                                     (P, M, 0, D, Cn, "contact_capacity")):
            run = Run(ctx, 33, xyz, r, offs, group, ng, pcap, mcap, ccap, dcap)      # (Run checks the guards)
            assert run.error is not None and word in run.error and str(number) in run.error, run.error
            for k in ("ps", "pg", "areas", "so", "pa", "pb", "cf", "cp", "cn", "ca", "bm", "dp"):
                assert np.all(run.raw[k] == -7), k
            assert Run(ctx, 33, xyz, r, offs, group, ng, P, M, Cn, D).bytes() == good.bytes()   # the call after a failed one
        short = Run(ctx, 33, xyz, r, offs, group, ng, P, M, Cn - 1, D)
        assert "contact rows" in short.error
    finally:
        ctx.close()


def test_refusals_leave_the_context_usable(fa, edge):
    xyz, r, offs, group, ng = edge
    ps, pg, so, pa = cr.edge_table()
    P, M = len(ps), len(pa)
    _, _, want = cr.edge_contacts(31)
    Cn, D = len(want["contact_partner"]), len(want["dot_partner"])
    ctx = fa.GpuContext(0)
    try:
        good = Run(ctx, 31, xyz, r, offs, group, ng, P, M, Cn, D)
        assert good.error is None
        for kw, words in ((dict(alg=0), ("Lee-Richards",)), (dict(misalign=True), ("16 bytes",))):
            bad = Run(ctx, 31, xyz, r, offs, group, ng, P, M, Cn, D, **kw)
            assert bad.error is not None and all(w in bad.error for w in words), bad.error
            assert all(np.all(v == -7) for v in bad.raw.values())
        bad = Run(ctx, 129, xyz, r, offs, group, ng, P, M, Cn, D)
        assert bad.error is not None and "128" in bad.error and all(np.all(v == -7) for v in bad.raw.values())
        assert Run(ctx, 31, xyz, r, offs, group, ng, P, M, Cn, D).bytes() == good.bytes()
    finally:
        ctx.close()


def test_no_pair_and_no_buried_point(fa):
    """P == 0: C = 0 and contact_first [1] = 0; a pair in contact that buries no point (N = 1): C = 0, contact_first [M + 1] zeros"""
    ctx = fa.GpuContext(0)
    try:
        xyz, r = np.array([[0.0, 0, 0], [50.0, 0, 0]]), np.array([1.5, 1.5])
        none = Run(ctx, 100, xyz, r, np.array([0, 2]), np.array([0, 1], np.int32), np.array([2], np.int32), 2, 4, 4, 4)
        assert none.error is None and (none.P, none.M, none.C, none.D) == (0, 0, 0, 0) and np.array_equal(none.cf, [0])
        xyz = np.array([[0.0, 0, 0], [0, 3.0, 0]])
        dry = Run(ctx, 1, xyz, r, np.array([0, 2]), np.array([0, 1], np.int32), np.array([2], np.int32), 2, 4, 4, 4)
        assert dry.error is None and (dry.P, dry.M, dry.C, dry.D) == (1, 2, 0, 0) and np.array_equal(dry.cf, [0, 0, 0])
        assert not dry.bm.any() and np.all(dry.pb == 0)
        wet = Run(ctx, 100, xyz, r, np.array([0, 2]), np.array([0, 1], np.int32), np.array([2], np.int32), 2, 4, 4, 400)
        assert wet.error is None and wet.C == 2 and np.array_equal(wet.cp, [1, 0]) and wet.D == wet.cn.sum() > 0
    finally:
        ctx.close()


def test_the_host_form_gives_the_device_forms_bytes(fa, edge):
    xyz, r, offs, group, ng = edge
    ps, pg, so, pa = cr.edge_table()
    P, M = len(ps), len(pa)
    _, _, want = cr.edge_contacts(100)
    ctx = fa.GpuContext(0)
    try:
        run = Run(ctx, 100, xyz, r, offs, group, ng, P, M, len(want["contact_partner"]), len(want["dot_partner"]))
    finally:
        ctx.close()
    got = fa.calc_interface_contacts(xyz, r, offs, group, ng, probe=cr.PROBE, n_points=100)
    assert (got.n_pairs, got.n_contacts, got.n_buried_dots) == (P, run.C, run.D)
    host = b"".join(a.tobytes() for a in (got.sasa, got.iso, got.totals, got.group_totals, got.pair_struct, got.pair_groups, got.pair_areas,
                                          got.side_offsets, got.pair_atom, got.pair_buried, got.contact_first, got.contact_partner,
                                          got.contact_points, got.contact_area, got.buried_masks))
    assert host == run.bytes()[:len(host)] and len(host) == len(run.bytes()) - run.dp.nbytes
    plain = fa.calc_interfaces(xyz, r, offs, group, ng, alg=SR, resolution=100, per_atom=True)
    for name in ("sasa", "iso", "totals", "group_totals", "pair_struct", "pair_groups", "pair_areas", "side_offsets", "pair_atom", "pair_buried"):
        assert getattr(got, name).tobytes() == getattr(plain, name).tobytes(), name
    # the interface patch drawn from the buried masks: as many dots as the table has points
    px, pr, _ = ir.pair_structures(xyz, r, so, pa)
    dots, first = fa.dots_from_masks(px, pr, got.buried_masks, got.n_buried_dots, probe=cr.PROBE, n_points=100)
    assert len(dots) == got.contact_points.sum() and first[-1] == got.n_buried_dots


def _golden():
    from freesasa_amd import ingest
    b = ingest.load_files([os.path.join(GOLDEN, "pdb", "2jo4.pdb")])
    g, n, st = b.chain_groups(None, separate_chains=True)
    assert st[0] == 0 and n[0] == 4
    return b, g, n


def test_golden_pdb(fa):
    b, g, n = _golden()
    got = fa.calc_interface_contacts(b.xyz, b.radii, b.offsets, g, n, n_points=100)
    plain = fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg=SR, resolution=100, per_atom=True)
    for name in ("sasa", "iso", "totals", "group_totals", "pair_struct", "pair_groups", "pair_areas", "side_offsets", "pair_atom", "pair_buried"):
        assert getattr(got, name).tobytes() == getattr(plain, name).tobytes(), name
    assert got.n_pairs >= 1 and got.n_contacts > 0
    px, pr, _ = ir.pair_structures(b.xyz, b.radii, got.side_offsets, got.pair_atom)
    unit = cr.unit_points(100)
    side, pair = cr.masks(px, pr, got.side_offsets, cr.PROBE, unit)
    want = cr.contacts(px, pr, got.side_offsets, cr.PROBE, unit, side, pair)
    for k in ("contact_first", "contact_partner", "contact_points", "contact_area", "buried_masks"):
        assert getattr(got, k).tobytes() == want[k].tobytes(), k
    for p in range(got.n_pairs):
        for s in (0, 1):
            rows = got.side_rows(p, s)
            assert rows.stop > rows.start
            other = got.contact_partner[rows]
            assert np.all((other >= got.side_offsets[2 * p + 1 - s]) & (other < got.side_offsets[2 * p + 2 - s]))


def test_the_tool_writes_the_contact_tables(fa, tmp_path):
    from tools import interfaces
    path = os.path.join(GOLDEN, "pdb", "2jo4.pdb")
    a, c, atoms, res = str(tmp_path / "a.tsv"), str(tmp_path / "c.tsv"), str(tmp_path / "atoms.tsv"), str(tmp_path / "res.tsv")
    interfaces.main([path, "-o", a, "--alg", "sr"])
    interfaces.main([path, "-o", c, "--alg", "sr", "--contacts", atoms, "--residue-contacts", res])
    assert open(a, "rb").read() == open(c, "rb").read()
    b, g, n = _golden()
    got = fa.calc_interface_contacts(b.xyz, b.radii, b.offsets, g, n, n_points=100)
    lines = open(atoms).read().splitlines()
    assert lines[0] == interfaces.CONTACT_HEADER and len(lines) == 1 + got.n_contacts
    names = [v.decode().strip() for v in b.atom_name_raw.tolist()]
    rows_atom = np.repeat(np.arange(len(got.pair_atom)), np.diff(got.contact_first))
    for line, i, j, k, area in zip(lines[1:], rows_atom, got.contact_partner, got.contact_points, got.contact_area):
        f = line.split("\t")
        assert len(f) == 13 and f[0] == "2jo4.pdb" and f[6] == names[got.pair_atom[i]] and f[10] == names[got.pair_atom[j]]
        assert f[11] == str(k) and f[12] == "%.3f" % area
    rlines = open(res).read().splitlines()
    assert rlines[0] == interfaces.RESIDUE_CONTACT_HEADER and 1 < len(rlines) <= len(lines)
    assert sum(int(l.split("\t")[9]) for l in rlines[1:]) == got.contact_points.sum() == got.n_buried_dots
