"""Residue-residue contact tables of the interfaces between chain groups on the device (include/freesasa_gpu.h:
freesasa_gpu_interface_residue_contacts_dev, freesasa_gpu_calc_interface_residue_contacts) against the numpy restatement
(tests/interface_residue_contacts_ref.py) on its batch at 1, 31, 32, 33, 100 and 128 test points and on a golden PDB file; the
contact entry's outputs untouched, the identities of the fold, capacities, repeated calls and another tile shape, the host form,
the refusals and tools/interfaces.py --contact-map.  Reads nothing outside the repository.

The restatement is never fed from the entry under test: its contact rows come from tests/interface_contacts_ref.py on the pair
structures cut on the host by tests/interfaces_ref.py.  Every new array is compared byte for byte: the counts are integers and
the areas are sums in a defined order, so no tolerance is needed."""
import os

import numpy as np
import pytest

import interface_contacts_ref as cr
import interface_residue_contacts_ref as qr
import interface_residues_ref as rr
import interfaces_ref as ir
from conftest import GOLDEN
from test_interface_contacts_gpu import Run as ContactRun, with_cfg
from test_interfaces_gpu import GUARD, _dev, _guarded

pytestmark = pytest.mark.gpu
SR = 1


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0, "no HIP device: the GPU tests cannot run"
    return freesasa_amd


@pytest.fixture(scope="module")
def batch():
    b = qr.rescontacts_batch()
    return tuple(np.array(a) for a in b[:5]) + (np.array(b[6]),)      # (copies: the restatement's own arrays stay read-only)


def _sizes(n_points):
    ps, pg, so, pa = qr.batch_table()
    c, f = qr.batch_contacts(n_points), qr.batch_fold(n_points)
    return len(ps), len(pa), len(c["contact_partner"]), len(c["dot_partner"]), len(f["rescontact_area"])


class Run:
    """one freesasa_gpu_interface_residue_contacts_dev call: the outputs as host arrays, the guards checked"""

    def __init__(self, ctx, n_points, xyz, r, offs, group, n_groups, res_first, pcap, mcap, ccap, dcap, qcap, alg=SR, misalign=False):
        import torch
        n, ns, G = len(r), len(offs) - 1, int(np.sum(n_groups))
        d_x, d_r, d_g = _dev(np.asarray(xyz).reshape(-1), np.float64), _dev(r, np.float64), _dev(group, np.int32)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        self.sizes = dict(sasa=n, iso=n, totals=ns, gt=3 * G, ps=pcap, pg=2 * pcap, areas=6 * pcap, so=2 * pcap + 1, pa=mcap, pb=mcap,
                          cf=mcap + 1, cp=ccap, cn=ccap, ca=ccap, bm=4 * mcap, dp=dcap, qo=2 * pcap + 1, qr=2 * qcap, qc=2 * qcap, qa=qcap, qv=qcap)
        self.sizes = {k: max(v, 0) for k, v in self.sizes.items()}          # (a negative capacity, refused: arrays of no rows)
        kinds = dict(sasa=f64, iso=f64, totals=f64, gt=f64, ps=i32, pg=i32, areas=f64, so=i64, pa=i32, pb=f64, cf=i64, cp=i32, cn=i32, ca=f64,
                     bm=i32, dp=i32, qo=i64, qr=i32, qc=i32, qa=f64, qv=i32)
        out = {k: _guarded(v, kinds[k], -7.0 if kinds[k] is f64 else -7) for k, v in self.sizes.items()}
        self.error = None
        p = {k: v.data_ptr() for k, v in out.items()}
        try:
            self.P, self.M, self.C, self.D, self.Q = ctx.interface_residue_contacts(
                d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), n_groups, res_first, p["sasa"], p["iso"], pcap, p["areas"], qcap, p["qa"],
                d_rescontact_offsets=p["qo"], d_rescontact_residues=p["qr"], d_rescontact_counts=p["qc"], d_rescontact_reverse=p["qv"],
                contact_capacity=ccap, d_contact_first=p["cf"], d_contact_partner=p["cp"], d_contact_points=p["cn"], d_contact_area=p["ca"],
                d_buried_masks=p["bm"] + (4 if misalign else 0), dot_capacity=dcap, d_dot_partner=p["dp"], d_pair_struct=p["ps"],
                d_pair_groups=p["pg"], atom_capacity=mcap, d_side_offsets=p["so"], d_pair_atom=p["pa"], d_pair_buried=p["pb"],
                d_totals=p["totals"], d_group_totals=p["gt"], alg=alg, n_points=n_points)
        except RuntimeError as e:
            self.error = str(e)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        for k, v in host.items():
            assert len(v) == self.sizes[k] + GUARD and np.all(v[self.sizes[k]:] == -7), f"the guard behind {k} was written"
        self.raw = {k: v[:self.sizes[k]] for k, v in host.items()}
        if self.error is None:
            P, M, Cn, D, Q = self.P, self.M, self.C, self.D, self.Q
            used = dict(sasa=n, iso=n, totals=ns, gt=3 * G, ps=P, pg=2 * P, areas=6 * P, so=2 * P + 1, pa=M, pb=M, cf=M + 1 if P else 1, cp=Cn, cn=Cn,
                        ca=Cn, bm=4 * M, dp=D, qo=2 * P + 1, qr=2 * Q, qc=2 * Q, qa=Q, qv=Q)
            for k, u in used.items():
                assert np.all(self.raw[k][u:] == -7), f"{k} was written beyond its rows"
            self.out = {k: self.raw[k][:u] for k, u in used.items()}
            self.qo, self.qr, self.qc = self.out["qo"], self.out["qr"].reshape(Q, 2), self.out["qc"].reshape(Q, 2)
            self.qa, self.qv = self.out["qa"], self.out["qv"]

    def contact_bytes(self):
        """the bytes of ContactRun.bytes(): the interface outputs and the contact entry's"""
        return b"".join(self.out[k].tobytes() for k in ("sasa", "iso", "totals", "gt", "ps", "pg", "areas", "so", "pa", "pb", "cf", "cp", "cn", "ca", "bm", "dp"))

    def folded_bytes(self):
        return b"".join(self.out[k].tobytes() for k in ("qo", "qr", "qc", "qa", "qv"))

    def untouched(self):
        return all(np.all(self.raw[k] == -7) for k in self.raw if k not in ("sasa", "iso", "totals", "gt"))


def _same_fold(run, want):
    assert run.Q == len(want["rescontact_area"])
    for got, k in ((run.qo, "rescontact_offsets"), (run.qr, "rescontact_residues"), (run.qc, "rescontact_counts"), (run.qa, "rescontact_area"),
                   (run.qv, "rescontact_reverse")):
        assert got.dtype == want[k].dtype and got.shape == want[k].shape and got.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("n_points", qr.N_POINTS)
def test_the_table_on_the_batch(fa, batch, n_points):
    xyz, r, offs, group, ng, rf = batch
    P, M, Cn, D, Q = _sizes(n_points)
    ctx = fa.GpuContext(0)
    try:
        old = ContactRun(ctx, n_points, xyz, r, offs, group, ng, P, M, Cn, D)
        run = Run(ctx, n_points, xyz, r, offs, group, ng, rf, P, M, Cn, D, Q)
        again = Run(ctx, n_points, xyz, r, offs, group, ng, rf, P + 3, M + 5, Cn + 5, D + 5, Q + 7)
        assert old.error is None and run.error is None and again.error is None, (old.error, run.error, again.error)
        after = ContactRun(ctx, n_points, xyz, r, offs, group, ng, P, M, Cn, D)          # the contact entry behind the new one
        assert after.error is None and after.bytes() == old.bytes()
    finally:
        ctx.close()
    assert (run.P, run.M, run.C, run.D) == (P, M, Cn, D)
    assert run.contact_bytes() == old.bytes()                                            # the contact entry's outputs: untouched
    _same_fold(run, qr.batch_fold(n_points))
    assert again.folded_bytes() == run.folded_bytes() and again.contact_bytes() == run.contact_bytes()


def test_identities(fa, batch):
    xyz, r, offs, group, ng, rf = batch
    P, M, Cn, D, Q = _sizes(100)
    ctx = fa.GpuContext(0)
    try:
        run = Run(ctx, 100, xyz, r, offs, group, ng, rf, P, M, Cn, D, Q)
        atoms = Run(ctx, 100, xyz, r, offs, group, ng, np.arange(len(r) + 1), P, M, Cn, D, Cn)
        assert run.error is None and atoms.error is None, (run.error, atoms.error)
    finally:
        ctx.close()
    so, pa, cf, cp, cn, ca = (run.out[k] for k in ("so", "pa", "cf", "cp", "cn", "ca"))
    _, first, seg_res, seg_side = rr.segments(so, pa, rf)
    # the rows of a segment are contiguous and ascend in the partner residue: a folded row's segment is found from its place
    seg_q = np.bincount(seg_side, minlength=2 * P)
    row_side = np.searchsorted(run.qo, np.arange(run.Q), side="right") - 1
    rows_per_seg, k = [], 0
    for a in range(len(seg_res)):
        n = 0
        while k < run.Q and row_side[k] == seg_side[a] and run.qr[k, 0] == seg_res[a]:
            n += run.qc[k, 0]; k += 1
        rows_per_seg.append(n)
    assert k == run.Q and np.array_equal(rows_per_seg, cf[first[1:]] - cf[first[:-1]])          # n_rows per segment
    assert seg_q.sum() == len(seg_res)
    for q in range(2 * P):                                                                         # n_points per side
        assert run.qc[run.qo[q]:run.qo[q + 1], 1].sum() == cn[cf[so[q]]:cf[so[q + 1]]].sum(), q
    has = np.nonzero(run.qv >= 0)[0]
    assert len(has) and np.array_equal(run.qv[run.qv[has]], has) and np.array_equal(run.qr[run.qv[has]], run.qr[has][:, ::-1])
    assert np.array_equal(row_side[run.qv[has]], row_side[has] ^ 1)                                # ... in the same pair, on the other side
    # residues of one atom: the folded table IS the atom table
    rows_atom = np.repeat(np.arange(M), np.diff(cf))
    assert atoms.Q == Cn and np.array_equal(atoms.qr, np.stack([pa[rows_atom], pa[cp]], axis=1))
    assert np.array_equal(atoms.qc, np.stack([np.ones(Cn, np.int32), cn], axis=1)) and atoms.qa.tobytes() == ca.tobytes()
    assert np.array_equal(atoms.qo, cf[so]) and atoms.contact_bytes() == run.contact_bytes()


def test_another_tile_shape_gives_the_same_bytes(fa, batch):
    xyz, r, offs, group, ng, rf = batch
    sizes = _sizes(100)

    def run():
        ctx = fa.GpuContext(0)
        try:
            return Run(ctx, 100, xyz, r, offs, group, ng, rf, *sizes)
        finally:
            ctx.close()

    base = run()
    assert base.error is None, base.error
    for cfg in ("64,3,48,0", "256,8,112,0"):
        other = with_cfg(cfg, run)
        assert other.error is None and other.folded_bytes() == base.folded_bytes() and other.contact_bytes() == base.contact_bytes(), (cfg, other.error)


def test_capacities(fa, batch):
    xyz, r, offs, group, ng, rf = batch
    P, M, Cn, D, Q = _sizes(33)
    ctx = fa.GpuContext(0)
    try:
        good = Run(ctx, 33, xyz, r, offs, group, ng, rf, P, M, Cn, D, Q)
        assert good.error is None and (good.C, good.D, good.Q) == (Cn, D, Q)
        for caps, number, word in (((P - 1, M, Cn, D, Q), P, "pair_capacity"), ((P, M - 1, Cn, D, Q), M, "atom_capacity"),
                                   ((P, M, Cn - 1, D, Q), Cn, "contact_capacity"), ((P, M, Cn, D - 1, Q), D, "dot_capacity"),
                                   ((P, M, Cn, D, Q - 1), Q, "rescontact_capacity"), ((P, M, Cn, D, 0), Q, "rescontact_capacity"),
                                   ((P - 1, M - 1, Cn - 1, D - 1, Q - 1), P, "pair_capacity"), ((P, M, Cn - 1, D, Q - 1), Cn, "contact_capacity")):
            run = Run(ctx, 33, xyz, r, offs, group, ng, rf, *caps)      # (Run checks the guards)
            assert run.error is not None and word in run.error and str(number) in run.error, run.error
            assert run.untouched(), word
            again = Run(ctx, 33, xyz, r, offs, group, ng, rf, P, M, Cn, D, Q)                      # the call after a failed one
            assert again.folded_bytes() == good.folded_bytes() and again.contact_bytes() == good.contact_bytes()
        short = Run(ctx, 33, xyz, r, offs, group, ng, rf, P, M, Cn, D, Q - 1)
        assert short.error.endswith(f"rescontact_capacity {Q - 1} is too small: the interfaces have {Q} residue contact rows")
    finally:
        ctx.close()


def test_no_pair_and_no_buried_point(fa):
    """P == 0: Q = 0 and rescontact_offsets [1] = 0; a pair in contact that buries no point (N = 1): Q = 0, offsets [2 P + 1] zeros"""
    ctx = fa.GpuContext(0)
    try:
        r, off, g, ng, rf = np.array([1.5, 1.5]), np.array([0, 2]), np.array([0, 1], np.int32), np.array([2], np.int32), np.array([0, 1, 2])
        none = Run(ctx, 100, np.array([[0.0, 0, 0], [50.0, 0, 0]]), r, off, g, ng, rf, 2, 4, 4, 4, 4)
        assert none.error is None and (none.P, none.M, none.C, none.D, none.Q) == (0, 0, 0, 0, 0) and np.array_equal(none.qo, [0])
        xyz = np.array([[0.0, 0, 0], [0, 3.0, 0]])
        dry = Run(ctx, 1, xyz, r, off, g, ng, rf, 2, 4, 4, 4, 0)
        assert dry.error is None and (dry.P, dry.M, dry.C, dry.D, dry.Q) == (1, 2, 0, 0, 0) and np.array_equal(dry.qo, [0, 0, 0])
        wet = Run(ctx, 100, xyz, r, off, g, ng, rf, 2, 4, 4, 400, 2)
        assert wet.error is None and wet.Q == 2 and np.array_equal(wet.qr, [[0, 1], [1, 0]]) and np.array_equal(wet.qv, [1, 0])
        assert np.array_equal(wet.qo, [0, 1, 2]) and np.array_equal(wet.qc[:, 0], [1, 1]) and wet.qc[:, 1].sum() == wet.D
        assert wet.qa.tobytes() == wet.out["ca"].tobytes()
        one = Run(ctx, 100, xyz, r, off, g, ng, np.array([0, 2]), 2, 4, 4, 400, 2)                   # one residue over both groups: in contact with itself
        assert one.error is None and np.array_equal(one.qr, [[0, 0], [0, 0]]) and np.array_equal(one.qv, [1, 0])
    finally:
        ctx.close()


def test_refusals_leave_the_context_usable(fa, batch):
    xyz, r, offs, group, ng, rf = batch
    sizes = _sizes(31)
    ctx = fa.GpuContext(0)
    try:
        good = Run(ctx, 31, xyz, r, offs, group, ng, rf, *sizes)
        assert good.error is None
        split = rf.copy(); split[np.searchsorted(rf, offs[1])] += 1          # a residue across the first structure boundary
        for kw, words in ((dict(alg=0), ("Lee-Richards",)), (dict(misalign=True), ("16 bytes",))):
            bad = Run(ctx, 31, xyz, r, offs, group, ng, rf, *sizes, **kw)
            assert bad.error is not None and all(w in bad.error for w in words), bad.error
            assert all(np.all(v == -7) for v in bad.raw.values())
        for bad_rf, words in ((split, ("spans the boundary",)), (rf[:-1], ("res_first[n_res]", "atoms")), (rf[1:], ("res_first[0] must be 0",))):
            bad = Run(ctx, 31, xyz, r, offs, group, ng, bad_rf, *sizes)
            assert bad.error is not None and all(w in bad.error for w in words), bad.error
            assert all(np.all(v == -7) for v in bad.raw.values())
        bad = Run(ctx, 31, xyz, r, offs, group, ng, rf, *sizes[:4], -1)
        assert bad.error is not None and "rescontact_capacity must be >= 0" in bad.error and all(np.all(v == -7) for v in bad.raw.values())
        again = Run(ctx, 31, xyz, r, offs, group, ng, rf, *sizes)
        assert again.folded_bytes() == good.folded_bytes() and again.contact_bytes() == good.contact_bytes()
    finally:
        ctx.close()


def test_the_host_form_gives_the_device_forms_bytes(fa, batch):
    xyz, r, offs, group, ng, rf = batch
    sizes = _sizes(100)
    ctx = fa.GpuContext(0)
    try:
        run = Run(ctx, 100, xyz, r, offs, group, ng, rf, *sizes)
    finally:
        ctx.close()
    assert run.error is None, run.error
    got = fa.calc_interface_contacts(xyz, r, offs, group, ng, probe=qr.PROBE, n_points=100, res_first=rf)
    plain = fa.calc_interface_contacts(xyz, r, offs, group, ng, probe=qr.PROBE, n_points=100)
    assert (got.n_pairs, got.n_contacts, got.n_buried_dots, got.n_rescontacts) == (run.P, run.C, run.D, run.Q) and plain.n_rescontacts is None
    names = ("sasa", "iso", "totals", "group_totals", "pair_struct", "pair_groups", "pair_areas", "side_offsets", "pair_atom", "pair_buried",
             "contact_first", "contact_partner", "contact_points", "contact_area", "buried_masks")
    host = b"".join(getattr(got, k).tobytes() for k in names)
    assert host == b"".join(getattr(plain, k).tobytes() for k in names)
    assert host == run.contact_bytes()[:len(host)] and len(host) == len(run.contact_bytes()) - run.out["dp"].nbytes
    assert b"".join(getattr(got, k).tobytes() for k in qr.KEYS) == run.folded_bytes()
    assert got.rescontact_residues.shape == (run.Q, 2) and got.rescontact_counts.shape == (run.Q, 2)
    for p in range(got.n_pairs):
        for s in (0, 1):
            assert got.residue_side_rows(p, s) == range(int(run.qo[2 * p + s]), int(run.qo[2 * p + s + 1]))


def _golden():
    from freesasa_amd import ingest
    b = ingest.load_files([os.path.join(GOLDEN, "pdb", "2jo4.pdb")])
    g, n, st = b.chain_groups(None, separate_chains=True)
    assert st[0] == 0 and n[0] == 4
    return b, g, n


def test_golden_pdb(fa):
    from tools import interfaces
    b, g, n = _golden()
    got = fa.calc_interface_contacts(b.xyz, b.radii, b.offsets, g, n, n_points=100, res_first=b.res_first)
    assert got.n_pairs >= 1 and got.n_rescontacts > 0
    # the table equals the restatement, made of the restatement's own contact rows
    px, pr, _ = ir.pair_structures(b.xyz, b.radii, got.side_offsets, got.pair_atom)
    unit = cr.unit_points(100)
    side, pair = cr.masks(px, pr, got.side_offsets, cr.PROBE, unit)
    c = cr.contacts(px, pr, got.side_offsets, cr.PROBE, unit, side, pair)
    want = qr.fold_of(c, b.res_first, got.side_offsets, got.pair_atom)
    for k in qr.KEYS:
        assert getattr(got, k).dtype == want[k].dtype and getattr(got, k).tobytes() == want[k].tobytes(), k
    # as a dictionary it equals the tool's host fold of the atom rows: both add in row order
    atom_res = np.repeat(np.arange(b.n_residues, dtype=np.int64), np.diff(b.res_first))
    row_pair, ai, aj = interfaces.contact_row_keys(got.side_offsets, got.pair_atom, got.contact_first, got.contact_partner)
    fold = interfaces.fold_contact_rows(row_pair, atom_res[ai], atom_res[aj], got.contact_points, got.contact_area)
    host = {(int(p), int(ri), int(rj)): (int(k), float(a).hex()) for p, ri, rj, k, a in zip(*fold)}
    row_p = (np.searchsorted(got.rescontact_offsets, np.arange(got.n_rescontacts), side="right") - 1) // 2
    dev = {(int(p), int(ri), int(rj)): (int(k), float(a).hex())
           for p, (ri, rj), (_, k), a in zip(row_p, got.rescontact_residues, got.rescontact_counts, got.rescontact_area)}
    assert len(dev) == got.n_rescontacts and dev == host
    # the source residues with rows are the interface residues of the per-residue table
    res = fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg=SR, resolution=100, res_first=b.res_first, min_buried=0.0)
    for p in range(got.n_pairs):
        for s in (0, 1):
            rows = got.residue_side_rows(p, s)
            mine = np.unique(got.rescontact_residues[rows.start:rows.stop, 0])
            assert np.array_equal(mine, res.res_index[res.side_rows(p, s)]), (p, s)


def test_the_tool_writes_the_contact_map(fa, tmp_path):
    from tools import interfaces
    path = os.path.join(GOLDEN, "pdb", "2jo4.pdb")
    out = {k: str(tmp_path / f"{k}.tsv") for k in ("a", "b", "c", "atoms", "res", "atoms2", "res2", "map", "map2")}
    interfaces.main([path, "-o", out["a"], "--alg", "sr", "--contacts", out["atoms"], "--residue-contacts", out["res"]])
    interfaces.main([path, "-o", out["b"], "--alg", "sr", "--contact-map", out["map"]])
    interfaces.main([path, "-o", out["c"], "--alg", "sr", "--contacts", out["atoms2"], "--residue-contacts", out["res2"], "--contact-map", out["map2"]])
    read = lambda k: open(out[k], "rb").read()
    assert read("a") == read("b") == read("c") and read("atoms") == read("atoms2") and read("res") == read("res2") and read("map") == read("map2")
    b, g, n = _golden()
    got = fa.calc_interface_contacts(b.xyz, b.radii, b.offsets, g, n, n_points=100, res_first=b.res_first)
    lines = open(out["map"]).read().splitlines()
    assert lines[0] == interfaces.CONTACT_MAP_HEADER
    pairs = int(np.count_nonzero(got.rescontact_reverse >= 0)) // 2 + int(np.count_nonzero(got.rescontact_reverse < 0))
    assert len(lines) == 1 + pairs
    fields = [l.split("\t") for l in lines[1:]]
    assert all(len(f) == 15 and f[0] == "2jo4.pdb" for f in fields)
    assert sum(int(f[10]) + int(f[13]) for f in fields) == got.n_buried_dots == got.contact_points.sum()
    assert sum(int(f[9]) + int(f[12]) for f in fields) == got.n_contacts
