"""Chain groups on the device (include/freesasa_gpu.h, freesasa_gpu_groups_dev / freesasa_gpu_calc_groups): complex
areas bit-identical to the plain batch entries, isolated areas and totals bit-identical to the plain entries on the
groups cut out on the host, the buried totals, the reference (per atom and committed totals), a docking-sized batch,
errors and allocation failures.  Reads nothing outside the repository."""
import json
import math
import os

import numpy as np
import pytest

import tools
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LR_TOL = 1e-8          # A^2 per atom, as in tests/test_gpu_parity.py
LR, SR = 0, 1
RES = {LR: 20, SR: 100}


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0, "no HIP device: the GPU tests cannot run"
    return freesasa_amd


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(torch.device("cuda:0"))


def _empty(n, dtype=None):
    import torch
    return torch.empty(max(n, 1), dtype=dtype or torch.float64, device=torch.device("cuda:0"))


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def run_groups(ctx, alg, xyz, r, offs, group, n_groups):
    d_x, d_r, d_g = _dev(xyz.reshape(-1), np.float64), _dev(r, np.float64), _dev(group, np.int32)
    n, ns, G = len(r), len(offs) - 1, int(np.sum(n_groups))
    d_s, d_i, d_t, d_gt = _empty(n), _empty(n), _empty(ns), _empty(3 * G)
    ctx.groups(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), n_groups, d_s.data_ptr(), d_i.data_ptr(),
               d_t.data_ptr(), d_gt.data_ptr(), alg=alg, resolution=RES[alg])
    return (d_s.cpu().numpy()[:n], d_i.cpu().numpy()[:n], d_t.cpu().numpy()[:ns], d_gt.cpu().numpy()[:3 * G].reshape(G, 3))


def run_plain(ctx, alg, xyz, r, offs):
    d_x, d_r = _dev(xyz.reshape(-1), np.float64), _dev(r, np.float64)
    d_s, d_t = _empty(len(r)), _empty(len(offs) - 1)
    if alg == LR:
        ctx.lee_richards(d_x.data_ptr(), d_r.data_ptr(), offs, d_s.data_ptr(), d_t.data_ptr(), n_slices=RES[LR])
    else:
        ctx.shrake_rupley(d_x.data_ptr(), d_r.data_ptr(), offs, d_s.data_ptr(), 0, d_t.data_ptr(), n_points=RES[SR])
    return d_s.cpu().numpy()[:len(r)], d_t.cpu().numpy()[:len(offs) - 1]


def isolated(xyz, r, offs, group, n_groups):
    """the groups cut out on the host, structure-major: (xyz, radii, offsets, input index of every atom)"""
    idx, sizes = [], []
    for s in range(len(offs) - 1):
        ids = group[offs[s]:offs[s + 1]]
        for g in range(n_groups[s]):
            sel = offs[s] + np.nonzero(ids == g)[0]
            idx.append(sel)
            sizes.append(sel.size)
    idx = np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)
    return xyz[idx], r[idx], _offsets(sizes), idx


def check_consistency(ctx, alg, xyz, r, offs, group, n_groups):
    sasa, iso, tot, gt = run_groups(ctx, alg, xyz, r, offs, group, n_groups)
    want, want_tot = run_plain(ctx, alg, xyz, r, offs)
    assert np.array_equal(sasa, want)
    assert np.array_equal(tot, want_tot)
    ix, ir, ioffs, idx = isolated(xyz, r, offs, group, n_groups)
    if idx.size:
        iso_want, iso_tot = run_plain(ctx, alg, ix, ir, ioffs)
        assert np.array_equal(iso[idx], iso_want)
        assert np.array_equal(gt[:, 0], iso_tot)
    free = np.ones(len(r), bool)
    free[idx] = False
    assert np.array_equal(iso[free], sasa[free])
    assert np.array_equal(gt[:, 2], gt[:, 0] - gt[:, 1])
    for k in range(len(ioffs) - 1):
        f = math.fsum(sasa[idx[ioffs[k]:ioffs[k + 1]]])
        assert abs(gt[k, 1] - f) <= 1e-9 * abs(f), (k, gt[k, 1], f)
    assert np.all(iso >= sasa - 1e-9)     # an atom can only lose area to the rest of its complex
    return sasa, iso, gt


def _mixed_batch(seed):
    rng = np.random.default_rng(seed)
    parts, groups, ngs = [], [], []
    for k in range(6):                                   # coils and globules, 1 to 5 groups, some atoms in none
        n = int(rng.integers(800, 2500))
        x, r = tools.coil(n, 500 + k) if k % 2 else tools.globule(n, 600 + k)
        ng = 1 + k % 5
        g = rng.integers(-1, ng, size=n).astype(np.int32) if k % 3 == 0 else np.sort(rng.integers(0, ng, size=n)).astype(np.int32)
        parts.append((x, r)); groups.append(g); ngs.append(ng)
    x, r = tools.globule(1500, 41)                       # n_groups = 0
    parts.append((x, r)); groups.append(np.full(1500, -1, np.int32)); ngs.append(0)
    x, r = tools.coil(1200, 42)                          # an empty group (1) and a one-atom group (2)
    g = np.where(np.arange(1200) < 700, 0, 3).astype(np.int32)
    g[555] = 2
    parts.append((x, r)); groups.append(g); ngs.append(4)
    x, r = tools.globule(4000, 43)                       # 300 groups, interleaved
    parts.append((x, r)); groups.append(rng.integers(0, 300, size=4000).astype(np.int32)); ngs.append(300)
    xyz = np.concatenate([p[0] for p in parts]); r = np.concatenate([p[1] for p in parts])
    return xyz, r, _offsets([len(p[1]) for p in parts]), np.concatenate(groups), np.array(ngs, np.int32)


@pytest.mark.parametrize("alg", [LR, SR])
def test_groups_are_the_plain_entries_bit_for_bit(fa, alg):
    ctx = fa.GpuContext(0)
    try:
        for seed in (1, 2):
            check_consistency(ctx, alg, *_mixed_batch(seed))
    finally:
        ctx.close()


def _docking_batch(n_complex, n_each, seed):
    rng = np.random.default_rng(seed)
    xs, rs = [], []
    for k in range(n_complex):
        pair = []
        for h in range(2):
            x, r = tools.globule(n_each, 10_000 + 2 * k + h)
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            x = (x - x.mean(axis=0)) @ q
            pair.append((x, r))
        a, b = pair
        b_x = b[0] + np.array([a[0][:, 0].max() - b[0][:, 0].min() - 8.0, 0.0, 0.0])   # in contact along x
        xs += [a[0], b_x]; rs += [a[1], b[1]]
    xyz, r = np.concatenate(xs), np.concatenate(rs)
    group = np.tile(np.repeat(np.array([0, 1], np.int32), n_each), n_complex)
    return xyz, r, _offsets([2 * n_each] * n_complex), group, np.full(n_complex, 2, np.int32)


@pytest.mark.parametrize("alg", [LR, SR])
def test_docking_sized_batch(fa, alg):
    """200 complexes of two 5 000-atom globules in contact, random orientations."""
    xyz, r, offs, group, ng = _docking_batch(200, 5000, 7)
    ctx = fa.GpuContext(0)
    try:
        sasa, iso, gt = check_consistency(ctx, alg, xyz, r, offs, group, ng)
    finally:
        ctx.close()
    assert np.all(gt[:, 2] >= 0)
    assert np.all(gt[:, 2].reshape(-1, 2).sum(axis=1) > 0)   # every pair buries some area


def _load_cases():
    from freesasa_amd import ingest
    with open(os.path.join(GOLDEN, "chain_groups.json")) as fh:
        cases = json.load(fh)
    out = []
    for c in cases:
        b = ingest.load_pdb_files([os.path.join(GOLDEN, "pdb", c["file"])])
        g, n, st = b.chain_groups(c["spec"], separate_chains=c["spec"] is None)
        assert st[0] == 0
        out.append((c, b, g, n))
    return out


@pytest.mark.parametrize("alg", [LR, SR])
def test_against_the_reference(fa, alg, reference_lib):
    import oracle
    key = "lr20" if alg == LR else "sr100"
    ctx = fa.GpuContext(0)
    try:
        for c, b, g, n in _load_cases():
            sasa, iso, tot, gt = run_groups(ctx, alg, b.xyz, b.radii, b.offsets, g, n)
            assert len(gt) == len(c["groups"])
            want = c["complex"][key]
            assert abs(tot[0] - want) <= 1e-8 * len(b.radii) + 1e-12 * want, (c["file"], tot[0], want)
            for k, wg in enumerate(c["groups"]):
                sel = g == k
                assert int(sel.sum()) == wg["atoms"]
                assert abs(gt[k, 0] - wg[key]) <= 1e-8 * wg["atoms"] + 1e-12 * wg[key], (c["file"], k, gt[k, 0], wg[key])
                ref, _ = reference_lib.calc_coord(b.xyz[sel], b.radii[sel], oracle.LEE_RICHARDS if alg == LR else oracle.SHRAKE_RUPLEY,
                                                  1.4, n_points=100, n_slices=20)
                if alg == SR:
                    assert np.array_equal(iso[sel], ref), (c["file"], k)
                else:
                    assert np.max(np.abs(iso[sel] - ref)) < LR_TOL, (c["file"], k)
    finally:
        ctx.close()


def test_golden_totals_without_the_reference(fa):
    """The committed totals alone (no reference library needed): every group of every case."""
    ctx = fa.GpuContext(0)
    try:
        for c, b, g, n in _load_cases():
            for alg, key in ((LR, "lr20"), (SR, "sr100")):
                _, _, tot, gt = run_groups(ctx, alg, b.xyz, b.radii, b.offsets, g, n)
                for k, wg in enumerate(c["groups"]):
                    assert abs(gt[k, 0] - wg[key]) <= 1e-8 * wg["atoms"] + 1e-12 * wg[key]
                    assert gt[k, 2] >= 0
    finally:
        ctx.close()


def test_errors_leave_the_context_usable(fa):
    import ctypes as C
    xyz, r = tools.coil(2000, 5)
    offs = np.array([0, 1200, 2000], np.int64)
    group = np.where(np.arange(2000) % 3 == 0, 0, 1).astype(np.int32)
    ng = np.array([2, 2], np.int32)
    ctx = fa.GpuContext(0)
    L = fa.lib()
    try:
        want = run_groups(ctx, LR, xyz, r, offs, group, ng)
        for bad_at, bad in ((17, -2), (1500, 2), (1999, 7)):
            g2 = group.copy()
            g2[bad_at] = bad
            with pytest.raises(RuntimeError, match="group id"):
                run_groups(ctx, LR, xyz, r, offs, g2, ng)
            assert str(bad_at) in ctx.error()
        for ng_bad in ([-1, 2], [2, 70000]):
            with pytest.raises(RuntimeError, match="n_groups"):
                run_groups(ctx, LR, xyz, r, offs, group, np.array(ng_bad, np.int32))
        d_x, d_r, d_g = _dev(xyz.reshape(-1)), _dev(r), _dev(group, np.int32)
        d_s, d_i = _empty(2000), _empty(2000)
        ngp = ng.ctypes.data_as(C.POINTER(C.c_int32))
        op = offs.ctypes.data_as(C.POINTER(C.c_int64))
        args = [ctx._h, 0, d_x.data_ptr(), d_r.data_ptr(), op, 2, d_g.data_ptr(), ngp, 1.4, 20, d_s.data_ptr(), d_i.data_ptr(), None, None]
        for k in (2, 3, 4, 6, 7, 10, 11):
            a = list(args)
            a[k] = None
            assert L.freesasa_gpu_groups_dev(*a) == -1
            assert "null argument" in ctx.error()
        assert L.freesasa_gpu_groups_dev(None, *args[1:]) == -1
        got = run_groups(ctx, LR, xyz, r, offs, group, ng)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    finally:
        ctx.close()


def test_every_allocation_failure_is_clean(fa):
    xyz, r = tools.coil(3000, 9)
    offs = np.array([0, 1000, 3000], np.int64)
    group = (np.arange(3000) % 2).astype(np.int32)
    ng = np.array([2, 2], np.int32)
    ctx = fa.GpuContext(0)
    want = run_groups(ctx, SR, xyz, r, offs, group, ng)
    ctx.close()
    L = fa.lib()
    failures = 0
    try:
        for n in range(1, 200):
            ctx = fa.GpuContext(0)                  # a fresh context: every buffer is allocated in this call
            try:
                L.freesasa_gpu_test_fail_after(n)
                try:
                    got = run_groups(ctx, SR, xyz, r, offs, group, ng)
                    ok = True
                except RuntimeError:
                    ok = False
                L.freesasa_gpu_test_fail_after(0)
                again = run_groups(ctx, SR, xyz, r, offs, group, ng)   # the next call succeeds
                for a, b in zip(again, want):
                    assert np.array_equal(a, b)
            finally:
                L.freesasa_gpu_test_fail_after(0)
                ctx.close()
            if ok:
                for a, b in zip(got, want):
                    assert np.array_equal(a, b)
                break
            failures += 1
        assert failures >= 10, failures             # the groups' own buffers and run_batch's
    finally:
        L.freesasa_gpu_test_fail_after(0)


def test_async_batch_in_flight_is_collected_first(fa):
    xyz, r, offs, group, ng = _mixed_batch(3)
    bx, br, boffs = tools.coil_batch(4, 3000, seed0=77)
    ctx = fa.GpuContext(0)
    try:
        want_b, _ = run_plain(ctx, LR, bx, br, boffs)
        want = run_groups(ctx, LR, xyz, r, offs, group, ng)
        d_x, d_r, d_s = _dev(bx.reshape(-1)), _dev(br), _empty(len(br))
        d_s.fill_(-1.0)
        ctx.lee_richards_async(d_x.data_ptr(), d_r.data_ptr(), boffs, d_s.data_ptr())
        got = run_groups(ctx, LR, xyz, r, offs, group, ng)
        assert np.array_equal(d_s.cpu().numpy(), want_b)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    finally:
        ctx.close()


@pytest.mark.parametrize("alg", [LR, SR])
def test_host_arrays_equal_the_device_entry(fa, alg):
    xyz, r, offs, group, ng = _mixed_batch(4)
    ctx = fa.GpuContext(0)
    try:
        want = run_groups(ctx, alg, xyz, r, offs, group, ng)
    finally:
        ctx.close()
    got = fa.calc_groups(xyz, r, offs, group, ng, alg=alg, resolution=RES[alg])
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    with pytest.raises(RuntimeError, match="group id"):
        fa.calc_groups(xyz, r, offs, np.full_like(group, 400), ng, alg=alg, resolution=RES[alg])
