"""The cell sort on the device, on its own, through the test hook freesasa_gpu_cell_sort_dev - the engine's own launches, one
pass, forced into each of the three arrangements (0 the general pipeline k_prep_general / k_count / k_scan / k_scatter, 1
k_sort_struct with the dense table, 2 k_sort_struct with the compact table) - against the numpy reference
(tests/cell_sort_ref.py): grids, cell bases, the cell total, the sorted records, every table entry and every entry nobody may
write, the density samples, and the three arrangements against each other.  Everything is an integer or a copied double: every
comparison is exact.  tests/test_cell_sort.py proves the reference, its case builders and check_sorted without a device."""
import numpy as np
import pytest
import torch

import cell_sort_ref as ref
import freesasa_amd as fa
import tools

pytestmark = pytest.mark.gpu

FUSED, GENERAL = ref.cases_fused(), ref.cases_general()
BY_NAME = {c.name: c for c in FUSED + GENERAL}


@pytest.fixture(scope="module")
def ctx():
    c = fa.GpuContext()
    yield c
    c.close()


def upload(xyz, radii):
    return (torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1)).cuda(), torch.from_numpy(np.ascontiguousarray(radii, dtype=np.float64)).cuda())


def sort(ctx, dev, case, arrangement, cells_cap=None):
    return ctx.cell_sort(dev[0].data_ptr(), dev[1].data_ptr(), case.offsets, case.probe, arrangement,
                         case.cap(arrangement) if cells_cap is None else cells_cap, case.shared)


def good_pass(ctx, case, arrangements=None, dev=None, cells_cap=None):
    """the case under every arrangement it names: each a good pass, and per cell the same sets of atoms in all of them"""
    case.check_claims()
    dev = dev or upload(case.xyz, case.radii)
    locs, outs = [], []
    for a in arrangements or case.arrangements:
        out = sort(ctx, dev, case, a, cells_cap)
        locs.append(ref.check_sorted(out, case.xyz, case.radii, case.offsets, case.probe, a, case.shared, ref=case.ref))
        outs.append(out)
    assert all(np.array_equal(locs[0], l) for l in locs)
    return outs


# ---------------------------------------------------------------- a., b. good passes

@pytest.mark.parametrize("case", FUSED, ids=repr)
def test_shapes_of_the_one_workgroup_sort(ctx, case):
    good_pass(ctx, case)


@pytest.mark.parametrize("case", GENERAL, ids=repr)
def test_shapes_of_the_general_pipeline(ctx, case):
    good_pass(ctx, case)


def test_stale_tables_of_an_earlier_batch():
    """one context: about 3e5 cells, then 40 cells in the same buffers, then the first batch again - under the general pipeline,
    which clears its histogram itself, and under k_sort_struct with the dense table, which writes its runs only"""
    big, small = BY_NAME["about 3e5 cells"], ref.one("40 cells", (5, 4, 2), 30)
    c = fa.GpuContext()
    try:
        for a in (0, 1):
            (first,) = good_pass(c, big, (a,))
            good_pass(c, small, (a,))
            (again,) = good_pass(c, big, (a,))
            assert again["status"][ref.ST_CELLS:].tobytes() == first["status"][ref.ST_CELLS:].tobytes()
            assert np.array_equal(again["ncells"], first["ncells"])
            if a == 0:      # (k_sort_struct hands out the runs in the order its workgroups arrive)
                assert again["grid"].tobytes() == first["grid"].tobytes() and np.array_equal(again["cell_start"], first["cell_start"])
    finally:
        c.close()


# ---------------------------------------------------------------- c. declined and failed passes

ROUND_32 = ref.Case("structures of 31, 63, 95 and 31 cells", lambda: [ref.line(31, seed=1), ref.line(63, seed=2), ref.lattice((19, 5, 1), ref.random_cells((19, 5, 1), 30, 3), 3), ref.line(31, seed=4)],
                    [("every structure's cells and the entry behind them fill whole table words", lambda R: ((R.C + 1) % 32 == 0).all())])


@pytest.mark.parametrize("case", [BY_NAME["65 atoms"], BY_NAME["600 structures of 1 to 40 atoms"], BY_NAME["about 3e5 cells"],
                                  BY_NAME["five passes, single atoms and SORT_ATOMS in one batch"], ROUND_32], ids=repr)
def test_capacity_is_exact(ctx, case):
    """a table of exactly the batch's total is accepted, one cell less is declined with the full total counted.  With the compact
    table a structure takes its C + 1 entries rounded up to 32 and needs the first C + 1 of them: one cell less is declined where
    every structure's C + 1 is a multiple of 32 (ROUND_32); elsewhere whichever structure arrives last needs at least total - 31,
    so 32 less is declined whatever the order of arrival"""
    case.check_claims()
    dev = upload(case.xyz, case.radii)
    for a in (0, 1, 2):
        total = case.ref.total(a)
        good_pass(ctx, case, (a,), dev, cells_cap=total)
        less = total - 32 if a == 2 and case is not ROUND_32 else total - 1
        out = sort(ctx, dev, case, a, less)
        assert out["error"] == 0 and out["retry"] & 1 and out["cells"] == total, (a, out["error"], out["retry"], out["cells"], total)
        if a == 0:
            assert out["retry"] == 1


def test_a_structure_too_long_for_one_workgroup(ctx):
    dims = (30, 30, 30)
    long_one = ref.lattice(dims, ref.random_cells(dims, ref.SORT_ATOMS + 1, 5), 5, origin=(500, 0, 0))
    parts = ref.small_batch(9, 31) + [long_one] + ref.small_batch(5, 32)
    case = ref.Case("SORT_ATOMS + 1 atoms among ordinary structures", parts, [("", lambda R: np.diff(R.offsets).max() == ref.SORT_ATOMS + 1)])
    dev = upload(case.xyz, case.radii)
    good_pass(ctx, case, (0,), dev)
    for a in (1, 2):
        out = sort(ctx, dev, case, a)
        others = case.ref.total(a) - ref.take_of(int(case.ref.C[9]), a)
        assert out["error"] == 0 and out["retry"] & 2 and out["cells"] == others, (a, out["error"], out["retry"], out["cells"], others)


def test_more_cells_than_one_workgroup_numbers(ctx):
    case = ref.declined_513()
    case.check_claims()
    dev = upload(case.xyz, case.radii)
    C = int(case.ref.C[0])
    out = sort(ctx, dev, case, 2, 0)
    assert out["error"] == 0 and out["retry"] & 2 and out["cells"] == ref.take_of(C, 2), (out["error"], out["retry"], out["cells"])
    out = sort(ctx, dev, case, 0, 5000)
    assert (out["error"], out["retry"], out["cells"]) == (0, 1, C)


def bad_batches():
    parts = ref.small_batch(6, 77, sizes=(5, 30))
    xyz = np.concatenate([p[0] for p in parts])
    radii = np.concatenate([p[1] for p in parts])
    offsets = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.int64)
    b, e = int(offsets[2]), int(offsets[3])
    out = {}
    for name, value in (("a NaN coordinate", np.nan), ("an infinite coordinate", np.inf)):
        x = xyz.copy()
        x[b + 1, 1] = value
        out[name] = (x, radii, ref.ERR_BAD_COORD)
    r = radii.copy()
    r[b + 2] = np.nan
    out["a NaN radius"] = (xyz, r, ref.ERR_BAD_RADIUS)
    r = radii.copy()
    r[b:e] = -ref.PROBE
    out["radius + probe == 0 in a whole structure"] = (xyz, r, ref.ERR_BAD_RADIUS)
    x = xyz.copy()
    x[b], x[b + 1] = 0.0, 1e7 / np.sqrt(3.0)
    assert abs(np.linalg.norm(x[b + 1] - x[b]) - 1e7) < 1e-6
    out["two atoms 1e7 apart"] = (x, radii, ref.ERR_GRID_TOO_BIG)
    return out, ref.Case("the batch without the error", parts)


@pytest.mark.parametrize("name", ["a NaN coordinate", "an infinite coordinate", "a NaN radius", "radius + probe == 0 in a whole structure", "two atoms 1e7 apart"])
def test_errors_of_both_implementations(ctx, name):
    bad, good = bad_batches()
    xyz, radii, code = bad[name]
    dev = upload(xyz, radii)
    for a in (0, 1, 2):
        out = ctx.cell_sort(dev[0].data_ptr(), dev[1].data_ptr(), good.offsets, ref.PROBE, a)
        assert out["error"] == code, (a, out["error"], out["retry"])
        good_pass(ctx, good, (a,))


# ---------------------------------------------------------------- d. the hook itself

def test_hook_refusals(ctx):
    case = BY_NAME["65 atoms"]
    dx, dr = upload(case.xyz, case.radii)
    x, r, o = dx.data_ptr(), dr.data_ptr(), case.offsets
    for args, kw, text in (((0, r, o), {}, "null argument"), ((x, 0, o), {}, "null argument"),
                           ((x, r, [0]), {}, "n_structs must be > 0"), ((x, r, [1, 65]), {}, "offsets[0] must be 0"),
                           ((x, r, [0, 40, 30, 65]), {}, "offsets must be non-decreasing"), ((x, r, [0, 0, 0]), {}, "empty batch"),
                           ((x, r, o), {"arrangement": 3}, "unknown arrangement 3 (0: general pipeline, 1: k_sort_struct with the dense table, 2: with the compact table)"),
                           ((x, r, o), {"arrangement": -1}, "unknown arrangement -1 (0: general pipeline, 1: k_sort_struct with the dense table, 2: with the compact table)"),
                           ((x, r, o), {"cells_cap": -1}, "cells_cap must not be negative")):
        with pytest.raises(ValueError) as e:
            ctx.cell_sort(*args, probe=case.probe, **kw)
        assert str(e.value) == "freesasa_gpu_cell_sort_dev: " + text
    good_pass(ctx, case, dev=(dx, dr))


@pytest.mark.parametrize("arrangement", [0, 1, 2])
def test_every_allocation_of_the_hook_failing(arrangement):
    """a new context for every n: its n-th allocation fails, the call says so, and the next call on that context works; the
    first n at which nothing fails is one more than the allocations the hook makes - the workspace of the sort, the chunk
    table, the cell table: more than one of each kind of buffer"""
    case = BY_NAME["65 atoms"]
    dev = upload(case.xyz, case.radii)
    failed, done = 0, False
    for nth in range(1, 100):
        c = fa.GpuContext()
        try:
            fa.lib().freesasa_gpu_test_fail_after(nth)
            try:
                sort(c, dev, case, arrangement)
                done = True
            except ValueError as e:
                assert "dev_malloc" in str(e), str(e)
                done = False
            finally:
                fa.lib().freesasa_gpu_test_fail_after(0)
            good_pass(c, case, (arrangement,), dev)
        finally:
            c.close()
        if done:
            break
        failed += 1
    assert done and failed >= 3, (done, failed)


def test_the_hook_collects_batches_in_flight_first():
    """a fresh context, a batch submitted asynchronously, then the hook with cells_cap = 0: collecting the batch raises what the
    context has seen, and with it the engine's sizing - the capacity the arrays are sized with and the one the pass takes are the
    same number, and the pass is a good one; a capacity the pass does not take is refused and nothing is copied"""
    parts = [tools.coil(700 + 40 * k, 90 + k) for k in range(8)]
    coils = ref.Case("eight coils", parts, probe=1.4)
    case = BY_NAME["65 atoms"]
    dx, dr = upload(coils.xyz, coils.radii)
    dev = upload(case.xyz, case.radii)
    out = torch.zeros(coils.ref.n, dtype=torch.float64, device="cuda")
    for a in (0, 1, 2):
        c = fa.GpuContext()
        try:
            first_batch = fa.lib().freesasa_gpu_cell_sort_cap(c._h, case.ref.n, 1, 0)
            assert first_batch == 10 * case.ref.n + 256
            c.lee_richards_async(dx.data_ptr(), dr.data_ptr(), coils.offsets, out.data_ptr(), probe=1.4, n_slices=20)
            (got,) = good_pass(c, case, (a,), dev, cells_cap=0)
            assert got["cells_cap"] > coils.ref.total(2) > first_batch         # (what the collected batch taught the context)
            assert c.stats()["n_cells"] == coils.ref.total(2)                  # (... and it was collected, with its own verdict)
            # the arrays' capacity is part of the call: one the pass would not take is refused before anything is copied
            status = np.zeros(ref.STATUS_WORDS, dtype=np.int32)
            word = np.zeros(16, dtype=np.int64)
            p = lambda v: v.ctypes.data
            rc = fa.lib().freesasa_gpu_cell_sort_dev(c._h, dev[0].data_ptr(), dev[1].data_ptr(), case.offsets.ctypes.data_as(fa._lp), 1, case.probe, a, 0,
                                                     first_batch, 0, p(status), p(word), p(word), p(word), p(word), p(word), p(word), p(word), p(word))
            assert rc == -1 and c.error() == "the table arrays are sized for %d cells, the pass takes %d (freesasa_gpu_cell_sort_cap)" % (first_batch, got["cells_cap"])
            assert not status.any() and not word.any()
        finally:
            c.close()


def test_hook_calls_leave_what_the_context_learnt(oracle_lib):
    """hook calls that raise "not a batch for k_sort_struct" and "the table is too small" between the batches of a context: it
    goes on sorting eight coils with k_sort_struct and the compact table (the batch's cell total is that arrangement's), and
    Lee-Richards and Shrake-Rupley match the oracle as in tests/test_gpu_parity.py"""
    parts = [tools.coil(700 + 40 * k, 90 + k) for k in range(8)]
    coils = ref.Case("eight coils", parts, probe=1.4)
    dx, dr = upload(coils.xyz, coils.radii)
    n = coils.ref.n
    out, cnt = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    c = fa.GpuContext()
    try:
        c.lee_richards(dx.data_ptr(), dr.data_ptr(), coils.offsets, out.data_ptr())
        lr_first, cells = out.cpu().numpy().copy(), c.stats()["n_cells"]
        assert cells == coils.ref.total(2)
        big = ref.declined_513()
        dims = (30, 30, 30)
        long_one = ref.Case("", [ref.lattice(dims, ref.random_cells(dims, ref.SORT_ATOMS + 1, 5), 5)])
        for case, a, cap in ((big, 2, 0), (long_one, 1, 0), (long_one, 2, 0), (coils, 0, 100), (coils, 2, 100), (big, 0, 5000)):
            dev = upload(case.xyz, case.radii)
            assert sort(c, dev, case, a, cap)["retry"] != 0
        c.lee_richards(dx.data_ptr(), dr.data_ptr(), coils.offsets, out.data_ptr())
        assert c.stats()["n_cells"] == cells
        lr = out.cpu().numpy()
        assert np.array_equal(lr, lr_first)
        c.shrake_rupley(dx.data_ptr(), dr.data_ptr(), coils.offsets, out.data_ptr(), cnt.data_ptr())
        assert c.stats()["n_cells"] == cells
        counts = cnt.cpu().numpy()
        for k in range(8):
            sl = slice(int(coils.offsets[k]), int(coils.offsets[k + 1]))
            assert np.max(np.abs(lr[sl] - oracle_lib.lee_richards(coils.xyz[sl], coils.radii[sl], 1.4, 20))) < 1e-8
            assert np.array_equal(counts[sl], oracle_lib.shrake_rupley(coils.xyz[sl], coils.radii[sl])[1])
    finally:
        c.close()
