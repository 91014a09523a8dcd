"""The cell sort without a device: the numpy reference (tests/cell_sort_ref.py) and its case builders are proved here before
anything goes to a GPU.  Every case asserts that it reaches the edge it is named for; the CPU emulation of the general pipeline's
phase functions (tests/emu/emu.cpp, emu_cell_sort: the loops emu_run_batch runs) is held to the reference by the same
check_sorted that tests/test_cell_sort_gpu.py holds the device to; and check_sorted is itself checked - it accepts the outputs
the reference builds for all three arrangements, the compact table read through the Python twin of cell_first_atom included, and
refuses them with one entry changed."""
import numpy as np
import pytest

import cell_sort_ref as ref
import emu

FUSED, GENERAL = ref.cases_fused(), ref.cases_general()
EMU_CELLS = 304_000            # (the emulation scans every cell: the cases beyond are left to the device)
BEYOND_EMU = {"five passes, none in the middle one", "512x512x256: 2^26 cells", "five passes, single atoms and SORT_ATOMS in one batch",
              "off the lattice: coils, a globule, the diagonal"}


@pytest.mark.parametrize("case", FUSED + GENERAL + [ref.declined_513()], ids=repr)
def test_every_case_reaches_its_edge(case):
    case.check_claims()


def test_the_cases_left_to_the_device_are_the_large_ones():
    assert {c.name for c in FUSED + GENERAL if c.ref.C.sum() > EMU_CELLS} == BEYOND_EMU


@pytest.mark.parametrize("case", [c for c in FUSED + GENERAL if c.name not in BEYOND_EMU], ids=repr)
def test_emulated_general_pipeline_against_the_reference(case):
    out = emu.cell_sort(case.xyz, case.radii, case.offsets, case.probe, case.cap(0), case.shared)
    ref.check_sorted(out, case.xyz, case.radii, case.offsets, case.probe, 0, case.shared, ref=case.ref)


@pytest.mark.parametrize("case", FUSED + GENERAL, ids=repr)
def test_the_reference_passes_its_own_check_in_every_arrangement(case):
    """... with the structures' runs in another order than theirs for k_sort_struct's arrangements: first() read through the
    compact twin from a table the reference built equals the dense definition"""
    R = case.ref
    live = [s for s in range(R.ns) if R.offsets[s + 1] > R.offsets[s]]
    locs = [ref.check_sorted(R.expected(a, order=live[::-1] if a else None), case.xyz, case.radii, case.offsets, case.probe, a, case.shared, ref=R)
            for a in ((2,) if R.C.max() > 1 << 24 else (0, 1, 2))]
    assert all(np.array_equal(locs[0], l) for l in locs)


def refused(out, case, arrangement):
    with pytest.raises(AssertionError):
        ref.check_sorted(out, case.xyz, case.radii, case.offsets, case.probe, arrangement, case.shared, ref=case.ref)
    return True


def test_the_check_refuses_a_wrong_entry():
    """one changed entry at a time, in the outputs the reference built for a structure of 64x64x64 cells (the sentinel word)
    and for a two-pass one: what the three one-line changes to the kernels that the stage's tests must catch leave behind.

    The changes themselves, tried on copies of the sources (the first two on the device, hook-only tests; the third here):

    1. k_sort_struct without the sentinel word: in tests/test_cell_sort_gpu.py, test_shapes_of_the_one_workgroup_sort
       [SORT_ATOMS atoms, a cell each], [32 cells (4x4x2)], [32 cells (8x4x1)], [C % 32 == 0, last cell occupied], [C % 32 == 0,
       last cell empty], [8192x2x2], [2x8192x2], [64x64x64: one pass, the sentinel word], [65x64x64: two passes], [64x64x65: two
       passes], [65x64x64: the second pass holds the corner only], [five passes, none in the middle one], [512x512x256: 2^26
       cells], [600 structures of 1 to 40 atoms], [five passes, single atoms and SORT_ATOMS in one batch];
       test_shapes_of_the_general_pipeline [one structure of 4095 / 4096 / 4097 / 8193 atoms], [33 / 257 / 600 structures], [4095 /
       4096 / 4097 / 8192 / 8207 / 8208 cells], [about 3e5 cells]; test_capacity_is_exact [600 structures of 1 to 40 atoms],
       [about 3e5 cells], [five passes, single atoms and SORT_ATOMS in one batch]; all five cases of
       test_errors_of_both_implementations (the good pass behind each error): 37 tests, each at a structure whose cell count is
       a multiple of 32 under arrangement 2.
    2. occ_done not added in stage F: test_shapes_of_the_one_workgroup_sort [65x64x64: two passes], [64x64x65: two passes],
       [65x64x64: the second pass holds the corner only], [five passes, none in the middle one], [512x512x256: 2^26 cells], [five
       passes, single atoms and SORT_ATOMS in one batch], [off the lattice: coils, a globule, the diagonal]; test_capacity_is_exact
       [five passes, single atoms and SORT_ATOMS in one batch]: 8 tests, the structures of more than one pass.
    3. scan_phase3 without cell_start[n] = run: here, every case of test_emulated_general_pipeline_against_the_reference (56) and
       test_declined_by_capacity_in_the_emulation."""
    by_name = {c.name: c for c in FUSED}
    one_pass, two_pass = by_name["64x64x64: one pass, the sentinel word"], by_name["65x64x64: two passes"]
    R = one_pass.ref
    C, n = int(R.C[0]), R.n
    # the sentinel word dropped: it stays all-ones
    out = R.expected(2)
    out["cell_tbl"][C >> 5] = ref.ONES64
    assert refused(out, one_pass, 2)
    # occ_done not added in stage F: the second pass's words count from the structure's first occupied cell again
    R2 = two_pass.ref
    out = R2.expected(2)
    w0 = ref.SORT_CELLS >> 5
    occ_first_pass = int((R2.occupied(0) < ref.SORT_CELLS).sum())
    assert occ_first_pass > 0
    out["cell_tbl"][w0:(int(R2.C[0]) >> 5) + 1] -= np.uint64(occ_first_pass) << np.uint64(32)
    assert refused(out, two_pass, 2)
    # the general pipeline's sentinel entry cell_start[total] left as the histogram's zero
    out = R.expected(0)
    assert out["cell_start"][C] == n
    out["cell_start"][C] = 0
    assert refused(out, one_pass, 0)
    # ... and one atom in a neighboring cell's run, a record's flag, a radius, a density sample
    for a in (0, 1, 2):
        out = R.expected(a)
        out["s_idx"]["cell"][5] ^= 1 << 32
        assert refused(out, one_pass, a)
        out = R.expected(a)
        out["sq"][7, 3] = np.nextafter(out["sq"][7, 3], 9.0)
        assert refused(out, one_pass, a)
        out = R.expected(a)
        out["occ_sum"] += 1
        assert refused(out, one_pass, a)
        out = R.expected(a)
        out["s_idx"][[3, 200]] = out["s_idx"][[200, 3]]
        out["sq"][[3, 200]] = out["sq"][[200, 3]]
        assert refused(out, one_pass, a)


def test_declined_by_capacity_in_the_emulation():
    """the capacity reaches the phase functions (PipeArgs::cells_cap): cellbase_phase1b declines, and counts the full total"""
    case = GENERAL[0]
    total = case.ref.total(0)
    out = emu.cell_sort(case.xyz, case.radii, case.offsets, case.probe, total)
    ref.check_sorted(out, case.xyz, case.radii, case.offsets, case.probe, 0, ref=case.ref)
    out = emu.cell_sort(case.xyz, case.radii, case.offsets, case.probe, total - 1)
    assert (out["error"], out["retry"], out["cells"]) == (0, 1, total)
