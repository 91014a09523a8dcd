"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the per-residue interface tables: the
n-th host allocation of calc_interfaces(..., res_first=...) (freesasa_gpu_calc_interface_pairs,
freesasa_gpu_calc_interface_residues) fails, n = 1, 2, ...; every call fails with a message or succeeds with the un-faulted
bytes, the call after the walk gives them bit for bit, and the walk is longer than the one without residues by the stage's own
allocation (its copy of the residue boundaries).

walk() steps by one up to n = 48 and by n // 6 beyond, and calc_interfaces makes 77 (L&R) / 80 (S&R) allocations without
residues and 78 / 81 with them (measured on the MI355X): walk() fires 51 times either way, because both counts lie between its
steps 75 and 87, and cannot tell them apart.  So "one more with residues" is held on a walk of this file that steps by one all
the way (every_allocation) - the same hook, the same bar per call - next to walk() itself."""
import numpy as np
import pytest

import freesasa_amd as fa
import interface_residues_ref as rr
from test_hostfault import walk

pytestmark = pytest.mark.gpu


def every_allocation(call, limit=1000):
    """walk() with a step of one throughout: (faults that fired, calls that failed) are then the allocations the call makes and
    how many of them it cannot do without"""
    fired = failed = 0
    for n in range(1, limit + 1):
        fa.host_test_fail_after(n)
        try:
            ok, msg = call()
        finally:
            left = fa.host_test_fail_after(0)
        if left > 0:
            assert ok, msg
            return fired, failed
        fired += 1
        if not ok:
            failed += 1
            assert msg, f"failure without a message at n = {n}"
    raise AssertionError("the walk did not end")


def _bytes(got, residues):
    arrays = [got.sasa, got.iso, got.totals, got.group_totals, got.pair_struct, got.pair_groups, got.pair_areas, got.side_offsets, got.pair_atom,
              got.pair_buried]
    if residues:
        arrays += [got.res_offsets, got.res_index, got.res_atoms, got.res_areas]
    return b"".join(a.tobytes() for a in arrays)


@pytest.mark.parametrize("alg", [fa.LEE_RICHARDS, fa.SHRAKE_RUPLEY])
def test_calc_interfaces_with_residues_survives_every_allocation_failing(alg):
    b = rr.residue_edge_batch()
    xyz, radii, offsets, group, n_groups = (np.array(a) for a in b[:5])
    res_first = np.array(b[6])
    kw = dict(alg=alg, resolution=20 if alg == fa.LEE_RICHARDS else 100, per_atom=True)
    counts = {}
    for residues in (False, True):
        kw_r = dict(kw, res_first=res_first) if residues else kw
        want = _bytes(fa.calc_interfaces(xyz, radii, offsets, group, n_groups, **kw_r), residues)

        def call():
            try:
                got = fa.calc_interfaces(xyz, radii, offsets, group, n_groups, **kw_r)
            except RuntimeError as e:
                return False, str(e).split(": ", 1)[1]
            assert _bytes(got, residues) == want
            return True, ""

        fired, failed = walk(call)
        assert fired >= 5 and failed >= 5, (fired, failed)
        assert _bytes(fa.calc_interfaces(xyz, radii, offsets, group, n_groups, **kw_r), residues) == want
        counts[residues] = every_allocation(call)
        assert _bytes(fa.calc_interfaces(xyz, radii, offsets, group, n_groups, **kw_r), residues) == want
    (fired0, failed0), (fired1, failed1) = counts[False], counts[True]
    assert fired0 >= 5 and failed0 >= 5, counts
    assert fired1 >= fired0 + 1 and failed1 >= failed0 + 1, counts
