"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the residue-residue contact tables of the
interfaces: the n-th host allocation of calc_interface_contacts(..., res_first=...) (freesasa_gpu_calc_interface_pairs, then
freesasa_gpu_calc_interface_contacts for the counts, then freesasa_gpu_calc_interface_residue_contacts for the arrays) fails,
n = 1, 2, ...; every call fails with a message or succeeds with the un-faulted bytes, and the call after the walk gives them bit
for bit."""
import numpy as np
import pytest

import freesasa_amd as fa
import interface_residue_contacts_ref as qr
from test_hostfault import walk

pytestmark = pytest.mark.gpu


def _bytes(got):
    return b"".join(a.tobytes() for a in (got.sasa, got.iso, got.totals, got.group_totals, got.pair_struct, got.pair_groups, got.pair_areas,
                                          got.side_offsets, got.pair_atom, got.pair_buried, got.contact_first, got.contact_partner,
                                          got.contact_points, got.contact_area, got.buried_masks, got.rescontact_offsets,
                                          got.rescontact_residues, got.rescontact_counts, got.rescontact_area, got.rescontact_reverse))


def test_calc_interface_contacts_with_residues_survives_every_allocation_failing():
    b = qr.rescontacts_batch()
    xyz, radii, offsets, group, n_groups = (np.array(a) for a in b[:5])
    res_first = np.array(b[6])
    first = fa.calc_interface_contacts(xyz, radii, offsets, group, n_groups, n_points=33, res_first=res_first)
    want = _bytes(first)
    assert first.n_rescontacts == len(qr.batch_fold(33)["rescontact_area"]) > 0

    def call():
        try:
            got = fa.calc_interface_contacts(xyz, radii, offsets, group, n_groups, n_points=33, res_first=res_first)
        except RuntimeError as e:
            return False, str(e).split(": ", 1)[1]
        assert _bytes(got) == want
        return True, ""

    fired, failed = walk(call)
    assert fired >= 5 and failed >= 5, (fired, failed)
    assert _bytes(fa.calc_interface_contacts(xyz, radii, offsets, group, n_groups, n_points=33, res_first=res_first)) == want
