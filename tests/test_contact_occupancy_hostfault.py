"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the residue contact occupancy map: the
n-th host allocation of an accumulator's life - freesasa_gpu_contact_occupancy_open, _add_frames in two calls, _add_rows, _table -
fails, n = 1, 2, ...; every life fails with a message or ends with the un-faulted bytes, and the life after the walk gives them
bit for bit."""
import numpy as np
import pytest

import contact_occupancy_ref as occ
import freesasa_amd as fa
from test_hostfault import walk

pytestmark = pytest.mark.gpu


def _bytes(t):
    return b"".join(getattr(t, k).tobytes() for k in occ.COLUMNS) + str(t.n_frames).encode()


def _life():
    radii, group, n_groups, res_first = occ.traj_system()
    xyz = np.array(occ.traj_frames())
    extra = occ.row_arrays(occ.lists_frames()[2:5])
    with fa.ContactOccupancy(np.array(radii), np.array(group), n_groups, np.array(res_first), n_points=33, frames_per_batch=5) as acc:
        counts = [acc.add(xyz[:4]), acc.add(xyz[4:])]
        acc.add_rows(*extra)
        return _bytes(acc.table()) + np.concatenate(counts).tobytes()


def test_an_accumulator_survives_every_allocation_failing():
    want = _life()
    assert len(want) > 1000

    def call():
        try:
            got = _life()
        except RuntimeError as e:
            return False, str(e).split(": ", 1)[1]
        assert got == want
        return True, ""

    fired, failed = walk(call)
    assert fired >= 5 and failed >= 5, (fired, failed)
    assert _life() == want
