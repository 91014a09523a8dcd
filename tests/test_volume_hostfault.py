"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the volume entries: the n-th host
allocation or thread creation of freesasa_gpu_calc_volume and freesasa_gpu_trajectory_volume fails, n = 1, 2, ...; every call
fails with a message or succeeds with the un-faulted numbers, and the call after the walk gives them bit for bit."""
import numpy as np
import pytest

import freesasa_amd as fa
import volume_ref as vr
from test_hostfault import walk
from test_volume_gpu import system  # noqa: F401 (the trajectory tests' topology and frames)

pytestmark = pytest.mark.gpu


def test_calc_volume_survives_every_allocation_failing():
    xyz, radii, offsets = vr.batch()
    want = fa.calc_volume(xyz, radii, offsets, n_points=100, per_atom=True)

    def call():
        try:
            got = fa.calc_volume(xyz, radii, offsets, n_points=100, per_atom=True)
        except RuntimeError as e:
            return False, str(e)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        return True, ""

    fired, failed = walk(call)
    assert fired >= 1 and failed >= 1, (fired, failed)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fa.calc_volume(xyz, radii, offsets, n_points=100, per_atom=True), want))


def test_trajectory_volume_survives_every_allocation_failing(system):
    one, full32, index, _ = system
    frames = full32.astype(np.float64)
    kw = dict(atom_index=index, alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=3, devices=[0, 0], volumes=True)
    want = fa.trajectory_topology(frames, one, **kw)

    def call():
        try:
            got = fa.trajectory_topology(frames, one, **kw)
        except RuntimeError as e:
            return False, str(e)
        assert got.volumes.tobytes() == want.volumes.tobytes() and got.totals.tobytes() == want.totals.tobytes()
        return True, ""

    fired, failed = walk(call)
    assert fired >= 3 and failed >= 3, (fired, failed)
    assert fa.trajectory_topology(frames, one, **kw).volumes.tobytes() == want.volumes.tobytes()
