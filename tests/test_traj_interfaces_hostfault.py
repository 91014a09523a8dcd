"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the interfaces between chain groups in
the trajectory drivers: the n-th host allocation of the memory entry fails, n = 1, 2, ...; every call fails with -1 and a message
or succeeds with the un-faulted bytes - nothing of a failed call is left in flight - and the call after the walk gives them bit
for bit."""
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from test_hostfault import walk

pytestmark = pytest.mark.gpu


def test_the_memory_entry_survives_every_allocation_failing():
    b = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    ids = np.repeat(np.arange(4, dtype=np.int32), 129)
    rng = np.random.default_rng(3)
    frames = b.xyz[None] + rng.uniform(-0.3, 0.3, (3,) + b.xyz.shape)

    def run():
        r = fa.trajectory_topology(frames, b, per_atom=True, frames_per_batch=2, devices=[0], group=ids, n_groups=4,
                                   interface_pairs=[(0, 1), (2, 3), (0, 3), (1, 2)])
        return b"".join(np.ascontiguousarray(a).tobytes() for a in (r.totals, r.sasa, r.isolated, r.group_areas, r.pair_areas))

    want = run()

    def call():
        try:
            got = run()
        except RuntimeError as e:
            assert str(e).startswith("freesasa_gpu_trajectory_interfaces: ")
            return False, str(e).split(": ", 1)[1]
        assert got == want
        return True, ""

    fired, failed = walk(call)
    assert run() == want
    # the duplicate check's keys, the groups' cut, the pairs' cut (three vectors), the run's offsets, the lanes, the engine's own
    assert fired >= 8 and failed >= 8, (fired, failed)
    fa.lib().freesasa_gpu_release_pool()
