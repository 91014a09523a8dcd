"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the interfaces between chain groups among
periodic images: the n-th host allocation of each of the two file entries fails, n = 1, 2, ...; every call fails with a message
or succeeds with the un-faulted bytes - nothing of a failed call is left in flight - and the call after the walk gives them
byte for byte."""
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from test_dcd import write_dcd
from test_hostfault import walk
from test_pbc_gpu import patch_cells

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("residues", [False, True])
def test_the_file_entries_survive_every_allocation_failing(tmp_path, residues):
    b = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    ids = np.repeat(np.arange(4, dtype=np.int32), 129)
    rng = np.random.default_rng(3)
    x0 = np.asarray(b.xyz, dtype=np.float64).reshape(-1, 3)
    frames = (x0[None] + rng.uniform(-0.3, 0.3, (3,) + x0.shape)).astype(np.float32)
    ext = np.ceil(x0.max(0) - x0.min(0)) + 3.0
    path = tmp_path / "frames.dcd"
    write_dcd(path, frames, cell=True)
    patch_cells(path, [tuple(float(e) for e in ext)] * 3)
    p = {k: str(tmp_path / k) for k in ("totals", "sasa", "iso", "groups", "pairs", "pres")}
    name = "freesasa_gpu_trajectory_file_interface_residues_periodic" if residues else "freesasa_gpu_trajectory_file_interfaces_periodic"
    more = dict(pair_residues_path=p["pres"], min_buried=1.0) if residues else {}
    kinds = [k for k in p if residues or k != "pres"]

    def run():
        for k in kinds:
            if os.path.exists(p[k]):
                os.remove(p[k])
        done, n_frames, _ = fa.trajectory_file_groups_periodic(path, b, p["totals"], sasa_path=p["sasa"], isolated_path=p["iso"], group=ids,
                                                               n_groups=4, group_areas_path=p["groups"], frames_per_batch=2, devices=[0], dcd=True,
                                                               interface_pairs=[(0, 1), (2, 3), (0, 3), (1, 2)], pair_areas_path=p["pairs"], **more)
        assert done and n_frames == 3
        return b"".join(open(p[k], "rb").read() for k in kinds)

    want = run()
    assert len(want) == 8 * 3 * (1 + 516 + 516 + 12 + 24) + (os.path.getsize(p["pres"]) if residues else 0)

    def call():
        try:
            got = run()
        except RuntimeError as e:
            assert str(e).startswith(name + ": ")
            return False, str(e).split(": ", 1)[1]
        assert got == want
        return True, ""

    fired, failed = walk(call)
    assert run() == want
    # the duplicate check's keys, the groups' cut, the pairs' cut (three vectors), the run's offsets, the lanes, the periodic stage's
    # vectors, the engine's own
    assert fired >= 8 and failed >= 8, (fired, failed)
    fa.lib().freesasa_gpu_release_pool()
