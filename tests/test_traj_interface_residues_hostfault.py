"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the per-residue interface tables per frame
of a trajectory: the n-th host allocation of the memory entry, of the file entry and of the segments entry fails, n = 1, 2, ...;
every call fails with -1 and a message or succeeds with the un-faulted bytes - nothing of a failed call is left in flight - and
the call after the walk gives them bit for bit."""
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from test_hostfault import walk

PAIRS = [(0, 1), (2, 3), (0, 3), (1, 2)]
PREFIXES = ("freesasa_gpu_trajectory_interface_residues: ", "freesasa_gpu_trajectory_file_interface_residues: ",
            "freesasa_gpu_trajectory_interface_segments: ")


def system():
    b = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    ids = np.repeat(np.arange(4, dtype=np.int32), 129)
    rng = np.random.default_rng(3)
    return b, ids, b.xyz[None] + rng.uniform(-0.3, 0.3, (3,) + b.xyz.shape)


def walked(run):
    want = run()

    def call():
        try:
            got = run()
        except RuntimeError as e:
            assert str(e).startswith(PREFIXES), str(e)
            return False, str(e).split(": ", 1)[1]
        assert got == want
        return True, ""

    fired, failed = walk(call)
    assert run() == want
    return fired, failed


def test_the_segments_entry_survives_every_allocation_failing():
    """no device is needed: the topology's residues, the groups' cut, the pairs' cut and the segments are host vectors"""
    b, ids, _ = system()

    def run():
        return b"".join(a.tobytes() for a in fa.traj_pair_segments(b, ids, 4, PAIRS))

    fired, failed = walked(run)
    # (two calls a run - the count, then the arrays - each with the duplicate check's keys, the residues, the two cuts, the segments)
    assert fired >= 8 and failed >= 8, (fired, failed)


@pytest.mark.gpu
def test_the_memory_entry_survives_every_allocation_failing():
    b, ids, frames = system()

    def run():
        r = fa.trajectory_topology(frames, b, per_atom=True, frames_per_batch=2, devices=[0], group=ids, n_groups=4,
                                   interface_pairs=PAIRS, interface_residues=True, min_buried=0.5, stats=("pairs", "pair_residues"))
        return b"".join(np.ascontiguousarray(a).tobytes() for a in (r.totals, r.sasa, r.isolated, r.group_areas, r.pair_areas, r.pair_residues,
                                                                    r.stats.raw, r.stats.partials))

    fired, failed = walked(run)
    assert fired >= 12 and failed >= 12, (fired, failed)
    fa.lib().freesasa_gpu_release_pool()


@pytest.mark.gpu
def test_the_file_entry_survives_every_allocation_failing(tmp_path):
    b, ids, frames = system()
    path = tmp_path / "frames.f64"
    frames.tofile(path)
    p = {k: str(tmp_path / k) for k in ("totals", "pairs", "pres", "stats", "parts")}

    def run():
        for k in p:
            if os.path.exists(p[k]):
                os.unlink(p[k])
        done, n_frames, _ = fa.trajectory_file_topology(path, b, p["totals"], frames_per_batch=2, devices=[0], group=ids, n_groups=4,
                                                        interface_pairs=PAIRS, pair_areas_path=p["pairs"], pair_residues_path=p["pres"],
                                                        min_buried=0.5, stats=("pair_residues",), stats_path=p["stats"], partials_path=p["parts"])
        assert done and n_frames == 3
        return b"".join(open(p[k], "rb").read() for k in p)

    fired, failed = walked(run)
    assert fired >= 8 and failed >= 8, (fired, failed)
    fa.lib().freesasa_gpu_release_pool()
