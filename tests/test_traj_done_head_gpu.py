"""The first line of the done-list of every file entry of the trajectory drivers - the plain ones and each entry with a topology -
against tests/golden/traj_done_heads.json, recorded before the entries were rewritten over one call description
(gpu_drivers.hip, TrajCall): byte for byte, since the line decides whether a later call resumes the run.  Three frames of a
13-atom dimer, frames_per_batch = 2: one full shard and a short one; the same call again finds both done and runs none."""
import importlib.util
import json
import os

import pytest

from freesasa_amd import ingest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
spec = importlib.util.spec_from_file_location("make_traj_done_heads_golden", os.path.join(GOLDEN, "make_traj_done_heads_golden.py"))
maker = importlib.util.module_from_spec(spec)
spec.loader.exec_module(maker)
with open(os.path.join(GOLDEN, "traj_done_heads.json")) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def system(tmp_path_factory):
    b, ids = maker.dimer(tmp_path_factory.mktemp("dimer"))
    sel = ingest.Selection(["a, chain A"])
    yield b, ids, sel
    sel.close()


def test_the_fixture_covers_every_case():
    assert list(WANT) == list(maker.CASES) and len(WANT) == 13


@pytest.mark.parametrize("case", list(maker.CASES))
def test_done_list_head_is_the_recorded_one(case, system, tmp_path):
    complete, n_frames, done = maker.run_case(tmp_path, case, *system)
    assert complete and n_frames == maker.F
    with open(done, "rb") as fh:
        lines = fh.readlines()
    assert lines[0] == WANT[case].encode()
    assert sorted(lines[1:]) == [b"shard 0 0 2\n", b"shard 1 2 1\n"]
    # the same call again: the run is complete and no shard is run
    complete, n_frames, _ = maker.run_case(tmp_path, case, *system)
    assert complete and n_frames == maker.F
    with open(done, "rb") as fh:
        assert fh.readlines() == lines
