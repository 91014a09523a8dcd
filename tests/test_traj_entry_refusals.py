"""The argument checks of the trajectory entries with a topology, all of them: for every single defect of
tests/golden/make_traj_entry_refusals_golden.py and for every pair of defects, every entry answers what
tests/golden/traj_entry_refusals.json recorded before the entries were rewritten over one call description (gpu_drivers.hip,
TrajCall) - which refusal speaks first when two things are wrong, and its exact words.  (The per-feature suites check one defect
at a time.)  No GPU and no frame file; the structure is a dimer of 13 atoms."""
import importlib.util
import json
import os

import freesasa_amd as fa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_every_entry_refuses_single_and_paired_defects_as_recorded(tmp_path):
    spec = importlib.util.spec_from_file_location("make_traj_entry_refusals_golden", os.path.join(GOLDEN, "make_traj_entry_refusals_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(os.path.join(GOLDEN, "traj_entry_refusals.json")) as f:
        want = json.load(f)
    assert os.path.getsize(os.path.join(GOLDEN, "traj_entry_refusals.json")) < os.path.getsize(os.path.join(GOLDEN, "ingest_classifiers.json"))
    rows = [(e, tuple(c), rc, want["messages"][m]) for e, c, rc, m in want["rows"]]
    # answers at or past the device check are the machine's (no device: the device list is refused; with one: the frame file
    # that does not exist is, and the memory form runs) and compare as one class, which must stay small
    past = maker.past(rows)
    assert len(past) <= 5 and len(set(want["messages"]) - past) >= 30
    assert sum(len(c) == 2 for _, c, _, _ in rows) > 2000
    entries, defects, got = maker.table(fa._stats_proto(fa._topology_proto(fa.lib())), tmp_path)
    assert entries == want["entries"] and defects == want["defects"] and len(got) == len(rows)
    for g, w in zip(got, rows):
        assert g[:2] == w[:2]
        where = (entries[w[0]], [defects[k] for k in w[1]])
        if w[3] in past:
            assert g[2] in (0, -1) and g[3] in past and (g[2] == 0) == (g[3] == ""), (where, g, w)
        else:
            assert g == w, where
