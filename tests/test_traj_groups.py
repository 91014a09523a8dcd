"""Chain groups in the trajectory drivers (freesasa_gpu_trajectory_groups / _trajectory_file_groups, include/freesasa_gpu.h)
without a GPU: the host cut and the traj_group_* phase functions of csrc/traj_kernels.h driven on the CPU
(tests/emu/emu_traj_groups.cpp) against the chain-group entry's own phase functions (group_kernels.h) on every frame as a batch
of its own, with == ; and the argument checks, which the library makes before it touches a device or a file."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from emu import groups_emu, traj_groups_emu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
NF = 5


@pytest.fixture(scope="module")
def jo4():
    """2jo4: chains A, B, C, D of 129 atoms; "AC+B": group 0 in two runs, group 1 between them, D in no group - the ids as the
    device's ids kernel makes them (its emulation), which are the host's"""
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    assert b.n_atoms == 516
    ids, ng, st = groups_emu.run(b, "AC+B")
    host_ids, host_ng, host_st = b.chain_groups("AC+B")
    assert np.array_equal(ids, host_ids) and ng[0] == host_ng[0] == 2 and st[0] == host_st[0] == 0
    assert np.array_equal(ids, np.repeat(np.array([0, 1, 0, -1], np.int32), 129))
    return b, ids


def variants(ids):
    """(name, ids, G): the fixture's own cut, the same with an empty third group, and with a one-atom group"""
    one = ids.copy()
    one[300] = 2                                       # an atom of chain C alone in group 2, inside group 0's second run
    return [("AC+B", ids, 2), ("empty group", ids, 3), ("one-atom group", one, 3)]


def seeded(n, n_iso, seed):
    rng = np.random.default_rng(seed)
    frames = rng.normal(0, 20, (NF, n, 3))
    csasa = rng.uniform(0.0, 60.0, NF * (n + n_iso)) * (rng.random(NF * (n + n_iso)) > 0.3)
    return frames, csasa


@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_cut_is_the_rank_kernels_order(jo4, which):
    b, ids0 = jo4
    name, ids, G = variants(ids0)[which]
    gfirst, src = traj_groups_emu.cut(ids, G)
    counts = np.bincount(ids[ids >= 0], minlength=G)
    assert np.array_equal(gfirst, np.concatenate([[0], np.cumsum(counts)]))
    want = np.concatenate([np.nonzero(ids == g)[0] for g in range(G)])          # group-major, input order within a group
    assert np.array_equal(src, want)
    rank_src, cxyz, cradii = traj_groups_emu.groups_one(b.xyz, b.radii, ids, G)
    assert np.array_equal(src, rank_src), name
    assert np.array_equal(cxyz[516:], b.xyz[src]) and np.array_equal(cradii[516:], b.radii[src])
    if which == 1:
        assert gfirst[2] == gfirst[3] == src.size
    if which == 2:
        assert gfirst[3] - gfirst[2] == 1 and src[-1] == 300


def test_a_bad_id_names_its_atom(jo4):
    _, ids = jo4
    for at, bad in ((17, -2), (400, 2)):
        g = ids.copy()
        g[at] = bad
        with pytest.raises(ValueError, match="atom %d " % at):
            traj_groups_emu.cut(g, 2)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_shard_equals_the_group_kernels_on_every_frame(jo4, which):
    b, ids0 = jo4
    name, ids, G = variants(ids0)[which]
    n = b.n_atoms
    _, src = traj_groups_emu.cut(ids, G)
    n_iso = src.size
    frames, csasa = seeded(n, n_iso, 20261018 + which)
    xyz, cradii, iso, totals, areas = traj_groups_emu.shard(ids, G, b.radii, frames, csasa)
    # the gather and the radii: exact indexed copies, the frames in front untouched
    assert np.array_equal(xyz[:NF * n].reshape(NF, n, 3), frames)
    assert np.array_equal(xyz[NF * n:].reshape(NF, n_iso, 3), frames[:, src])
    assert np.array_equal(cradii[:NF * n].reshape(NF, n), np.tile(b.radii, (NF, 1)))
    assert np.array_equal(cradii[NF * n:].reshape(NF, n_iso), np.tile(b.radii[src], (NF, 1)))
    # finish and totals: frame f as a batch of its own through grp_count / grp_rank / grp_finish / the totals kernels / grp_totals
    for f in range(NF):
        c_f = np.concatenate([csasa[f * n:(f + 1) * n], csasa[NF * n + f * n_iso:NF * n + (f + 1) * n_iso]])
        sasa, want_iso, want_total, want_gt = traj_groups_emu.groups_one(frames[f], b.radii, ids, G, c_f)
        assert np.array_equal(sasa, csasa[f * n:(f + 1) * n])
        assert np.array_equal(iso[f], want_iso), (name, f)
        assert totals[f] == want_total, (name, f)
        assert np.array_equal(areas[f], want_gt), (name, f)
        assert np.array_equal(iso[f][ids < 0], sasa[ids < 0])
    assert np.all(areas[:, :, 2] == areas[:, :, 0] - areas[:, :, 1])
    if which == 1:
        assert np.all(areas[:, 2] == 0)
    # without the isolated per-atom output the sums are the same
    _, _, none, totals2, areas2 = traj_groups_emu.shard(ids, G, b.radii, frames, csasa, want_iso=False)
    assert none is None and np.array_equal(totals2, totals) and np.array_equal(areas2, areas)


# ------------------------------------------------------------------------------------------------ the argument checks

def _bad_group_calls(ids):
    low, high = ids.copy(), ids.copy()
    low[7] = -2
    high[409] = 2
    return [
        ("id < -1", dict(group=low, n_groups=2, areas=True), ("atom 7 ", "group id -2")),
        ("id >= n_groups", dict(group=high, n_groups=2, areas=True), ("atom 409 ", "group id 2")),
        ("n_groups 0", dict(group=ids, n_groups=0, areas=True), ("n_groups must be",)),
        ("n_groups 65536", dict(group=ids, n_groups=65536, areas=True), ("n_groups must be",)),
        ("no group areas", dict(group=ids, n_groups=2, areas=False), ("group ids are given",)),
        ("group areas without ids", dict(group=None, n_groups=2, areas=True), ("need group ids",)),
    ]


def test_argument_errors_come_before_any_device_or_file(jo4, tmp_path):
    b, ids = jo4
    n = b.n_atoms
    L = fa._topology_proto(fa.lib())
    cb = b._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp, i32 = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    frames_path = tmp_path / "frames.f64"
    np.zeros((2, n, 3)).tofile(frames_path)
    enc = lambda p: str(p).encode()
    for what, kw, texts in _bad_group_calls(ids):
        g = kw["group"]
        pg = None if g is None else g.ctypes.data_as(i32)
        outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "groups", "iso")] + [tmp_path / "done.txt"]
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_groups(enc(frames_path), 0, 0, 0, C.byref(cb), 0, n, None, None, pg, kw["n_groups"],
                                                   fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), None, None, None, None,
                                                   enc(outs[2]) if kw["areas"] else None, enc(outs[3]) if g is not None else None,
                                                   enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
        assert rc == -1 and all(t in err.value.decode() for t in texts), (what, err.value)
        assert not any(p.exists() for p in outs), what
        frames, totals, areas = np.zeros((2, n, 3)), np.zeros(2), np.zeros((2, 3, 3))
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_groups(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, n, None, None, pg, kw["n_groups"],
                                              fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                              areas.ctypes.data_as(dp) if kw["areas"] else None, None,
                                              devs.ctypes.data_as(ip), 1, err, 512)
        assert rc == -1 and all(t in err.value.decode() for t in texts), (what, err.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["frames.f64"]
    # the isolated areas alone need ids too, and the topology's own checks still come first
    iso = np.zeros((2, n))
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_groups(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, n, None, None, None, 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                          totals.ctypes.data_as(dp), None, None, None, None, None, None, iso.ctypes.data_as(dp),
                                          devs.ctypes.data_as(ip), 1, err, 512)
    assert rc == -1 and "need group ids" in err.value.decode()
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_groups(frames.ctypes.data_as(dp), 2, C.byref(cb), 3, n, None, None, ids.ctypes.data_as(i32), 2,
                                          fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                          areas.ctypes.data_as(dp), None, devs.ctypes.data_as(ip), 1, err, 512)
    assert rc == -1 and "structure out of range" in err.value.decode()


def test_python_refuses_inconsistent_group_keywords(jo4):
    b, ids = jo4
    frames = np.zeros((2, b.n_atoms, 3))
    with pytest.raises(ValueError, match="not both"):
        fa.trajectory_topology(frames, b, chain_groups="AC+B", group=ids, n_groups=2)
    with pytest.raises(ValueError, match="n_groups"):
        fa.trajectory_topology(frames, b, group=ids)
    with pytest.raises(ValueError, match="one id per atom"):
        fa.trajectory_topology(frames, b, group=ids[:-1], n_groups=2)
    with pytest.raises(ValueError, match="EGROUP"):
        fa.trajectory_topology(frames, b, chain_groups="AZ+B")          # no chain Z in 2jo4
    with pytest.raises(ValueError):
        fa.trajectory_topology(frames, b, chain_groups="A+A")           # overlapping groups: Batch.chain_groups's error


def test_the_old_entries_are_what_they_were(jo4, tmp_path):
    """The entries without groups keep their signatures and their checks; the Python keywords default to "no groups"."""
    b, ids = jo4
    n = b.n_atoms
    L = fa._topology_proto(fa.lib())
    for f in (fa.trajectory_topology, fa.trajectory_file_topology):
        p = inspect.signature(f).parameters
        assert [p[k].default for k in ("chain_groups", "separate_chains", "long", "group", "n_groups")] == [None, False, False, None, None]
    assert inspect.signature(fa.trajectory_file_topology).parameters["group_areas_path"].default is None
    assert inspect.signature(fa.trajectory_file_topology).parameters["isolated_path"].default is None
    r = fa.TopologyResult(1, 2, 3, 4, 5, 6, 7)
    assert (r.totals, r.res_ref, r.group_areas, r.group_atoms, r.isolated) == (1, 7, None, None, None)
    cb = b._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    twice = np.arange(n, dtype=np.int32)
    twice[9] = twice[8]
    frames, totals = np.zeros((2, n + 3, 3)), np.zeros(2)
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_topology(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, n + 3, twice.ctypes.data_as(C.POINTER(C.c_int32)), None,
                                            fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                            devs.ctypes.data_as(ip), 1, err, 512)
    assert rc == -1 and "twice" in err.value.decode()
    out = tmp_path / "totals.bin"
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_file_topology(str(tmp_path / "none.f64").encode(), 0, 0, 0, C.byref(cb), 0, n + 3,
                                                 twice.ctypes.data_as(C.POINTER(C.c_int32)), None, fa.LEE_RICHARDS, 1.4, 20, 0,
                                                 str(out).encode(), None, None, None, None, None, None, 0, devs.ctypes.data_as(ip), 1,
                                                 None, err, 512)
    assert rc == -1 and "twice" in err.value.decode() and not out.exists()
