"""Interfaces between chain groups in the trajectory drivers (freesasa_gpu_trajectory_interfaces / _trajectory_file_interfaces,
include/freesasa_gpu.h) without a GPU: the host cut of the pair structures and the traj_pair_* phase functions of
csrc/traj_kernels.h driven on the CPU behind the groups' (tests/emu/emu_traj_pairs.cpp) against a numpy restatement
(tests/traj_interfaces_ref.py) with == ; the restatement of the totals kernel's order against that kernel's phase functions; and
the argument checks, which the library makes before it touches a device or a file."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import interfaces_ref as ir
import traj_interfaces_ref as tr
from freesasa_amd import ingest
from emu import traj_groups_emu, traj_pairs_emu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
NF = 5


@pytest.fixture(scope="module")
def jo4():
    """2jo4: chains A, B, C, D of 129 atoms; "AC+B": group 0 in two runs, group 1 between them, D in no group"""
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    assert b.n_atoms == 516
    ids, ng, st = b.chain_groups("AC+B")
    assert ng[0] == 2 and st[0] == 0 and np.array_equal(ids, np.repeat(np.array([0, 1, 0, -1], np.int32), 129))
    return b, ids


def variants(ids):
    """(name, ids, G) of tests/test_traj_groups.py: the fixture's own cut, the same with an empty third group, and with a one-atom
    group inside group 0's second run"""
    one = ids.copy()
    one[300] = 2
    return [("AC+B", ids, 2), ("empty group", ids, 3), ("one-atom group", one, 3)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_cut_is_the_members_of_g_then_h(jo4, which):
    _, ids0 = jo4
    name, ids, G = variants(ids0)[which]
    pairs = tr.all_pairs(G)
    assert len(pairs) == G * (G - 1) // 2
    pfirst, pside, psrc = traj_pairs_emu.cut(ids, G, pairs)
    want_first, want_src = tr.cut(ids, pairs)
    assert np.array_equal(pfirst, want_first) and np.array_equal(psrc, want_src), name
    offsets = np.array([0, ids.size])
    for k, (g, h) in enumerate(pairs):
        mg, mh = ir.members(offsets, ids, 0, g), ir.members(offsets, ids, 0, h)
        assert pside[2 * k] == pfirst[k] and pside[2 * k + 1] == pfirst[k] + len(mg), (name, k)
        assert np.array_equal(psrc[pfirst[k]:pfirst[k + 1]], np.concatenate([mg, mh])), (name, k)
    assert pside[-1] == pfirst[-1] == psrc.size
    if which == 1:      # (0, 1), (0, 2), (1, 2): the empty group's sides hold nothing
        assert np.array_equal(np.diff(pfirst), [387, 258, 129])
    if which == 2:
        assert np.array_equal(np.diff(pfirst), [386, 258, 130]) and psrc[pfirst[2] - 1] == 300 == psrc[-1]


def seeded(n, extra, seed):
    rng = np.random.default_rng(seed)
    frames = rng.normal(0, 20, (NF, n, 3))
    csasa = rng.uniform(0.0, 60.0, NF * (n + extra)) * (rng.random(NF * (n + extra)) > 0.3)
    return frames, csasa


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_shard_through_the_phase_functions(jo4, which):
    b, ids0 = jo4
    name, ids, G = variants(ids0)[which]
    n = b.n_atoms
    pairs = tr.all_pairs(G)
    K = len(pairs)
    _, src = traj_groups_emu.cut(ids, G)
    pfirst, pside, psrc = traj_pairs_emu.cut(ids, G, pairs)
    n_iso, n_pair = src.size, psrc.size
    frames, csasa = seeded(n, n_iso + n_pair, 20261021 + which)
    xyz, cradii, iso, totals, gout, pout, side_off = traj_pairs_emu.shard(ids, G, pairs, b.radii, frames, csasa)
    ng = NF * (n + n_iso)                                   # the groups' part of the combined batch
    # the gather and the radii: exact indexed copies of every frame
    assert np.array_equal(xyz[ng:].reshape(NF, n_pair, 3), frames[:, psrc])
    assert np.array_equal(cradii[ng:].reshape(NF, n_pair), np.tile(b.radii[psrc], (NF, 1)))
    # the sides' boundaries
    want_off = np.concatenate([ng + f * n_pair + pside[:-1] for f in range(NF)] + [[ng + NF * n_pair]])
    assert np.array_equal(side_off, want_off)
    # the groups' part of every array is what the groups' run has there
    g_xyz, g_cradii, g_iso, g_totals, g_areas = traj_groups_emu.shard(ids, G, b.radii, frames, csasa[:ng])
    assert xyz[:ng].tobytes() == g_xyz.tobytes() and cradii[:ng].tobytes() == g_cradii.tobytes()
    assert iso.tobytes() == g_iso.tobytes() and totals.tobytes() == g_totals.tobytes() and gout.tobytes() == g_areas.tobytes()
    # the six columns: the restatement on every frame
    for f in range(NF):
        want = tr.frame_rows(ids, pairs, gout[f, :, 0], csasa[ng + f * n_pair:ng + (f + 1) * n_pair])
        assert np.array_equal(pout[f], want), (name, f)
    assert np.all(pout[:, :, 4] == pout[:, :, 0] - pout[:, :, 2]) and np.all(pout[:, :, 5] == pout[:, :, 1] - pout[:, :, 3])
    for k, (g, h) in enumerate(pairs):
        assert np.array_equal(pout[:, k, 0], gout[:, g, 0]) and np.array_equal(pout[:, k, 1], gout[:, h, 0])
    if which == 1:                                          # the empty group is side h of pairs 1 and 2
        assert np.all(pout[:, 1:, 1::2] == 0) and np.all(pout[:, 0] != 0)
    # without the isolated per-atom output the rows are the same
    _, _, none, _, gout2, pout2, _ = traj_pairs_emu.shard(ids, G, pairs, b.radii, frames, csasa, want_iso=False)
    assert none is None and np.array_equal(gout2, gout) and np.array_equal(pout2, pout)


def test_a_subset_of_the_pairs_in_another_order_gives_their_rows(jo4):
    """a row depends on its frame and its pair, not on the other pairs of the run"""
    b, ids0 = jo4
    ids = np.repeat(np.arange(4, dtype=np.int32), 129)
    n = b.n_atoms
    every = tr.all_pairs(4)
    pick = np.array([[2, 3], [0, 2]], np.int32)
    rng = np.random.default_rng(3)
    frames = rng.normal(0, 20, (NF, n, 3))
    base = rng.uniform(0.0, 60.0, NF * 2 * n)               # the frames and the isolated groups
    areas = {(g, h): rng.uniform(0.0, 60.0, (NF, 258)) for g, h in every}
    def run(pairs):
        tail = np.concatenate([areas[(g, h)][f] for f in range(NF) for g, h in pairs])
        return traj_pairs_emu.shard(ids, 4, pairs, b.radii, frames, np.concatenate([base, tail]))[5]
    full, part = run(every), run(pick)
    assert np.array_equal(part[:, 0], full[:, 5]) and np.array_equal(part[:, 1], full[:, 1])


def test_the_restated_sum_order_is_the_totals_kernels():
    B = traj_pairs_emu.tot_b()
    assert B == tr.TOT_B
    rng = np.random.default_rng(20261021)
    differs = 0
    for n in (0, 1, B - 1, B, B + 1, 4 * B + 3):
        v = rng.uniform(0.0, 60.0, n) * (rng.random(n) > 0.3)
        got, want = traj_pairs_emu.k_totals(v), tr.k_totals_sum(v)
        assert got == want, n
        seq = 0.0
        for x in v:
            seq += float(x)
        differs += seq != want
    assert tr.k_totals_sum([]) == 0.0 and tr.k_totals_sum([3.5]) == 3.5
    assert differs >= 1     # the order matters at these sizes: the check above is not one of sums that agree in any order


# ------------------------------------------------------------------------------------------------ the argument checks

def _bad_pair_calls(ids):
    i32 = lambda a: np.array(a, np.int32).reshape(-1, 2)
    ok = i32([(0, 1)])
    return [
        ("group NULL", dict(group=None, pairs=ok, K=1), ("need chain groups", "group is NULL")),
        ("n_pairs 0", dict(group=ids, pairs=ok, K=0), ("n_pairs < 1",)),
        ("n_pairs -3", dict(group=ids, pairs=ok, K=-3), ("n_pairs < 1",)),
        ("g == h", dict(group=ids, pairs=i32([(0, 1), (1, 1)]), K=2), ("pair 1 is (1, 1)",)),
        ("g > h", dict(group=ids, pairs=i32([(1, 0)]), K=1), ("pair 0 is (1, 0)",)),
        ("id >= G", dict(group=ids, pairs=i32([(0, 1), (0, 2)]), K=2), ("pair 1 is (0, 2)", "n_groups = 2")),
        ("id < 0", dict(group=ids, pairs=i32([(-1, 1)]), K=1), ("pair 0 is (-1, 1)",)),
        ("twice", dict(group=ids, pairs=i32([(0, 2), (1, 2), (0, 1), (1, 2)]), K=4, G=3), ("pairs 1 and 3", "(1, 2)", "at most once")),
    ]


def _interfaces_protos():
    return fa._stats_proto(fa._topology_proto(fa.lib()))


def test_argument_errors_come_before_any_device_or_file(jo4, tmp_path):
    b, ids = jo4
    n = b.n_atoms
    L = _interfaces_protos()
    cb = b._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp, i32 = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    frames_path = tmp_path / "frames.f64"
    np.zeros((2, n, 3)).tofile(frames_path)
    enc = lambda p: str(p).encode()
    frames, totals, areas, pair_areas = np.zeros((2, n, 3)), np.zeros(2), np.zeros((2, 3, 3)), np.zeros((2, 4, 6))
    outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "groups", "iso", "pairs")] + [tmp_path / "done.txt"]

    def file_call(group, G, pairs, K, bits=0, pair_path=outs[4]):
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_interfaces(enc(frames_path), bits, 0, 0, C.byref(cb), 0, n, None, None,
                                                       None if group is None else group.ctypes.data_as(i32), G,
                                                       fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), None, None, None, None,
                                                       enc(outs[2]), enc(outs[3]), enc(outs[5]), 0, devs.ctypes.data_as(ip), 1, None,
                                                       0, None, None, None if pairs is None else pairs.ctypes.data_as(i32), K,
                                                       None if pair_path is None else enc(pair_path), err, 512)
        assert not any(p.exists() for p in outs)
        return rc, err.value.decode()

    def mem_call(group, G, pairs, K, out=pair_areas):
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_interfaces(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, n, None, None,
                                                  None if group is None else group.ctypes.data_as(i32), G,
                                                  fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                                  areas.ctypes.data_as(dp), None, devs.ctypes.data_as(ip), 1, 0, None, None,
                                                  None if pairs is None else pairs.ctypes.data_as(i32), K,
                                                  None if out is None else out.ctypes.data_as(dp), err, 512)
        return rc, err.value.decode()

    for what, kw, texts in _bad_pair_calls(ids):
        for call in (file_call, mem_call):
            rc, msg = call(kw["group"], kw.get("G", 2), kw["pairs"], kw["K"])
            assert rc == -1 and all(t in msg for t in texts), (what, call.__name__, msg)
    ok = np.array([[0, 1]], np.int32)
    for call in (file_call, mem_call):
        rc, msg = call(ids, 2, None, 1)
        assert rc == -1 and "null argument: the pairs" in msg
        rc, msg = call(ids, 2, ok, 1, **({"pair_path": None} if call is file_call else {"out": None}))
        assert rc == -1 and "nowhere to go" in msg
    # periodic images: bit 3, and bit 4 with it
    for bits in (fa.FRAMES_DCD | fa.FRAMES_PBC, fa.FRAMES_DCD | fa.FRAMES_PBC | fa.FRAMES_TRICLINIC):
        rc, msg = file_call(ids, 2, ok, 1, bits=bits)
        assert rc == -1 and "interfaces among periodic images are not offered" in msg
    # the groups' and the topology's own checks still hold behind the pairs'
    bad = ids.copy()
    bad[7] = -2
    rc, msg = mem_call(bad, 2, ok, 1)
    assert rc == -1 and "atom 7 " in msg and "group id -2" in msg
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_interfaces(frames.ctypes.data_as(dp), 2, C.byref(cb), 3, n, None, None, ids.ctypes.data_as(i32), 2,
                                              fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                              None, None, devs.ctypes.data_as(ip), 1, 0, None, None, ok.ctypes.data_as(i32), 1,
                                              pair_areas.ctypes.data_as(dp), err, 512)
    assert rc == -1 and "structure out of range" in err.value.decode()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["frames.f64"]


def test_python_keywords(jo4, tmp_path):
    b, ids = jo4
    frames = np.zeros((2, b.n_atoms, 3))
    for f in (fa.trajectory_topology, fa.trajectory_file_topology):
        assert inspect.signature(f).parameters["interface_pairs"].default is None
    assert inspect.signature(fa.trajectory_file_topology).parameters["pair_areas_path"].default is None
    r = fa.TopologyResult(1, 2, 3, 4, 5, 6, 7)
    assert r.pair_areas is None and r.pair_groups is None
    with pytest.raises(ValueError, match="needs chain groups"):
        fa.trajectory_topology(frames, b, interface_pairs="all")
    with pytest.raises(ValueError, match="needs chain groups"):
        fa.trajectory_file_topology(tmp_path / "none.f64", b, tmp_path / "t", interface_pairs=[(0, 1)], pair_areas_path=tmp_path / "p")
    with pytest.raises(ValueError, match='"all"'):
        fa.trajectory_topology(frames, b, chain_groups="AC+B", interface_pairs="every")
    with pytest.raises(ValueError, match=r"\[K, 2\]"):
        fa.trajectory_topology(frames, b, chain_groups="AC+B", interface_pairs=[0, 1, 2])
    with pytest.raises(ValueError, match="go together"):
        fa.trajectory_file_topology(tmp_path / "none.f64", b, tmp_path / "t", chain_groups="AC+B", interface_pairs="all")
    with pytest.raises(ValueError, match="not offered"):
        fa.trajectory_topology(frames, b, chain_groups="AC+B", interface_pairs="all", volumes=True)
    # the library's refusals come through as RuntimeError with its message, before a device is asked for
    with pytest.raises(RuntimeError, match="pair 0 is"):
        fa.trajectory_topology(frames, b, chain_groups="AC+B", interface_pairs=[(1, 0)])
    with pytest.raises(RuntimeError, match="n_pairs < 1"):
        fa.trajectory_topology(frames, b, chain_groups="AC+B", interface_pairs=[])
    assert np.array_equal(fa._interface_pairs("all", ids, 4), tr.all_pairs(4))
    assert list(tmp_path.iterdir()) == []
