"""Per-residue interface tables per frame of a trajectory (freesasa_gpu_trajectory_interface_residues / _file_interface_residues /
_interface_segments, include/freesasa_gpu.h) without a GPU: the segments entry against the restatement
(tests/traj_interface_residues_ref.py) on a synthetic topology that holds every case coverage() lists; the kernel's phase function
driven on the CPU (tests/emu/emu_traj_pair_res.cpp) against the restatement with == ; the widths of the two new statistics
bits; and the argument checks, which the library makes before it touches a device or a file."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import traj_interface_residues_ref as tq
import traj_interfaces_ref as tr
from freesasa_amd import ingest
from emu import traj_pair_res_emu
from test_traj_interfaces import _bad_pair_calls

PDB = os.path.join(ROOT, "tests", "golden", "pdb")


def synthetic_batch():
    """2jo4's atoms under the residues of tq.synthetic(): (batch, group, G, pairs, res_first)"""
    group, G, pairs, res_first = tq.synthetic()
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    assert b.n_atoms == tq.N_SYNTH == group.size and b.n_structs == 1
    R = res_first.size - 1
    b.n_residues = R
    b.res_first, b.res_offsets = res_first.copy(), np.array([0, R], np.int64)
    b.res_ref = np.full(R, -1, np.int16)
    b.res_name_raw = np.array([b"RES "] * R, dtype="S4")
    b.res_number_raw = np.array([b"%6d" % r for r in range(R)], dtype="S6")
    b.res_chain_raw = np.array([b"A   "] * R, dtype="S4")
    return b, group, G, pairs, res_first


@pytest.fixture(scope="module")
def synth():
    return synthetic_batch()


def test_the_synthetic_topology_holds_every_case():
    cov = tq.coverage()
    assert len(cov) == 12 and all(cov.values()), [k for k, v in cov.items() if not v]


# ------------------------------------------------------------------------------------------------ the segments

def test_the_segments_entry_equals_the_restatement(synth):
    b, group, G, pairs, res_first = synth
    first, seg_res, seg_side, pside, psrc = tq.segments(group, G, pairs, res_first)
    offs, res, atoms = fa.traj_pair_segments(b, group, G, pairs)
    assert res.dtype == np.int32 and atoms.dtype == np.int32 and offs.dtype == np.int64
    assert np.array_equal(res, seg_res) and np.array_equal(atoms, np.diff(first)) and np.array_equal(offs, tq.side_offsets(seg_side, len(pairs)))
    assert atoms.max() == tq.LONG and offs[-1] == res.size and offs[7] == offs[8]      # (the empty group's side)
    # the host cut of the emulation is the same function
    e_first, e_res, e_side, e_iso = traj_pair_res_emu.cut(group, G, pairs, res_first)
    assert np.array_equal(e_first, first) and np.array_equal(e_res, seg_res) and np.array_equal(e_side, seg_side)
    # a segment's place in the isolated part: its side's group begins at gfirst[g], the segment as far into it as into the side
    gfirst = np.concatenate([[0], np.cumsum(np.bincount(group[group >= 0], minlength=G))])
    assert np.array_equal(e_iso, gfirst[pairs.reshape(-1)[seg_side]] + (first[:-1] - pside[seg_side]))
    # a subset of the pairs in another order: the segments of those sides
    offs2, res2, atoms2 = fa.traj_pair_segments(b, group, G, pairs[[2, 0]])
    for k2, k in enumerate((2, 0)):
        for q in (0, 1):
            a, a2 = slice(offs[2 * k + q], offs[2 * k + q + 1]), slice(offs2[2 * k2 + q], offs2[2 * k2 + q + 1])
            assert np.array_equal(res2[a2], res[a]) and np.array_equal(atoms2[a2], atoms[a])


def _segments_call(b, group, G, pairs, cap, structure=0, K=None):
    L = fa._stats_proto(fa.lib())
    cb = b._as_c()
    i32 = C.POINTER(C.c_int32)
    K = len(pairs) if K is None else K
    S, err = C.c_longlong(-5), C.create_string_buffer(512)
    offs, res, atoms = np.full(2 * max(K, 0) + 1, -7, np.int64), np.full(max(cap, 0) + 1, -7, np.int32), np.full(max(cap, 0) + 1, -7, np.int32)
    rc = L.freesasa_gpu_trajectory_interface_segments(C.byref(cb), structure, None if group is None else group.ctypes.data_as(i32), G,
                                                      pairs.ctypes.data_as(i32), K, cap, C.byref(S), offs.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                      res.ctypes.data_as(i32), atoms.ctypes.data_as(i32), err, 512)
    return rc, S.value, err.value.decode(), offs, res, atoms


def test_a_capacity_one_too_small_fails_with_S_and_writes_nothing(synth):
    b, group, G, pairs, res_first = synth
    S = tq.segments(group, G, pairs, res_first)[1].size
    rc, n, msg, offs, res, atoms = _segments_call(b, group, G, pairs, S - 1)
    assert rc == -1 and n == S and str(S) in msg and "seg_capacity" in msg
    assert np.all(offs == -7) and np.all(res == -7) and np.all(atoms == -7)
    rc, n, msg, offs, res, atoms = _segments_call(b, group, G, pairs, S)
    assert rc == 0 and n == S and msg == "" and res[-1] == -7 and atoms[-1] == -7 and np.all(res[:-1] >= 0) and offs[-1] == S


def test_the_segments_entry_refuses_what_the_run_refuses(synth):
    b, group, G, pairs, _ = synth
    ids2 = (group % 2).astype(np.int32)
    for what, kw, texts in _bad_pair_calls(ids2):
        rc, _, msg, *_ = _segments_call(b, kw["group"], kw.get("G", 2), kw["pairs"], 1000, K=kw["K"])
        assert rc == -1 and all(t in msg for t in texts), (what, msg)
    bad = group.copy()
    bad[7] = -2
    rc, _, msg, *_ = _segments_call(b, bad, G, pairs, 1000)
    assert rc == -1 and "atom 7 " in msg and "group id -2" in msg
    rc, _, msg, *_ = _segments_call(b, group, G, pairs, 1000, structure=3)
    assert rc == -1 and "structure out of range" in msg
    rc, _, msg, *_ = _segments_call(b, None, G, pairs, 1000)
    assert rc == -1 and "group is NULL" in msg
    with pytest.raises(RuntimeError, match="n_pairs < 1"):
        fa.traj_pair_segments(b, group, G, np.zeros((0, 2), np.int32))


# ------------------------------------------------------------------------------------------------ the kernel, emulated

@pytest.mark.parametrize("nf", [1, 3, 9])
def test_the_phase_function_equals_the_restatement(synth, nf):
    b, group, G, pairs, res_first = synth
    n = group.size
    first, seg_res, seg_side, pside, psrc = tq.segments(group, G, pairs, res_first)
    nc = n + int((group >= 0).sum()) + psrc.size
    rng = np.random.default_rng(20261021 + nf)
    csasa = rng.uniform(0.0, 60.0, nf * nc) * (rng.random(nf * nc) > 0.3)
    # in frame 0 the pair part of pair 0 is its atoms' isolated areas: buried is exactly 0 there, and not above min_buried = 0
    src = np.concatenate([np.nonzero(group == g)[0] for g in range(G)])
    place = np.full(n, -1)
    place[src] = np.arange(src.size)
    csasa[nf * (n + src.size):nf * (n + src.size) + pside[2]] = csasa[nf * n + place[psrc[:pside[2]]]]
    for min_buried in (0.0, 25.0):
        got = traj_pair_res_emu.shard(group, G, pairs, res_first, nf, csasa, min_buried)
        want = tq.combined_table(csasa, nf, n, group, G, pairs, res_first, min_buried)
        assert got.shape == want.shape == (nf, seg_res.size, 4)
        assert np.all(got == want), (nf, min_buried, np.argwhere(got != want)[:5])
        assert np.all(got[:, :, 2] == got[:, :, 0] - got[:, :, 1]) and set(np.unique(got[:, :, 3])) <= {0.0, 1.0}
        assert 0 < got[:, :, 3].sum() < got[:, :, 3].size
    zero = seg_side < 2
    assert np.all(got[0, zero, 2] == 0.0) and np.all(traj_pair_res_emu.shard(group, G, pairs, res_first, nf, csasa, 0.0)[0, zero, 3] == 0.0)


def test_stand_alone_sanitizer_program():
    """the host cut and the phase function under AddressSanitizer + UBSan, in a program of their own (nothing is preloaded anywhere)"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/pair_res_check"], check=True, stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "pair_res_check")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.split("\n")[:2] == ["cut ok", "shard ok"], res.stdout


# ------------------------------------------------------------------------------------------------ the widths

def test_the_widths_of_the_two_new_bits():
    n, R, S, G, K, NS = 516, 90, 5, 4, 6, 240
    width = [1, n, n, 3, 6 * R, S, 3 * G, 6 * K, 4 * NS]
    for word in (0, 1, 127, 128, 256, 384, 511, 128 | 64 | 2, 256 | 1):
        W, first = fa.traj_stats_width_pairs(word, n, R, S, G, K, NS)
        at, want = 0, []
        for k in range(9):
            want.append(at if word >> k & 1 else -1)
            at += width[k] if word >> k & 1 else 0
        assert W == at and first.tolist() == want, word
        if word < 128:      # with the seven bits it is the old function
            W7, first7 = fa.traj_stats_width(word, n, R, S, G)
            assert W7 == W and first7.tolist() == want[:7]
    assert fa.traj_stats_width_pairs(("pairs", "pair_residues"), n, R, S, G, K, NS)[0] == 6 * K + 4 * NS
    # the old function is unchanged for 128 and 256, and the new one knows nothing above 256
    L = fa._stats_proto(fa.lib())
    for word in (128, 256, 128 | 1, 511):
        assert L.freesasa_gpu_traj_stats_width(word, n, R, S, G, None) == -1
        with pytest.raises(ValueError):
            fa.traj_stats_width(word, n, R, S, G)
    for bad in ((512, n, R, S, G, K, NS), (-1, n, R, S, G, K, NS), (128, n, R, S, G, -1, NS), (256, n, R, S, G, K, -1)):
        assert L.freesasa_gpu_traj_stats_width_pairs(*bad, None) == -1
    assert tuple(fa.STATS_BITS) == ("totals", "atoms", "isolated", "classes", "residues", "selections", "groups")
    assert fa.PAIR_STATS_BITS == {"pairs": 128, "pair_residues": 256}
    assert fa.stats_word(("groups", "pairs"), pairs=True) == 192
    with pytest.raises(ValueError, match="unknown statistics output"):
        fa.stats_word(("pairs",))


# ------------------------------------------------------------------------------------------------ the argument checks

def test_argument_errors_come_before_any_device_or_file(synth, tmp_path):
    b, _, _, _, _ = synth
    n = b.n_atoms
    ids = np.repeat(np.array([0, 1, 0, -1], np.int32), 129)
    L = fa._stats_proto(fa._topology_proto(fa.lib()))
    cb = b._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp, i32 = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    frames_path = tmp_path / "frames.f64"
    np.zeros((2, n, 3)).tofile(frames_path)
    enc = lambda p: None if p is None else str(p).encode()
    frames, totals, areas = np.zeros((2, n, 3)), np.zeros(2), np.zeros((2, 3, 3))
    pair_areas, pair_res, stats_out = np.zeros((2, 4, 6)), np.zeros((2, 4 * n, 4)), np.zeros(4 * (40 * n))
    outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "groups", "iso", "pairs", "pres", "stats", "parts")] + [tmp_path / "done.txt"]

    def file_call(group, G, pairs, K, bits=0, pair_path=outs[4], res_path=outs[5], stats=0, min_buried=0.0):
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_interface_residues(enc(frames_path), bits, 0, 0, C.byref(cb), 0, n, None, None,
                                                               None if group is None else group.ctypes.data_as(i32), G,
                                                               fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), None, None, None, None,
                                                               enc(outs[2]), enc(outs[3]), enc(outs[8]), 0, devs.ctypes.data_as(ip), 1, None,
                                                               stats, enc(outs[6]), enc(outs[7]), None if pairs is None else pairs.ctypes.data_as(i32), K,
                                                               enc(pair_path), min_buried, enc(res_path), err, 512)
        assert not any(p.exists() for p in outs)
        return rc, err.value.decode()

    def mem_call(group, G, pairs, K, pair_out=pair_areas, res_out=pair_res, stats=0, min_buried=0.0):
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_interface_residues(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, n, None, None,
                                                          None if group is None else group.ctypes.data_as(i32), G,
                                                          fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                                          areas.ctypes.data_as(dp), None, devs.ctypes.data_as(ip), 1, stats, stats_out.ctypes.data_as(dp), None,
                                                          None if pairs is None else pairs.ctypes.data_as(i32), K,
                                                          None if pair_out is None else pair_out.ctypes.data_as(dp), min_buried,
                                                          None if res_out is None else res_out.ctypes.data_as(dp), err, 512)
        return rc, err.value.decode()

    # everything the interface entries refuse about the groups and the pairs
    for what, kw, texts in _bad_pair_calls(ids):
        for call in (file_call, mem_call):
            rc, msg = call(kw["group"], kw.get("G", 2), kw["pairs"], kw["K"])
            assert rc == -1 and all(t in msg for t in texts), (what, call.__name__, msg)
    ok = np.array([[0, 1]], np.int32)
    for call in (file_call, mem_call):
        rc, msg = call(ids, 2, None, 1)
        assert rc == -1 and "null argument: the pairs" in msg
    for bits in (fa.FRAMES_DCD | fa.FRAMES_PBC, fa.FRAMES_DCD | fa.FRAMES_PBC | fa.FRAMES_TRICLINIC):
        rc, msg = file_call(ids, 2, ok, 1, bits=bits)
        assert rc == -1 and "interfaces among periodic images are not offered" in msg
    # nowhere to go: neither output delivered nor in the statistics word - and a statistics bit of another output does not help
    for stats in (0, fa.STATS_BITS["groups"]):
        rc, msg = file_call(ids, 2, ok, 1, pair_path=None, res_path=None, stats=stats)
        assert rc == -1 and "nowhere to go" in msg and "pair residues" in msg, msg
        rc, msg = mem_call(ids, 2, ok, 1, pair_out=None, res_out=None, stats=stats)
        assert rc == -1 and "nowhere to go" in msg and "pair residues" in msg, msg
    # a min_buried that is not finite
    for v in (float("nan"), float("inf"), float("-inf")):
        for call in (file_call, mem_call):
            rc, msg = call(ids, 2, ok, 1, min_buried=v)
            assert rc == -1 and "min_buried must be finite" in msg, (v, msg)
    # a bit above the nine, and statistics without a place for them, as every statistics entry refuses them
    rc, msg = mem_call(ids, 2, ok, 1, stats=512)
    assert rc == -1 and "unknown bit" in msg
    rc, msg = file_call(ids, 2, ok, 1, stats=1024 | 128)
    assert rc == -1 and "unknown bit" in msg
    # the groups' and the topology's own checks still hold behind the pairs'
    bad = ids.copy()
    bad[7] = -2
    for call in (file_call, mem_call):
        rc, msg = call(bad, 2, ok, 1)
        assert rc == -1 and "atom 7 " in msg and "group id -2" in msg
    # the parents keep refusing the two new bits
    for word in (128, 256):
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_interfaces(frames.ctypes.data_as(dp), 2, C.byref(cb), 0, n, None, None, ids.ctypes.data_as(i32), 2,
                                                  fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                                  areas.ctypes.data_as(dp), None, devs.ctypes.data_as(ip), 1, word, stats_out.ctypes.data_as(dp), None,
                                                  ok.ctypes.data_as(i32), 1, pair_areas.ctypes.data_as(dp), err, 512)
        assert rc == -1 and "unknown bit" in err.value.decode()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["frames.f64"]


def test_python_keywords(synth, tmp_path):
    b, group, G, pairs, _ = synth
    frames = np.zeros((2, b.n_atoms, 3))
    assert inspect.signature(fa.trajectory_topology).parameters["interface_residues"].default is False
    assert inspect.signature(fa.trajectory_topology).parameters["min_buried"].default == 0.0
    for k in ("pair_residues_path", "min_buried"):
        assert inspect.signature(fa.trajectory_file_topology).parameters[k].default is None
    r = fa.TopologyResult(1, 2, 3, 4, 5, 6, 7)
    assert r.pair_residues is None and r.pair_res_offsets is None and r.pair_res_index is None and r.pair_res_atoms is None
    r = fa.TopologyResult(1, 2, 3, 4, 5, 6, 7, pair_res_offsets=np.array([0, 3, 5, 5, 9]))
    assert r.side_segments(0, 1) == slice(3, 5) and r.side_segments(1, 0) == slice(5, 5) and r.side_segments(1, 1) == slice(5, 9)
    with pytest.raises(ValueError, match="needs interface_pairs"):
        fa.trajectory_topology(frames, b, group=group, n_groups=G, interface_residues=True)
    with pytest.raises(ValueError, match="need interface_pairs"):
        fa.trajectory_file_topology(tmp_path / "none.f64", b, tmp_path / "t", group=group, n_groups=G, pair_residues_path=tmp_path / "p")
    with pytest.raises(ValueError, match="unknown statistics output"):
        fa.trajectory_topology(frames, b, group=group, n_groups=G, interface_pairs=pairs, stats=("pair_residues",))
    # the library's refusals come through as RuntimeError with its message, before a device is asked for
    with pytest.raises(RuntimeError, match="pair 0 is"):
        fa.trajectory_topology(frames, b, group=group, n_groups=G, interface_pairs=[(1, 0)], interface_residues=True)
    with pytest.raises(RuntimeError, match="min_buried must be finite"):
        fa.trajectory_topology(frames, b, group=group, n_groups=G, interface_pairs=pairs, interface_residues=True, min_buried=float("nan"))
    with pytest.raises(RuntimeError, match="min_buried must be finite"):
        fa.trajectory_file_topology(tmp_path / "none.f64", b, tmp_path / "t", group=group, n_groups=G, interface_pairs=pairs,
                                    pair_residues_path=tmp_path / "p", min_buried=float("inf"))
    assert list(tmp_path.iterdir()) == []
