"""Interfaces between chain groups among periodic images in the trajectory drivers (include/freesasa_gpu.h,
freesasa_gpu_trajectory_file_interfaces_periodic / _interface_residues_periodic) without a GPU: the two phases of the groups'
periodic run (csrc/pbc_kernels.h, GpbcArgs) with the PAIR PART of a shard's combined batch - frames | isolated groups | pair
structures - driven thread by thread on a made-up expanded batch whose areas name their slot, so that every output element has
exactly one right value; k_fixed = 0 against the groups' run's own entries; and the refusals that come before a device is
touched or a file opened."""
import ctypes as C
import inspect

import numpy as np
import pytest

import freesasa_amd as fa
import traj_interfaces_ref as tr
from emu import traj_pairs_pbc_emu as pe

G = 3
N = 11                                                          # atoms of a frame
# ids of a frame's atoms: two atoms in no group, group 1 EMPTY (a pair with an empty side); and groups 1 AND 2 empty (pair
# (1, 2) is then a pair structure of 0 atoms)
LAYOUTS = {"one empty group": np.array([0, 2, -1, 2, 0, 0, 2, -1, 2, 0, 2], np.int32),
           "two empty groups": np.array([0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 0], np.int32)}
S = pe.SENTINEL


def shard(ids, nf, K):
    """the combined batch of a shard as TrajRun::batch_offsets lays it out, image counts that differ per structure, and
    expanded areas that name their slot -> (coff, eoff, esasa, src, pairs, frame_of [n_comb], n_iso, n_pair)"""
    pairs = tr.all_pairs(G)[:K]
    src = np.concatenate([np.flatnonzero(ids == g) for g in range(G)]).astype(np.int32)
    gsize = np.bincount(ids[ids >= 0], minlength=G)
    gfirst = np.concatenate([[0], np.cumsum(gsize)])
    pfirst, psrc = tr.cut(ids, pairs) if K else (np.zeros(1, np.int64), np.zeros(0, np.int32))
    n_iso, n_pair = int(src.size), int(psrc.size)
    sizes = [N] * nf + [int(gsize[g]) for f in range(nf) for g in range(G)] + [int(pfirst[k + 1] - pfirst[k]) for f in range(nf) for k in range(K)]
    coff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    # (TrajRun::batch_offsets, term by term)
    for f in range(nf):
        for g in range(G + 1):
            assert coff[nf + f * G + g] == nf * N + f * n_iso + gfirst[g]
        for k in range(K + 1):
            assert coff[nf * (1 + G) + f * K + k] == nf * (N + n_iso) + f * n_pair + pfirst[k]
    images = np.array([0 if sz == 0 else (7 * k + 3) % 11 + 1 for k, sz in enumerate(sizes)])
    eoff = np.concatenate([[0], np.cumsum(np.array(sizes) + images)]).astype(np.int64)
    assert all(eoff[k] != coff[k] for k in range(1, len(sizes) + 1))                 # eoff differs from coff everywhere behind 0
    esasa = np.concatenate([1000.0 * (k + 1) + 0.25 + np.arange(eoff[k + 1] - eoff[k]) for k in range(len(sizes))])
    frame_of = np.array(list(range(nf)) + [f for f in range(nf) for _ in range(G)] + [f for f in range(nf) for _ in range(K)])
    return coff, eoff, esasa, src, pairs, frame_of, n_iso, n_pair


def slot(k, j):
    return 1000.0 * (k + 1) + 0.25 + j


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("nf", [2, 3])
def test_every_output_element_has_its_one_right_value(nf, K, layout):
    ids = LAYOUTS[layout]
    coff, eoff, esasa, src, pairs, frame_of, n_iso, n_pair = shard(ids, nf, K)
    n_comb, n_all, pair_first = nf * (1 + G + K), int(coff[-1]), nf * (N + n_iso)
    assert n_all == nf * (N + n_iso + n_pair)
    sizes = np.diff(coff)
    if layout == "one empty group":
        assert sizes[nf + 1] == 0 and sizes[nf * (1 + G)] == 4                       # pair (0, 1): one side empty
    if layout == "two empty groups" and K == 3:
        assert sizes[nf * (1 + G) + 2] == 0                                          # pair (1, 2): a structure of 0 atoms
    # the cells: every combined structure its frame's row, for both widths; nothing behind the array's end
    for W in (3, 9):
        cells = 100.0 * (np.arange(nf)[:, None] + 1) + np.arange(W)[None, :]
        got = pe.cells(cells, G, K)
        assert got[:n_comb].tobytes() == cells[frame_of].tobytes()
        assert np.all(got[n_comb:] == S)
    # the finish
    sasa, iso, carea, cgath = pe.finish(nf, G, K, coff, eoff, esasa, src, ids)
    w_carea = np.concatenate([slot(k, np.arange(sizes[k])) for k in range(n_comb)])
    assert np.array_equal(carea[:n_all], w_carea) and np.all(carea[n_all:] == S)
    w_sasa = w_carea[:nf * N]
    assert np.array_equal(sasa[:nf * N], w_sasa) and np.all(sasa[nf * N:] == S)      # (the pair part and the guard: untouched)
    w_iso = np.full(nf * N, np.nan)
    w_cgath = np.full(pair_first, np.nan)
    w_cgath[:nf * N] = w_sasa
    for f in range(nf):
        for i in np.flatnonzero(ids < 0):
            w_iso[f * N + i] = w_sasa[f * N + i]                                     # in no group: its complex area
        for q, i in enumerate(src):
            t = nf * N + f * n_iso + q
            w_iso[f * N + i] = w_carea[t]                                            # its area in its isolated group
            w_cgath[t] = w_sasa[f * N + i]                                           # beside it the source atom's complex area
    assert not np.isnan(w_iso).any() and not np.isnan(w_cgath).any()
    assert np.array_equal(iso[:nf * N], w_iso) and np.all(iso[nf * N:] == S)
    assert np.array_equal(cgath[:pair_first], w_cgath)
    assert np.all(cgath[pair_first:] == S)                                           # the pair part of cgath: never written
    # the parts in front of the pairs are the groups' run's, byte for byte: the same batch cut off behind its groups
    cut = nf * (1 + G)
    o_sasa, o_iso, o_carea, o_cgath = pe.finish(nf, G, 0, coff[:cut + 1], eoff[:cut + 1], esasa[:eoff[cut]], src, ids, old=True)
    assert sasa[:nf * N].tobytes() == o_sasa[:nf * N].tobytes() and iso[:nf * N].tobytes() == o_iso[:nf * N].tobytes()
    assert carea[:pair_first].tobytes() == o_carea[:pair_first].tobytes() and cgath[:pair_first].tobytes() == o_cgath[:pair_first].tobytes()


@pytest.mark.parametrize("nf", [2, 3])
def test_without_pairs_the_results_are_the_old_ones(nf):
    """k_fixed = 0 through the new entries against the groups' run's own (tests/emu/emu_groups_pbc.cpp): whole arrays, guards included"""
    ids = LAYOUTS["one empty group"]
    coff, eoff, esasa, src, *_ = shard(ids, nf, 0)
    for W in (3, 9):
        cells = 100.0 * (np.arange(nf)[:, None] + 1) + np.arange(W)[None, :]
        assert pe.cells(cells, G, 0).tobytes() == pe.cells(cells, G, 0, old=True).tobytes()
    new, old = pe.finish(nf, G, 0, coff, eoff, esasa, src, ids), pe.finish(nf, G, 0, coff, eoff, esasa, src, ids, old=True)
    for a, b in zip(new, old):
        assert a.tobytes() == b.tobytes()
    assert not np.any(new[3][:coff[-1]] == S)                                        # without pairs all of cgath is written


# ------------------------------------------------------------------------------------------------ the refusals, without a device

def _protos():
    return fa._stats_proto(fa._topology_proto(fa.lib()))


@pytest.fixture(scope="module")
def jo4():
    import os
    from conftest import ROOT
    from freesasa_amd import ingest
    b = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    return b, np.repeat(np.arange(2, dtype=np.int32), 258)


PBC = fa.FRAMES_DCD | fa.FRAMES_PBC


def test_the_new_entries_refuse_before_a_device_or_a_file(jo4, tmp_path):
    b, ids = jo4
    n = b.n_atoms
    L = _protos()
    cb = b._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, i32 = C.POINTER(C.c_int), C.POINTER(C.c_int32)
    enc = lambda p: None if p is None else str(p).encode()
    outs = {k: tmp_path / f"{k}.bin" for k in ("totals", "groups", "pairs", "pres")}
    ok = np.array([[0, 1]], np.int32)

    def call(residues, bits=PBC, group=ids, n_groups=2, pairs=ok, K=1, pair_path=outs["pairs"], pres_path=outs["pres"], min_buried=0.0, stats=0):
        err = C.create_string_buffer(512)
        head = (enc(tmp_path / "frames.dcd"), bits, 0, 0, C.byref(cb), 0, n, None, None, None if group is None else group.ctypes.data_as(i32), n_groups,
                fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs["totals"]), None, None, None, None, None, enc(outs["groups"]), None, None, 0,
                devs.ctypes.data_as(ip), 1, None, stats, None, None, None if pairs is None else pairs.ctypes.data_as(i32), K, enc(pair_path))
        if residues:
            rc = L.freesasa_gpu_trajectory_file_interface_residues_periodic(*head, min_buried, enc(pres_path), err, 512)
        else:
            rc = L.freesasa_gpu_trajectory_file_interfaces_periodic(*head, err, 512)
        assert rc == -1 and list(tmp_path.iterdir()) == []
        return err.value.decode()

    for residues, sibling in ((False, "freesasa_gpu_trajectory_file_interfaces's"), (True, "freesasa_gpu_trajectory_file_interface_residues's")):
        # bit 3 is required (bit 4 needs it), and the message names the non-periodic entry
        for bits in (fa.FRAMES_DCD, fa.FRAMES_DCD | fa.FRAMES_TRICLINIC, 0):
            msg = call(residues, bits=bits)
            assert "need bit 3 of frames_f32" in msg and msg.endswith(sibling)
        msg = call(residues, group=None)
        assert "need chain groups" in msg and "group is NULL" in msg
        assert "pair 0 is (1, 0)" in call(residues, pairs=np.array([[1, 0]], np.int32))
        msg = call(residues, pairs=np.array([[0, 1], [0, 2]], np.int32), K=2)
        assert "pair 1 is (0, 2)" in msg and "n_groups = 2" in msg
        msg = call(residues, n_groups=3, pairs=np.array([[0, 2], [1, 2], [0, 1], [1, 2]], np.int32), K=4)
        assert "pairs 1 and 3" in msg and "(1, 2)" in msg and "at most once" in msg
        assert "n_pairs < 1" in call(residues, K=0)
        assert "null argument: the pairs" in call(residues, pairs=None)
        assert "nowhere to go" in call(residues, pair_path=None, pres_path=None)
    for bad in (np.nan, np.inf, -np.inf):
        assert "min_buried must be finite" in call(True, min_buried=bad)
    # the statistics bits of the pair outputs are the residues entry's alone
    assert "unknown bit in the statistics word" in call(False, stats=128)
    # behind the pairs' checks the groups' own still hold
    bad = ids.copy()
    bad[7] = -2
    msg = call(False, group=bad)
    assert "atom 7 " in msg and "group id -2" in msg


def test_the_old_entries_keep_refusing_with_the_old_text(jo4, tmp_path):
    b, ids = jo4
    for tri in (False, True):
        for kw in ({"pair_areas_path": tmp_path / "p"}, {"pair_residues_path": tmp_path / "r"}):
            with pytest.raises(RuntimeError, match="interfaces among periodic images are not offered") as e:
                fa.trajectory_file_topology(tmp_path / "f.dcd", b, tmp_path / "t", group=ids, n_groups=2, group_areas_path=tmp_path / "g", dcd=True, frame_atoms=b.n_atoms,
                                            pbc=True, triclinic=tri, interface_pairs="all", **kw)
            assert "freesasa_gpu_trajectory_file_interfaces_periodic" in str(e.value)     # ... and goes on to name the new entry
    assert list(tmp_path.iterdir()) == []


def test_python_keywords(jo4, tmp_path):
    b, ids = jo4
    par = inspect.signature(fa.trajectory_file_groups_periodic).parameters
    assert all(par[k].default is None for k in ("interface_pairs", "pair_areas_path", "pair_residues_path", "min_buried"))
    kw = dict(group=ids, n_groups=2, group_areas_path=tmp_path / "g", dcd=True, frame_atoms=b.n_atoms)
    with pytest.raises(ValueError, match="go together"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, tmp_path / "t", interface_pairs="all", **kw)
    with pytest.raises(ValueError, match="go together"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, tmp_path / "t", pair_areas_path=tmp_path / "p", **kw)
    with pytest.raises(ValueError, match="need interface_pairs"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, tmp_path / "t", min_buried=1.0, **kw)
    with pytest.raises(ValueError, match="needs chain groups"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, tmp_path / "t", interface_pairs="all", pair_areas_path=tmp_path / "p", dcd=True,
                                           frame_atoms=b.n_atoms)
    # the C entry is chosen by what is asked for, and its refusals come through with its name
    with pytest.raises(RuntimeError, match=r"freesasa_gpu_trajectory_file_interfaces_periodic: .*pair 0 is \(1, 0\)"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, tmp_path / "t", interface_pairs=[(1, 0)], pair_areas_path=tmp_path / "p", **kw)
    with pytest.raises(RuntimeError, match=r"freesasa_gpu_trajectory_file_interface_residues_periodic: .*min_buried must be finite"):
        fa.trajectory_file_groups_periodic(tmp_path / "f.dcd", b, tmp_path / "t", interface_pairs="all", pair_areas_path=tmp_path / "p", min_buried=float("nan"), **kw)
    assert list(tmp_path.iterdir()) == []
