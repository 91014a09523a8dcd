"""The trajectory drivers' topology (freesasa_gpu_trajectory_topology / _trajectory_file_topology, include/freesasa_gpu.h)
without a GPU: the phase functions of csrc/traj_kernels.h driven on the CPU (tests/emu/emu_traj.cpp) against plain host sums
and against the emulations of the kernels they mirror (class sums, selection sums) on every frame as a batch of its own;
and the argument checks, which the library makes before it touches a device or a file."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import emu
import freesasa_amd as fa
from freesasa_amd import ingest
from emu import select_emu, traj_emu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
COMMANDS = ["a, resi -10", "b, chain A", "c, resn LYS and not name CA+N", "d, symbol O", "e, resi 70-", "f, name CB",
            "g, resn ILE+LEU+VAL", "h, resi 20-40 and symbol N", "i, not symbol C", "j, resi 1+76"]


def fixture(name):
    return os.path.join(PDB, name)


@pytest.fixture(scope="module")
def topo():
    """structure 1 of [3bkr, 1ubq] (batch-wide residue and atom offsets that do not start at 0), 1ubq loaded alone, 5 frames of
    seeded per-atom areas"""
    two = ingest.load_pdb_files([fixture("3bkr.pdb"), fixture("1ubq.pdb")])
    one = ingest.load_pdb_files([fixture("1ubq.pdb")])
    assert two.offsets[1] > 0 and two.res_offsets[1] > 0 and one.n_atoms == two.offsets[2] - two.offsets[1] == 602
    rng = np.random.default_rng(20261017)
    sasa = rng.uniform(0.0, 60.0, (5, one.n_atoms)) * (rng.random((5, one.n_atoms)) > 0.3)
    return two, one, sasa


def test_residue_sums_are_plain_left_to_right_sums(topo):
    two, one, sasa = topo
    _, res = traj_emu.sums(two, 1, sasa)
    assert res.shape == (5, 76, 6)
    first = one.res_first
    cols = [np.ones(one.n_atoms, bool), one.atom_backbone != 0, one.atom_backbone == 0, one.atom_class == 1,
            one.atom_class == 0, one.atom_class > 1]
    for f in range(5):
        for r in range(76):
            a, b = first[r], first[r + 1]
            for k, m in enumerate(cols):
                v = sasa[f, a:b][m[a:b]]
                want = np.cumsum(v)[-1] if v.size else 0.0       # (cumsum: sequential, in atom order)
                assert res[f, r, k] == want, (f, r, k)


def test_class_and_selection_sums_equal_the_per_structure_kernels_on_each_frame(topo):
    two, one, sasa = topo
    sel = ingest.Selection(COMMANDS)
    cls, _, bits, areas, counts = traj_emu.sums(two, 1, sasa, sel)
    L = emu._load()
    dp = C.POINTER(C.c_double)
    offs = np.array([0, one.n_atoms], dtype=np.int64)
    for f in range(5):
        want_bits, want_area, want_count = select_emu.run(sel, one, sasa[f])
        assert np.array_equal(bits, want_bits)
        assert np.array_equal(areas[f], want_area[0]) and np.array_equal(counts[f], want_count[0])
        want_cls = np.full(3, np.nan)
        row = np.ascontiguousarray(sasa[f])
        L.emu_class_sums(row.ctypes.data_as(dp), one.atom_class.ctypes.data_as(C.POINTER(C.c_ubyte)),
                         offs.ctypes.data_as(C.POINTER(C.c_int64)), 1, want_cls.ctypes.data_as(dp))
        assert np.array_equal(cls[f], want_cls)
    assert counts[0].min() > 0 and counts[0, 0] < one.n_atoms     # the open range and the others select something, not all
    sel.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gather_is_an_exact_indexed_copy(dtype):
    n, extra, F = 602, 37, 5
    rng = np.random.default_rng(7)
    frames = rng.normal(0, 30, (F, n + extra, 3)).astype(dtype)
    index = rng.permutation(n + extra)[:n].astype(np.int32)      # shuffled in: any order, the 37 others dropped
    got = traj_emu.gather(frames, index)
    assert np.array_equal(got, frames[:, index].astype(np.float64))


def _bad_calls():
    good = ingest.load_pdb_files([fixture("1ubq.pdb"), fixture("does_not_exist.pdb")])
    n = int(good.offsets[1])
    ident = np.arange(n, dtype=np.int32)
    out_of_range = ident.copy(); out_of_range[5] = n + 3
    twice = ident.copy(); twice[9] = twice[8]
    return good, n, [
        ("index out of range", dict(structure=0, atom_index=out_of_range, frame_atoms=n + 3), "out of range"),
        ("duplicate index", dict(structure=0, atom_index=twice, frame_atoms=n + 3), "twice"),
        ("frame_atoms < n", dict(structure=0, atom_index=ident, frame_atoms=n - 1), "smaller"),
        ("no index, frame_atoms != n", dict(structure=0, atom_index=None, frame_atoms=n + 3), "without an atom index"),
        ("structure out of range", dict(structure=2, atom_index=None, frame_atoms=n), "structure out of range"),
        ("negative structure", dict(structure=-1, atom_index=None, frame_atoms=n), "structure out of range"),
        ("failed structure", dict(structure=1, atom_index=None, frame_atoms=n), "failed to load"),
    ]


def test_argument_errors_come_before_any_device_or_file(tmp_path):
    batch, n, cases = _bad_calls()
    L = fa._topology_proto(fa.lib())
    cb = batch._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    frames_path = tmp_path / "frames.f64"
    np.zeros((2, n + 3, 3)).tofile(frames_path)
    for what, kw, text in cases:
        idx = kw["atom_index"]
        pidx = None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32))
        # the file form: -1, a message that names the error, no result file and no done-list
        outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "cls", "res", "sel")] + [tmp_path / "done.txt"]
        err = C.create_string_buffer(512)
        enc = lambda p: str(p).encode()
        rc = L.freesasa_gpu_trajectory_file_topology(enc(frames_path), 0, 0, 0, C.byref(cb), kw["structure"], kw["frame_atoms"], pidx, None,
                                                     fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), enc(outs[2]), enc(outs[3]),
                                                     None, None, enc(outs[5]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
        assert rc == -1 and text in err.value.decode(), (what, err.value)
        assert not any(p.exists() for p in outs), what
        # the memory form
        frames = np.zeros((2, kw["frame_atoms"], 3))
        totals = np.zeros(2)
        err = C.create_string_buffer(512)
        dp = C.POINTER(C.c_double)
        rc = L.freesasa_gpu_trajectory_topology(frames.ctypes.data_as(dp), 2, C.byref(cb), kw["structure"], kw["frame_atoms"], pidx, None,
                                                fa.LEE_RICHARDS, 1.4, 20, 0, totals.ctypes.data_as(dp), None, None, None, None, None,
                                                devs.ctypes.data_as(ip), 1, err, 512)
        assert rc == -1 and text in err.value.decode(), (what, err.value)
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_topology(None, 2, None, 0, n, None, None, fa.LEE_RICHARDS, 1.4, 20, 0, None, None, None, None, None, None,
                                            devs.ctypes.data_as(ip), 1, err, 512)
    assert rc == -1 and err.value
