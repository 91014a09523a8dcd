"""DCD input of the trajectory file drivers (FREESASA_GPU_FRAMES_DCD, include/freesasa_gpu.h) on the device.  Every comparison
is byte for byte between result files: one run reads a raw fp32 frame file - a path the existing tests pin to the
per-structure entries - the other a DCD file of the same values, written by tests/test_dcd.py's writer in the byte orders and
with the per-frame records the format allows.  Small seeded systems; frames_per_batch = 2 over 5 frames gives shards of 2, 2
and 1 frames: non-zero frame offsets and a short last shard."""
import os
import struct

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import tools
from freesasa_amd import ingest
from test_dcd import write_dcd

pytestmark = pytest.mark.gpu

PDB = os.path.join(ROOT, "tests", "golden", "pdb")
N, F, FPB = 37, 5, 2
ALGS = {"lr20": (fa.LEE_RICHARDS, 20), "sr100": (fa.SHRAKE_RUPLEY, 100)}
KINDS = {"little": dict(endian="<"), "big": dict(endian=">"), "cell": dict(endian="<", cell=True),
         "cell4d": dict(endian="<", cell=True, dim4=True), "big-cell4d": dict(endian=">", cell=True, dim4=True)}
COMMANDS = ["bb, name n+ca+c+o", "late, resi 10- and not symbol c"]


def jittered(xyz, n_frames, seed):
    """the structure and a seeded +-0.3 A jitter per frame, rounded to fp32: what both files hold"""
    rng = np.random.default_rng(seed)
    return (xyz[None] + rng.uniform(-0.3, 0.3, (n_frames,) + xyz.shape)).astype(np.float32)


@pytest.fixture(scope="module")
def coil():
    xyz, radii = tools.coil(N, 20261018)
    return jittered(xyz, F, 1), radii


def plain_run(tmp, tag, path, radii, alg="lr20", **kw):
    """trajectory_file into files of their own: ({output: bytes}, the done-list's path, complete, frames)"""
    a, res = ALGS[alg]
    paths = {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "done")}
    done, n_frames = fa.trajectory_file(path, radii, paths["totals"], paths["sasa"], done_path=paths["done"], alg=a, resolution=res,
                                        frames_per_batch=FPB, **kw)
    return {k: open(paths[k], "rb").read() for k in ("totals", "sasa")}, paths["done"], done, n_frames


_RAW = {}


@pytest.fixture
def raw_plain(coil, tmp_path_factory):
    """the raw fp32 run of the coil's frames, once per (algorithm, fp32 output)"""
    frames, radii = coil

    def get(alg, out_f32):
        if (alg, out_f32) not in _RAW:
            tmp = tmp_path_factory.mktemp("raw")
            frames.tofile(tmp / "frames.f32")
            got, _, done, n_frames = plain_run(tmp, "raw", tmp / "frames.f32", radii, alg, f32=True, out_f32=out_f32)
            assert done and n_frames == F and len(got["totals"]) == 8 * F and len(got["sasa"]) == (4 if out_f32 else 8) * F * N
            assert np.all(np.frombuffer(got["totals"]) > 0)
            _RAW[(alg, out_f32)] = got
        return _RAW[(alg, out_f32)]
    return get


@pytest.mark.parametrize("kind, alg, out_f32", [("little", "lr20", False), ("big", "lr20", False), ("cell", "lr20", False),
                                                 ("cell4d", "lr20", False), ("big-cell4d", "sr100", False), ("cell", "lr20", True)])
def test_plain_driver_equals_the_raw_run(coil, raw_plain, tmp_path, kind, alg, out_f32):
    frames, radii = coil
    want = raw_plain(alg, out_f32)
    write_dcd(tmp_path / "frames.dcd", frames, nset_header=0, **KINDS[kind])
    got, done_path, done, n_frames = plain_run(tmp_path, kind, tmp_path / "frames.dcd", radii, alg, dcd=True, out_f32=out_f32)
    assert done and n_frames == F
    assert got["totals"] == want["totals"] and got["sasa"] == want["sasa"]
    info = fa.dcd_info(tmp_path / "frames.dcd")
    head = open(done_path).readline()
    assert f" f32={4 | (2 if out_f32 else 0)} " in head and f" header_bytes={info.first_frame} " in head and f" n_frames={F} " in head


@pytest.fixture(scope="module")
def solvated():
    """2jo4 (516 atoms, chains A - D) as the solute of frames with 41 solvent atoms, the solute's atoms scattered among them: a
    shuffled, non-monotonic index; 3 * 516 * 2 coordinates per full shard are thirteen workgroups of the gather"""
    b = ingest.load_pdb_files([os.path.join(PDB, "2jo4.pdb")])
    n = int(b.n_atoms)
    assert n == 516
    solute = jittered(b.xyz, F, 2)
    rng = np.random.default_rng(3)
    index = rng.permutation(n + 41)[:n].astype(np.int32)
    assert np.any(np.diff(index) < 0)
    full = rng.uniform(b.xyz.min(0), b.xyz.max(0), (F, n + 41, 3)).astype(np.float32)
    full[:, index] = solute
    return b, full, index


OUTS = ("totals", "sasa", "cls", "res", "sel", "grp", "iso")


def topo_run(tmp, tag, path, system, sel, groups, **kw):
    b, _, index = system
    p = {k: str(tmp / f"{tag}.{k}") for k in OUTS + ("done",)}
    gkw = dict(separate_chains=True, group_areas_path=p["grp"], isolated_path=p["iso"]) if groups else {}
    done, n_frames, atoms = fa.trajectory_file_topology(path, b, p["totals"], atom_index=index, selection=sel, sasa_path=p["sasa"],
                                                        class_sums_path=p["cls"], residues_path=p["res"], selections_path=p["sel"],
                                                        done_path=p["done"], frames_per_batch=FPB, devices=[0, 0], **gkw, **kw)
    assert done and n_frames == F
    return {k: open(p[k], "rb").read() for k in OUTS if os.path.exists(p[k])}, atoms


@pytest.mark.parametrize("groups", [False, True], ids=["topology", "chain-groups"])
def test_topology_and_chain_groups_equal_the_raw_run(solvated, tmp_path, groups):
    b, full, index = solvated
    n, R = int(b.n_atoms), int(b.n_residues)
    full.tofile(tmp_path / "frames.f32")
    sel = ingest.Selection(COMMANDS)
    try:
        want, want_atoms = topo_run(tmp_path, "raw", tmp_path / "frames.f32", solvated, sel, groups, frame_atoms=n + 41, f32=True)
        for kind in ("big-cell4d", "little"):
            write_dcd(tmp_path / "frames.dcd", full, **KINDS[kind])
            got, atoms = topo_run(tmp_path, kind, tmp_path / "frames.dcd", solvated, sel, groups, dcd=True)    # (frame_atoms: the file's NATOM)
            assert sorted(got) == sorted(want) == sorted(OUTS if groups else OUTS[:5])
            for k in got:
                assert got[k] == want[k], (kind, k)
            assert np.array_equal(atoms, want_atoms) and atoms.min() > 0
    finally:
        sel.close()
    assert len(want["totals"]) == 8 * F and len(want["sasa"]) == 8 * F * n and len(want["res"]) == 8 * 6 * R * F and len(want["sel"]) == 8 * 2 * F
    if groups:
        assert len(want["grp"]) == 8 * 3 * 4 * F and len(want["iso"]) == 8 * F * n
        g = np.frombuffer(want["grp"]).reshape(F, 4, 3)
        assert np.all(g[:, :, 0] > 0)


def test_resume_done_lists_and_device_lists(coil, raw_plain, tmp_path):
    frames, radii = coil
    want = raw_plain("lr20", False)
    dcd, raw = tmp_path / "frames.dcd", tmp_path / "frames.f32"
    write_dcd(dcd, frames, cell=True)
    frames.tofile(raw)
    # stopped after one shard, then finished: the files of an uninterrupted run
    a, res = ALGS["lr20"]
    p = {k: str(tmp_path / f"part.{k}") for k in ("totals", "sasa", "done")}
    kw = dict(done_path=p["done"], alg=a, resolution=res, frames_per_batch=FPB)
    done, n_frames = fa.trajectory_file(dcd, radii, p["totals"], p["sasa"], dcd=True, max_new_shards=1, **kw)
    assert not done and n_frames == F and open(p["done"]).read().count("shard ") == 1
    done, _ = fa.trajectory_file(dcd, radii, p["totals"], p["sasa"], dcd=True, **kw)
    assert done and open(p["done"]).read().count("shard ") == 3
    assert open(p["totals"], "rb").read() == want["totals"] and open(p["sasa"], "rb").read() == want["sasa"]
    # a DCD run's list is not a raw run's, and the other way round: refused, files untouched
    before = open(p["done"]).read()
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
        fa.trajectory_file(raw, radii, p["totals"], p["sasa"], f32=True, **kw)
    got, raw_done, done, _ = plain_run(tmp_path, "rawlist", raw, radii, f32=True)
    assert done and got == want
    raw_list = open(raw_done).read()
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):
        fa.trajectory_file(dcd, radii, str(tmp_path / "rawlist.totals"), str(tmp_path / "rawlist.sasa"), dcd=True,
                           **dict(kw, done_path=raw_done))
    assert open(p["done"]).read() == before and open(raw_done).read() == raw_list
    assert open(tmp_path / "rawlist.totals", "rb").read() == want["totals"] and open(p["totals"], "rb").read() == want["totals"]
    assert " f32=1 " in raw_list.splitlines()[0] and " header_bytes=0 " in raw_list.splitlines()[0]
    # two lanes' worth of one device
    got, _, done, _ = plain_run(tmp_path, "two", dcd, radii, dcd=True, devices=[0, 0])
    assert done and got == want


def test_a_damaged_frame_ends_the_run_and_is_not_listed(coil, tmp_path):
    """a host check on the staged bytes: nothing of the damaged shard reaches the device"""
    frames, radii = coil
    dcd = tmp_path / "frames.dcd"
    data = bytearray(write_dcd(dcd, frames, cell=True))
    info = fa.dcd_info(dcd)
    at = info.first_frame + 3 * info.frame_bytes + 56 + info.plane_bytes          # the marker in front of frame 3's y record
    assert struct.unpack_from("<i", data, at)[0] == 4 * N
    struct.pack_into("<i", data, at, 4 * N + 4)
    dcd.write_bytes(bytes(data))
    assert fa.dcd_info(dcd).n_frames == F                                          # the header is whole: only the frame is not
    paths = {k: str(tmp_path / f"bad.{k}") for k in ("totals", "sasa", "done")}
    with pytest.raises(RuntimeError, match="frame 3 of the DCD file is damaged"):
        fa.trajectory_file(dcd, radii, paths["totals"], paths["sasa"], done_path=paths["done"], frames_per_batch=FPB, dcd=True, device=0)
    for line in open(paths["done"]).read().splitlines()[1:]:
        _, k, f0, nf = line.split()
        assert not int(f0) <= 3 < int(f0) + int(nf), line
