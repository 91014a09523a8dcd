"""Molecular volume on the device (freesasa_gpu_calc_volume / freesasa_gpu_sr_volume_dev and the volume output of the trajectory
topology entries).  The yardstick is the numpy restatement of the definition (tests/volume_ref.py): on the seeded batch its
counts are the engine's on every atom (tests/test_volume.py holds that against the oracle), and under that condition the
exposed-point vectors, the atoms' terms and the structures' volumes are compared BIT FOR BIT; areas, counts and totals are
calc_batch's byte for byte.  The trajectory entries are held to calc_volume on every frame."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
import volume_ref as vr
from test_dcd import write_dcd

pytestmark = pytest.mark.gpu

PROBE = 1.4
F, N, FA, FPB = 7, 70, 90, 3


@pytest.fixture(scope="module")
def batch():
    return vr.batch()


_REF, _GOT = {}, {}


def reference(batch, n_points):
    if n_points not in _REF:
        _REF[n_points] = vr.volume_batch(*batch, PROBE, fa.test_points(n_points))
    return _REF[n_points]


def device(batch, n_points):
    """calc_volume on the batch, once per point count: (sasa, counts, totals, volumes, evec, vol)"""
    if n_points not in _GOT:
        _GOT[n_points] = fa.calc_volume(*batch, probe=PROBE, n_points=n_points, per_atom=True)
    return _GOT[n_points]


@pytest.mark.parametrize("n_points", vr.POINT_COUNTS)
def test_the_batch_equals_the_definition_bit_for_bit(batch, n_points):
    xyz, radii, offsets = batch
    sasa, counts, totals, volumes, evec, vol = device(batch, n_points)
    want_sasa, want_counts, want_totals = fa.calc_batch(xyz, radii, offsets, fa.SHRAKE_RUPLEY, probe=PROBE, resolution=n_points)
    assert sasa.tobytes() == want_sasa.tobytes() and counts.tobytes() == want_counts.tobytes() and totals.tobytes() == want_totals.tobytes()
    ref = reference(batch, n_points)
    assert np.array_equal(counts, ref["counts"]), "the condition on the inputs does not hold: another seed"
    assert evec.tobytes() == ref["evec"].tobytes()
    assert vol.tobytes() == ref["vol"].tobytes()
    assert volumes.tobytes() == ref["volumes"].tobytes()
    assert volumes[4] == 0 and vol[6] == 0 and np.all(evec[6] == 0)           # no atoms; the atom inside another
    # without the per-atom outputs the others are the same
    lean = fa.calc_volume(xyz, radii, offsets, probe=PROBE, n_points=n_points)
    assert len(lean) == 4 and all(a.tobytes() == b.tobytes() for a, b in zip(lean, (sasa, counts, totals, volumes)))


def test_the_device_pointer_entry(batch):
    import torch
    xyz, radii, offsets = batch
    sasa, counts, totals, volumes, evec, vol = device(batch, 100)
    dev = torch.device("cuda:0")
    n, ns = len(radii), len(offsets) - 1
    d_xyz, d_r = torch.from_numpy(xyz.reshape(-1)).to(dev), torch.from_numpy(radii).to(dev)
    d_sasa, d_vols = torch.full((n,), -7.0, dtype=torch.float64, device=dev), torch.full((ns,), -7.0, dtype=torch.float64, device=dev)
    d_counts = torch.zeros(n, dtype=torch.int32, device=dev)
    d_evec, d_vol, d_tot = (torch.zeros(k, dtype=torch.float64, device=dev) for k in (3 * n, n, ns))
    ctx = fa.GpuContext(0)
    try:
        # only what is required, then everything
        ctx.volume(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_vols.data_ptr(), probe=PROBE)
        assert d_sasa.cpu().numpy().tobytes() == sasa.tobytes() and d_vols.cpu().numpy().tobytes() == volumes.tobytes()
        d_vols.fill_(-7.0)
        ctx.volume(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_vols.data_ptr(), d_counts.data_ptr(), d_evec.data_ptr(),
                   d_vol.data_ptr(), d_tot.data_ptr(), probe=PROBE)
        for got, want in ((d_vols, volumes), (d_counts, counts), (d_evec, evec), (d_vol, vol), (d_tot, totals)):
            assert got.cpu().numpy().tobytes() == want.tobytes()
        # refused: more than 128 points - -1 with the reason, no volume written, the context good for an ordinary batch
        d_vols.fill_(-7.0)
        with pytest.raises(RuntimeError, match="up to 128 test points .129 asked for"):
            ctx.volume(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_vols.data_ptr(), probe=PROBE, n_points=129)
        assert np.all(d_vols.cpu().numpy() == -7.0)
        with pytest.raises(RuntimeError, match="n_points must be > 0"):
            ctx.volume(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_vols.data_ptr(), probe=PROBE, n_points=0)
        with pytest.raises(RuntimeError, match="null argument"):
            ctx.volume(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), 0, probe=PROBE)
        ctx.shrake_rupley(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_counts.data_ptr(), probe=PROBE, n_points=100)
        assert d_sasa.cpu().numpy().tobytes() == sasa.tobytes() and d_counts.cpu().numpy().tobytes() == counts.tobytes()
    finally:
        ctx.close()


def test_translation_moves_the_origin_with_the_structure(batch):
    xyz, radii, offsets = batch
    b, e = int(offsets[6]), int(offsets[7])
    sasa, counts, totals, volumes, evec, vol = device(batch, 100)
    moved = fa.calc_volume(xyz[b:e] + vr.SHIFT, radii[b:e], [0, e - b], probe=PROBE, n_points=100)
    assert np.array_equal(moved[1], counts[b:e])
    assert abs(moved[3][0] - volumes[6]) <= 1e-9 * volumes[6]


def with_cfg(cfg, fn):
    old = os.environ.get("FREESASA_AMD_CFG")
    os.environ["FREESASA_AMD_CFG"] = cfg
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("FREESASA_AMD_CFG", None)
        else:
            os.environ["FREESASA_AMD_CFG"] = old


def test_volumes_do_not_depend_on_the_batch_or_the_tile_shape(batch):
    xyz, radii, offsets = batch
    b, e = int(offsets[6]), int(offsets[7])
    sasa, counts, totals, volumes, evec, vol = device(batch, 100)
    alone = fa.calc_volume(xyz[b:e], radii[b:e], [0, e - b], probe=PROBE, n_points=100, per_atom=True)
    assert alone[3].tobytes() == volumes[6:7].tobytes() and alone[4].tobytes() == evec[b:e].tobytes() and alone[5].tobytes() == vol[b:e].tobytes()
    # "B,TA,records per atom,ds": one-wave tiles of 3 atoms; 256 threads x 8 atoms; and segments of 16 records, which the dense
    # tiles overflow - they store nothing in the main launch and are redone by the second: every vector written once
    for cfg in ("64,3,48,0", "256,8,112,0", "128,5,16,0"):
        got = with_cfg(cfg, lambda: fa.calc_volume(xyz, radii, offsets, probe=PROBE, n_points=100, per_atom=True))
        for a, w in zip(got, (sasa, counts, totals, volumes, evec, vol)):
            assert a.tobytes() == w.tobytes(), cfg


def raw_call(batch, n_points):
    """freesasa_gpu_calc_volume on arrays full of a sentinel -> (rc, message, every output untouched?)"""
    xyz, radii, offsets = batch
    n, ns = len(radii), len(offsets) - 1
    dp = C.POINTER(C.c_double)
    out = [np.full(k, -7.0) for k in (n, 3 * n, n, ns, ns)]
    cnt = np.full(n, -7, dtype=np.int32)
    err = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data_as(dp)
    rc = fa.lib().freesasa_gpu_calc_volume(p(xyz.reshape(-1)), p(radii), offsets.ctypes.data_as(C.POINTER(C.c_int64)), ns, PROBE, n_points, p(out[0]),
                                           cnt.ctypes.data_as(C.POINTER(C.c_int)), p(out[1]), p(out[2]), p(out[3]), p(out[4]), -1, err, 512)
    return rc, err.value.decode(), all(np.all(a == -7.0) for a in out) and np.all(cnt == -7)


def test_refusals_name_the_reason_write_nothing_and_leave_the_context_usable(batch):
    xyz, radii, offsets = batch
    sasa, counts, totals, volumes, evec, vol = device(batch, 100)
    rc, msg, untouched = raw_call(batch, 129)
    assert rc == -1 and "up to 128 test points (129 asked for)" in msg and untouched
    # a tile shape that launch_sr sends to the second arrangement: 136 records per atom (refused before anything is launched)
    rc, msg, untouched = with_cfg("128,6,136,0", lambda: raw_call(batch, 100))
    assert rc == -1 and "this tile shape runs the second arrangement (136 records per atom" in msg and untouched
    # the pooled context the refusals went through serves the next calls
    again = fa.calc_volume(xyz, radii, offsets, probe=PROBE, n_points=100)
    assert again[3].tobytes() == volumes.tobytes()
    want = fa.calc_batch(xyz, radii, offsets, fa.SHRAKE_RUPLEY, probe=PROBE, resolution=129)
    assert np.all(want[0] >= 0)


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, freesasa_amd as fa, volume_ref as vr
xyz, radii, offsets = vr.batch()
try:
    fa.calc_volume(xyz, radii, offsets, n_points=100)
    print("RETURNED")
except RuntimeError as e:
    print("REFUSED", e)
sasa, counts, totals = fa.calc_batch(xyz, radii, offsets, fa.SHRAKE_RUPLEY, resolution=100)
print("TOTAL", repr(float(totals[6])))
"""


def test_refused_without_the_cap_mask_kernel(batch):
    """FREESASA_AMD_SR_CAPS=0 is read when a context first sees a set of test points: a fresh process"""
    env = dict(os.environ, FREESASA_AMD_SR_CAPS="0")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "REFUSED freesasa_gpu_calc_volume: the volume needs the cap-mask kernel, which FREESASA_AMD_SR_CAPS=0 switches off" in r.stdout
    assert "TOTAL " + repr(float(device(batch, 100)[2][6])) in r.stdout            # ... and the ordinary call behind it is the ordinary call


# ---------------------------------------------------------------- trajectories

@pytest.fixture(scope="module")
def system(tmp_path_factory):
    """the first 70 atoms of 1UBQ as the topology; 7 frames of them (frame 0: the file's coordinates, 1-6 a seeded +-0.3 A
    jitter) scattered into frames of 90 atoms (a non-monotonic index), rounded to fp32 so that every input format holds the
    same numbers"""
    src = os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb")
    lines = [l for l in open(src) if l.startswith("ATOM")][:N]
    tmp = tmp_path_factory.mktemp("vol")
    (tmp / "ubq70.pdb").write_text("".join(lines) + "END\n")
    one = ingest.load_pdb_files([str(tmp / "ubq70.pdb")])
    assert one.n_atoms == N
    rng = np.random.default_rng(vr.SEED)
    frames = np.repeat(one.xyz[None], F, 0)
    frames[1:] += rng.uniform(-0.3, 0.3, (F - 1, N, 3))
    index = rng.permutation(FA)[:N].astype(np.int32)
    full = rng.uniform(one.xyz.min(0), one.xyz.max(0), (F, FA, 3))
    full[:, index] = frames
    full32 = full.astype(np.float32)
    assert np.any(np.diff(index) < 0)
    return one, full32, index, tmp


@pytest.fixture(scope="module")
def memory_form(system):
    one, full32, index, _ = system
    kw = dict(atom_index=index, per_atom=True, alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=FPB, devices=[0, 0])
    return fa.trajectory_topology(full32.astype(np.float64), one, volumes=True, **kw), fa.trajectory_topology(full32.astype(np.float64), one, **kw)


def test_trajectory_volumes_equal_calc_volume_of_every_frame(system, memory_form):
    one, full32, index, _ = system
    got, plain = memory_form
    assert plain.volumes is None and got.volumes.shape == (F,)
    frames = full32.astype(np.float64)[:, index]
    for f in range(F):
        sasa, counts, totals, volumes = fa.calc_volume(frames[f], one.radii, [0, N], probe=PROBE, n_points=100)
        assert got.volumes[f] == volumes[0] and got.totals[f] == totals[0] and got.sasa[f].tobytes() == sasa.tobytes()
    assert np.all(got.volumes > 0) and len(set(got.volumes)) == F
    # everything else is the run without volumes, byte for byte
    for k in ("totals", "sasa", "residues", "class_sums"):
        assert getattr(got, k).tobytes() == getattr(plain, k).tobytes(), k


def file_run(tmp, tag, frames_path, one, index, volumes=True, **kw):
    paths = {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "cls", "res", "vol", "done")}
    done, n_frames, _ = fa.trajectory_file_topology(frames_path, one, paths["totals"], atom_index=index, frame_atoms=FA, sasa_path=paths["sasa"],
                                                    class_sums_path=paths["cls"], residues_path=paths["res"],
                                                    volumes_path=paths["vol"] if volumes else None, done_path=paths["done"],
                                                    alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=FPB, **kw)
    return paths, done, n_frames


@pytest.mark.parametrize("fmt", ["f32", "dcd"])
def test_file_forms_resume_on_any_device_list_byte_for_byte(system, memory_form, fmt):
    one, full32, index, tmp = system
    got, _ = memory_form
    path = tmp / f"frames.{fmt}"
    if fmt == "f32":
        full32.tofile(path)
        kw = dict(f32=True)
    else:
        write_dcd(path, full32)
        kw = dict(dcd=True)
    whole, done, n_frames = file_run(tmp, fmt + "-whole", path, one, index, devices=[0], **kw)
    assert done and n_frames == F
    assert " outputs=71" in open(whole["done"]).readline()                         # per-atom 1, class sums 2, residues 4, volumes 64
    assert open(whole["vol"], "rb").read() == got.volumes.tobytes()
    for k, w in (("totals", got.totals), ("sasa", got.sasa), ("cls", got.class_sums), ("res", got.residues)):
        assert open(whole[k], "rb").read() == w.tobytes(), k
    # a shard at a time, on alternating device lists, to the end
    for step, devs in enumerate(([0, 0], [0], [0, 0])):
        part, done, _ = file_run(tmp, fmt + "-part", path, one, index, devices=devs, max_new_shards=1, **kw)
        assert done == (step == 2) and open(part["done"]).read().count("shard ") == step + 1
    for k in ("totals", "sasa", "cls", "res", "vol"):
        assert open(part[k], "rb").read() == open(whole[k], "rb").read(), k


def test_done_lists_with_and_without_the_volume_refuse_each_other(system):
    one, full32, index, tmp = system
    path = tmp / "frames.done.f32"
    full32.tofile(path)
    with_vol, done, _ = file_run(tmp, "dl-vol", path, one, index, devices=[0], f32=True)
    without, done2, _ = file_run(tmp, "dl-plain", path, one, index, volumes=False, devices=[0], f32=True)
    assert done and done2
    assert " outputs=71" in open(with_vol["done"]).readline() and " outputs=7\n" in open(without["done"]).readline()
    before = {k: open(p, "rb").read() for k, p in list(with_vol.items()) + [("p-" + k, p) for k, p in without.items() if os.path.exists(p)]}
    paths = dict(with_vol)
    kw = dict(atom_index=index, frame_atoms=FA, sasa_path=paths["sasa"], class_sums_path=paths["cls"], residues_path=paths["res"],
              alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=FPB, f32=True, devices=[0])
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):      # a volume run's list, a run without
        fa.trajectory_file_topology(path, one, paths["totals"], done_path=with_vol["done"], **kw)
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):      # and the other way round
        fa.trajectory_file_topology(path, one, paths["totals"], done_path=without["done"], volumes_path=paths["vol"], **kw)
    after = {k: open(p, "rb").read() for k, p in list(with_vol.items()) + [("p-" + k, p) for k, p in without.items() if os.path.exists(p)]}
    assert after == before
