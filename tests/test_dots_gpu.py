"""Exposure masks and surface dots on the device (freesasa_gpu_calc_masks / freesasa_gpu_sr_masks_dev, freesasa_gpu_dots_count_dev /
freesasa_gpu_dots_expand_dev / freesasa_gpu_dots_from_masks and the mask output of the trajectory topology entries).  The
yardsticks are tests/volume_ref.py's exposed_mask - on the seeded batch its counts are the engine's on every atom
(tests/test_volume.py holds that against the oracle) - and the numpy restatement of the dots (tests/dots_ref.py); everything is
compared BIT FOR BIT, areas, counts and totals against calc_batch byte for byte.  The trajectory entries are held to calc_masks
on every frame."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import dots_ref as dr
import volume_ref as vr
from test_dcd import write_dcd
from test_volume_gpu import system, with_cfg, F, N, FA, FPB  # noqa: F401 (the trajectory tests' topology and frames)

pytestmark = pytest.mark.gpu

PROBE = 1.4


@pytest.fixture(scope="module")
def batch():
    return vr.batch()


_REF, _GOT = {}, {}


def reference_masks(batch, n_points):
    if n_points not in _REF:
        xyz, radii, offsets = batch
        unit = fa.test_points(n_points)
        rows = [vr.exposed_mask(xyz[b:e], radii[b:e] + PROBE, unit) for b, e in zip(offsets[:-1], offsets[1:]) if e > b]
        _REF[n_points] = dr.masks_of(np.concatenate(rows))
    return _REF[n_points]


def device(batch, n_points):
    """calc_masks on the batch, once per point count: (sasa, counts, totals, masks)"""
    if n_points not in _GOT:
        _GOT[n_points] = fa.calc_masks(*batch, probe=PROBE, n_points=n_points)
    return _GOT[n_points]


@pytest.mark.parametrize("n_points", vr.POINT_COUNTS)
def test_the_masks_of_the_batch_equal_the_definition_bit_for_bit(batch, n_points):
    xyz, radii, offsets = batch
    sasa, counts, totals, masks = device(batch, n_points)
    want_sasa, want_counts, want_totals = fa.calc_batch(xyz, radii, offsets, fa.SHRAKE_RUPLEY, probe=PROBE, resolution=n_points)
    assert sasa.tobytes() == want_sasa.tobytes() and counts.tobytes() == want_counts.tobytes() and totals.tobytes() == want_totals.tobytes()
    assert masks.dtype == np.uint32 and masks.shape == (len(radii), 4)
    assert masks.tobytes() == reference_masks(batch, n_points).tobytes()
    assert np.array_equal(dr.popcounts(masks, n_points), counts) and not np.any(masks & ~dr.full_words(n_points))
    assert not masks[6].any()                                                 # the atom wholly inside another
    assert np.array_equal(masks[0], dr.full_words(n_points))                  # the lone atom


def test_the_device_pointer_entries(batch):
    import torch
    xyz, radii, offsets = batch
    sasa, counts, totals, masks = device(batch, 100)
    dev = torch.device("cuda:0")
    n, ns = len(radii), len(offsets) - 1
    d_xyz, d_r = torch.from_numpy(xyz.reshape(-1)).to(dev), torch.from_numpy(radii).to(dev)
    d_sasa, d_tot = torch.full((n,), -7.0, dtype=torch.float64, device=dev), torch.full((ns,), -7.0, dtype=torch.float64, device=dev)
    d_counts = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_masks = torch.full((n, 4), -7, dtype=torch.int32, device=dev)
    as_u32 = lambda t: t.cpu().numpy().view(np.uint32)
    ctx = fa.GpuContext(0)
    try:
        # only what is required, then everything
        ctx.masks(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_masks.data_ptr(), probe=PROBE)
        assert d_sasa.cpu().numpy().tobytes() == sasa.tobytes() and as_u32(d_masks).tobytes() == masks.tobytes()
        assert np.all(d_counts.cpu().numpy() == -7) and np.all(d_tot.cpu().numpy() == -7.0)
        d_masks.fill_(-7)
        ctx.masks(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_masks.data_ptr(), d_counts.data_ptr(), d_tot.data_ptr(), probe=PROBE)
        assert as_u32(d_masks).tobytes() == masks.tobytes()
        assert d_counts.cpu().numpy().tobytes() == counts.tobytes() and d_tot.cpu().numpy().tobytes() == totals.tobytes()
        # refused: -1 with the reason, the sentinel-filled outputs untouched, the context good for an ordinary batch
        for t in (d_sasa, d_tot):
            t.fill_(-7.0)
        for t in (d_counts, d_masks):
            t.fill_(-7)

        def untouched():
            return (np.all(d_sasa.cpu().numpy() == -7.0) and np.all(d_tot.cpu().numpy() == -7.0) and np.all(d_counts.cpu().numpy() == -7)
                    and np.all(d_masks.cpu().numpy() == -7))

        all_out = (d_counts.data_ptr(), d_tot.data_ptr())
        with pytest.raises(RuntimeError, match="exposure masks are offered up to 128 test points .129 asked for"):
            ctx.masks(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_masks.data_ptr(), *all_out, probe=PROBE, n_points=129)
        assert untouched()
        with pytest.raises(RuntimeError, match="n_points must be > 0"):
            ctx.masks(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_masks.data_ptr(), *all_out, probe=PROBE, n_points=0)
        assert untouched()
        with pytest.raises(RuntimeError, match="null argument"):
            ctx.masks(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), 0, *all_out, probe=PROBE)
        assert untouched()
        with pytest.raises(RuntimeError, match="aligned to 16 bytes"):
            ctx.masks(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_masks.data_ptr() + 4, *all_out, probe=PROBE)
        assert untouched()
        ctx.shrake_rupley(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_sasa.data_ptr(), d_counts.data_ptr(), probe=PROBE, n_points=100)
        assert d_sasa.cpu().numpy().tobytes() == sasa.tobytes() and d_counts.cpu().numpy().tobytes() == counts.tobytes()
        assert np.all(d_masks.cpu().numpy() == -7)
    finally:
        ctx.close()


def test_masks_do_not_depend_on_the_batch_or_the_tile_shape(batch):
    xyz, radii, offsets = batch
    b, e = int(offsets[6]), int(offsets[7])
    sasa, counts, totals, masks = device(batch, 100)
    alone = fa.calc_masks(xyz[b:e], radii[b:e], [0, e - b], probe=PROBE, n_points=100)
    assert alone[3].tobytes() == masks[b:e].tobytes() and alone[0].tobytes() == sasa[b:e].tobytes()
    # "B,TA,records per atom,ds": one-wave tiles of 3 atoms; 256 threads x 8 atoms; and segments of 16 records, which the dense
    # tiles overflow - they store nothing in the main launch and are redone by the second: every mask written once
    for cfg in ("64,3,48,0", "256,8,112,0", "128,5,16,0"):
        got = with_cfg(cfg, lambda: fa.calc_masks(xyz, radii, offsets, probe=PROBE, n_points=100))
        for a, w in zip(got, (sasa, counts, totals, masks)):
            assert a.tobytes() == w.tobytes(), cfg


def raw_call(batch, n_points):
    """freesasa_gpu_calc_masks on arrays full of a sentinel -> (rc, message, every output untouched?)"""
    xyz, radii, offsets = batch
    n, ns = len(radii), len(offsets) - 1
    dp = C.POINTER(C.c_double)
    sasa, totals = np.full(n, -7.0), np.full(ns, -7.0)
    cnt, masks = np.full(n, -7, dtype=np.int32), np.full((n, 4), 7, dtype=np.uint32)
    err = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data_as(dp)
    rc = fa.lib().freesasa_gpu_calc_masks(p(xyz.reshape(-1)), p(radii), offsets.ctypes.data_as(C.POINTER(C.c_int64)), ns, PROBE, n_points, p(sasa),
                                          cnt.ctypes.data_as(C.POINTER(C.c_int)), p(totals), masks.ctypes.data_as(C.POINTER(C.c_uint32)), -1, err, 512)
    return rc, err.value.decode(), bool(np.all(sasa == -7.0) and np.all(totals == -7.0) and np.all(cnt == -7) and np.all(masks == 7))


def test_refusals_name_the_reason_write_nothing_and_leave_the_context_usable(batch):
    xyz, radii, offsets = batch
    sasa, counts, totals, masks = device(batch, 100)
    rc, msg, untouched = raw_call(batch, 129)
    assert rc == -1 and "the exposure masks are offered up to 128 test points (129 asked for)" in msg and untouched
    # a tile shape that launch_sr sends to the second arrangement: 136 records per atom (refused before anything is launched)
    rc, msg, untouched = with_cfg("128,6,136,0", lambda: raw_call(batch, 100))
    assert rc == -1 and "the exposure masks need the cap-mask kernel, and this tile shape runs the second arrangement (136 records per atom" in msg and untouched
    again = fa.calc_masks(xyz, radii, offsets, probe=PROBE, n_points=100)
    assert again[3].tobytes() == masks.tobytes()
    want = fa.calc_batch(xyz, radii, offsets, fa.SHRAKE_RUPLEY, probe=PROBE, resolution=129)
    assert np.all(want[0] >= 0)


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, freesasa_amd as fa, volume_ref as vr
xyz, radii, offsets = vr.batch()
try:
    fa.calc_masks(xyz, radii, offsets, n_points=100)
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
    assert "REFUSED freesasa_gpu_calc_masks: the exposure masks need the cap-mask kernel, which FREESASA_AMD_SR_CAPS=0 switches off" in r.stdout
    assert "TOTAL " + repr(float(device(batch, 100)[2][6])) in r.stdout            # ... and the ordinary call behind it is the ordinary call


SHAPE_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, freesasa_amd as fa, volume_ref as vr
xyz, radii, offsets = vr.batch()
sasa, counts, totals, masks = fa.calc_masks(xyz, radii, offsets, n_points=100)
b, e = int(offsets[5]), int(offsets[6])
alone = fa.calc_masks(xyz[b:e], radii[b:e], [0, e - b], n_points=100)
assert alone[3].tobytes() == masks[b:e].tobytes()
sys.stdout.write("MASKS " + masks.tobytes().hex() + "\\n")
"""


@pytest.mark.parametrize("cfg", ["64,3,48,0", "128,5,16,0"])
def test_masks_under_a_tile_shape_set_for_a_whole_process(batch, cfg):
    """FREESASA_AMD_CFG from the first batch of a process on: the masks are the default shape's"""
    env = dict(os.environ, FREESASA_AMD_CFG=cfg)
    r = subprocess.run([sys.executable, "-c", SHAPE_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "MASKS " + device(batch, 100)[3].tobytes().hex() in r.stdout


# ---------------------------------------------------------------- the scan and the expansion without the engine

def scan_on_device(ctx, masks, n_points):
    import torch
    d_masks = torch.from_numpy(masks.view(np.int32)).to("cuda:0")
    d_first = torch.full((len(masks) + 1,), -7, dtype=torch.int64, device="cuda:0")
    D = ctx.dots_count(d_masks.data_ptr(), len(masks), d_first.data_ptr(), n_points=n_points)
    return D, d_first.cpu().numpy()


def test_the_scan_on_synthetic_masks():
    B, T = 1024, 256                                    # DOTS_SCAN_B, DOTS_SCAN_T (tests/test_dots.py reads them from the emulation)
    ctx = fa.GpuContext(0)
    try:
        for k, n in enumerate((1, B - 1, B, B + 1, 2 * B + 3, B * T + 1)):
            rng = np.random.default_rng(200 + k)
            masks = dr.random_masks(rng, n, 100, stray=True)
            D, first = scan_on_device(ctx, masks, 100)
            want = dr.dot_first(masks, 100)
            assert np.array_equal(first, want) and D == want[-1], n
        D, first = scan_on_device(ctx, np.zeros((2 * B + 3, 4), dtype=np.uint32), 100)
        assert D == 0 and not first.any()
        import torch
        with pytest.raises(RuntimeError, match="null argument"):
            ctx.dots_count(0, 5, 0)
        d = torch.zeros(64, dtype=torch.int64, device="cuda:0")
        with pytest.raises(RuntimeError, match="n_atoms must be > 0"):
            ctx.dots_count(d.data_ptr(), 0, d.data_ptr())
        with pytest.raises(RuntimeError, match="hold up to 128 test points"):
            ctx.dots_count(d.data_ptr(), 2, d.data_ptr(), n_points=129)
    finally:
        ctx.close()


def test_the_scan_beyond_two_to_the_31_dots():
    """2^24 + 5 atoms with all 128 bits set: D = 128 (2^24 + 5) > 2^31, the smallest input at which a 32-bit sum goes wrong"""
    import torch
    n = (1 << 24) + 5
    d_masks = torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0")
    d_first = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    ctx = fa.GpuContext(0)
    try:
        D = ctx.dots_count(d_masks.data_ptr(), n, d_first.data_ptr(), n_points=128)
        assert D == 128 * n and D > (1 << 31)
        at = [0, 1, 1023, 1024, n // 2, (1 << 24) - 1, 1 << 24, n - 1, n]
        got = d_first[torch.tensor(at, device="cuda:0")].cpu().numpy()
        assert list(got) == [128 * i for i in at]
        assert bool((d_first[1:] - d_first[:-1] == 128).all())
        # ... and with 100 points the 28 stray bits of every atom are not counted
        assert ctx.dots_count(d_masks.data_ptr(), n, d_first.data_ptr(), n_points=100) == 100 * n
    finally:
        ctx.close()


def expand_on_device(ctx, xyz, radii, masks, n_points, short=0, guard=16):
    """scan and expansion -> (D, dot_first, dot_xyz, dot_atom, dot_point), the arrays `guard` dots longer than the capacity D - short"""
    import torch
    dev = "cuda:0"
    d_xyz, d_r = torch.from_numpy(np.ascontiguousarray(xyz).reshape(-1)).to(dev), torch.from_numpy(radii).to(dev)
    d_masks = torch.from_numpy(masks.view(np.int32)).to(dev)
    d_first = torch.full((len(masks) + 1,), -7, dtype=torch.int64, device=dev)
    D = ctx.dots_count(d_masks.data_ptr(), len(masks), d_first.data_ptr(), n_points=n_points)
    cap = max(D - short, 0)
    d_dx = torch.full((cap + guard, 3), float("nan"), dtype=torch.float64, device=dev)
    d_da, d_dp = (torch.full((cap + guard,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    ctx.dots_expand(d_xyz.data_ptr(), d_r.data_ptr(), len(masks), d_masks.data_ptr(), d_first.data_ptr(), cap, d_dx.data_ptr(), d_da.data_ptr(),
                    d_dp.data_ptr(), probe=PROBE, n_points=n_points)
    return D, d_first.cpu().numpy(), d_dx.cpu().numpy(), d_da.cpu().numpy(), d_dp.cpu().numpy()


@pytest.mark.parametrize("n_points,stray", [(100, False), (33, True)])
def test_the_expansion_on_synthetic_masks(n_points, stray):
    rng = np.random.default_rng(40 + n_points)
    n = 3001
    xyz, radii, masks = rng.uniform(-50, 50, (n, 3)), rng.uniform(1.0, 2.0, n), dr.random_masks(rng, n, n_points, stray)
    pc = dr.popcounts(masks, n_points)
    assert (pc == 0).any() and (pc == n_points).any()
    want_xyz, want_atom, want_point = dr.dots(xyz, radii, PROBE, fa.test_points(n_points), masks)
    ctx = fa.GpuContext(0)
    try:
        D, first, dx, da, dp = expand_on_device(ctx, xyz, radii, masks, n_points)
        assert D == len(want_xyz) and np.array_equal(first, dr.dot_first(masks, n_points))
        assert dx[:D].tobytes() == want_xyz.tobytes() and np.array_equal(da[:D], want_atom) and np.array_equal(dp[:D], want_point)
        assert np.all(np.isnan(dx[D:])) and np.all(da[D:] == -7) and np.all(dp[D:] == -7)
        # the capacity short by 3: the guard region behind it is intact
        D, first, dx, da, dp = expand_on_device(ctx, xyz, radii, masks, n_points, short=3)
        assert dx[:D - 3].tobytes() == want_xyz[:D - 3].tobytes() and np.array_equal(da[:D - 3], want_atom[:D - 3])
        assert np.all(np.isnan(dx[D - 3:])) and np.all(da[D - 3:] == -7) and np.all(dp[D - 3:] == -7)
        # without the index arrays
        import torch
        d_xyz, d_r = torch.from_numpy(xyz.reshape(-1)).to("cuda:0"), torch.from_numpy(radii).to("cuda:0")
        d_masks, d_first = torch.from_numpy(masks.view(np.int32)).to("cuda:0"), torch.from_numpy(first).to("cuda:0")
        d_dx = torch.zeros((D, 3), dtype=torch.float64, device="cuda:0")
        ctx.dots_expand(d_xyz.data_ptr(), d_r.data_ptr(), n, d_masks.data_ptr(), d_first.data_ptr(), D, d_dx.data_ptr(), probe=PROBE, n_points=n_points)
        assert d_dx.cpu().numpy().tobytes() == want_xyz.tobytes()
        # no dots: nothing is launched, nothing written
        zero = np.zeros((50, 4), dtype=np.uint32)
        D, first, dx, da, dp = expand_on_device(ctx, xyz[:50], radii[:50], zero, n_points)
        assert D == 0 and not first.any() and np.all(np.isnan(dx)) and np.all(da == -7)
    finally:
        ctx.close()


@pytest.mark.parametrize("n_points", [33, 100])
def test_calc_dots_on_the_batch(batch, n_points):
    xyz, radii, offsets = batch
    sasa, counts, totals, masks = device(batch, n_points)
    got = fa.calc_dots(xyz, radii, offsets, probe=PROBE, n_points=n_points, with_index=True)
    assert len(got) == 7 and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], (sasa, counts, totals)))
    dots, dot_offsets, dot_atom, dot_point = got[3:]
    want_xyz, want_atom, want_point = dr.dots(xyz, radii, PROBE, fa.test_points(n_points), reference_masks(batch, n_points))
    assert dots.shape == want_xyz.shape and dots.tobytes() == want_xyz.tobytes()
    assert dot_atom.dtype == np.int32 and np.array_equal(dot_atom, want_atom) and np.array_equal(dot_point, want_point)
    first = dr.dot_first(masks, n_points)
    assert dot_offsets.dtype == np.int64 and np.array_equal(dot_offsets, first[offsets]) and dot_offsets[-1] == len(dots) == counts.sum()
    assert dot_offsets[4] == dot_offsets[5]                                      # the structure without atoms has no dots
    lean = fa.calc_dots(xyz, radii, offsets, probe=PROBE, n_points=n_points)
    assert len(lean) == 5 and lean[3].tobytes() == dots.tobytes() and np.array_equal(lean[4], dot_offsets)
    # from the stored masks alone, and a structure whose every atom is buried but one
    again = fa.dots_from_masks(xyz, radii, masks, len(dots), probe=PROBE, n_points=n_points, with_index=True)
    assert again[0].tobytes() == dots.tobytes() and np.array_equal(again[1], first) and np.array_equal(again[2], dot_atom)
    none = fa.dots_from_masks(xyz[:3], radii[:3], np.zeros((3, 4), dtype=np.uint32), 0, probe=PROBE, n_points=n_points)
    assert none[0].shape == (0, 3) and not none[1].any()


# ---------------------------------------------------------------- trajectories

@pytest.fixture(scope="module")
def memory_form(system):
    one, full32, index, _ = system
    kw = dict(atom_index=index, per_atom=True, alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=FPB, devices=[0, 0])
    return fa.trajectory_topology(full32.astype(np.float64), one, masks=True, **kw), fa.trajectory_topology(full32.astype(np.float64), one, **kw)


def test_trajectory_masks_equal_calc_masks_of_every_frame(system, memory_form):
    one, full32, index, _ = system
    got, plain = memory_form
    assert plain.masks is None and got.masks.shape == (F, N, 4) and got.masks.dtype == np.uint32
    frames = full32.astype(np.float64)[:, index]
    for f in range(F):
        sasa, counts, totals, masks = fa.calc_masks(frames[f], one.radii, [0, N], probe=PROBE, n_points=100)
        assert got.masks[f].tobytes() == masks.tobytes() and got.totals[f] == totals[0] and got.sasa[f].tobytes() == sasa.tobytes()
    assert len({got.masks[f].tobytes() for f in range(F)}) == F
    # everything else is the run without masks, byte for byte
    for k in ("totals", "sasa", "residues", "class_sums"):
        assert getattr(got, k).tobytes() == getattr(plain, k).tobytes(), k


def test_page_locked_output_arrays_receive_the_masks_in_place(system, memory_form):
    """totals, per-atom areas and masks in page-locked arrays: the lanes copy every shard straight to its frames' place (no staging,
    4 bytes a value for the masks, 8 for the others)"""
    import torch
    one, full32, index, _ = system
    got, _ = memory_form
    frames = np.ascontiguousarray(full32.astype(np.float64))
    totals = torch.full((F,), -7.0, dtype=torch.float64).pin_memory()
    sasa = torch.full((F, N), -7.0, dtype=torch.float64).pin_memory()
    masks = torch.full((F, N, 4), -7, dtype=torch.int32).pin_memory()
    cls, res = np.zeros((F, 3)), np.zeros((F, one.n_residues, 6))
    L = fa._topology_proto(fa.lib())
    cb = one._as_c()
    dp = C.POINTER(C.c_double)
    dev = np.zeros(2, dtype=np.int32)
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_masks(frames.ctypes.data_as(dp), F, C.byref(cb), 0, FA, index.ctypes.data_as(C.POINTER(C.c_int32)), None,
                                         fa.SHRAKE_RUPLEY, PROBE, 100, FPB, C.cast(totals.data_ptr(), dp), C.cast(sasa.data_ptr(), dp),
                                         cls.ctypes.data_as(dp), res.ctypes.data_as(dp), None, None,
                                         C.cast(masks.data_ptr(), C.POINTER(C.c_uint32)), dev.ctypes.data_as(C.POINTER(C.c_int)), 2, err, 512)
    assert rc == 0, err.value.decode()
    assert masks.numpy().view(np.uint32).tobytes() == got.masks.tobytes()
    assert totals.numpy().tobytes() == got.totals.tobytes() and sasa.numpy().tobytes() == got.sasa.tobytes()
    assert cls.tobytes() == got.class_sums.tobytes() and res.tobytes() == got.residues.tobytes()


def file_run(tmp, tag, frames_path, one, index, masks=True, **kw):
    paths = {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "cls", "res", "masks", "done")}
    done, n_frames, _ = fa.trajectory_file_topology(frames_path, one, paths["totals"], atom_index=index, frame_atoms=FA, sasa_path=paths["sasa"],
                                                    class_sums_path=paths["cls"], residues_path=paths["res"],
                                                    masks_path=paths["masks"] if masks else None, done_path=paths["done"],
                                                    alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=FPB, **kw)
    return paths, done, n_frames


@pytest.mark.parametrize("fmt", ["f32", "dcd"])
def test_file_forms_resume_on_any_device_list_byte_for_byte(system, memory_form, fmt):
    one, full32, index, tmp = system
    got, _ = memory_form
    path = tmp / f"dots-frames.{fmt}"
    if fmt == "f32":
        full32.tofile(path)
        kw = dict(f32=True)
    else:
        write_dcd(path, full32)
        kw = dict(dcd=True)
    whole, done, n_frames = file_run(tmp, "dots-" + fmt + "-whole", path, one, index, devices=[0], **kw)
    assert done and n_frames == F
    assert " outputs=135" in open(whole["done"]).readline()                        # per-atom 1, class sums 2, residues 4, masks 128
    assert os.path.getsize(whole["masks"]) == 16 * N * F
    assert open(whole["masks"], "rb").read() == got.masks.tobytes()
    for k, w in (("totals", got.totals), ("sasa", got.sasa), ("cls", got.class_sums), ("res", got.residues)):
        assert open(whole[k], "rb").read() == w.tobytes(), k
    # a shard at a time, on alternating device lists, to the end
    for step, devs in enumerate(([0, 0], [0], [0, 0])):
        part, done, _ = file_run(tmp, "dots-" + fmt + "-part", path, one, index, devices=devs, max_new_shards=1, **kw)
        assert done == (step == 2) and open(part["done"]).read().count("shard ") == step + 1
    for k in ("totals", "sasa", "cls", "res", "masks"):
        assert open(part[k], "rb").read() == open(whole[k], "rb").read(), k


def test_done_lists_with_and_without_the_masks_refuse_each_other(system):
    one, full32, index, tmp = system
    path = tmp / "dots-frames.done.f32"
    full32.tofile(path)
    with_masks, done, _ = file_run(tmp, "dots-dl-masks", path, one, index, devices=[0], f32=True)
    without, done2, _ = file_run(tmp, "dots-dl-plain", path, one, index, masks=False, devices=[0], f32=True)
    assert done and done2
    assert " outputs=135" in open(with_masks["done"]).readline() and " outputs=7\n" in open(without["done"]).readline()
    files = list(with_masks.items()) + [("p-" + k, p) for k, p in without.items() if os.path.exists(p)]
    before = {k: open(p, "rb").read() for k, p in files}
    paths = dict(with_masks)
    kw = dict(atom_index=index, frame_atoms=FA, sasa_path=paths["sasa"], class_sums_path=paths["cls"], residues_path=paths["res"],
              alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=FPB, f32=True, devices=[0])
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):      # a mask run's list, a run without
        fa.trajectory_file_topology(path, one, paths["totals"], done_path=with_masks["done"], **kw)
    with pytest.raises(RuntimeError, match="done-list belongs to a run with other"):      # and the other way round
        fa.trajectory_file_topology(path, one, paths["totals"], done_path=without["done"], masks_path=paths["masks"], **kw)
    assert {k: open(p, "rb").read() for k, p in files} == before


def test_refused_trajectory_combinations_give_their_messages(system):
    one, full32, index, tmp = system
    frames = full32.astype(np.float64)
    kw = dict(atom_index=index, frames_per_batch=FPB, devices=[0])
    with pytest.raises(RuntimeError, match="Lee-Richards is not offered"):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.LEE_RICHARDS, **kw)
    with pytest.raises(RuntimeError, match="up to 128 test points .200 asked for"):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=200, **kw)
    with pytest.raises(ValueError, match="not offered with chain groups"):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=100, separate_chains=True, **kw)
    with pytest.raises(ValueError, match="stats="):
        fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=100, stats=("totals",), **kw)
    with pytest.raises(ValueError, match="volumes=True"):
        fa.trajectory_topology(frames, one, masks=True, volumes=True, alg=fa.SHRAKE_RUPLEY, resolution=100, **kw)
    path = tmp / "dots-frames.ref.dcd"
    write_dcd(path, full32)
    for bits in (dict(pbc=True), dict(pbc=True, triclinic=True)):
        with pytest.raises(RuntimeError, match="periodic images. are not offered with the exposure masks"):
            fa.trajectory_file_topology(path, one, str(tmp / "dots-ref.totals"), atom_index=index, frame_atoms=FA, masks_path=str(tmp / "dots-ref.masks"),
                                        done_path=str(tmp / "dots-ref.done"), alg=fa.SHRAKE_RUPLEY, resolution=100, dcd=True, devices=[0], **bits)
    assert not os.path.exists(tmp / "dots-ref.masks") and not os.path.exists(tmp / "dots-ref.done")
    # ... and the run behind the refusals is the ordinary run
    got = fa.trajectory_topology(frames, one, masks=True, alg=fa.SHRAKE_RUPLEY, resolution=100, **kw)
    assert got.masks.shape == (F, N, 4) and got.masks.any()
