"""Periodic images in a triclinic cell (include/freesasa_gpu.h: freesasa_gpu_calc_periodic_triclinic,
FREESASA_GPU_FRAMES_TRICLINIC) without a GPU: the kernels' phase functions (csrc/pbc_tri_kernels.h) driven on the CPU against
the numpy restatement of the definition (tests/pbc_tri_ref.py), byte for byte; their reduction to the orthorhombic kernels;
that restatement against the explicit 5 x 5 x 5 replica system through the oracle; the two host helpers; and the argument
checks that come before a device is touched or an output file opened."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
import pbc_ref
import pbc_tri_ref as tri
from emu import pbc_emu, pbc_tri_emu
from test_dcd import write_dcd

PROBE = 1.4
FOUR_CELLS = {"hexagonal": tri.HEXAGONAL, "octahedral": tri.OCTAHEDRAL, "skewed": tri.SKEWED, "right-angled": (12.0, 0.0, 14.0, 0.0, 0.0, 16.0)}


@pytest.fixture(scope="module")
def batch():
    return tri.batch()


@pytest.fixture(scope="module")
def expanded(batch):
    return tri.expand_batch(*batch, probe=PROBE)


def test_the_batch_is_what_the_kernels_can_go_wrong_on(batch, expanded):
    xyz, radii, offsets, cells6 = batch
    _, _, eoff, images = expanded
    assert list(np.diff(offsets)) == [0, 1, 2, 60, 516]
    # the one atom: widths 6.84, 6.84, 7.0 against c = 6.8 - both shifts on every axis, the nearest image at 7.0 A
    c = tri.cutoff(radii[0:1], PROBE)
    d = tri.widths(cells6[1])
    assert c == 2.0 * (2.0 + 1.4) and np.all(d >= c) and np.all(d < c + 0.21) and images[1] == 26
    ex, _, _ = tri.expand(xyz[0:1], radii[0:1], cells6[1], PROBE)
    assert abs(np.linalg.norm(ex[1:] - ex[0], axis=1).min() - 7.0) < 1e-12
    # the 60 atoms: a skewed cell with widths below 2 c - atoms with both shifts on one axis
    a, b = int(offsets[3]), int(offsets[4])
    c = tri.cutoff(radii[a:b], PROBE)
    d = tri.widths(cells6[3])
    g = tri.frac(tri.wrap(xyz[a:b], cells6[3]), cells6[3])
    both = (g * d < c) & ((1.0 - g) * d < c)
    assert c == 6.8 and np.all(d >= c) and d[0] < 2 * c and both[:, 0].any()
    assert np.all((g >= 0.0) & (g < 1.0))
    # every off-diagonal entry of that cell is at work, and the cell is not reduced
    assert all(cells6[3][k] != 0.0 for k in (1, 3, 4)) and abs(cells6[3][1]) > cells6[3][0] / 2
    # atoms up to 1.5 cells outside, in fractional coordinates, on both sides
    for s in (3, 4):
        q = tri.frac(xyz[offsets[s]:offsets[s + 1]], cells6[s])
        assert q.min() < -0.5 and q.max() > 1.5 and q.min() > -1.5 and q.max() < 2.5
    assert images[0] == 0 and np.all(images[1:] > 0)
    assert images[3] > 4 * 60                                                  # the periodic answer is another system
    print("images", images.tolist(), "widths of the flat cell", tri.widths(cells6[4]).tolist())


def test_emulated_kernels_equal_the_definition_byte_for_byte(batch, expanded):
    xyz, radii, offsets, cells6 = batch
    want_xyz, want_r, want_eoff, want_images = expanded
    got_xyz, got_r, eoff, images, rmax, ibase = pbc_tri_emu.expand(xyz, radii, offsets, tri.cell9(cells6), PROBE)
    assert np.array_equal(images, want_images) and np.array_equal(eoff, want_eoff)
    assert got_xyz.shape == want_xyz.shape
    assert got_xyz.tobytes() == want_xyz.tobytes() and got_r.tobytes() == want_r.tobytes()      # coordinates, radii, order
    for s in range(5):
        a, b = int(offsets[s]), int(offsets[s + 1])
        assert rmax[s] == (radii[a:b].max() if b > a else 0.0)
        if b > a:                                                               # the bases: an exclusive scan in atom order
            per_atom = np.diff(np.concatenate([ibase[a:b], [images[s]]]))
            assert ibase[a] == 0 and np.all(per_atom >= 0) and np.all(per_atom <= 26)
            c, d = tri.cutoff(radii[a:b], PROBE), tri.widths(cells6[s])
            g = tri.frac(tri.wrap(xyz[a:b], cells6[s]), cells6[s])
            assert np.array_equal(per_atom, np.prod(1 + (g * d < c).astype(int) + ((1.0 - g) * d < c).astype(int), axis=1) - 1)
    # collect is the orthorhombic path's, as it is
    fake = np.arange(eoff[-1], dtype=np.float64) + 0.5
    got = pbc_emu.collect(offsets, eoff, fake)
    want = np.concatenate([fake[eoff[s]:eoff[s] + offsets[s + 1] - offsets[s]] for s in range(5)])
    assert np.array_equal(got, want)


def test_emulated_kernels_on_frames_that_share_their_radii():
    """the trajectory lanes' form: no offsets, n atoms per structure, one set of radii, a cell per frame"""
    n, nf = 60, 3
    xyz0, radii = tri.sixty(tri.SKEWED, tri.SEED + 5)
    rng = np.random.default_rng(6)
    frames = np.stack([xyz0 + rng.uniform(-0.3, 0.3, xyz0.shape) for _ in range(nf)])
    cells6 = np.array([(13.0 + 0.3 * f, 9.0 - 0.5 * f, 12.0, -11.0 + f, 7.0, 15.0 - 0.2 * f) for f in range(nf)])
    got_xyz, got_r, eoff, images, _, _ = pbc_tri_emu.expand(frames, radii, None, tri.cell9(cells6), PROBE, n_fixed=n)
    for f in range(nf):
        x, r, k = tri.expand(frames[f], radii, cells6[f], PROBE)
        assert k > 0 and images[f] == k and eoff[f + 1] - eoff[f] == n + k
        assert got_xyz[eoff[f]:eoff[f + 1]].tobytes() == x.tobytes() and got_r[eoff[f]:eoff[f + 1]].tobytes() == r.tobytes()
    assert len(set(images.tolist())) > 1


def test_right_angled_cells_reduce_to_the_orthorhombic_kernels():
    """tests/pbc_ref.py's batch with its cells written as (Lx, 0, Ly, 0, 0, Lz): the triclinic kernels give the bytes of the
    orthorhombic definition - and the orthorhombic kernels, built from the same sources into this emulation, still do"""
    xyz, radii, offsets, cells = pbc_ref.batch()
    want_xyz, want_r, want_eoff, want_images = pbc_ref.expand_batch(xyz, radii, offsets, cells, PROBE)
    cells6 = np.zeros((5, 6))
    cells6[:, 0], cells6[:, 2], cells6[:, 5] = cells[:, 0], cells[:, 1], cells[:, 2]
    for h, L in zip(cells6, cells):
        assert fa.cell_widths(h).tobytes() == L.tobytes() and tri.widths(h).tobytes() == L.tobytes()
    got_xyz, got_r, eoff, images, _, _ = pbc_tri_emu.expand(xyz, radii, offsets, tri.cell9(cells6), PROBE)
    assert np.array_equal(images, want_images) and np.array_equal(eoff, want_eoff)
    assert got_xyz.tobytes() == want_xyz.tobytes() and got_r.tobytes() == want_r.tobytes()
    old_xyz, old_r, old_eoff, old_images, _, _ = pbc_tri_emu.expand(xyz, radii, offsets, cells, PROBE, orthorhombic=True)
    assert np.array_equal(old_images, want_images) and old_xyz.tobytes() == want_xyz.tobytes() and old_r.tobytes() == want_r.tobytes()
    # ... and the numpy restatements agree with each other
    t_xyz, t_r, t_eoff, t_images = tri.expand_batch(xyz, radii, offsets, cells6, PROBE)
    assert t_xyz.tobytes() == want_xyz.tobytes() and t_r.tobytes() == want_r.tobytes() and np.array_equal(t_images, want_images)


@pytest.mark.parametrize("case", ["hexagonal", "octahedral", "skewed"])
def test_the_yardstick_equals_the_explicit_125_replica_system(oracle_lib, case):
    """tests/pbc_tri_ref.py's expansion through the oracle against the central cell of the 5 x 5 x 5 replicas: S&R-100 exactly,
    L&R-20 within 1e-8 A^2 per atom (the project's asserted L&R bound on ordinary inputs)"""
    h = FOUR_CELLS[case]
    x, r = tri.sixty(h)
    n = r.size
    ex, er, k = tri.expand(x, r, h, PROBE)
    rx, rr = tri.replicas(x, r, h)
    assert 0 < k < 26 * n and rr.size == 125 * n
    sr_e, _ = oracle_lib.shrake_rupley(ex, er, PROBE, 100)
    sr_r, _ = oracle_lib.shrake_rupley(rx, rr, PROBE, 100)
    assert np.array_equal(sr_e[:n], sr_r[:n])
    lr_e = oracle_lib.lee_richards(ex, er, PROBE, 20)
    lr_r = oracle_lib.lee_richards(rx, rr, PROBE, 20)
    print(f"{case}: images {k}, L&R max |expansion - replicas| = {np.max(np.abs(lr_e[:n] - lr_r[:n])):.3e} A^2")
    assert np.max(np.abs(lr_e[:n] - lr_r[:n])) <= 1e-8
    # ... and it is another number than the non-periodic one
    lr_0 = oracle_lib.lee_richards(tri.wrap(x, h), r, PROBE, 20)
    print(f"{case}: non-periodic {lr_0.sum():.2f}, periodic {lr_e[:n].sum():.2f} A^2")
    assert lr_0.sum() > lr_e[:n].sum() + 100.0


# ---------------------------------------------------------------- the host helpers

def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_cell_from_dcd():
    # cosines: the numpy formula bit for bit
    for rec in [(18.0, 1.0 / 3.0, 18.0, -1.0 / 3.0, 1.0 / 3.0, 18.0), (14.0, -0.5, 14.0, 0.0, 0.0, 16.0), (13.0, 0.6, 15.0, -0.55, 0.12, 19.5),
                (20.0, 1e-3, 21.0, -0.999, 0.01, 22.0)]:
        want = tri.cell_from_cosines(*rec)
        assert np.all(np.isfinite(want)) and fa.cell_from_dcd(rec).tobytes() == want.tobytes()
    # degrees: within 4 ulp per entry of the formula on numpy's cosines (numpy's cos need not be the C library's)
    for rec in [(18.0, 70.528779, 18.0, 109.471221, 70.528779, 18.0), (14.0, 120.0, 14.0, 90.0, 90.0, 16.0), (13.0, 53.13, 15.0, 123.4, 83.1, 19.5),
                (20.0, 1.5, 21.0, 91.0, 90.5, 22.0)]:
        A, g, B, b, a, Cc = rec
        cos = [0.0 if abs(v - 90.0) <= 1e-4 else np.cos(np.float64(v) * np.pi / 180.0) for v in (g, b, a)]
        want = tri.cell_from_cosines(A, cos[0], B, cos[1], cos[2], Cc)
        got = fa.cell_from_dcd(rec)
        assert np.all(ulps(got, want)[want != 0.0] <= 4.0) and np.all(got[want == 0.0] == 0.0), (rec, got, want)
    # right angles in either form: (A, 0, B, 0, 0, C) exactly
    for ang in [(0.0, 0.0, 0.0), (90.0, 90.0, 90.0), (1e-6, -1e-6, 0.0), (90.00009, 89.99991, 90.0), (0.0, 90.0, -1e-7)]:
        got = fa.cell_from_dcd((12.3, ang[0], 45.6, ang[1], ang[2], 7.89))
        assert got.tobytes() == np.array([12.3, 0.0, 45.6, 0.0, 0.0, 7.89]).tobytes() and not np.signbit(got).any()
    # refusals
    for rec, why in [((10.0, 0.0, 10.0, 180.0, 90.0, 10.0), "neither a cosine nor degrees"), ((10.0, 181.0, 10.0, 90.0, 90.0, 10.0), "neither"),
                     ((10.0, -30.0, 10.0, 90.0, 90.0, 10.0), "neither"), ((10.0, np.nan, 10.0, 90.0, 90.0, 10.0), "neither"),
                     ((10.0, 10.0, 10.0, 10.0, 170.0, 10.0), "span no cell"),      # alpha > beta + gamma
                     ((10.0, 130.0, 10.0, 140.0, 100.0, 10.0), "span no cell"),    # the three add up to more than 360
                     ((10.0, 1.0, 10.0, 0.0, 0.0, 10.0), "span no cell"),          # cosine 1: b along a
                     ((10.0, 90.0, np.nan, 90.0, 90.0, 10.0), "edge B .* not finite"), ((np.inf, 90.0, 10.0, 90.0, 90.0, 10.0), "edge A .* not finite")]:
        with pytest.raises(ValueError, match=why):
            fa.cell_from_dcd(rec)
    with pytest.raises(ValueError, match="six numbers"):
        fa.cell_from_dcd((1.0, 2.0, 3.0))


def test_cell_widths():
    """the widths are the distances between opposite faces: V / |b x c|, V / |c x a|, V / |a x b|"""
    for name, h in FOUR_CELLS.items():
        a, b, c = tri.matrix(h)
        V = abs(np.dot(a, np.cross(b, c)))
        want = np.array([V / np.linalg.norm(np.cross(b, c)), V / np.linalg.norm(np.cross(c, a)), V / np.linalg.norm(np.cross(a, b))])
        got = fa.cell_widths(h)
        assert got.tobytes() == tri.widths(h).tobytes(), name
        assert np.all(np.abs(got - want) <= 1e-12 * want), (name, got, want)
    assert fa.cell_widths((12.0, 0.0, 14.0, 0.0, 0.0, 16.0)).tobytes() == np.array([12.0, 14.0, 16.0]).tobytes()
    for bad in [(12.0, 0.0, 0.0, 0.0, 0.0, 16.0), (-12.0, 0.0, 14.0, 0.0, 0.0, 16.0), (12.0, np.nan, 14.0, 0.0, 0.0, 16.0), (12.0, 0.0, 14.0, 0.0, np.inf, 16.0)]:
        with pytest.raises(ValueError):
            fa.cell_widths(bad)
    with pytest.raises(ValueError, match="six numbers"):
        fa.cell_widths((1.0, 2.0, 3.0))


def test_cell_helpers_under_sanitizers_stand_alone():
    """csrc/cell.c compiled with -fsanitize=address,undefined into a program of its own, run as a child process over records that
    decode and records that are refused (with a reason buffer of 256 bytes, of 8 bytes and none): exit status 0, no sanitizer
    report, the library's numbers bit for bit and its verdicts"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/cell_check"], check=True, stdout=subprocess.DEVNULL)
    records = [(18.0, 1.0 / 3.0, 18.0, -1.0 / 3.0, 1.0 / 3.0, 18.0), (14.0, 120.0, 14.0, 90.0, 90.0, 16.0), (12.3, 0.0, 45.6, 90.0, -1e-7, 7.89),
               (13.0, 53.13, 15.0, 123.4, 83.1, 19.5), (-13.0, 60.0, 15.0, 80.0, 70.0, 19.5), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
               (10.0, 10.0, 10.0, 10.0, 170.0, 10.0), (10.0, 180.0, 10.0, 90.0, 90.0, 10.0), (10.0, float("nan"), 10.0, 90.0, 90.0, 10.0),
               (float("inf"), 90.0, 10.0, 90.0, 90.0, 10.0), (1e308, 60.0, 1e308, 60.0, 60.0, 1e308), (1e-320, 0.5, 1e-320, 0.5, 0.5, 1e-320)]
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "cell_check")] + [repr(float(v)) for rec in records for v in rec],
                         capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(records)
    seen = set()
    for rec, line in zip(records, lines):
        word = line.split()
        try:
            h = fa.cell_from_dcd(rec)
        except ValueError as e:
            assert word[0] == "refused" and line[len("refused "):] in str(e), (rec, line)
            seen.add("refused")
            continue
        assert word[0] == "ok" and [float.fromhex(w) for w in word[1:7]] == h.tolist(), (rec, line)
        try:
            d = fa.cell_widths(h)
        except ValueError:
            assert word[8] == "refused", (rec, line)
            seen.add("no widths")
            continue
        assert [float.fromhex(w) for w in word[8:11]] == d.tolist(), (rec, line)
        seen.add("ok")
    assert seen == {"ok", "refused", "no widths"}


# ---------------------------------------------------------------- refusals that need no device

def paths(tmp, tag):
    return {k: str(tmp / f"{tag}.{k}") for k in ("totals", "sasa", "done")}


def test_calc_periodic_triclinic_refusals_before_a_device_is_touched(batch):
    xyz, radii, offsets, cells6 = batch
    # a width below c names the structure and the axis: the octahedral cell scaled until its width a is c - 0.01
    c = tri.cutoff(radii[offsets[2]:offsets[3]], PROBE)
    bad = cells6.copy()
    bad[2] *= (c - 0.01) / tri.widths(cells6[2])[0]
    assert tri.widths(bad[2])[0] < c < np.linalg.norm(tri.matrix(bad[2]), axis=1).min()   # (every EDGE is longer than c)
    with pytest.raises(RuntimeError, match=r"structure 2: width a of its cell is .* smaller than c"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, bad, probe=PROBE)
    bad = cells6.copy()
    bad[4] = (30.0, 4.0, 9.0, -7.0, 45.0, 9.1)                                            # by, cz > c, the width b is not
    with pytest.raises(RuntimeError, match=r"structure 4: width b of its cell"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, bad, probe=PROBE)
    bad = cells6.copy()
    bad[3][2] = 0.0
    with pytest.raises(RuntimeError, match=r"structure 3: entry by of its cell is 0: ax, by and cz must be > 0"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, bad, probe=PROBE)
    bad[3][2] = -12.0
    with pytest.raises(RuntimeError, match=r"structure 3: entry by of its cell is -12"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, bad, probe=PROBE)
    bad = cells6.copy()
    bad[3][4] = np.inf
    with pytest.raises(RuntimeError, match=r"structure 3: entry cy .* not finite"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, bad, probe=PROBE)
    bad = cells6.copy()
    bad[4][1] = np.nan
    with pytest.raises(RuntimeError, match=r"structure 4: entry bx .* not finite"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, bad, probe=PROBE)
    # a structure without atoms has no cell to check
    odd = cells6.copy()
    odd[0] = np.nan
    odd[1][0] = 1.0
    with pytest.raises(RuntimeError, match=r"structure 1: width a"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, odd, probe=PROBE)
    # cells6 of the wrong size
    with pytest.raises(ValueError, match="six numbers per structure"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, cells6[:, :3], probe=PROBE)
    with pytest.raises(ValueError, match="six numbers per structure"):
        fa.calc_periodic_triclinic(xyz, radii, offsets, cells6[:4], probe=PROBE)
    # the engine's 2^30 limit, from the offsets alone: no array is read (these hold one atom)
    with pytest.raises(RuntimeError, match="expanded batch is too large"):
        fa.calc_periodic_triclinic(np.zeros(3), np.ones(1), [0, (1 << 30) + 1], [tri.HEXAGONAL], probe=PROBE)


def test_file_driver_refusals_before_a_device_is_touched(tmp_path):
    rng = np.random.default_rng(1)
    frames = rng.uniform(100.0, 900.0, (3, 7, 3)).astype(np.float32)
    radii = np.full(7, 1.7)
    write_dcd(tmp_path / "cell.dcd", frames, cell=True)
    # bit 4 without bit 3, with and without bit 2
    p = paths(tmp_path, "no3")
    with pytest.raises(RuntimeError, match="bit 4 of frames_f32 .* needs bit 3 .* and bit 2"):
        fa.trajectory_file(tmp_path / "cell.dcd", radii, p["totals"], p["sasa"], done_path=p["done"], dcd=True, triclinic=True)
    frames.tofile(tmp_path / "frames.f32")
    q = paths(tmp_path, "raw")
    with pytest.raises(RuntimeError, match="bit 4 of frames_f32 .* needs bit 3 .* and bit 2"):
        fa.trajectory_file(tmp_path / "frames.f32", radii, q["totals"], q["sasa"], done_path=q["done"], f32=True, triclinic=True)
    # bits 3 and 4 without bit 2: the refusal bit 3 has always had
    with pytest.raises(RuntimeError, match="bit 3 of frames_f32 .* needs bit 2"):
        fa.trajectory_file(tmp_path / "frames.f32", radii, q["totals"], q["sasa"], done_path=q["done"], f32=True, pbc=True, triclinic=True)
    # a DCD file without a cell record
    write_dcd(tmp_path / "nocell.dcd", frames)
    r = paths(tmp_path, "nocell")
    with pytest.raises(RuntimeError, match="unit-cell record"):
        fa.trajectory_file(tmp_path / "nocell.dcd", radii, r["totals"], r["sasa"], done_path=r["done"], dcd=True, pbc=True, triclinic=True)
    assert not any(os.path.exists(f) for f in list(p.values()) + list(q.values()) + list(r.values())), "an output file was opened"


def test_chain_groups_refuse_triclinic_cells(tmp_path):
    b = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "2jo4.pdb")])
    n = int(b.n_atoms)
    write_dcd(tmp_path / "f.dcd", np.asarray(b.xyz, dtype=np.float32)[None] + 500.0, cell=True)
    with pytest.raises(RuntimeError, match="bit 4 of frames_f32 .* not offered with chain groups"):
        fa.trajectory_file_topology(tmp_path / "f.dcd", b, str(tmp_path / "t"), group=np.zeros(n, dtype=np.int32), n_groups=1,
                                    group_areas_path=str(tmp_path / "g"), dcd=True, pbc=True, triclinic=True)
    assert not os.path.exists(tmp_path / "t") and not os.path.exists(tmp_path / "g")
