"""GROMACS TRR input on the CPU: the pure-Python codec (tests/trr_codec.py) against itself; the host's pass over the records'
headers (freesasa_amd/csrc/trr.c), its index and its refusals, also stand-alone under AddressSanitizer + UBSan; the gather kernel
(traj_kernels.h, traj_gather_trr) driven on the CPU (tests/emu/emu_trr.cpp) against float64(x_nm) * 10.0, bit for bit; the
drivers' argument checks, which come before any device.  No GROMACS-written file is at hand: the codec, written from the
format's description, is the yardstick."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import trr_codec as tc
from emu import trr_emu
from freesasa_amd import ingest


def nm(n, seed, scale=2.0):
    """[n, 3] coordinates in nm that no precision holds exactly"""
    return np.random.default_rng(seed).uniform(-scale, scale, (n, 3)) / 3.0


BOX = np.array([[3.0, 0, 0], [0.5, 3.5, 0], [-0.25, 0.75, 4.0]])


def mixed_records(n, double, lead=True, between=True, tail=True, box0=True):
    """four coordinate frames of unequal length and, where asked, a velocity-only record in front of them, between frames 1 and
    2, and behind them: as nstxout, nstvout and nstfout that differ write them"""
    k = dict(natoms=n, double=double)
    vel = dict(k, v=nm(n, 90), step=-1)
    recs = [dict(k, box=BOX if box0 else None, x=nm(n, 1), v=nm(n, 2), f=nm(n, 3), step=0, t=0.0),
            dict(k, x=nm(n, 4), step=10, t=0.5),
            dict(k, box=BOX * 1.01, vir=BOX, pres=BOX, x=nm(n, 5), v=nm(n, 6), step=20, t=1.0, lam=0.25),
            dict(k, box=BOX, x=nm(n, 7), f=nm(n, 8), step=30, t=1.5)]
    if between:
        recs.insert(2, vel)
    if lead:
        recs.insert(0, vel)
    if tail:
        recs.append(dict(vel, f=nm(n, 91)))
    return recs


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
def test_codec_round_trip(double):
    n = 37
    recs = mixed_records(n, double)
    data = tc.write_trr(None, recs)
    got = tc.decode(data)
    assert len(got) == len(recs) and sum(r.size for r in got) == len(data) and len(data) % 4 == 0
    dt = np.float64 if double else np.float32
    w = 8 if double else 4
    for r, want in zip(got, recs):
        assert r.double == double and r.natoms == n and r.step == want["step"] and r.t == want.get("t", 0.0) and r.lam == want.get("lam", 0.0)
        body = 0
        for name in ("box", "vir", "pres", "x", "v", "f"):
            a, b = getattr(r, name), want.get(name)
            assert (a is None) == (b is None), name
            if a is not None:
                assert a.dtype == dt and np.array_equal(a, np.asarray(b).astype(dt))
                body += a.size * w
        assert r.size == tc.header_bytes(double) + body
    assert tc.header_bytes(False) == 84 and tc.header_bytes(True) == 92
    first_frame = got[1]
    assert first_frame.box_off - first_frame.offset == (92 if double else 84)
    assert first_frame.x_off - first_frame.offset == ((92 + 72) if double else (84 + 36))          # (164: a multiple of 4, not of 8)
    assert tc.frames_angstrom(got).shape == (4, n, 3)
    assert np.array_equal(tc.frames_angstrom(got)[1], np.asarray(recs[2]["x"]).astype(dt).astype(np.float64) * 10.0)
    for cut in (3, 50, 80, got[1].offset + 90, len(data) - 4):
        with pytest.raises(ValueError):
            tc.decode(data[:cut])
    assert len(tc.decode(data[:got[3].offset])) == 3


def index_of(path):
    L = fa.lib()
    L.freesasa_gpu_trr_index_read.argtypes = [C.c_char_p, C.POINTER(fa.TrrInfoC), C.POINTER(C.POINTER(C.c_int64)), C.c_char_p, C.c_int]
    L.freesasa_gpu_trr_index_free.argtypes = [C.POINTER(C.c_int64)]
    info, offs, err = fa.TrrInfoC(), C.POINTER(C.c_int64)(), C.create_string_buffer(512)
    if L.freesasa_gpu_trr_index_read(str(path).encode(), C.byref(info), C.byref(offs), err, 512):
        raise ValueError(err.value.decode())
    got = [offs[k] for k in range(info.n_frames + 1)]
    L.freesasa_gpu_trr_index_free(offs)
    return got


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
@pytest.mark.parametrize("n", [1, 10, 37, 516])
def test_info_and_index(tmp_path, n, double):
    p = tmp_path / "frames.trr"
    for lead, between, tail in ((True, True, True), (False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        data = tc.write_trr(p, mixed_records(n, double, lead, between, tail))
        recs = tc.decode(data)
        starts = [r.offset for r in recs if r.x is not None]
        spans = np.diff(starts + [len(data)])
        assert len(set(r.size for r in recs if r.x is not None)) == 4                               # unequal records
        info = fa.trr_info(p)
        assert (info.n_atoms, info.n_frames, info.n_records, info.real_bytes) == (n, 4, 4 + lead + between + tail, 8 if double else 4)
        assert info.max_frame_bytes == int(spans.max()) and info.has_box and info.has_velocities and info.has_forces
        assert index_of(p) == starts + [len(data)]
        assert (starts[0] > 0) == lead and (spans[1] > recs[2 if lead else 1].size) == between
    assert "n_frames=4" in repr(info) and "real_bytes=%d" % (8 if double else 4) in repr(info)
    # the first coordinate frame without a box, and with one that is all zero; no velocities, no forces
    tc.write_trr(p, mixed_records(n, double, box0=False))
    assert not fa.trr_info(p).has_box
    tc.write_trr(p, [dict(natoms=n, double=double, box=np.zeros((3, 3)), x=nm(n, 1)), dict(natoms=n, double=double, box=BOX, x=nm(n, 2))])
    info = fa.trr_info(p)
    assert not info.has_box and not info.has_velocities and not info.has_forces and (info.n_frames, info.n_records) == (2, 2)


def refused_files(tmp):
    """(name, path, what the message begins with, what it holds): a good file of four records of 12 atoms whose record 2 is replaced"""
    n = 12
    k = dict(natoms=n)
    good = [dict(k, box=BOX, x=nm(n, 1), v=nm(n, 2)), dict(k, v=nm(n, 3)), dict(k, box=BOX, x=nm(n, 4)), dict(k, x=nm(n, 5), f=nm(n, 6))]
    g = good[2]
    rb = tc.record_bytes
    variants = [("magic 7", rb(**g, magic=7), "its magic number is 7, not 1993"),
                ("version string", rb(**g, version=b"GMX_trn_filf"), "its version string is not"),
                ("version length", rb(**g, slen1=12), "its version string is not"),
                ("ir_size", rb(**g, ir_size=4), "its ir_size is 4"), ("e_size", rb(**g, e_size=8), "its e_size is 8"),
                ("top_size", rb(**g, top_size=-4), "its top_size is -4"), ("sym_size", rb(**g, sym_size=4), "its sym_size is 4"),
                ("width 2", rb(**dict(g, box=None), x_size=3 * n * 2), "its reals are 2 bytes wide"),
                ("width 16", rb(**g, box_size=9 * 16), "its reals are 16 bytes wide"),
                ("no part at all", rb(natoms=n), "its reals are 0 bytes wide"),
                ("negative x_size", rb(**dict(g, box=None), x_size=-3 * n * 4), "its reals are -4 bytes wide"),
                ("box_size", rb(**g, box_size=40), "its box_size is 40, not 9 reals of 4 bytes"),
                ("vir_size", rb(**g, vir_size=72), "its vir_size is 72, not 9 reals of 4 bytes"),
                ("pres_size", rb(**g, pres_size=-36), "its pres_size is -36"),
                ("x_size", rb(**g, x_size=3 * n * 4 + 4), "its x_size is 148, not 3 x 12 atoms x 4 bytes"),
                ("v_size", rb(**g, v_size=3 * n * 8), "its v_size is 288"), ("f_size", rb(**g, f_size=4), "its f_size is 4"),
                ("natoms 0", rb(**g, natoms_word=0), "it holds 0 atoms"), ("natoms -5", rb(**g, natoms_word=-5), "it holds -5 atoms"),
                ("other atom count", rb(natoms=11, box=BOX, x=nm(11, 1)), "it holds 11 atoms, record 0 holds 12"),
                ("other precision", rb(**g, double=True), "its reals are 8 bytes wide, record 0's are 4")]
    head = b"".join(rb(**r) for r in good[:2])
    out = []
    for name, third, text in variants:
        p = tmp / (name.replace(" ", "_") + ".trr")
        p.write_bytes(head + third + rb(**good[3]))
        out.append((name, p, "record 2 of the TRR file: ", text))
    for name, cut in (("ends in the magic", 2), ("ends in the version", 20), ("ends in the sizes", 50), ("ends in t", 80), ("ends in the body", 100),
                      ("ends in the last real", len(rb(**g)) - 1)):
        p = tmp / (name.replace(" ", "_") + ".trr")
        p.write_bytes(head + rb(**g)[:cut])
        out.append((name, p, "record 2 of the TRR file: ", "the file ends inside its header" if cut < 84 else "the file ends inside its body"))
    (tmp / "empty.trr").write_bytes(b"")
    out.append(("empty", tmp / "empty.trr", "", "the TRR file holds no coordinate frame"))
    (tmp / "velocities_only.trr").write_bytes(rb(**good[1]) * 3)
    out.append(("velocities only", tmp / "velocities_only.trr", "", "the TRR file holds no coordinate frame: none of its 3 records"))
    (tmp / "good.trr").write_bytes(b"".join(rb(**r) for r in good))
    return out


def test_refusals_each_with_its_own_message_that_names_the_record(tmp_path):
    msgs = {}
    for name, p, record, text in refused_files(tmp_path):
        with pytest.raises(ValueError) as e:
            fa.trr_info(p)
        msg = str(e.value)
        assert record in msg and text in msg, (name, msg)
        msgs[name] = msg
    # the reasons differ from check to check: magic, version, unused part, width, size of 9, size of 3 n, natoms, other atom
    # count, other precision, end in a header, end in a body, no coordinate frame
    kinds = {re.sub(r"-?\d+", "N", re.sub(r"\b\w+_size", "S_size", m.split("file: ", 1)[-1])) for m in msgs.values()}
    assert len(kinds) == 12, sorted(kinds)
    info = fa.trr_info(tmp_path / "good.trr")
    assert (info.n_frames, info.n_records) == (3, 4)
    # a file cut exactly between two records is a shorter file
    data = (tmp_path / "good.trr").read_bytes()
    recs = tc.decode(data)
    (tmp_path / "shorter.trr").write_bytes(data[:recs[3].offset])
    info = fa.trr_info(tmp_path / "shorter.trr")
    assert (info.n_frames, info.n_records) == (2, 3) and index_of(tmp_path / "shorter.trr") == [0, recs[2].offset, recs[3].offset]
    with pytest.raises(ValueError, match="cannot open"):
        fa.trr_info(tmp_path / "none.trr")
    # a short message buffer, and none
    L = fa.lib()
    L.freesasa_gpu_trr_info_read.argtypes = [C.c_char_p, C.POINTER(fa.TrrInfoC), C.c_char_p, C.c_int]
    for name in ("empty.trr", "magic_7.trr", "ends_in_the_body.trr"):
        err = C.create_string_buffer(b"x" * 15, 16)
        assert L.freesasa_gpu_trr_info_read(str(tmp_path / name).encode(), C.byref(fa.TrrInfoC()), err, 8) == -1
        assert len(err.value) == 7 and err.raw[8:15] == b"x" * 7
        assert L.freesasa_gpu_trr_info_read(str(tmp_path / name).encode(), C.byref(fa.TrrInfoC()), None, 0) == -1
        assert L.freesasa_gpu_trr_info_read(str(tmp_path / name).encode(), C.byref(fa.TrrInfoC()), None, 8) == -1


def verdict(p):
    """the line tests/emu/trr_check prints for the file, from the library"""
    try:
        info = fa.trr_info(p)
    except ValueError as e:
        return "refused " + str(e).split(": ", 1)[1]
    words = [info.n_atoms, info.n_frames, info.n_records, info.real_bytes, info.max_frame_bytes, info.has_box, info.has_velocities, info.has_forces]
    return "ok " + " ".join(str(int(v)) for v in words + index_of(p))


def test_header_walker_under_sanitizers_stand_alone(tmp_path):
    """csrc/trr.c compiled with -fsanitize=address,undefined into a program of its own, run as a child process over good files,
    every refused file, a three-record file cut at every length and with every header word of its second record overwritten: exit
    status 0, no sanitizer report, one line of verdict per file - the library's verdict"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/trr_check"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for n in (1, 10, 37, 516):
        for double in (False, True):
            p = tmp_path / f"good{n}_{int(double)}.trr"
            tc.write_trr(p, mixed_records(n, double))
            paths.append(p)
    paths += [p for _, p, _, _ in refused_files(tmp_path)] + [tmp_path / "good.trr", tmp_path / "does_not_exist.trr"]
    fuzz = tmp_path / "fuzz"
    fuzz.mkdir()
    n_words = 0
    for double in (False, True):
        k = dict(natoms=10, double=double)
        good = tc.write_trr(None, [dict(k, box=BOX, x=nm(10, 1)), dict(k, box=BOX, x=nm(10, 2), v=nm(10, 3)), dict(k, x=nm(10, 4), f=nm(10, 5))])
        recs = tc.decode(good)
        whole = {0: None, recs[1].offset: 1, recs[2].offset: 2, len(good): 3}
        for cut in range(len(good)):
            (fuzz / f"cut{int(double)}_{cut}.trr").write_bytes(good[:cut])
            paths.append(fuzz / f"cut{int(double)}_{cut}.trr")
        second = recs[1].offset
        for at in range(second, second + tc.header_bytes(double), 4):
            for v in (0, 0x7fffffff, 0x80000000, 0xffffffff, 0x7fc00000):
                p = fuzz / f"word{int(double)}_{at}_{v:x}.trr"
                p.write_bytes(good[:at] + struct.pack(">I", v) + good[at + 4:])
                paths.append(p)
                n_words += 1
        if double:
            whole_double = whole
        else:
            whole_single = whole
    assert n_words == 5 * (21 + 23)
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "trr_check")] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(paths)
    n_ok = 0
    for line, p in zip(lines, paths):
        assert line == verdict(p), (p, line)
        n_ok += line.startswith("ok ")
    for double, whole in ((0, whole_single), (1, whole_double)):  # a cut between two records is a shorter file, every other one is refused
        for cut in range(max(whole)):
            line = lines[paths.index(fuzz / f"cut{double}_{cut}.trr")]
            assert line.startswith("ok 10 %d %d " % (whole[cut], whole[cut])) if whole.get(cut) else line.startswith("refused "), (cut, line)
    assert n_ok >= 8 + 1 + 4 + 2 * 3 * 5                          # (good files; the cuts between records; step, nre, t, lambda: harmless words)


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
def test_emulated_gather_equals_float64_nm_times_ten(double):
    """traj_gather_trr thread by thread over a shard of unequal records, some without coordinates, 37 atoms (odd: 3 * 37 reals),
    the identity and a shuffled index that keeps 20 atoms: float64(x_nm) * 10.0, bit for bit, every element written"""
    n = 37
    data = tc.write_trr(None, mixed_records(n, double))
    recs = tc.decode(data)
    frames = [r for r in recs if r.x is not None]
    assert len({r.x_off - r.offset for r in frames}) > 1 and len({r.size for r in frames}) == 4
    assert not double or any(r.x_off % 8 == 4 for r in frames)                                      # offsets that are no multiple of 8
    want = tc.frames_angstrom(recs)
    assert want.dtype == np.float64 and want.shape == (4, n, 3)
    if not double:
        assert np.array_equal(want, np.array([r.x for r in frames]).astype(np.float64) * 10.0) and frames[0].x.dtype == np.float32
    shard = data[frames[0].offset:]                                                                 # (as the driver cuts it: from a frame's first byte)
    got = trr_emu.gather(shard, n, 4)
    assert not np.isnan(got).any() and got.tobytes() == want.tobytes()
    index = np.random.default_rng(5).permutation(n)[:20].astype(np.int32)
    got = trr_emu.gather(shard, n, 4, index)
    assert got.shape == (4, 20, 3) and not np.isnan(got).any() and got.tobytes() == want[:, index].tobytes()
    # a middle shard: frames 1 and 2 with the velocity-only record between them
    got = trr_emu.gather(data[frames[1].offset:frames[3].offset], n, 2, index)
    assert got.tobytes() == want[1:3, index].tobytes()
    # one rounding for a double, none for a float: against exact arithmetic on a few values
    from fractions import Fraction
    for v, g in zip(frames[2].x.reshape(-1)[:12], want[2].reshape(-1)[:12]):
        exact = Fraction(float(v)) * 10
        assert (Fraction(float(g)) == exact) if not double else abs(Fraction(float(g)) - exact) <= Fraction(float(np.spacing(abs(g)))) / 2


def test_driver_argument_errors_come_before_any_device_or_file(tmp_path):
    """through the four file entries: -1 with the message, and no output file"""
    L = fa._topology_proto(fa.lib())
    batch = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb")])
    n = int(batch.n_atoms)
    cb = batch._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    N = n + 41
    boxed, bare, zero = tmp_path / "frames.trr", tmp_path / "bare.trr", tmp_path / "zero.trr"
    k = dict(natoms=N, double=True)
    tc.write_trr(boxed, [dict(k, v=nm(N, 9)), dict(k, box=np.diag([9.0, 9.0, 9.0]), x=nm(N, 1)), dict(k, box=np.diag([9.0, 9.0, 9.0]), x=nm(N, 2))])
    tc.write_trr(bare, [dict(k, box=BOX, v=nm(N, 9)), dict(k, x=nm(N, 1)), dict(k, box=BOX, x=nm(N, 2))])   # (the first COORDINATE frame has none)
    tc.write_trr(zero, [dict(k, box=np.zeros((3, 3)), x=nm(N, 1)), dict(k, box=BOX, x=nm(N, 2))])
    radii = np.full(N, 1.5)
    enc = lambda p: str(p).encode()
    outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "cls", "res")] + [tmp_path / "done.txt"]
    T = fa.FRAMES_TRR
    assert T == 128
    ok = dict(header=0, n_plain=N, frame_atoms=N, path=boxed)
    GROUPS = "not offered with chain groups"
    NOBOX = "first coordinate frame has none, or one that is all zero"
    cases = [("atom count", dict(ok, bits=T, n_plain=N - 1, frame_atoms=N + 1), None, None),
             ("header_bytes", dict(ok, bits=T, header=8), "header_bytes must be 0 with a TRR file", None),
             ("bit 0", dict(ok, bits=T | 1), "bit 0 of frames_f32 (raw fp32 frames) and bit 7", None),
             ("bit 0 and fp32 output", dict(ok, bits=T | 3), "bit 0", None),
             ("bit 2", dict(ok, bits=T | 4), "bit 2 of frames_f32 (a DCD file) and bit 7", None),
             ("bit 5", dict(ok, bits=T | 32), "bit 5 of frames_f32 (an AMBER NetCDF file) and bit 7", None),
             ("bit 6", dict(ok, bits=T | 64), "bit 6 of frames_f32 (an XTC file) and bit 7", None),
             ("bit 3 without a box", dict(ok, bits=T | 8, path=bare), NOBOX, GROUPS),
             ("bit 3 with a zero box", dict(ok, bits=T | 8, path=zero), NOBOX, GROUPS),
             ("bits 3 and 4 with a zero box", dict(ok, bits=T | 24, path=zero), NOBOX, GROUPS),
             ("bit 4 without bit 3", dict(ok, bits=T | 16), "bit 4 of frames_f32 (triclinic cells) needs bit 3", GROUPS),
             ("bit 3 without a container", dict(ok, bits=8), "or bit 7 (a TRR file): raw frame files carry no cell", GROUPS),
             ("bit 4 without a container", dict(ok, bits=16), "or bit 7 (a TRR file)", GROUPS),
             ("chain groups with bit 3", dict(ok, bits=T | 8), "", GROUPS)]
    index = np.arange(n, dtype=np.int32)
    for what, kw, text, groups_text in cases:
        path = kw["path"]
        if text != "":
            err = C.create_string_buffer(512)
            rc = L.freesasa_gpu_trajectory_file(enc(path), kw["bits"], kw["header"], radii.ctypes.data_as(dp), kw["n_plain"], 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                                enc(outs[0]), enc(outs[1]), enc(outs[4]), 0, 0, None, err, 512)
            msg = err.value.decode()
            assert rc == -1 and (text in msg if text else (str(N) in msg and str(kw["n_plain"]) in msg and "TRR" in msg)), (what, msg)
            err = C.create_string_buffer(512)
            rc = L.freesasa_gpu_trajectory_file_devices(enc(path), kw["bits"], kw["header"], radii.ctypes.data_as(dp), kw["n_plain"], 0, fa.LEE_RICHARDS, 1.4,
                                                        20, 0, enc(outs[0]), enc(outs[1]), enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
            assert rc == -1 and err.value.decode() == msg, what
            err = C.create_string_buffer(512)
            rc = L.freesasa_gpu_trajectory_file_topology(enc(path), kw["bits"], kw["header"], 0, C.byref(cb), 0, kw["frame_atoms"],
                                                         index.ctypes.data_as(C.POINTER(C.c_int32)), None, fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]),
                                                         enc(outs[1]), enc(outs[2]), enc(outs[3]), None, None, enc(outs[4]), 0,
                                                         devs.ctypes.data_as(ip), 1, None, err, 512)
            msg = err.value.decode()
            assert rc == -1 and (text in msg if text else (str(N) in msg and str(kw["frame_atoms"]) in msg and "TRR" in msg)), (what, msg)
        ids = np.zeros(n, dtype=np.int32)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_groups(enc(path), kw["bits"], kw["header"], 0, C.byref(cb), 0, kw["frame_atoms"],
                                                   index.ctypes.data_as(C.POINTER(C.c_int32)), None, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                                   fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), enc(outs[2]), enc(outs[3]), None, None,
                                                   enc(outs[2]), None, enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
        assert rc == -1 and (groups_text in err.value.decode() if groups_text else err.value.decode() == msg), (what, err.value)
        assert not any(p.exists() for p in outs), what
    # the _stats forms share the path
    Ls = fa._stats_proto(L)
    err = C.create_string_buffer(512)
    rc = Ls.freesasa_gpu_trajectory_file_stats(enc(boxed), T | 1, 0, radii.ctypes.data_as(dp), N, 0, fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]),
                                               enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, fa.stats_word(("totals",)), enc(outs[2]), enc(outs[3]), err, 512)
    assert rc == -1 and "bit 0 of frames_f32 (raw fp32 frames) and bit 7" in err.value.decode() and not any(p.exists() for p in outs)
    # a file that is no TRR file, and one with a damaged header: the index pass's message, through the driver
    raw = tmp_path / "frames.f32"
    np.zeros((2, N, 3), dtype=np.float32).tofile(raw)
    damaged = tmp_path / "damaged.trr"
    data = bytearray(boxed.read_bytes())
    struct.pack_into(">i", data, tc.decode(bytes(data))[2].offset + tc.WORD_OF["e_size"], 99)
    damaged.write_bytes(bytes(data))
    for path, text in ((raw, "record 0 of the TRR file: its magic number is 0, not 1993"), (damaged, "record 2 of the TRR file: its e_size is 99")):
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file(enc(path), T, 0, radii.ctypes.data_as(dp), N, 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                            enc(outs[0]), None, None, 0, 0, None, err, 512)
        assert rc == -1 and text in err.value.decode() and not outs[0].exists(), err.value
    # the Python keywords: what cannot go with trr=True is refused before the library is asked
    for kw in (dict(f32=True), dict(header_bytes=8), dict(dcd=True), dict(netcdf=True), dict(xtc=True)):
        with pytest.raises(ValueError, match="trr=True"):
            fa.trajectory_file(boxed, radii, outs[0], trr=True, **kw)
        with pytest.raises(ValueError, match="trr=True"):
            fa.trajectory_file_topology(boxed, batch, outs[0], atom_index=index, trr=True, **kw)
    assert not any(p.exists() for p in outs)
