"""AMBER NetCDF input of the trajectory file drivers (include/freesasa_gpu.h, FREESASA_GPU_FRAMES_NETCDF) without a GPU: the
header parser (csrc/netcdf.c) on files written by tests/netcdf_writer.py and by scipy.io.netcdf_file in every variant the
drivers read and on files it must refuse, in the library and - under AddressSanitizer + UBSan, with truncated and overwritten
headers - in a stand-alone program; the cell arithmetic (csrc/cell.c, freesasa_gpu_cell_from_lengths_angles) against the DCD
decoder bit for bit; the gather kernel's phase function (csrc/traj_kernels.h, traj_gather_nc) driven on the CPU over the bytes of
such files against numpy reading the same bytes; and the drivers' argument checks, which come before a device is touched or an
output file opened."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
from freesasa_amd import ingest
from emu import nc_emu
from netcdf_writer import amber, write_amber, write_nc

N, F = 37, 5
GOLDEN = os.path.join(ROOT, "tests", "golden", "netcdf")
KINDS = {"coordinates": dict(time=False), "time": dict(), "cells": dict(cell=True), "cells+velocities": dict(cell=True, velocities=True)}
STRIDE = {"coordinates": 444, "time": 448, "cells": 496, "cells+velocities": 940}       # N = 37, as scipy lays the records out
VARIANTS = list(itertools.product((1, 2), KINDS))


def coords(n, nf, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 30, (nf, n, 3)).astype(np.float32)


def cells_of(nf):
    """a, b, c, alpha, beta, gamma per frame: every number its own"""
    return np.array([[50.0 + f, 60.0 + f, 70.0 + f, 80.0 + f, 95.0 - f, 100.0 + 2 * f] for f in range(nf)])


def content(frames, kind, **kw):
    k = dict(KINDS[kind], **kw)
    return amber(frames, cells_of(len(frames)) if k.pop("cell", False) else None, **k)


def scipy_write(path, dims, gatts, variables, version=2):
    """the same content through scipy.io.netcdf_file"""
    netcdf_file = pytest.importorskip("scipy.io").netcdf_file
    f = netcdf_file(str(path), "w", version=version)
    for k, v in gatts.items():
        setattr(f, k, v)
    for name, length in dims:
        f.createDimension(name, length)
    for name, d, atts, x in variables:
        x = np.asarray(x)
        v = f.createVariable(name, x.dtype.newbyteorder("="), d)
        for k, val in atts.items():
            setattr(v, k, val)
        v[:] = x
    f.close()
    return open(path, "rb").read()


def write(path, frames, kind, version=2, writer="struct", numrecs=None, **kw):
    c = content(frames, kind, **kw)
    if writer == "struct":
        return write_nc(path, *c, version=version, numrecs=numrecs)
    data = bytearray(scipy_write(path, *c, version=version))
    if numrecs is not None:
        struct.pack_into(">I", data, 4, numrecs & 0xffffffff)
        open(path, "wb").write(bytes(data))
    return bytes(data)


def expected(data, kind, version, n=N, nf=F, numrecs=None):
    rec = STRIDE[kind] + 12 * (n - N) * (2 if kind == "cells+velocities" else 1)
    t = 0 if kind == "coordinates" else 4
    cell = kind.startswith("cells")
    return dict(n_atoms=n, n_frames=nf, n_frames_header=nf if numrecs is None else numrecs, first_record=len(data) - nf * rec, record_bytes=rec,
                coord_off=t, lengths_off=t + 12 * n if cell else -1, angles_off=t + 12 * n + 24 if cell else -1, version=version, has_cell=cell,
                has_time=kind != "coordinates", has_velocities=kind == "cells+velocities")


def fields(info):
    return {k: getattr(info, k) for k, _ in fa.NcInfoC._fields_}


@pytest.mark.parametrize("version, kind", VARIANTS)
def test_the_writer_equals_scipy_byte_for_byte(tmp_path, version, kind):
    pytest.importorskip("scipy")
    frames = coords(N, F, 1)
    ours = write(tmp_path / "a.nc", frames, kind, version)
    theirs = write(tmp_path / "b.nc", frames, kind, version, writer="scipy")
    assert ours == theirs
    assert (len(ours) - fa.nc_info(tmp_path / "a.nc").first_record) == F * STRIDE[kind]


@pytest.mark.parametrize("writer", ["struct", "scipy"])
@pytest.mark.parametrize("version, kind", VARIANTS)
def test_header_variants(tmp_path, version, kind, writer):
    p = tmp_path / "a.nc"
    frames = coords(N, F, 1)
    data = write(p, frames, kind, version, writer)
    want = expected(data, kind, version)
    assert fields(fa.nc_info(p)) == want
    assert want["first_record"] > 0 and want["first_record"] % 4 == 0
    # the coordinates lie where the fields say
    for f in (0, F - 1):
        got = np.frombuffer(data, ">f4", 3 * N, want["first_record"] + f * want["record_bytes"] + want["coord_off"])
        assert got.tobytes() == frames[f].astype(">f4").tobytes()
    # the frame count follows the file size, whatever the header claims: a stale numrecs, a streaming one
    for numrecs in (2, 99, -1):
        write(p, frames, kind, version, writer, numrecs=numrecs)
        assert fields(fa.nc_info(p)) == dict(want, n_frames_header=numrecs)
    # cut in the middle of the last record: one frame fewer, the tail ignored
    p.write_bytes(data[:len(data) - want["record_bytes"] // 2])
    assert fields(fa.nc_info(p)) == dict(want, n_frames=F - 1)


def test_a_scale_factor_of_one_and_other_conventions_tokens_are_accepted(tmp_path):
    p = tmp_path / "a.nc"
    for kw in (dict(coord_atts={"scale_factor": 1.0}), dict(coord_atts={"scale_factor": np.float64(1.0)}), dict(conventions="CF-1.0, AMBER"),
               dict(conventions="AMBER,CF-1.0")):
        data = write(p, coords(N, F, 1), "cells", **kw)
        assert fields(fa.nc_info(p)) == expected(data, "cells", 2), kw


def refused_files(tmp):
    """(name, path, a word of the message it must be refused with)"""
    frames = coords(N, F, 2)
    good = write(tmp / "good.nc", frames, "cells+velocities")
    info = fa.nc_info(tmp / "good.nc")
    patch = lambda at, b: good[:at] + b + good[at + len(b):]
    at_coord = good.index(b"coordinates")           # name (11 bytes, padded to 12) | ndims | dimid[3]
    at_begin = good.index(struct.pack(">q", info.first_record + info.coord_off))
    assert at_begin < info.first_record and good[at_coord - 4:at_coord] == struct.pack(">i", 11)
    big = bytearray(good + bytes(70000))
    cases = [("CDF-5", patch(3, b"\x05"), "CDF-5"),
             ("HDF5", b"\x89HDF\r\n\x1a\n" + good[8:], "nccopy -k classic"),
             ("not CDF", b"CORD" + good[4:], "does not begin with CDF"),
             ("version 3", patch(3, b"\x03"), "neither 1 nor 2"),
             ("three bytes", good[:3], "shorter than 4 bytes"),
             ("cut behind the dimension tag", good[:12], "ends before its grammar"),
             ("cut inside the variables", good[:at_coord + 14], "ends before its grammar"),
             ("dimension count", patch(12, struct.pack(">I", 0x7fffffff)), "dimension count"),
             ("dimension tag", patch(8, struct.pack(">I", 0x0B)), "dimension list"),
             ("name length", patch(16, struct.pack(">I", 0x7fffffff)), "name length"),
             ("dimid", patch(at_coord + 16, struct.pack(">I", 99)), "dimid"),
             ("begin", patch(at_begin, struct.pack(">q", 1 << 40)), "begin"),
             ("begin inside the header", patch(at_begin, struct.pack(">q", 64)), "into the header"),
             ("atoms too many", patch(good.index(b"atom") + 4, struct.pack(">I", 0x10000000)), "too large"),
             ("header but no record", good[:info.first_record + info.record_bytes - 4], "no whole record")]
    out = []
    for name, data, text in cases:
        p = tmp / (name.replace(" ", "_") + ".nc")
        p.write_bytes(data)
        out.append((name, p, text))

    def edited(name, text, edit, kind="cells+velocities", **kw):
        dims, gatts, variables = content(frames, kind, **kw)
        dims, gatts, variables = edit(dims, gatts, variables)
        p = tmp / (name.replace(" ", "_") + ".nc")
        write_nc(p, dims, gatts, variables)
        out.append((name, p, text))
    same = lambda d, g, v: (d, g, v)
    swap = lambda name, f: (lambda d, g, v: (d, g, [f(x) if x[0] == name else x for x in v]))
    edited("header of 70 KB", "longer than 64 KiB", lambda d, g, v: (d, dict(g, title="t" * 70000), v))
    edited("no Conventions", "no global attribute Conventions", same, conventions=None)
    edited("other Conventions", "do not name AMBER", same, conventions="CF-1.0,AMBERX")
    edited("restart", "a restart file, not a trajectory", same, conventions="AMBERRESTART")
    edited("no coordinates", "no variable `coordinates`", lambda d, g, v: (d, g, [x for x in v if x[0] != "coordinates"]))
    edited("coordinates fp64", "`coordinates`", swap("coordinates", lambda x: (x[0], x[1], x[2], x[3].astype(">f8"))))
    edited("coordinates transposed", "`coordinates`",
           swap("coordinates", lambda x: (x[0], ("frame", "spatial", "atom"), x[2], np.ascontiguousarray(x[3].transpose(0, 2, 1)))))
    edited("coordinates not per frame", "`coordinates`", swap("coordinates", lambda x: (x[0], ("atom", "spatial"), x[2], x[3][0])))
    edited("scale factor", "scale_factor other than 1", same, coord_atts={"scale_factor": 0.5})
    edited("scale factor twice", "scale_factor other than 1", same, coord_atts={"scale_factor": np.array([1.0, 1.0], dtype=np.float32)})
    edited("cell lengths fp32", "`cell_lengths`", swap("cell_lengths", lambda x: (x[0], x[1], x[2], x[3].astype(">f4"))))
    edited("cell angles by label", "`cell_angles`", swap("cell_angles", lambda x: (x[0], ("frame", "label"), x[2], np.zeros((F, 5)))))
    p = tmp / "no_atoms.nc"
    write_amber(p, np.zeros((F, 0, 3), dtype=np.float32))
    out.append(("no atoms", p, "must be > 0"))
    return out


KINDS_OF_REFUSAL = ["CDF-5", "HDF5", "not CDF", "cut behind the dimension tag", "header of 70 KB", "dimension count", "name length", "dimid", "begin",
                    "header but no record", "no Conventions", "other Conventions", "restart", "no coordinates", "coordinates fp64", "scale factor",
                    "atoms too many", "no atoms", "cell lengths fp32", "cell angles by label"]


def test_refusals_each_with_its_own_message(tmp_path):
    L = fa.lib()
    L.freesasa_gpu_nc_info_read.argtypes = [C.c_char_p, C.POINTER(fa.NcInfoC), C.c_char_p, C.c_int]
    seen = {}
    for name, p, text in refused_files(tmp_path):
        c, err = fa.NcInfoC(), C.create_string_buffer(256)
        assert L.freesasa_gpu_nc_info_read(str(p).encode(), C.byref(c), err, 256) == -1, name
        assert text in err.value.decode(), (name, err.value)
        with pytest.raises(ValueError, match="freesasa_gpu_nc_info_read"):
            fa.nc_info(p)
        seen[name] = err.value.decode()
    assert len({seen[k] for k in KINDS_OF_REFUSAL}) == len(KINDS_OF_REFUSAL)
    with pytest.raises(ValueError, match="cannot open"):
        fa.nc_info(tmp_path / "does_not_exist.nc")
    info = fa.nc_info(tmp_path / "good.nc")
    assert info.has_cell and info.has_velocities
    # a short message buffer, and none
    err = C.create_string_buffer(8)
    assert L.freesasa_gpu_nc_info_read(str(tmp_path / "restart.nc").encode(), C.byref(fa.NcInfoC()), err, 8) == -1 and len(err.value) == 7
    assert L.freesasa_gpu_nc_info_read(str(tmp_path / "restart.nc").encode(), C.byref(fa.NcInfoC()), None, 0) == -1


def test_header_parser_under_sanitizers_stand_alone(tmp_path):
    """csrc/netcdf.c and csrc/cell.c compiled with -fsanitize=address,undefined into a program of their own, run as a child process
    over every variant, every refused file, the cells + velocities header cut at every length and with every 32-bit word of it
    overwritten: exit status 0, no sanitizer report, every file parsed or refused with a message, the verdicts of the library"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/nc_check"], check=True, stdout=subprocess.DEVNULL)
    paths, want = [], []
    for k, (version, kind) in enumerate(VARIANTS):
        p = tmp_path / f"v{k}.nc"
        numrecs = (None, 99, -1)[k % 3]
        data = write(p, coords(N, F, 1), kind, version, numrecs=numrecs)
        e = expected(data, kind, version, numrecs=numrecs)
        if k % 2:
            p.write_bytes(data[:-5])                                    # a tail that is no whole record
            e["n_frames"] = F - 1
        paths.append(p)
        want.append("ok " + " ".join(str(int(e[name])) for name, _ in fa.NcInfoC._fields_))
    for name, p, text in refused_files(tmp_path):
        paths.append(p)
        want.append(text)
    paths.append(tmp_path / "does_not_exist.nc")
    want.append("cannot open")
    good = (tmp_path / "good.nc").read_bytes()
    head = fa.nc_info(tmp_path / "good.nc").first_record
    fuzz = tmp_path / "fuzz"
    fuzz.mkdir()
    for cut in range(head + 1):
        (fuzz / f"cut{cut}.nc").write_bytes(good[:cut])
        paths.append(fuzz / f"cut{cut}.nc")
    for at in range(0, head, 4):
        for v in (0x7fffffff, 0xffffffff):
            p = fuzz / f"word{at}_{v:x}.nc"
            p.write_bytes(good[:at] + struct.pack(">I", v) + good[at + 4:])
            paths.append(p)
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "nc_check")] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
    lines = [line for line in res.stdout.splitlines() if not line.startswith("cell ")]
    assert len(lines) == len(paths)
    for line, p in zip(lines, paths):
        assert line.startswith("ok ") or (line.startswith("refused ") and len(line) > 20), (p, line)
    for line, w, p in zip(lines, want, paths):
        if w.startswith("ok "):
            assert line == w, p
        else:
            assert line.startswith("refused ") and w in line, (p, line)
    assert all(line.startswith("refused ") for line in lines[len(want):len(want) + head])     # (every cut but the whole header ...)
    assert lines[len(want) + head].startswith("refused ")                                      # (... and that one holds no record)
    assert sum(line.startswith("ok ") for line in lines[len(want) + head + 1:]) > 10           # (numrecs, attribute bytes: harmless words)
    # the decoded cells of a whole file: what the library's arithmetic gives
    cell_lines = [line.split() for line in res.stdout.splitlines() if line.startswith("cell ")]
    first = [c for c in cell_lines[:F]]
    assert [int(c[1]) for c in first] == list(range(F))
    for f, c in enumerate(first):
        rec = cells_of(F)[f]
        assert [float.fromhex(v) for v in c[2:8]] == list(rec) and c[8] == "ok"
        assert np.array([float.fromhex(v) for v in c[9:15]]).tobytes() == fa.cell_from_lengths_angles(rec[:3], rec[3:]).tobytes()


SHAPES = {"truncated octahedron": ((60.0, 60.0, 60.0), (109.4712190, 109.4712190, 109.4712190)),
          "hexagonal prism": ((50.0, 50.0, 70.0), (90.0, 90.0, 120.0)),
          "hexagonal prism, 60": ((50.0, 50.0, 70.0), (90.0, 90.0, 60.0)),
          "rhombic dodecahedron": ((55.0, 55.0, 55.0), (60.0, 60.0, 90.0)),
          "rhombic dodecahedron, xy square": ((55.0, 55.0, 55.0), (60.0, 90.0, 60.0)),
          "right-angled": ((31.5, 42.25, 53.125), (90.0, 90.0, 90.0)),
          "nearly right-angled": ((31.5, 42.25, 53.125), (90.00005, 89.99995, 90.0)),
          "general": ((14.3, 13.0, 12.1), (95.0, 98.0, 76.0))}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cell_arithmetic_equals_the_dcd_decoder_bit_for_bit(shape):
    l, a = SHAPES[shape]
    got = fa.cell_from_lengths_angles(l, a)
    assert got.tobytes() == fa.cell_from_dcd([l[0], a[2], l[1], a[1], a[0], l[2]]).tobytes()
    if shape.endswith("right-angled"):
        assert got.tobytes() == np.array([l[0], 0.0, l[1], 0.0, 0.0, l[2]]).tobytes()
    else:
        assert got[1] != 0.0 or got[3] != 0.0 or got[4] != 0.0
    # the cell it describes: |a|, |b|, |c| and the angles between them
    va, vb, vc = np.array([got[0], 0, 0]), np.array([got[1], got[2], 0]), np.array(got[3:])
    assert np.allclose([np.linalg.norm(va), np.linalg.norm(vb), np.linalg.norm(vc)], l, rtol=1e-12)
    ang = lambda u, v: np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v)))
    assert np.allclose([ang(vb, vc), ang(va, vc), ang(va, vb)], a, atol=1.1e-4)


def test_cell_arithmetic_refusals():
    l = (50.0, 60.0, 70.0)
    for k, name in enumerate(("alpha", "beta", "gamma")):
        for bad in (0.0, 180.0, -5.0, 200.0, float("nan"), float("inf")):
            a = [90.0, 90.0, 90.0]
            a[k] = bad
            with pytest.raises(ValueError, match=f"angle {name} of its cell is .*not degrees in \\(0, 180\\)"):
                fa.cell_from_lengths_angles(l, a)
    with pytest.raises(ValueError, match="span no cell"):
        fa.cell_from_lengths_angles(l, (10.0, 10.0, 170.0))
    with pytest.raises(ValueError, match="span no cell"):
        fa.cell_from_lengths_angles(l, (125.0, 125.0, 125.0))
    for k in range(3):
        e = list(l)
        e[k] = float("inf")
        with pytest.raises(ValueError, match=f"edge {'ABC'[k]} of its cell is not finite"):
            fa.cell_from_lengths_angles(e, (90.0, 90.0, 90.0))
    with pytest.raises(ValueError, match="three lengths and three angles"):
        fa.cell_from_lengths_angles(l, (90.0, 90.0))


@pytest.mark.parametrize("n", [1, 37, 516])        # 3 * 5 * 516 = 7740 coordinates: thirty-one workgroups of TRAJ_B = 256, the last short
@pytest.mark.parametrize("kind", list(KINDS))
def test_emulated_gather_is_an_exact_indexed_copy(tmp_path, n, kind):
    frames = coords(n, F, 4 + n)
    frames[0, 0] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38)]        # a signed zero, a denormal, a large number
    rng = np.random.default_rng(n)
    index = rng.permutation(n)[:max(n - 2, 1)].astype(np.int32)
    assert n == 1 or np.any(np.diff(index) < 0)
    p = tmp_path / "a.nc"
    data = write(p, frames, kind, version=1 + n % 2)
    info = fa.nc_info(p)
    assert info.record_bytes == expected(data, kind, 1 + n % 2, n=n)["record_bytes"] and (n != N or info.record_bytes == STRIDE[kind])
    filed = np.stack([np.frombuffer(data, ">f4", 3 * n, info.first_record + f * info.record_bytes + info.coord_off).reshape(n, 3).astype("<f4")
                      for f in range(F)])
    assert filed.tobytes() == frames.tobytes()
    for idx in (index, None):
        got = nc_emu.gather(data, info, F, idx)
        want = (filed if idx is None else filed[:, idx, :]).astype("<f8")
        assert not np.isnan(got).any()
        assert got.tobytes() == want.tobytes(), idx is None
    # frames of a later shard: a non-zero frame offset is the driver's pread, the kernel starts at its frame 0
    got = nc_emu.gather(data[:info.first_record] + data[info.first_record + info.record_bytes:], info, F - 1, index)
    assert got.tobytes() == filed[1:, index, :].astype("<f8").tobytes()


def test_driver_argument_errors_come_before_any_device_or_file(tmp_path):
    """through the four file entries: -1 with the message, and no output file"""
    L = fa._topology_proto(fa.lib())
    batch = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb")])
    n = int(batch.n_atoms)
    cb = batch._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nc, bare = tmp_path / "frames.nc", tmp_path / "bare.nc"
    write_amber(nc, coords(n + 41, 2, 5), cells_of(2))
    write_amber(bare, coords(n + 41, 2, 5))
    radii = np.full(n + 41, 1.5)
    enc = lambda p: str(p).encode()
    outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "cls", "res")] + [tmp_path / "done.txt"]
    NC = fa.FRAMES_NETCDF
    assert NC == 32
    ok = dict(header=0, n_plain=n + 41, frame_atoms=n + 41, path=nc)
    GROUPS = "not offered with chain groups"
    cases = [("atom count", dict(ok, bits=NC, n_plain=n + 40, frame_atoms=n + 42), None, None),
             ("header_bytes", dict(ok, bits=NC, header=8), "header_bytes must be 0", None),
             ("bit 0", dict(ok, bits=NC | 1), "bit 0", None),
             ("bit 0 and fp32 output", dict(ok, bits=NC | 3), "bit 0", None),
             ("bit 2", dict(ok, bits=NC | 4), "bit 2 of frames_f32 (a DCD file) and bit 5", None),
             ("bit 3 without cells", dict(ok, bits=NC | 8, path=bare), "this one has no cell", GROUPS),
             ("bits 3 and 4 without cells", dict(ok, bits=NC | 24, path=bare), "this one has no cell", GROUPS),
             ("bit 4 without bit 3", dict(ok, bits=NC | 16), "bit 4 of frames_f32 (triclinic cells) needs bit 3", GROUPS),
             ("chain groups with bit 3", dict(ok, bits=NC | 8), "", GROUPS)]
    index = np.arange(n, dtype=np.int32)
    for what, kw, text, groups_text in cases:
        path = kw["path"]
        if text != "":
            err = C.create_string_buffer(512)
            rc = L.freesasa_gpu_trajectory_file(enc(path), kw["bits"], kw["header"], radii.ctypes.data_as(dp), kw["n_plain"], 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                                enc(outs[0]), enc(outs[1]), enc(outs[4]), 0, 0, None, err, 512)
            msg = err.value.decode()
            assert rc == -1 and (text in msg if text else (str(n + 41) in msg and str(kw["n_plain"]) in msg and "NetCDF" in msg)), (what, msg)
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
            assert rc == -1 and (text in msg if text else (str(n + 41) in msg and str(kw["frame_atoms"]) in msg and "NetCDF" in msg)), (what, msg)
        ids = np.zeros(n, dtype=np.int32)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_groups(enc(path), kw["bits"], kw["header"], 0, C.byref(cb), 0, kw["frame_atoms"],
                                                   index.ctypes.data_as(C.POINTER(C.c_int32)), None, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                                   fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), enc(outs[2]), enc(outs[3]), None, None,
                                                   enc(outs[2]), None, enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
        assert rc == -1 and (groups_text in err.value.decode() if groups_text else err.value.decode() == msg), (what, err.value)
        assert not any(p.exists() for p in outs), what
    # a file that is no NetCDF: the parser's message, through the driver
    raw = tmp_path / "frames.f32"
    coords(n + 41, 2, 5).tofile(raw)
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_file(enc(raw), NC, 0, radii.ctypes.data_as(dp), n + 41, 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                        enc(outs[0]), None, None, 0, 0, None, err, 512)
    assert rc == -1 and "does not begin with CDF" in err.value.decode() and not outs[0].exists()
    # the Python keywords: what cannot go with netcdf=True is refused before the library is asked
    for kw in (dict(f32=True), dict(header_bytes=8), dict(dcd=True)):
        with pytest.raises(ValueError, match="netcdf=True"):
            fa.trajectory_file(nc, radii, outs[0], netcdf=True, **kw)
        with pytest.raises(ValueError, match="netcdf=True"):
            fa.trajectory_file_topology(nc, batch, outs[0], atom_index=index, netcdf=True, **kw)
    assert not any(p.exists() for p in outs)


def test_the_committed_scipy_written_file(tmp_path):
    """tests/golden/netcdf/amber_37x5_cell.nc: version 2 with time, cells and velocities, written by scipy.io.netcdf_file;
    amber_37x5_cell.npz holds what went in.  The parser, the cell helper and the emulated gather give it back."""
    path = os.path.join(GOLDEN, "amber_37x5_cell.nc")
    want = np.load(os.path.join(GOLDEN, "amber_37x5_cell.npz"))
    frames, cells = want["frames"], want["cells"]
    assert frames.shape == (F, N, 3) and frames.dtype == np.float32 and cells.shape == (F, 6) and cells.dtype == np.float64
    data = open(path, "rb").read()
    info = fa.nc_info(path)
    assert fields(info) == expected(data, "cells+velocities", 2)
    assert nc_emu.gather(data, info, F).tobytes() == frames.astype(np.float64).tobytes()
    index = np.array([36, 0, 17, 5], dtype=np.int32)
    assert nc_emu.gather(data, info, F, index).tobytes() == frames[:, index].astype(np.float64).tobytes()
    L = fa.lib()
    L.freesasa_gpu_nc_cell_record.argtypes = [C.POINTER(fa.NcInfoC), C.c_char_p, C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.freesasa_gpu_nc_cell_record.restype = None
    c = fa.NcInfoC()
    L.freesasa_gpu_nc_info_read.argtypes = [C.c_char_p, C.POINTER(fa.NcInfoC), C.c_char_p, C.c_int]
    assert L.freesasa_gpu_nc_info_read(path.encode(), C.byref(c), None, 0) == 0
    for f in range(F):
        got = np.empty(6)
        L.freesasa_gpu_nc_cell_record(C.byref(c), data[info.first_record:], f, got[:3].ctypes.data_as(C.POINTER(C.c_double)),
                                      got[3:].ctypes.data_as(C.POINTER(C.c_double)))
        assert got.tobytes() == cells[f].tobytes()
    # the struct writer gives the same file
    assert write_amber(tmp_path / "again.nc", frames, cells, velocities=True) == data
