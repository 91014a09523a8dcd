"""DCD input of the trajectory file drivers (include/freesasa_gpu.h, FREESASA_GPU_FRAMES_DCD) without a GPU: the header
parser (csrc/dcd.c) on files written here in every variant the format allows and on files it must refuse, in the library and
- under AddressSanitizer + UBSan - in a stand-alone program; the gather kernel's phase function (csrc/traj_kernels.h,
traj_gather_dcd) driven on the CPU over the bytes of such files against plain numpy indexing; and the drivers' argument checks,
which come before a device is touched or an output file opened."""
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
from emu import dcd_emu

N, F = 7, 3
NAN32 = 0x7fc00001   # a NaN as fp32: what the poisoned record markers hold, in the file's byte order


def write_dcd(path, frames, endian="<", cell=False, dim4=False, ntitle=2, nset_header=None, fixed=0, version=24, natom=None,
              markers64=False, poison=False):
    """A DCD file of frames [F, N, 3] (written as fp32) in byte order `endian` ("<" or ">"), with a unit-cell record and / or a
    4th-dimension record per frame, NTITLE title lines; nset_header: the frame count the header claims (None: the true one).
    version 0 is X-PLOR.
    poison: the cell, the 4th dimension and every FRAME record marker hold NaN patterns (such a file is for the gather's
    emulation only: the drivers refuse it).  Returns the bytes written."""
    frames = np.asarray(frames, dtype=np.float32)
    nf, n = frames.shape[:2]
    i32, mk = endian + "i", (endian + "q") if markers64 else (endian + "i")
    icntrl = [0] * 20
    icntrl[0] = nf if nset_header is None else nset_header
    icntrl[1], icntrl[2], icntrl[3] = 1, 1, icntrl[0]
    icntrl[8], icntrl[10], icntrl[11], icntrl[19] = fixed, int(cell), int(dim4), version
    rec = lambda body: struct.pack(mk, len(body)) + body + struct.pack(mk, len(body))
    out = [rec(b"CORD" + struct.pack(endian + "20i", *icntrl)),
           rec(struct.pack(i32, ntitle) + b"".join((b"REMARKS line %d" % k).ljust(80) for k in range(ntitle))),
           rec(struct.pack(i32, n if natom is None else natom))]
    nan_word = struct.pack(endian + "I", NAN32)
    frec = (lambda body: nan_word + body + nan_word) if poison else rec
    for f in range(nf):
        if cell:
            out.append(frec(np.full(6, np.nan if poison else 50.0 + f).astype(endian + "f8").tobytes()))
        for k in range(3):
            out.append(frec(frames[f, :, k].astype(endian + "f4").tobytes()))
        if dim4:
            out.append(frec(np.full(n, np.nan if poison else 0.25, dtype=endian + "f4").tobytes()))
    data = b"".join(out)
    with open(path, "wb") as fh:
        fh.write(data)
    return data


def coords(n, nf, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 30, (nf, n, 3)).astype(np.float32)


VARIANTS = list(itertools.product("<>", (False, True), (False, True), (0, 2)))


def expected(endian, cell, dim4, ntitle, n=N, nf=F, nset=None):
    plane = 4 * n + 8
    return dict(n_atoms=n, n_frames=nf, n_frames_header=nf if nset is None else nset, first_frame=92 + (8 + 4 + 80 * ntitle) + 12,
                frame_bytes=56 * cell + (3 + dim4) * plane, x_off=60 if cell else 4, plane_bytes=plane, big_endian=endian == ">",
                has_cell=cell, has_4d=dim4, charmm_version=24)


def fields(info):
    return {k: getattr(info, k) for k, _ in fa.DcdInfoC._fields_}


@pytest.mark.parametrize("endian, cell, dim4, ntitle", VARIANTS)
def test_header_variants(tmp_path, endian, cell, dim4, ntitle):
    p = tmp_path / "a.dcd"
    data = write_dcd(p, coords(N, F, 1), endian, cell, dim4, ntitle)
    want = expected(endian, cell, dim4, ntitle)
    assert fields(fa.dcd_info(p)) == want
    assert len(data) == want["first_frame"] + F * want["frame_bytes"]
    # the frame count follows the file size, whatever the header claims
    for nset in (0, 99):
        write_dcd(p, coords(N, F, 1), endian, cell, dim4, ntitle, nset_header=nset)
        assert fields(fa.dcd_info(p)) == expected(endian, cell, dim4, ntitle, nset=nset)
    # cut in the middle of the last frame: one frame fewer, the tail ignored
    with open(p, "wb") as fh:
        fh.write(data[:len(data) - want["frame_bytes"] // 2])
    assert fields(fa.dcd_info(p)) == dict(want, n_frames=F - 1)


def refused_files(tmp):
    """(name, path, a word of the message it must be refused with)"""
    good = write_dcd(tmp / "good.dcd", coords(N, F, 2), cell=True)
    patch = lambda at, b: good[:at] + b + good[at + len(b):]
    cases = [("first word 83", patch(0, struct.pack("<i", 83)), "first word"),
             ("CORD replaced", patch(4, b"VELD"), "CORD"),
             ("title marker wrong", patch(92, struct.pack("<i", 4 + 80 * 2 + 4)), "title record"),
             ("title end marker wrong", patch(96 + 164, struct.pack("<i", 160)), "title record do not match"),
             ("first record end marker wrong", patch(88, struct.pack("<i", 80)), "first record"),
             ("atom record marker wrong", patch(96 + 164 + 4, struct.pack("<i", 8)), "atom-count record"),
             ("cut inside the header", good[:50], "shorter than the DCD header"),
             ("cut inside the title", good[:120], "shorter than the DCD header"),
             ("header but no frame", good[:92 + 172 + 12 + 40], "no whole frame")]
    out = []
    for name, data, text in cases:
        p = tmp / (name.replace(" ", "_") + ".dcd")
        p.write_bytes(data)
        out.append((name, p, text))
    for name, kw, text in [("64-bit markers", dict(markers64=True), "64-bit record markers are not supported"),
                           ("64-bit markers, big-endian", dict(markers64=True, endian=">"), "64-bit record markers are not supported"),
                           ("fixed atoms", dict(fixed=2), "fixed atoms"),
                           ("NATOM 0", dict(natom=0), "NATOM")]:
        p = tmp / (name.replace(" ", "_").replace(",", "") + ".dcd")
        write_dcd(p, coords(N, F, 2), **kw)
        out.append((name, p, text))
    return out


def test_refusals_each_with_its_own_message(tmp_path):
    L = fa.lib()
    seen = {}
    for name, p, text in refused_files(tmp_path):
        c, err = fa.DcdInfoC(), C.create_string_buffer(256)
        L.freesasa_gpu_dcd_info_read.argtypes = [C.c_char_p, C.POINTER(fa.DcdInfoC), C.c_char_p, C.c_int]
        assert L.freesasa_gpu_dcd_info_read(str(p).encode(), C.byref(c), err, 256) == -1, name
        assert text in err.value.decode(), (name, err.value)
        with pytest.raises(ValueError, match="freesasa_gpu_dcd_info_read"):
            fa.dcd_info(p)
        seen[name] = err.value.decode()
    assert "names 2" in seen["fixed atoms"] and " 0:" in seen["NATOM 0"]
    # the kinds of refusal the format table lists have messages of their own
    kinds = ["first word 83", "CORD replaced", "64-bit markers", "fixed atoms", "NATOM 0", "title marker wrong", "cut inside the header",
             "header but no frame"]
    assert len({seen[k] for k in kinds}) == len(kinds)
    with pytest.raises(ValueError, match="cannot open"):
        fa.dcd_info(tmp_path / "does_not_exist.dcd")
    assert fa.dcd_info(tmp_path / "good.dcd").has_cell


def test_xplor_files_have_no_cell_whatever_word_10_says(tmp_path):
    """version 0 with words 10 and 11 set, written WITHOUT the records (X-PLOR never has them): accepted, no cell record"""
    p = tmp_path / "xplor.dcd"
    data = bytearray(write_dcd(p, coords(N, F, 3), version=0, ntitle=1))
    data[8 + 4 * 10:8 + 4 * 12] = struct.pack("<2i", 1, 1)
    p.write_bytes(bytes(data))
    info = fa.dcd_info(p)
    assert fields(info) == dict(expected("<", False, False, 1), charmm_version=0)


@pytest.mark.parametrize("n", [7, 300])           # 3 * 3 * 300 = 2700 coordinates: eleven workgroups of TRAJ_B = 256, the last short
@pytest.mark.parametrize("endian", "<>")
def test_emulated_gather_is_an_exact_indexed_copy(tmp_path, n, endian):
    frames = coords(n, F, 4 + n)
    rng = np.random.default_rng(n)
    index = rng.permutation(n)[:max(n - 2, 1)].astype(np.int32)
    assert np.any(np.diff(index) < 0)
    for cell, dim4 in ((False, False), (True, True)):
        p = tmp_path / "clean.dcd"
        write_dcd(p, frames, endian, cell, dim4)
        info = fa.dcd_info(p)
        # the bytes the kernel reads come from a file whose cell, 4th dimension and markers are NaN patterns: none may arrive
        data = write_dcd(tmp_path / "poisoned.dcd", frames, endian, cell, dim4, poison=True)
        assert len(data) == info.first_frame + F * info.frame_bytes
        for idx in (index, None):
            got = dcd_emu.gather(data, info, F, idx)
            want = (frames if idx is None else frames[:, idx, :]).astype(np.float64)
            assert not np.isnan(got).any()
            assert got.tobytes() == want.tobytes(), (cell, dim4, idx is None)
        # frames of a later shard: a non-zero frame offset is the driver's pread, the kernel starts at its frame 0
        got = dcd_emu.gather(data[:info.first_frame] + data[info.first_frame + info.frame_bytes:], info, F - 1, index)
        assert got.tobytes() == frames[1:, index, :].astype(np.float64).tobytes()


def test_driver_argument_errors_come_before_any_device_or_file(tmp_path):
    """through the file entries, plain and with a topology: -1 with the message, and no output file"""
    L = fa._topology_proto(fa.lib())
    batch = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb")])
    n = int(batch.n_atoms)
    cb = batch._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    dcd = tmp_path / "frames.dcd"
    write_dcd(dcd, coords(n + 41, 2, 5), cell=True)
    radii = np.full(n + 41, 1.5)
    enc = lambda p: str(p).encode()
    outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "cls", "res")] + [tmp_path / "done.txt"]
    DCD = fa.FRAMES_DCD
    assert DCD == 4
    cases = [("atom count", dict(bits=DCD, header=0, n_plain=n + 40, frame_atoms=n + 42), None),
             ("header_bytes", dict(bits=DCD, header=8, n_plain=n + 41, frame_atoms=n + 41), "header_bytes must be 0"),
             ("bit 0", dict(bits=DCD | 1, header=0, n_plain=n + 41, frame_atoms=n + 41), "bit 0"),
             ("bit 0 and fp32 output", dict(bits=DCD | 3, header=0, n_plain=n + 41, frame_atoms=n + 41), "bit 0")]
    index = np.arange(n, dtype=np.int32)
    for what, kw, text in cases:
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file(enc(dcd), kw["bits"], kw["header"], radii.ctypes.data_as(dp), kw["n_plain"], 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                            enc(outs[0]), enc(outs[1]), enc(outs[4]), 0, 0, None, err, 512)
        msg = err.value.decode()
        assert rc == -1 and (text in msg if text else (str(n + 41) in msg and str(kw["n_plain"]) in msg)), (what, msg)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_devices(enc(dcd), kw["bits"], kw["header"], radii.ctypes.data_as(dp), kw["n_plain"], 0, fa.LEE_RICHARDS, 1.4,
                                                    20, 0, enc(outs[0]), enc(outs[1]), enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
        assert rc == -1 and err.value.decode() == msg, what
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_topology(enc(dcd), kw["bits"], kw["header"], 0, C.byref(cb), 0, kw["frame_atoms"],
                                                     index.ctypes.data_as(C.POINTER(C.c_int32)), None, fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]),
                                                     enc(outs[1]), enc(outs[2]), enc(outs[3]), None, None, enc(outs[4]), 0,
                                                     devs.ctypes.data_as(ip), 1, None, err, 512)
        msg = err.value.decode()
        assert rc == -1 and (text in msg if text else (str(n + 41) in msg and str(kw["frame_atoms"]) in msg)), (what, msg)
        ids = np.zeros(n, dtype=np.int32)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_groups(enc(dcd), kw["bits"], kw["header"], 0, C.byref(cb), 0, kw["frame_atoms"],
                                                   index.ctypes.data_as(C.POINTER(C.c_int32)), None, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                                   fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), enc(outs[2]), enc(outs[3]), None, None,
                                                   enc(outs[2]), None, enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
        assert rc == -1 and err.value.decode() == msg, what
        assert not any(p.exists() for p in outs), what
    # a file that is no DCD: the parser's message, through the driver
    raw = tmp_path / "frames.f32"
    coords(n + 41, 2, 5).tofile(raw)
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_file(enc(raw), DCD, 0, radii.ctypes.data_as(dp), n + 41, 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                        enc(outs[0]), None, None, 0, 0, None, err, 512)
    assert rc == -1 and "first word" in err.value.decode() and not outs[0].exists()
    # the Python keywords: what cannot go with dcd=True is refused before the library is asked
    for kw in (dict(f32=True), dict(header_bytes=8)):
        with pytest.raises(ValueError, match="dcd=True"):
            fa.trajectory_file(dcd, radii, outs[0], dcd=True, **kw)
        with pytest.raises(ValueError, match="dcd=True"):
            fa.trajectory_file_topology(dcd, batch, outs[0], atom_index=index, dcd=True, **kw)
    assert not any(p.exists() for p in outs)


def test_header_parser_under_sanitizers_stand_alone(tmp_path):
    """csrc/dcd.c compiled with -fsanitize=address,undefined into a program of its own, run as a child process over every
    variant and every refused file: exit status 0, no sanitizer report, the verdicts and fields of the library"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/dcd_check"], check=True, stdout=subprocess.DEVNULL)
    paths, want = [], []
    for k, (endian, cell, dim4, ntitle) in enumerate(VARIANTS):
        p = tmp_path / f"v{k}.dcd"
        data = write_dcd(p, coords(N, F, 1), endian, cell, dim4, ntitle, nset_header=99 if k % 2 else None)
        if k % 3 == 0:
            p.write_bytes(data[:-5])                                   # a tail that is no whole frame
        paths.append(p)
        e = expected(endian, cell, dim4, ntitle, nf=F - 1 if k % 3 == 0 else F, nset=99 if k % 2 else F)
        want.append("ok " + " ".join(str(int(e[name])) for name, _ in fa.DcdInfoC._fields_))
    for name, p, text in refused_files(tmp_path):
        paths.append(p)
        want.append(text)
    paths.append(tmp_path / "does_not_exist.dcd")
    want.append("cannot open")
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "dcd_check")] + [str(p) for p in paths], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(paths)
    for line, w, p in zip(lines, want, paths):
        if w.startswith("ok "):
            assert line == w, p
        else:
            assert line.startswith("refused ") and w in line, (p, line)
