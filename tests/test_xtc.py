"""GROMACS XTC input on the CPU: the pure-Python codec (tests/xtc_codec.py) against itself on plans that force every path of the
format; the host's pass over the headers (freesasa_amd/csrc/xtc.c) and its refusals, also stand-alone under AddressSanitizer +
UBSan; the two decode kernels (xtc_kernels.h) driven on the CPU (tests/emu/emu_xtc.cpp) against the codec, bit for bit, and -
in a stand-alone sanitizer build - over about 2000 damaged streams; the drivers' argument checks, which come before any device.
No GROMACS-written file is at hand: the codec, written from the format's description, is the yardstick."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import freesasa_amd as fa
import xtc_codec as xc
from emu import xtc_emu
from freesasa_amd import ingest

M = xc.MAGICINTS


def synth(plan, smallidx, seed, span=200000, lo=None):
    """integer coordinates [n, 3] in output order that the plan fits: every small atom within its index's range of the atom it
    is coded against (the small range follows the plan's steps)"""
    rng = np.random.default_rng(seed)
    lo = np.array([-span, -span // 2, 0] if lo is None else lo)
    out = []
    for k, step in plan:
        half = M[smallidx] // 2
        big = lo + rng.integers(half + 8, span, 3)
        prev, smalls = big, []
        for _ in range(k):
            prev = prev + rng.integers(-half, M[smallidx] - half, 3)
            smalls.append(prev)
        out += ([smalls[0], big] + smalls[1:]) if k else [big]
        smallidx += step
    return np.array(out, dtype=np.int64)


def pad_plan(plan, n):
    """the plan, and single atoms up to n atoms"""
    have = sum(1 + k for k, _ in plan)
    assert have <= n
    return list(plan) + [(0, 0)] * (n - have)


# name -> (plan, first smallidx, keywords of synth): every path of the format
CASES = {
    "runs 0..8": ([(k, 0) for k in range(9)], 20, {}),
    "runs 8..0, flags forced": ([(k, 0) for k in range(8, -1, -1)], 24, {}),
    "smallidx up and down": ([(2, 1), (2, 1), (3, 1), (1, -1), (2, -1), (0, -1), (4, 0), (2, 1), (0, 0), (0, -1), (1, 0)], 15, {}),
    "a flag-0 group inherits its run": ([(3, 0), (3, 0), (3, 0), (0, 0), (0, 0), (2, 0), (2, 0)], 18, {}),
    "no flag at all": ([(0, 0)] * 12, 12, {}),
    "smallidx held at 9": ([(3, 0), (1, 0), (8, 0), (0, 0), (2, 0)], 9, {}),
    "smallidx down to 9 and up": ([(2, -1), (2, -1), (3, 0), (1, 1), (2, 0)], 11, {}),
    "smallidx held at 72": ([(3, 0), (2, 0), (8, 0), (1, 0)], 72, dict(span=1 << 26)),
    "smallidx up to 72": ([(2, 1), (2, 1), (3, 0), (1, -1), (4, 0)], 70, dict(span=1 << 26)),
    "bitsize 0": ([(2, 0), (0, 0), (3, 1), (1, 0), (0, -1), (4, 0)], 21, dict(span=1 << 26)),
    "the last group ends at natoms": ([(0, 0), (1, 0), (0, 0), (8, 0)], 30, {}),
    "ten atoms": ([(8, 0), (0, 0)], 16, {}),
}


def case_frame(name, n=None, seed=7):
    plan, smallidx, kw = CASES[name]
    if n is not None:
        plan = pad_plan(plan, n)
    ints = synth(plan, smallidx, seed, **kw)
    data = xc.encode(ints, 1000.0, box=np.diag([3.0, 4.0, 5.0]), plan=plan, smallidx=smallidx, force_flag="forced" in name)
    return plan, smallidx, ints, data


@pytest.mark.parametrize("name", list(CASES))
def test_codec_round_trip(name, tmp_path):
    plan, smallidx, ints, data = case_frame(name)
    assert len(data) % 4 == 0
    (tmp_path / "one.xtc").write_bytes(data)                       # (what the codec writes is a frame to the library's header walker)
    info = fa.xtc_info(tmp_path / "one.xtc")
    assert (info.n_atoms, info.n_frames, info.max_frame_bytes, info.has_box) == (len(ints), 1, len(data), True)
    (f,) = xc.decode(data)
    assert f.natoms == len(ints) and np.array_equal(f.ints, ints) and f.smallidx == smallidx
    assert [t[2] for t in f.trace] == [3 * k for k, _ in plan]
    assert [t[1] for t in f.trace] == list(np.cumsum([0] + [1 + k for k, _ in plan[:-1]]))
    assert [t[3] for t in f.trace] == list(smallidx + np.cumsum([0] + [s for _, s in plan[:-1]]))
    assert f.trace[-1][1] + 1 + f.trace[-1][2] // 3 == f.natoms
    sizeint = [f.maxint[k] - f.minint[k] + 1 for k in range(3)]
    assert (xc.bit_sizes(sizeint)[0] == 0) == (CASES[name][2].get("span", 0) > 1 << 24)      # ("bitsize 0", and the widest small ranges)
    assert np.array_equal(f.box, np.diag([3.0, 4.0, 5.0]).astype(np.float32)) and f.precision == np.float32(1000.0)
    # the values: two fp32 products, not one
    want = (f.ints.astype(np.float32) * np.float32(1.0 / 1000.0)) * np.float32(10.0)
    assert f.xyz.dtype == np.float32 and np.array_equal(f.xyz, want)
    if name == "no flag at all":
        bits = sum(xc.bit_sizes(sizeint)[0] + 1 for _ in plan)
        assert f.bytecount == (bits + 7) // 8


def test_codec_extremes_and_padding(tmp_path):
    assert [xc.sizeofint(s) for s in (1, 2, 3, 4, 255, 256, 0xffffff, 0x1000000, 0xffffffff)] == [1, 2, 2, 3, 8, 9, 24, 25, 32]
    assert xc.bit_sizes([1, 1, 1]) == (1, [0, 0, 0]) and xc.bit_sizes([0xffffff] * 3)[0] == 72
    assert xc.bit_sizes([0x1000000, 5, 7]) == (0, [25, 3, 3])
    assert (M[37], M[57], M[69]) == (5060, 524287, 8388607) and M[9] == 8 and M[72] == 16777216 and M[8] == 0
    # every remainder of the byte count modulo 4, by the number of single atoms behind a fixed plan
    seen = {}
    for n in range(45, 80):
        _, _, ints, data = case_frame("runs 0..8", n=n)
        (f,) = xc.decode(data)
        assert np.array_equal(f.ints, ints) and len(data) == xc.HEADER + (f.bytecount + 3) // 4 * 4
        seen.setdefault(f.bytecount % 4, data)
    assert sorted(seen) == [0, 1, 2, 3]
    for k in range(4):                                           # (the index steps over every padding: twice the frame)
        (tmp_path / "two.xtc").write_bytes(seen[k] + seen[k])
        assert index_of(tmp_path / "two.xtc") == [0, len(seen[k]), 2 * len(seen[k])]
    # the default plan: greedy runs, decoded to what went in, for a chain whose steps fit the small range
    rng = np.random.default_rng(3)
    ints = np.cumsum(rng.integers(-40, 41, (516, 3)), 0) + 100000
    (f,) = xc.decode(xc.encode(ints, 1000.0))
    assert np.array_equal(f.ints, ints) and max(t[2] for t in f.trace) > 3 and len(f.trace) < 516
    # what a decoder must refuse
    _, _, _, data = case_frame("runs 0..8")
    (f,) = xc.decode(data)
    for bad in (f.stream[:-3], f.stream[:5]):
        with pytest.raises(ValueError):
            xc.decode_stream(bad, f.natoms, f.minint, f.maxint, f.smallidx)
    with pytest.raises(ValueError, match="runs past"):
        xc.decode_stream(f.stream, f.natoms - 1, f.minint, f.maxint, f.smallidx)


def jittered_ints(n, n_frames, seed, step=60):
    """a chain of n atoms (steps that fit a small range) and a per-frame jitter: frames of differing lengths"""
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.integers(-step, step + 1, (n, 3)), 0) + 50000
    return [base + rng.integers(-25 * (f + 1), 25 * (f + 1) + 1, (n, 3)) for f in range(n_frames)]


def xtc_file(path, n, n_frames, seed, boxes=None, precision=1000.0):
    data = b"".join(xc.encode(ints, precision, None if boxes is None else boxes[f], step=f, time=0.5 * f)
                    for f, ints in enumerate(jittered_ints(n, n_frames, seed)))
    path.write_bytes(data)
    return data


def index_of(path):
    L = fa.lib()
    L.freesasa_gpu_xtc_index_read.argtypes = [C.c_char_p, C.POINTER(fa.XtcInfoC), C.POINTER(C.POINTER(C.c_int64)), C.c_char_p, C.c_int]
    L.freesasa_gpu_xtc_index_free.argtypes = [C.POINTER(C.c_int64)]
    info, offs, err = fa.XtcInfoC(), C.POINTER(C.c_int64)(), C.create_string_buffer(512)
    if L.freesasa_gpu_xtc_index_read(str(path).encode(), C.byref(info), C.byref(offs), err, 512):
        raise ValueError(err.value.decode())
    got = [offs[k] for k in range(info.n_frames + 1)]
    L.freesasa_gpu_xtc_index_free(offs)
    return got


@pytest.mark.parametrize("n", [10, 37, 516])
def test_info_and_index(tmp_path, n):
    p = tmp_path / "frames.xtc"
    data = xtc_file(p, n, 7, n, boxes=[np.diag([3.0, 3.5, 4.0])] * 7, precision=500.0)
    frames = xc.decode(data)
    sizes = [f.size for f in frames]
    assert len(set(sizes)) > 1                                   # frames of differing lengths
    info = fa.xtc_info(p)
    assert (info.n_atoms, info.n_frames, info.max_frame_bytes, info.precision, info.has_box) == (n, 7, max(sizes), 500.0, True)
    assert index_of(p) == [f.offset for f in frames] + [len(data)]
    assert "n_frames=7" in repr(info)
    xtc_file(p, n, 2, n)
    assert not fa.xtc_info(p).has_box and fa.xtc_info(p).precision == 1000.0


def refused_files(tmp):
    """(name, path, what the message holds): a good file of four frames of 12 atoms whose frame 2 is replaced"""
    frames = [xc.decode(xc.encode(ints, 1000.0))[0] for ints in jittered_ints(12, 4, 5)]
    eleven = xc.decode(xc.encode(jittered_ints(11, 1, 6)[0], 1000.0))[0]

    def fb(f, **kw):
        a = dict(natoms=f.natoms, step=0, time=0.0, box=np.zeros((3, 3)), precision=float(f.precision), minint=f.minint, maxint=f.maxint,
                 smallidx=f.smallidx, stream=f.stream)
        bytecount = kw.pop("bytecount", None)
        a.update(kw)
        b = xc.frame_bytes(**a)
        return b if bytecount is None else b[:88] + struct.pack(">i", bytecount) + b[92:]

    g = frames[2]
    swapped = list(g.minint)
    swapped[1] = g.maxint[1] + 1
    variants = [("magic 2023", fb(g, magic=2023), "2023"), ("magic 7", fb(g, magic=7), "its magic number is 7, not 1995"),
                ("nine atoms", fb(g, natoms=9), "it holds 9 atoms"), ("atom counts differ", fb(g, natoms2=13), "its two atom counts differ: 12 and 13"),
                ("other atom count", fb(eleven), "it holds 11 atoms, frame 0 holds 12"),
                ("precision nan", fb(g, precision=float("nan")), "its precision is nan"), ("precision inf", fb(g, precision=float("inf")), "its precision is inf"),
                ("precision 0", fb(g, precision=0.0), "its precision is 0"), ("precision -1", fb(g, precision=-1.0), "its precision is -1"),
                ("minint > maxint", fb(g, minint=swapped), "exceeds maxint"),
                ("whole range", fb(g, minint=[-2 ** 31, g.minint[1], g.minint[2]], maxint=[2 ** 31 - 1, g.maxint[1], g.maxint[2]]), "spans all 2^32"),
                ("smallidx 8", fb(g, smallidx=8), "its smallidx is 8"), ("smallidx 73", fb(g, smallidx=73), "its smallidx is 73"),
                ("bytecount -1", fb(g, bytecount=-1), "its byte count is -1: negative"), ("bytecount 2^28", fb(g, bytecount=1 << 28), "2^28"),
                ("bytecount past the end", fb(g, bytecount=100000), "runs past the end of the file")]
    head = b"".join(fb(f) for f in frames[:2])
    out = []
    for name, third, text in variants:
        p = tmp / (name.replace(" ", "_").replace(">", "gt").replace("^", "") + ".xtc")
        p.write_bytes(head + third + fb(frames[3]))
        out.append((name, p, "frame 2 of the XTC file: ", text))
    for name, cut in (("ends in a header", 50), ("ends in a header's first words", 4), ("ends in the stream", 96)):
        p = tmp / (name.replace(" ", "_").replace("'", "") + ".xtc")
        p.write_bytes(head + fb(g)[:cut])
        out.append((name, p, "frame 2 of the XTC file: ", "the file ends inside its header" if cut < 92 else "runs past the end of the file"))
    (tmp / "empty.xtc").write_bytes(b"")
    out.append(("empty", tmp / "empty.xtc", "", "holds no frame"))
    (tmp / "good.xtc").write_bytes(head + fb(g) + fb(frames[3]))
    return out


def test_refusals_each_with_its_own_message_that_names_the_frame(tmp_path):
    msgs = {}
    for name, p, frame, text in refused_files(tmp_path):
        with pytest.raises(ValueError) as e:
            fa.xtc_info(p)
        msg = str(e.value)
        assert frame in msg and text in msg, (name, msg)
        msgs[name] = msg.replace("nan", "X").replace("inf", "X").replace("-1:", "X").replace("0:", "X")
    # the reasons differ from check to check (variants of one check - four precisions, two smallidx - share theirs)
    assert len({m.split(": ", 2)[-1][:24] for m in msgs.values()}) >= 13
    assert fa.xtc_info(tmp_path / "good.xtc").n_frames == 4
    with pytest.raises(ValueError, match="cannot open"):
        fa.xtc_info(tmp_path / "none.xtc")
    # a short message buffer, and none
    L = fa.lib()
    err = C.create_string_buffer(8)
    assert L.freesasa_gpu_xtc_info_read(str(tmp_path / "empty.xtc").encode(), C.byref(fa.XtcInfoC()), err, 8) == -1 and len(err.value) == 7
    assert L.freesasa_gpu_xtc_info_read(str(tmp_path / "empty.xtc").encode(), C.byref(fa.XtcInfoC()), None, 0) == -1


def test_header_walker_under_sanitizers_stand_alone(tmp_path):
    """csrc/xtc.c compiled with -fsanitize=address,undefined into a program of its own, run as a child process over good files,
    every refused file, a three-frame file cut at every length and with every header word of its second frame overwritten: exit
    status 0, no sanitizer report, one line of verdict per file - the library's verdict"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/xtc_check"], check=True, stdout=subprocess.DEVNULL)
    paths = []
    for n in (10, 37, 516):
        xtc_file(tmp_path / f"good{n}.xtc", n, 5, n)
        paths.append(tmp_path / f"good{n}.xtc")
    paths += [p for _, p, _, _ in refused_files(tmp_path)] + [tmp_path / "good.xtc", tmp_path / "does_not_exist.xtc"]
    good = xtc_file(tmp_path / "three.xtc", 10, 3, 1)
    second = xc.decode(good)[1].offset
    fuzz = tmp_path / "fuzz"
    fuzz.mkdir()
    for cut in range(len(good)):
        (fuzz / f"cut{cut}.xtc").write_bytes(good[:cut])
        paths.append(fuzz / f"cut{cut}.xtc")
    for at in range(second, second + xc.HEADER, 4):
        for v in (0, 0x7fffffff, 0x80000000, 0xffffffff, 0x7fc00000):
            p = fuzz / f"word{at}_{v:x}.xtc"
            p.write_bytes(good[:at] + struct.pack(">I", v) + good[at + 4:])
            paths.append(p)
    res = subprocess.run([os.path.join(ROOT, "tests", "emu", "xtc_check")] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(paths)
    n_ok = 0
    for line, p in zip(lines, paths):
        try:
            info = fa.xtc_info(p)
            want = f"ok {info.n_atoms} {info.n_frames} {info.max_frame_bytes} {float(info.precision).hex()} {int(info.has_box)} {os.path.getsize(p)}"
            assert line.split()[:4] == want.split()[:4] and line.split()[5:] == want.split()[5:], (p, line, want)
            assert float.fromhex(line.split()[4]) == info.precision
            n_ok += 1
        except ValueError as e:
            assert line == "refused " + str(e).split(": ", 1)[1], (p, line)
    frames = xc.decode(good)
    whole = {0: None, frames[1].offset: 1, frames[2].offset: 2, len(good): 3}
    for cut in range(len(good)):                                   # a cut between two frames is a shorter file, every other one is refused
        line = lines[paths.index(fuzz / f"cut{cut}.xtc")]
        assert line.startswith("ok 10 %d " % whole[cut]) if whole.get(cut) else line.startswith("refused "), (cut, line)
    assert n_ok > 40                                               # (step, time, box: harmless words)


def records_as_trace(rec):
    return [tuple(int(v) for v in r) for r in rec]


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_kernels_equal_the_codec(name):
    """group records = the codec's trace; fp32 output = the codec's, bit for bit; every element of the NaN-prefilled output written"""
    datas = [case_frame(name, seed=s)[3] for s in (7, 8)]
    if name == "runs 0..8":                                        # every remainder of the byte count, and frames of unequal length in one shard
        datas += [case_frame(name, n=n)[3] for n in range(45, 53)]
    for data in datas:
        (f,) = xc.decode(data)
        rec, status, xyz = xtc_emu.decode(data, 1, f.natoms)
        assert status[0] == 0
        assert records_as_trace(rec[0]) == f.trace
        assert not np.isnan(xyz).any() and xyz[0].tobytes() == f.xyz.tobytes()


def test_emulated_kernels_on_a_shard_of_unequal_frames_and_a_long_stream():
    """several frames in one call, as the driver cuts a shard: every frame's stream at its own offset; and a stream longer than the
    scan's window of 2 KiB (3000 atoms), so that the window moves more than once"""
    for n, n_frames in ((37, 5), (516, 3), (3000, 2)):
        data = b"".join(xc.encode(ints, 1000.0) for ints in jittered_ints(n, n_frames, n))
        frames = xc.decode(data)
        assert len({f.size for f in frames}) > 1 and (n < 3000 or min(f.bytecount for f in frames) > 2 * 2048)
        rec, status, xyz = xtc_emu.decode(data, n_frames, n)
        assert not status.any() and not np.isnan(xyz).any()
        for k, f in enumerate(frames):
            assert records_as_trace(rec[k]) == f.trace and xyz[k].tobytes() == f.xyz.tobytes()
    with pytest.raises(ValueError, match="it holds 3000 atoms, frame 0 holds 2999"):
        xtc_emu.decode(data, 2, 2999)


def fnv1a(b):
    h = 1469598103934665603
    for v in b:
        h = ((h ^ v) * 1099511628211) & 0xffffffffffffffff
    return h


def mutants(n_mutants=2000, seed=11):
    """(frame bytes with a valid header, stream): streams of 20-atom frames with one to three bits flipped, or cut short"""
    rng = np.random.default_rng(seed)
    bases = []
    for name in ("runs 0..8", "smallidx up and down", "smallidx held at 9", "smallidx up to 72", "bitsize 0", "a flag-0 group inherits its run"):
        plan, smallidx, kw = CASES[name]
        plan = [g for g in plan if g[0] < 6][:5]
        plan = pad_plan(plan, max(20, sum(1 + k for k, _ in plan)))
        ints = synth(plan, smallidx, 3, **kw)
        bases.append(xc.decode(xc.encode(ints, 1000.0, plan=plan, smallidx=smallidx))[0])
    out = []
    for k in range(n_mutants):
        f = bases[k % len(bases)]
        s = bytearray(f.stream)
        if k % 4 == 3:
            s = s[:int(rng.integers(0, len(s)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                bit = int(rng.integers(0, 8 * len(s)))
                s[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((f, bytes(s)))
    return out


def test_damaged_streams_decode_as_the_codec_does_or_get_a_status(tmp_path):
    """the emulation, stand-alone under AddressSanitizer + UBSan (not loaded into Python), over about 2000 streams with valid
    headers: no sanitizer report; a frame whose status is 0 is, records and values, what the codec decodes"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/xtc_emu_check"], check=True, stdout=subprocess.DEVNULL)
    ms = mutants()
    by_atoms = {}
    for f, s in ms:
        by_atoms.setdefault(f.natoms, []).append((f, s))
    n_same = n_status = 0
    for natoms, group in by_atoms.items():                         # (a file holds frames of one atom count)
        p = tmp_path / f"mutants{natoms}.xtc"
        p.write_bytes(b"".join(xc.frame_bytes(f.natoms, 0, 0.0, np.zeros((3, 3)), float(f.precision), f.minint, f.maxint, f.smallidx, s) for f, s in group))
        res = subprocess.run([os.path.join(ROOT, "tests", "emu", "xtc_emu_check"), str(p)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr[-2000:]
        assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
        lines = res.stdout.splitlines()
        assert len(lines) == len(group)
        for k, (line, (f, s)) in enumerate(zip(lines, group)):
            w = line.split()
            assert w[0] == "frame" and int(w[1]) == k and w[2] == "status", line
            try:
                ints, trace = xc.decode_stream(s, f.natoms, f.minint, f.maxint, f.smallidx)
            except ValueError:
                ints = None
            if int(w[3]) != 0:
                n_status += 1
                assert ints is None, (k, line)                     # (more than is asked: the two agree on what is damaged, too)
                continue
            assert ints is not None, (k, line)
            rec = np.array(trace, dtype=np.int32).reshape(-1, 4)
            assert int(w[5]) == len(trace) and int(w[7], 16) == fnv1a(rec.tobytes()) and int(w[9], 16) == fnv1a(xc.to_angstrom(ints, f.precision).tobytes()), (k, line)
            n_same += 1
    assert n_same + n_status == len(ms) and n_same > 100 and n_status > 500


def test_driver_argument_errors_come_before_any_device_or_file(tmp_path):
    """through the four file entries: -1 with the message, and no output file"""
    L = fa._topology_proto(fa.lib())
    batch = ingest.load_pdb_files([os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb")])
    n = int(batch.n_atoms)
    cb = batch._as_c()
    devs = np.zeros(1, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    boxed, bare = tmp_path / "frames.xtc", tmp_path / "bare.xtc"
    xtc_file(boxed, n + 41, 2, 5, boxes=[np.diag([9.0, 9.0, 9.0])] * 2)
    xtc_file(bare, n + 41, 2, 5)
    radii = np.full(n + 41, 1.5)
    enc = lambda p: str(p).encode()
    outs = [tmp_path / f"{k}.bin" for k in ("totals", "sasa", "cls", "res")] + [tmp_path / "done.txt"]
    X = fa.FRAMES_XTC
    assert X == 64
    ok = dict(header=0, n_plain=n + 41, frame_atoms=n + 41, path=boxed)
    GROUPS = "not offered with chain groups"
    cases = [("atom count", dict(ok, bits=X, n_plain=n + 40, frame_atoms=n + 42), None, None),
             ("header_bytes", dict(ok, bits=X, header=8), "header_bytes must be 0 with an XTC file", None),
             ("bit 0", dict(ok, bits=X | 1), "bit 0 of frames_f32 (raw fp32 frames) and bit 6", None),
             ("bit 0 and fp32 output", dict(ok, bits=X | 3), "bit 0", None),
             ("bit 2", dict(ok, bits=X | 4), "bit 2 of frames_f32 (a DCD file) and bit 6", None),
             ("bit 5", dict(ok, bits=X | 32), "bit 5 of frames_f32 (an AMBER NetCDF file) and bit 6", None),
             ("bit 3 with a zero box", dict(ok, bits=X | 8, path=bare), "first frame is all zero", GROUPS),
             ("bits 3 and 4 with a zero box", dict(ok, bits=X | 24, path=bare), "first frame is all zero", GROUPS),
             ("bit 4 without bit 3", dict(ok, bits=X | 16), "bit 4 of frames_f32 (triclinic cells) needs bit 3", GROUPS),
             ("chain groups with bit 3", dict(ok, bits=X | 8), "", GROUPS)]
    index = np.arange(n, dtype=np.int32)
    for what, kw, text, groups_text in cases:
        path = kw["path"]
        if text != "":
            err = C.create_string_buffer(512)
            rc = L.freesasa_gpu_trajectory_file(enc(path), kw["bits"], kw["header"], radii.ctypes.data_as(dp), kw["n_plain"], 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                                enc(outs[0]), enc(outs[1]), enc(outs[4]), 0, 0, None, err, 512)
            msg = err.value.decode()
            assert rc == -1 and (text in msg if text else (str(n + 41) in msg and str(kw["n_plain"]) in msg and "XTC" in msg)), (what, msg)
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
            assert rc == -1 and (text in msg if text else (str(n + 41) in msg and str(kw["frame_atoms"]) in msg and "XTC" in msg)), (what, msg)
        ids = np.zeros(n, dtype=np.int32)
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file_groups(enc(path), kw["bits"], kw["header"], 0, C.byref(cb), 0, kw["frame_atoms"],
                                                   index.ctypes.data_as(C.POINTER(C.c_int32)), None, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                                   fa.LEE_RICHARDS, 1.4, 20, 0, enc(outs[0]), enc(outs[1]), enc(outs[2]), enc(outs[3]), None, None,
                                                   enc(outs[2]), None, enc(outs[4]), 0, devs.ctypes.data_as(ip), 1, None, err, 512)
        assert rc == -1 and (groups_text in err.value.decode() if groups_text else err.value.decode() == msg), (what, err.value)
        assert not any(p.exists() for p in outs), what
    # a file that is no XTC file, and one with a damaged header: the index pass's message, through the driver
    raw = tmp_path / "frames.f32"
    np.zeros((2, n + 41, 3), dtype=np.float32).tofile(raw)
    damaged = tmp_path / "damaged.xtc"
    data = bytearray(boxed.read_bytes())
    struct.pack_into(">i", data, xc.decode(bytes(data))[1].offset + 84, 99)
    damaged.write_bytes(bytes(data))
    for path, text in ((raw, "frame 0 of the XTC file: its magic number is 0, not 1995"), (damaged, "frame 1 of the XTC file: its smallidx is 99")):
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_trajectory_file(enc(path), X, 0, radii.ctypes.data_as(dp), n + 41, 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                            enc(outs[0]), None, None, 0, 0, None, err, 512)
        assert rc == -1 and text in err.value.decode() and not outs[0].exists(), err.value
    # the Python keywords: what cannot go with xtc=True is refused before the library is asked
    for kw in (dict(f32=True), dict(header_bytes=8), dict(dcd=True), dict(netcdf=True)):
        with pytest.raises(ValueError, match="xtc=True"):
            fa.trajectory_file(boxed, radii, outs[0], xtc=True, **kw)
        with pytest.raises(ValueError, match="xtc=True"):
            fa.trajectory_file_topology(boxed, batch, outs[0], atom_index=index, xtc=True, **kw)
    assert not any(p.exists() for p in outs)


def test_decode_hook_argument_errors_come_with_their_messages_and_without_a_device():
    """freesasa_gpu_xtc_decode_check is what freesasa_gpu_xtc_decode_dev (the test hook of tests/test_xtc_decode_gpu.py) refuses
    before its first device call: host only; the hook copies the message into its context's error text.  Without a context the
    hook has nowhere to put one."""
    L = fa.lib()
    _, _, ints, data = case_frame("ten atoms")
    n = len(ints)
    rec, count, out = np.zeros((n, 4), dtype=np.int32), np.zeros(2, dtype=np.int32), np.full((n, 3), np.nan, dtype=np.float32)
    good = dict(bytes=data, len=len(data), n_frames=1, n_atoms=n, rec=rec.ctypes.data, count=count.ctypes.data, out=out.ctypes.data)

    def check(**kw):
        a = dict(good, **kw)
        err = C.create_string_buffer(b"untouched", 200)
        rc = L.freesasa_gpu_xtc_decode_check(a["bytes"], a["len"], a["n_frames"], a["n_atoms"], a["rec"], a["count"], a["out"], err, 200)
        return rc, err.value.decode()

    assert check() == (0, "")
    for kw, text in ((dict(bytes=None), "null argument"), (dict(rec=None), "null argument"), (dict(count=None), "null argument"),
                     (dict(out=None), "null argument"), (dict(n_frames=0), "n_frames must be at least 1"), (dict(n_frames=-3), "n_frames must be at least 1"),
                     (dict(n_atoms=0), "n_atoms must be at least 1"), (dict(n_atoms=-1), "n_atoms must be at least 1"),
                     (dict(len=0), "len must be at least 1"), (dict(len=-92), "len must be at least 1"),
                     (dict(n_frames=1 << 16, n_atoms=1 << 15), "n_frames * n_atoms does not fit an int"),
                     (dict(n_frames=2 ** 31 - 1, n_atoms=2 ** 31 - 1), "n_frames * n_atoms does not fit an int")):
        assert check(**kw) == (-1, "xtc_decode: " + text), kw
    assert check(n_frames=(1 << 16) - 1, n_atoms=1 << 15) == (0, "")               # (2^31 - 2^15 slots: the most an int holds, nearly)
    # a short message buffer, and none
    err = C.create_string_buffer(8)
    assert L.freesasa_gpu_xtc_decode_check(None, 1, 1, 10, None, None, None, err, 8) == -1 and err.value == b"xtc_dec"
    assert L.freesasa_gpu_xtc_decode_check(None, 1, 1, 10, None, None, None, None, 0) == -1
    assert L.freesasa_gpu_xtc_decode_dev(None, data, len(data), 1, n, rec.ctypes.data, count.ctypes.data, out.ctypes.data) == -1
    assert not rec.any() and not count.any() and np.isnan(out).all()
