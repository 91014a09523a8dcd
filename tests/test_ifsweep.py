"""The file sweep's interface kernels on the CPU (freesasa_amd/csrc/ifsweep_kernels.h through tests/emu/emu_ifsweep.cpp, grid for
grid as gpu_kernels.hip launches them) against their numpy restatement (tests/ifsweep_ref.py), byte for byte; the same phases
under sanitizers in a program of its own; and the refusals of freesasa_gpu_sweep_files_interfaces through the C ABI, which need
no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import freesasa_amd as fa
from freesasa_amd import ingest
import ifsweep_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
_dp, _lp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_ubyte)
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ROOT, "tests/emu/libifsweep_emu.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(EMU, "libifsweep_emu.so"))
        _lib.emu_ifs_side_class.argtypes = [_ip, C.c_longlong, _bp, _bp]
        _lib.emu_ifs_side_class_sums.argtypes = [_ip, C.c_longlong, _bp, _dp, _lp, C.c_int, _dp]
        _lib.emu_ifs_res_rows.argtypes = [C.c_longlong, C.c_longlong, _lp, _ip, _lp, _lp, C.c_longlong, C.c_longlong, _ip, _bp, _bp, _ip, _bp]
    return _lib


def ptr(a, t):
    return a.ctypes.data_as(t) if a is not None and a.size else None


# ------------------------------------------------------------------------------------------------ 1. the gather and the class sums

@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_side_class_and_its_sums(M):
    assert emu().emu_ifsweep_threads() == 256
    rng = np.random.default_rng(M)
    n = 400
    cls = rng.integers(0, 3, n).astype(np.uint8)
    assert M < 3 or set(cls.tolist()) == {0, 1, 2}
    pair_atom = rng.integers(0, n, M).astype(np.int32)
    pair_atom[-1] = n - 1                                         # the last input atom is somebody's
    got = np.full(M + 1, 0xEE, np.uint8)                          # (a guard behind the M bytes)
    assert emu().emu_ifs_side_class(ptr(pair_atom, _ip), M, ptr(cls, _bp), ptr(got, _bp)) == 0
    assert got[M] == 0xEE and got[:M].tobytes() == ref.side_class(pair_atom, cls).tobytes()
    # the sides' class sums behind it, in the class-sum kernel's order: empty sides at the start, in the middle and at the end
    buried = rng.uniform(0, 40, M)
    cuts = np.sort(rng.integers(0, M + 1, 3))
    side_off = np.array([0, 0, cuts[0], cuts[1], cuts[1], cuts[2], M, M], np.int64)
    out = np.full(3 * 7 + 1, np.nan)
    assert emu().emu_ifs_side_class_sums(ptr(pair_atom, _ip), M, ptr(cls, _bp), ptr(buried, _dp), ptr(side_off, _lp), 7, ptr(out, _dp)) == 0
    want = ref.class_sums(buried, ref.side_class(pair_atom, cls), side_off)
    assert np.isnan(out[-1]) and out[:-1].tobytes() == want.reshape(-1).tobytes()
    assert np.all(want[[0, 3, 6]] == 0)


# ------------------------------------------------------------------------------------------------ 2. the rows

def labels(rng, n, odd):
    """n residues' label bytes: names [n, 4], chains [n, 4], numbers [n, 6]; bytes >= 0x80, blanks, and - odd - an insertion code"""
    name = rng.integers(0x20, 0x100, (n, 4)).astype(np.uint8)
    chain = rng.integers(0x20, 0x100, (n, 4)).astype(np.uint8)
    number = np.frombuffer(b"".join(b"%4d%s " % (k % 10000, b"A" if odd and k % 3 == 0 else b" ") for k in range(n)), np.uint8).reshape(n, 6).copy()
    if n:
        name[::5] = 0x20                                          # blank names
        chain[::7, 1:] = 0                                        # a one-letter chain as the loader pads it
        name[n // 2] = [0x80, 0xFF, 0xC3, 0xA9]
    return name, chain, number


def make_case(R, share, seed, n_structs=9):
    """n_structs structures: structure 1 has no atoms and lies between two that have pairs; the first and the last have pairs;
    structure 4 has atoms and no pair; residues of 1 .. 4 atoms; `share` of the residues are the device parser's.  R rows dealt
    to the sides so that the first side, a side in the middle and the last side have none (ties of the search)."""
    rng = np.random.default_rng(seed)
    offsets, res_first, first_res = [0], [], []
    for s in range(n_structs):
        first_res.append(len(res_first))
        at = offsets[-1]
        for _ in range(0 if s == 1 else int(rng.integers(2, 9))):
            res_first.append(at)
            at += int(rng.integers(1, 5))
        offsets.append(at)
    n_res = len(res_first)
    first_res.append(n_res)
    res_first.append(offsets[-1])
    pair_struct = [0, 0, 2, 3, 3, 5, 6, n_structs - 1]
    n_sides = 2 * len(pair_struct)
    free = [q for q in range(n_sides) if q not in (0, n_sides // 2, n_sides - 1)]
    per = np.bincount(rng.choice(free, R), minlength=n_sides) if R > 1 else np.bincount([n_sides - 2], minlength=n_sides)
    res_off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    res_index = np.zeros(R, np.int32)
    for q in range(n_sides):
        s = pair_struct[q // 2]
        res_index[res_off[q]:res_off[q + 1]] = rng.integers(first_res[s], first_res[s + 1], per[q])
    Rd = int(round(share * n_res))
    return dict(R=R, n_sides=n_sides, res_off=res_off, pair_struct=np.array(pair_struct, np.int32), offsets=np.array(offsets, np.int64),
                res_first=np.array(res_first, np.int64), n_res=n_res, Rd=Rd, res_index=res_index, first_res=first_res,
                lab_d=labels(rng, Rd, True), lab_h=labels(rng, n_res - Rd, False))


def run_rows(c):
    R = c["R"]
    planes = lambda lab: np.concatenate([a.reshape(-1) for a in lab]) if lab[0].size else None
    local = np.full(R + 1, -7, np.int32)
    out = np.full(14 * R + 2, 0xEE, np.uint8)
    rc = emu().emu_ifs_res_rows(R, c["n_sides"], ptr(c["res_off"], _lp), ptr(c["pair_struct"], _ip), ptr(c["offsets"], _lp), ptr(c["res_first"], _lp),
                                c["n_res"], c["Rd"], ptr(c["res_index"], _ip), ptr(planes(c["lab_d"]), _bp) if c["Rd"] else None,
                                ptr(planes(c["lab_h"]), _bp) if c["Rd"] < c["n_res"] else None, ptr(local, _ip), ptr(out, _bp))
    assert rc == 0 and local[R] == -7 and np.all(out[14 * R:] == 0xEE)
    return local[:R], out[:4 * R].reshape(R, 4), out[4 * R:8 * R].reshape(R, 4), out[8 * R:14 * R].reshape(R, 6)


def same_rows(c):
    got = run_rows(c)
    want = ref.res_rows(c["res_off"], c["pair_struct"], c["offsets"], c["res_first"], c["Rd"], c["res_index"], c["lab_d"], c["lab_h"])
    for g, w, what in zip(got, want, ("place", "names", "chains", "numbers")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what
    return got


@pytest.mark.parametrize("R", [1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("share", [0.5, 0.0, 1.0], ids=["both-parsers", "Rd=0", "Rh=0"])
def test_rows_equal_the_restatement(R, share):
    c = make_case(R, share, 1000 * R + int(10 * share))
    local, name, chain, number = same_rows(c)
    assert local.min() >= 0
    if R >= 63:     # the sides without a row are ties of the search; the first and the last structure own rows
        per = np.diff(c["res_off"])
        assert per[0] == 0 and per[c["n_sides"] // 2] == 0 and per[-1] == 0 and per[1] > 0 and per[-2] > 0
        assert (number[:, 4] == ord("A")).any() == (share > 0)    # a number with an insertion code came through


def test_rows_at_the_seam_between_the_parsers():
    """rows whose residue is Rd - 1 and Rd, in a structure that holds the seam"""
    c = make_case(64, 0.5, 7)
    s = 3                                                                 # a structure with pairs: the seam goes behind its first residue
    Rd = c["first_res"][s] + 1
    c["Rd"], c["lab_d"], c["lab_h"] = Rd, labels(np.random.default_rng(1), Rd, True), labels(np.random.default_rng(2), c["n_res"] - Rd, False)
    assert c["first_res"][s] < Rd < c["first_res"][s + 1]
    q = 2 * c["pair_struct"].tolist().index(s) + 1
    rows = slice(int(c["res_off"][q]), int(c["res_off"][q + 1]))
    assert rows.stop - rows.start >= 2
    c["res_index"][rows.start], c["res_index"][rows.start + 1] = Rd - 1, Rd
    local, name, chain, number = same_rows(c)
    assert local[rows.start] + 1 == local[rows.start + 1] == Rd - c["first_res"][s]
    assert name[rows.start].tobytes() == c["lab_d"][0][Rd - 1].tobytes() and name[rows.start + 1].tobytes() == c["lab_h"][0][0].tobytes()


def test_the_phases_under_sanitizers():
    """tests/emu/ifsweep_check: a program of its own built with -fsanitize=address,undefined; one line per case"""
    subprocess.run(["make", "-C", ROOT, "tests/emu/ifsweep_check"], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(EMU, "ifsweep_check")], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(lines) >= 28 and all(" ok " in l for l in lines), out.stdout


# ------------------------------------------------------------------------------------------------ 3. the refusals, without a device

def test_refusals_through_the_c_abi():
    L = fa._ifsweep_proto(fa.lib())
    arr = (C.c_char_p * 1)(b"does_not_exist.pdb")
    tot, st, gst, ist = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    ip = C.POINTER(C.c_int)

    def call(spec=None, flags=ingest.SEPARATE_CHAINS, min_buried=0.0, gstatus=gst, istatus=ist, table=True, alg=0, devices=None, n_devices=0):
        g, t = fa.GroupTableC(), fa.InterfaceTableC()
        C.memset(C.byref(g), 0x5a, C.sizeof(g))
        C.memset(C.byref(t), 0x5a, C.sizeof(t))
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_sweep_files_interfaces(arr, 1, 0, 1, alg, 1.4, 20, 0, tot.ctypes.data_as(_dp), None, None, st.ctypes.data_as(ip),
                                                   devices, n_devices, None, spec, flags, None if gstatus is None else gstatus.ctypes.data_as(ip),
                                                   C.byref(g), 1, min_buried, None if istatus is None else istatus.ctypes.data_as(ip),
                                                   C.byref(t) if table else None, err, 512)
        assert rc == -1 and bytes(g) == bytes(C.sizeof(g)) and (not table or bytes(t) == bytes(C.sizeof(t))), "tables not zeroed after a refusal"
        return err.value.decode()

    # the group entry's own, with its messages
    gerr = C.create_string_buffer(512)
    g = fa.GroupTableC()
    Lg = fa._groups_proto(fa.lib())
    for spec, flags in ((b"A+A", 0), (b"A++B", 0), (b"A+B", ingest.SEPARATE_CHAINS), (None, 0), (b"A+B", 1 << 20)):
        assert Lg.freesasa_gpu_sweep_files_groups(arr, 1, 0, 1, 0, 1.4, 20, 0, tot.ctypes.data_as(_dp), None, None, st.ctypes.data_as(ip), None, 0, None,
                                                  spec, flags, gst.ctypes.data_as(ip), C.byref(g), gerr, 512) == -1
        assert gerr.value and call(spec, flags) == gerr.value.decode(), spec
    assert call(gstatus=None) == "null argument"
    # min_buried, with the per-residue entry's message
    for bad in (-1.0, float("nan"), float("inf"), -0.5e-300):
        assert call(min_buried=bad) == "min_buried must be finite and >= 0"
    assert call(istatus=None) == "null argument" and call(table=False) == "null argument"
    # ... and behind them the sweep's own, still before a device is touched
    assert call(alg=7) == "unknown algorithm"
    one = (C.c_int * 1)(10 ** 6)
    assert call(devices=one, n_devices=1)
