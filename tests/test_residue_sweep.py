"""The file sweep with a per-residue table (freesasa_gpu_sweep_files_residues, include/freesasa_gpu.h): absolute and relative
areas per residue for all files of a sweep, the per-atom areas never leaving the device, the residues themselves - boundaries,
labels, reference rows, backbone flags - built ON THE DEVICE when the device parses (csrc/gpu_parse.hip, kp_res_*).

The bars: the reference-minted vectors of the loader (tests/golden/ingest.json: res_first, labels, has_reference), the long
way round bit for bit (ingest.load_files -> calc_batch -> GpuContext.residue_areas: per-atom areas do not depend on the batch,
and k_residue_areas sums a residue in atom order in one thread - so equality is derived, not measured), and the reference
CLI's own --format=rsa / --format=seq outputs."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import freesasa_amd as fa
from freesasa_amd import ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDB = os.path.join(ROOT, "tests", "golden", "pdb")
CIF = os.path.join(ROOT, "tests", "golden", "cif")
CFG = os.path.join(ROOT, "tests", "golden", "classifiers")
with open(os.path.join(ROOT, "tests", "golden", "ingest.json")) as fh:
    GOLD = json.load(fh)
DEV = ingest.PARSE_ON_DEVICE

# (tests/test_device_parser.py) files the device is expected to parse itself under the default options
MUST_PARSE = {"1ubq.pdb", "1a0q.pdb", "3bkr.pdb", "3bzd_trimmed.pdb", "5dx9.pdb", "1d3z.pdb", "2jo4.pdb", "3gnn.pdb", "icode.pdb",
              "alt_model_twochain.pdb", "1ubq.cif", "3bkr.cif", "5dx9.cif", "7cma-assembly1.cif",
              "syn_altloc_icode_chain.pdb", "syn_altloc_icode_chains.cif", "syn_models_out_of_order.cif"}


def fixture(name):
    return os.path.join(CIF if name.endswith(".cif") else PDB, name)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def labels_digest(b, lo=0, hi=None):
    """(tests/test_ingest.py) b: anything with res_name / res_number / res_chain lists"""
    hi = b.n_residues if hi is None else hi
    name, number, chain = b.res_name, b.res_number, b.res_chain
    return hashlib.sha256("\n".join(f"{name[k]}|{number[k]}|{chain[k]}" for k in range(lo, hi)).encode()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_results(want, got, what=""):
    """totals, class sums, atoms, status of two sweeps: the same bits (model_mismatch.pdb under JOIN_MODELS has coinciding atoms:
    its total is NaN in every sweep, and NaN == NaN here)"""
    for x, y, name in zip(want[:4], got[:4], ("totals", "class sums", "atoms", "status")):
        if x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y)), (name, what)
        else:
            assert np.array_equal(x, y), (name, what)


# ------------------------------------------------------------------------------------------------ CPU: the C boundary

def _lib():
    fa.build()
    return fa._residue_proto(fa.lib())


def test_symbols_are_declared_and_exported():
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", fa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "freesasa_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for sym in ("freesasa_gpu_sweep_files_residues", "freesasa_gpu_residue_table_free"):
        assert sym in exported, sym
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
    assert "typedef struct freesasa_gpu_residue_table" in header


def test_table_struct_layout_matches_the_header():
    T = fa.ResidueTableC
    # int32_t, int64_t, then eight pointers: 80 bytes on LP64
    want = [("n_files", 0, 4), ("n_residues", 8, 8), ("res_offsets", 16, 8), ("res_atoms", 24, 8), ("res_ref", 32, 8),
            ("abs", 40, 8), ("rel", 48, 8), ("res_name", 56, 8), ("res_number", 64, 8), ("res_chain", 72, 8)]
    assert C.sizeof(T) == 80
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, _ in T._fields_] == want
    # the header's member order is the ctypes order
    header = open(os.path.join(ROOT, "include", "freesasa_gpu.h")).read()
    body = re.search(r"typedef struct freesasa_gpu_residue_table \{(.*?)\} freesasa_gpu_residue_table;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\*?\b(\w+)\s*(?=[,;])", body)
    assert members == [n for n, _ in T._fields_], members


def _raw_call(L, paths, totals, status, table, n=1):
    devs = (C.c_int * 1)(0)
    err = C.create_string_buffer(256)
    rc = L.freesasa_gpu_sweep_files_residues(paths, n, 0, 1, 0, 1.4, 20, 0, totals, None, None, status, devs, 1, None, table, err, 256)
    return rc, err.value.decode()


def test_null_arguments_are_refused_and_the_table_is_zeroed():
    L = _lib()
    paths = (C.c_char_p * 1)(fixture("1ubq.pdb").encode())
    totals, status = (C.c_double * 1)(), (C.c_int * 1)()
    dp, ip = C.cast(totals, C.POINTER(C.c_double)), C.cast(status, C.POINTER(C.c_int))

    def dirty():
        t = fa.ResidueTableC()
        C.memset(C.byref(t), 0x5a, C.sizeof(t))
        return t
    for args in ((None, dp, ip), (paths, None, ip), (paths, dp, None)):
        t = dirty()
        rc, msg = _raw_call(L, args[0], args[1], args[2], C.byref(t))
        assert rc == -1 and "null argument" in msg, (rc, msg)
        assert bytes(t) == bytes(C.sizeof(t)), "table not zeroed"
    rc, msg = _raw_call(L, paths, dp, ip, None)
    assert rc == -1 and "null argument" in msg
    # freeing a zeroed table, or none, does nothing
    t = fa.ResidueTableC()
    L.freesasa_gpu_residue_table_free(C.byref(t))
    L.freesasa_gpu_residue_table_free(C.byref(t))
    L.freesasa_gpu_residue_table_free(None)
    assert bytes(t) == bytes(C.sizeof(t))


def test_new_code_does_not_reference_the_oracle():
    """(tests/test_capi.py::test_product_never_references_the_oracle keeps passing: the same scan over the files this adds to)"""
    for rel in ("freesasa_amd/csrc/gpu_parse.hip", "freesasa_amd/csrc/gpu_drivers.hip", "freesasa_amd/csrc/gpu_frames.hip", "freesasa_amd/csrc/gpu_sweep.hip", "freesasa_amd/csrc/gpu_ops.hip", "freesasa_amd/__init__.py"):
        txt = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"#include\s+\"[^\"]*oracle|import\s+oracle|from\s+oracle|sasa_oracle|libsasa_emu", txt), rel


# ------------------------------------------------------------------------------------------------ GPU

gpu = pytest.mark.gpu


def long_way(paths, alg, res, opt=0, classifier=None):
    """ingest.load_files -> calc_batch -> GpuContext.residue_areas: (batch, abs [R, 6], rel [R, 5])"""
    import torch
    b = ingest.load_files(paths, options=opt, n_threads=4, classifier=classifier)
    keep = np.nonzero(b.status == 0)[0]
    offs = np.concatenate([[0], np.cumsum(np.diff(b.offsets)[keep])]).astype(np.int64)   # (failed inputs own no atoms)
    sasa, _, _ = fa.calc_batch(b.xyz, b.radii, offs, alg, resolution=res)
    dev = torch.device("cuda:0")
    d_sasa = torch.from_numpy(sasa).to(dev)
    d_cls, d_bb = torch.from_numpy(b.atom_class).to(dev), torch.from_numpy(b.atom_backbone).to(dev)
    d_abs = torch.empty(6 * b.n_residues, dtype=torch.float64, device=dev)
    d_rel = torch.empty(5 * b.n_residues, dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0)
    ctx.residue_areas(d_sasa.data_ptr(), d_cls.data_ptr(), d_bb.data_ptr(), b.res_first, d_abs.data_ptr(),
                      res_ref=b.res_ref, ref_table=ingest.residue_reference_table(), d_rel=d_rel.data_ptr())
    ctx.close()
    return b, d_abs.cpu().numpy().reshape(-1, 6), d_rel.cpu().numpy().reshape(-1, 5)


def same_table(t, b, A, R, what):
    assert t.n_residues == b.n_residues and t.n_files == b.n_structs, what
    assert np.array_equal(t.res_offsets, b.res_offsets), what
    assert np.array_equal(t.res_atoms, np.diff(b.res_first)), what
    assert np.array_equal(t.res_ref, b.res_ref), what
    assert t.res_name_raw.tobytes() == b.res_name_raw.tobytes() and t.res_number_raw.tobytes() == b.res_number_raw.tobytes() and \
        t.res_chain_raw.tobytes() == b.res_chain_raw.tobytes(), what
    assert np.array_equal(bits(t.abs), bits(A)), what
    nan_t, nan_r = np.isnan(t.rel), np.isnan(R)
    assert np.array_equal(nan_t, nan_r), what                                             # NaN == NaN
    assert np.array_equal(bits(t.rel)[~nan_t], bits(R)[~nan_r]), what


def tables_equal(a, b):
    for f in ("res_offsets", "res_atoms", "res_ref", "res_name_raw", "res_number_raw", "res_chain_raw"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert bits(a.abs).tobytes() == bits(b.abs).tobytes() and bits(a.rel).tobytes() == bits(b.rel).tobytes()


@gpu
@pytest.mark.parametrize("name", sorted(GOLD))
def test_residues_built_on_the_device_are_the_references(name):
    fa.sweep_parse_stats()
    on_device = 0
    for opt, exp in GOLD[name].items():
        if exp.get("crash"):
            continue
        totals, cls, atoms, status, t = fa.sweep_files_residues([fixture(name)], ingest_options=int(opt) | DEV)
        dev, host = fa.sweep_parse_stats()
        assert dev + host == 1
        on_device += dev
        if int(opt) == 0 and name in MUST_PARSE:
            assert (dev, host) == (1, 0), (name, "left to the host parser")
        assert t.n_files == 1 and t.res_offsets.tolist() == [0, t.n_residues]
        if exp.get("fail"):
            assert status[0] != ingest.OK and t.n_residues == 0 and atoms[0] == 0, (name, opt, status[0])
            continue
        assert status[0] == ingest.OK and atoms[0] == exp["n_atoms"], (name, opt, status[0])
        assert t.n_residues == exp["n_residues"], (name, opt, t.n_residues)
        res_first = np.concatenate([[0], np.cumsum(t.res_atoms)]).astype(np.int64)
        assert sha(res_first) == exp["res_first"], (name, opt)
        assert labels_digest(t) == exp["labels"], (name, opt)
        assert sha((t.res_ref >= 0).astype(np.uint8)) == exp["has_reference"], (name, opt)
    if name in MUST_PARSE:
        assert on_device >= 8, (name, on_device)      # (RADIUS_FROM_OCCUPANCY is the host's)


@gpu
@pytest.mark.parametrize("alg, res", [(fa.LEE_RICHARDS, 20), (fa.SHRAKE_RUPLEY, 100)])
def test_same_numbers_as_the_long_way_round_bit_for_bit(alg, res):
    names = sorted(GOLD) + ["does_not_exist.pdb"]
    paths = [fixture(n) for n in names]
    for opt in (0, ingest.INCLUDE_HETATM | ingest.INCLUDE_HYDROGEN, ingest.JOIN_MODELS, ingest.SKIP_UNKNOWN, ingest.HALT_AT_UNKNOWN):
        b, A, R = long_way(paths, alg, res, opt)
        for parser in (DEV, 0):
            # (the engine shapes a launch by what the context's previous batch taught it, and on the superposed models of
            # JOIN_MODELS two shapes differ in an area's last bits: both sweeps below run behind the same batch)
            fa.sweep_files(paths, alg, resolution=res, ingest_options=opt | parser, n_threads=4)
            fa.sweep_parse_stats()
            got = fa.sweep_files_residues(paths, alg, resolution=res, ingest_options=opt | parser, n_threads=4)
            dev, host = fa.sweep_parse_stats()
            if parser:
                assert dev >= 25 and dev + host == len(paths), (opt, dev, host)
            same_table(got[4], b, A, R, (alg, opt, parser))
            want = fa.sweep_files(paths, alg, resolution=res, ingest_options=opt | parser, n_threads=4)
            same_results(want, got, (alg, opt, parser))
            # the main / side chain columns are the backbone flags' doing
            assert np.array_equal(bits(got[4].abs[:, 1] + got[4].abs[:, 2]), bits(A[:, 1] + A[:, 2]))


def read_rsa(name):
    """(tests/test_ingest.py) rows of a reference --format=rsa file and its TOTAL line; rel None where the file says N/A"""
    rows, total = [], None
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        for line in fh:
            if line.startswith("RES "):
                res, chain, number = line[4:7], line[8:11].strip(), line[11:15].strip()
                f = line[16:].split()
                vals = [(float(f[2 * k]), None if f[2 * k + 1] == "N/A" else float(f[2 * k + 1])) for k in range(5)]
                rows.append((res, chain, number, vals))
            elif line.startswith("TOTAL"):
                total = [float(v) for v in line.split()[1:]]
    return rows, total


@gpu
@pytest.mark.parametrize("pdb, rsa, alg", [("1ubq.pdb", "1ubq.sr100.rsa", "sr"), ("1ubq.pdb", "1ubq.lr20.rsa", "lr"),
                                           ("3bkr.pdb", "3bkr.sr100.rsa", "sr")])
def test_the_references_own_rsa_files(pdb, rsa, alg):
    fa.sweep_parse_stats()
    a, r = (fa.SHRAKE_RUPLEY, 100) if alg == "sr" else (fa.LEE_RICHARDS, 20)
    tot, _, _, status, t = fa.sweep_files_residues([fixture(pdb)], a, resolution=r, ingest_options=DEV)
    assert fa.sweep_parse_stats() == (1, 0) and status[0] == 0
    A, R = t.abs, t.rel
    rows, total = read_rsa(rsa)
    assert len(rows) == t.n_residues
    name, chain_, number_ = t.res_name, t.res_chain, t.res_number
    cols = [0, 2, 1, 4, 3]       # file columns: all, side, main, apolar, polar  <-  table: total, main, side, polar, apolar
    for k, (res, chain, number, vals) in enumerate(rows):
        assert (name[k], chain_[k], number_[k].strip()) == (res.strip(), chain, number)
        for q, (av, rel) in enumerate(vals):
            assert abs(A[k, cols[q]] - av) <= 0.005 + 1e-9, (k, q)
            if rel is None:
                assert not np.isfinite(R[k, cols[q]]), (k, q)
            else:
                assert abs(R[k, cols[q]] - rel) <= 0.05 + 1e-9, (k, q)
    sums = A.sum(0)
    for q, want in enumerate(total):
        assert abs(sums[cols[q]] - want) <= 0.05 + 1e-6
    assert abs(sums[0] - tot[0]) < 1e-9 * tot[0] and np.all(A[:, 5] == 0)


@gpu
def test_the_references_seq_output_for_1ubq():
    from conftest import read_seq_reference
    _, _, _, _, t = fa.sweep_files_residues([fixture("3bkr.pdb"), fixture("1ubq.pdb")], fa.SHRAKE_RUPLEY, resolution=100, ingest_options=DEV)
    ref = read_seq_reference()
    s = t.file(1)
    assert s.stop - s.start == len(ref) == 76
    name, chain_, number_ = t.res_name[s], t.res_chain[s], t.res_number[s]
    for k, (chain, number, res, area) in enumerate(ref):
        assert (chain_[k], number_[k].strip(), name[k]) == (chain, number, res)
        assert abs(t.abs[s][k, 0] - area) <= 0.005 + 1e-9


@gpu
def test_independent_of_how_the_work_is_cut():
    names = ["1a0q.pdb", "syn_crlf.pdb", "1ubq.cif", "empty.pdb", "3bkr.pdb", "syn_reordered_columns.cif", "icode.pdb", "does_not_exist.pdb",
             "5dx9.cif", "1ubq.pdb", "2jo4.pdb", "alt_model_twochain.pdb"] * 3
    paths = [fixture(n) for n in names]
    for parser in (DEV, 0):
        ref = None
        for devices, batch_atoms in (([0], 0), ([0, 0, 0], 0), ([0], 1), ([0, 0, 0], 1), ([0, 0], 4000), ([0], 1 << 40)):
            fa.sweep_parse_stats()
            got = fa.sweep_files_residues(paths, batch_atoms=batch_atoms, devices=devices, ingest_options=parser, n_threads=4)
            dev, host = fa.sweep_parse_stats()
            if parser:
                assert host >= 9 and dev >= 24, (dev, host)    # refused files between accepted ones: syn_crlf, syn_reordered_columns, the missing one
            if ref is None:
                ref = got
                continue
            same_results(ref, got, (devices, batch_atoms))
            tables_equal(ref[4], got[4])
        # every file's residues at its own place: each file alone gives its slice
        t = ref[4]
        for k in sorted({names.index(n) for n in set(names)}):
            one = fa.sweep_files_residues([paths[k]], ingest_options=parser)[4]
            for j in (k, k + len(names) // 3):
                s = t.file(j)
                assert s.stop - s.start == one.n_residues, names[k]
                assert np.array_equal(bits(t.abs[s]), bits(one.abs)) and np.array_equal(t.res_atoms[s], one.res_atoms), names[k]
                assert t.res_name[s] == one.res_name and t.res_number[s] == one.res_number and t.res_chain[s] == one.res_chain, names[k]
        k = names.index("empty.pdb")
        assert t.file(k).start == t.file(k).stop and ref[3][k] != 0
        assert t.file(names.index("syn_crlf.pdb")).stop > t.file(names.index("syn_crlf.pdb")).start


@gpu
def test_user_classifier_gives_absolute_areas_only():
    nac = ingest.Classifier(path=os.path.join(CFG, "naccess.config"))
    names = ["1ubq.pdb", "3bkr.cif", "syn_crlf.pdb", "empty.pdb", "1a0q.pdb", "5dx9.cif"]
    paths = [fixture(n) for n in names] + [os.path.join(CFG, "syn_any.pdb"), os.path.join(CFG, "syn_any.cif")]
    b, A, R = long_way(paths, fa.LEE_RICHARDS, 20, classifier=nac)
    assert np.all(b.res_ref == -1) and np.all(np.isnan(R))
    for parser in (DEV, 0):
        got = fa.sweep_files_residues(paths, classifier=nac, ingest_options=parser, batch_atoms=3000)
        t = got[4]
        assert t.n_residues > 0 and np.all(t.res_ref == -1) and np.all(np.isnan(t.rel))
        same_table(t, b, A, R, parser)
        want = fa.sweep_files(paths, classifier=nac, ingest_options=parser, batch_atoms=3000)
        same_results(want, got, parser)


def _free_device_memory():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@gpu
@pytest.mark.parametrize("parser", ["device", "host"])
@pytest.mark.parametrize("hook", ["gpu", "host"])
def test_fault_walk(parser, hook):
    """The n-th device / page-locked allocation (freesasa_gpu_test_fail_after), the n-th host allocation or thread creation
    (freesasa_host_test_fail_after) failing, n = 1, 2, ... until a call goes through: -1 with a message and a zeroed table,
    and the next call gives the full result.  (Injected failures are reported errors; nothing here faults the GPU.)"""
    L = fa._residue_proto(fa.lib())
    names = ["1ubq.pdb", "3bkr.cif", "empty.pdb", "syn_crlf.pdb", "1a0q.pdb", "does_not_exist.pdb", "1ubq.cif", "icode.pdb"] * 2
    paths = [fixture(n) for n in names]
    opt = DEV if parser == "device" else 0
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    devs = (C.c_int * 3)(0, 0, 0)

    def call():
        totals, status = np.zeros(n), np.zeros(n, dtype=np.int32)
        t = fa.ResidueTableC()
        C.memset(C.byref(t), 0x5a, C.sizeof(t))
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_sweep_files_residues(arr, n, opt, 4, 0, 1.4, 20, 1500, totals.ctypes.data_as(C.POINTER(C.c_double)), None, None,
                                                 status.ctypes.data_as(C.POINTER(C.c_int)), devs, 3, None, C.byref(t), err, 512)
        if rc:
            assert rc == -1 and err.value, "failure without a message"
            assert bytes(t) == bytes(C.sizeof(t)), "table not zeroed after a failure"
            return None
        out = (totals, status, fa.ResidueTable(t))
        L.freesasa_gpu_residue_table_free(C.byref(t))
        assert bytes(t) == bytes(C.sizeof(t))
        return out

    def same(a, b):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
        tables_equal(a[2], b[2])

    want = call()
    assert want is not None and want[2].n_residues > 300
    free0 = None
    failures = fired = 0
    try:
        k = 1
        while k <= 100000:
            if hook == "gpu":
                L.freesasa_gpu_release_pool()            # fresh contexts: every buffer is allocated in this call
                L.freesasa_gpu_test_fail_after(k)
                got = call()
                L.freesasa_gpu_test_fail_after(0)
                left = 0 if got is None else 1           # (this hook does not report its countdown: the walk ends with the first success)
            else:
                fa.host_test_fail_after(k)
                try:
                    got = call()
                finally:
                    left = fa.host_test_fail_after(0)
            if got is None:
                failures += 1
            elif hook == "gpu":
                same(got, want)                          # (under the host hook a call may go through with a file's status ENOMEM: the loader's report)
            again = call()                               # the next call succeeds with the full result
            assert again is not None
            same(again, want)
            if free0 is None:
                L.freesasa_gpu_release_pool()
                free0 = _free_device_memory()
            if left > 0:
                break
            fired += 1
            k += 1 if k < 48 else max(1, k // 6)         # (tests/test_hostfault.py: steps grow once k is large)
        else:
            raise AssertionError("the walk did not end")
    finally:
        L.freesasa_gpu_test_fail_after(0)
        fa.host_test_fail_after(0)
    assert failures >= 10, (hook, parser, failures, fired)
    # device memory is back at its level (both readings with the context pool released: what a failed call left behind would show)
    same(call(), want)
    L.freesasa_gpu_release_pool()
    assert _free_device_memory() >= free0 - (8 << 20), (free0, _free_device_memory())
