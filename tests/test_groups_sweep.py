"""Chain groups in the file sweep (freesasa_gpu_sweep_files_groups, freesasa_gpu_chain_group_ids, include/freesasa_gpu.h), the
part that needs no GPU: the C boundary - symbols, the table's layout, the call errors, which are freesasa_ingest_chain_groups's
own and come before a device is touched - and the group-ids kernel's phase function (csrc/group_kernels.h, gid_struct) driven
on the CPU (tests/emu/emu_groups.cpp) against freesasa_ingest_chain_groups, the specification, on every fixture."""
import ctypes as C
import glob
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
FIXTURES = sorted(glob.glob(os.path.join(PDB, "*")) + glob.glob(os.path.join(CIF, "*")))
SPECS = [dict(separate_chains=True), dict(spec="H+L"), dict(spec="AB+CD"), dict(spec="A"), dict(spec="A+B"), dict(spec="A/B+C", long=True)]
SYMBOLS = ("freesasa_gpu_sweep_files_groups", "freesasa_gpu_group_table_free", "freesasa_gpu_chain_group_ids")


def _lib():
    fa.build()
    return fa._groups_proto(fa.lib())


def test_symbols_are_declared_and_exported():
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", fa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "freesasa_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for sym in SYMBOLS:
        assert sym in exported, sym
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
    assert "typedef struct freesasa_gpu_group_table" in header


def test_table_struct_layout_matches_the_header():
    T = fa.GroupTableC
    # int32_t, int64_t, then four pointers: 48 bytes on LP64
    want = [("n_files", 0, 4), ("n_groups", 8, 8), ("group_offsets", 16, 8), ("group_atoms", 24, 8), ("areas", 32, 8), ("chain", 40, 8)]
    assert C.sizeof(T) == 48
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, _ in T._fields_] == want
    header = open(os.path.join(ROOT, "include", "freesasa_gpu.h")).read()
    body = re.search(r"typedef struct freesasa_gpu_group_table \{(.*?)\} freesasa_gpu_group_table;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\*?\b(\w+)\s*(?=[,;])", body)
    assert members == [n for n, _ in T._fields_], members


def _dirty():
    t = fa.GroupTableC()
    C.memset(C.byref(t), 0x5a, C.sizeof(t))
    return t


def _sweep(L, paths, totals, status, gstatus, table, spec, flags, n=1):
    devs = (C.c_int * 1)(0)
    err = C.create_string_buffer(256)
    rc = L.freesasa_gpu_sweep_files_groups(paths, n, 0, 1, 0, 1.4, 20, 0, totals, None, None, status, devs, 1, None, spec, flags, gstatus, table, err, 256)
    return rc, err.value.decode()


def _host_message(spec, flags):
    """what freesasa_ingest_chain_groups says to the same spec and flags"""
    b = ingest.load_files([os.path.join(PDB, "1ubq.pdb")])
    L = ingest._proto()
    i32 = C.POINTER(C.c_int32)
    g, n, s = np.zeros(b.n_atoms, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    err = C.create_string_buffer(256)
    cb = b._as_c()
    rc = L.freesasa_ingest_chain_groups(C.byref(cb), spec, flags, g.ctypes.data_as(i32), n.ctypes.data_as(i32), s.ctypes.data_as(i32), err, 256)
    assert rc == -1
    return err.value.decode()


CALL_ERRORS = [(b"A+b!", 0), (b"A++B", 0), (b"+A", 0), (b"AB+BC", 0), (b"A/B+B", ingest.GROUPS_LONG), (b"ABCD/E", ingest.GROUPS_LONG),
               (b"A", ingest.SEPARATE_CHAINS), (None, 0), (None, ingest.GROUPS_LONG), (b"A", 2), (b"A", 1 << 8), (b"AA", 0)]


def test_call_errors_are_the_host_functions_and_need_no_device():
    L = _lib()
    paths = (C.c_char_p * 1)(os.path.join(PDB, "1ubq.pdb").encode())
    totals, status, gstatus = (C.c_double * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    dp, ip, gp = C.cast(totals, C.POINTER(C.c_double)), C.cast(status, C.POINTER(C.c_int)), C.cast(gstatus, C.POINTER(C.c_int))
    # NULL arguments
    for args in ((None, dp, ip, gp), (paths, None, ip, gp), (paths, dp, None, gp), (paths, dp, ip, None)):
        t = _dirty()
        rc, msg = _sweep(L, args[0], args[1], args[2], args[3], C.byref(t), None, ingest.SEPARATE_CHAINS)
        assert rc == -1 and "null argument" in msg, (rc, msg)
        assert bytes(t) == bytes(C.sizeof(t)), "table not zeroed"
    rc, msg = _sweep(L, paths, dp, ip, gp, None, None, ingest.SEPARATE_CHAINS)
    assert rc == -1 and "null argument" in msg
    # the spec's and the flags' errors, with the host function's words - on a machine without a device too: they come first
    b = ingest.load_files([os.path.join(PDB, "1ubq.pdb")])
    cb = b._as_c()
    i32 = C.POINTER(C.c_int32)
    g, n, s = np.zeros(b.n_atoms, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    seen = set()
    for spec, flags in CALL_ERRORS:
        want = _host_message(spec, flags)
        assert want
        seen.add(want.split("'")[0])
        t = _dirty()
        rc, msg = _sweep(L, paths, dp, ip, gp, C.byref(t), spec, flags)
        assert rc == -1 and msg == want, (spec, flags, msg, want)
        assert bytes(t) == bytes(C.sizeof(t)), "table not zeroed"
        err = C.create_string_buffer(256)
        rc = L.freesasa_gpu_chain_group_ids(C.byref(cb), spec, flags, g.ctypes.data_as(i32), n.ctypes.data_as(i32), s.ctypes.data_as(i32), 0, err, 256)
        assert rc == -1 and err.value.decode() == want, (spec, flags, err.value, want)
    assert len(seen) >= 8, seen     # bad character, empty group, overlap, twice in a group, long label, both, neither, unknown flags
    err = C.create_string_buffer(256)
    for args in ((None, g, n, s), (cb, None, n, s), (cb, g, None, s), (cb, g, n, None)):
        p = [None if a is None else (C.byref(a) if a is cb else a.ctypes.data_as(i32)) for a in args]
        assert L.freesasa_gpu_chain_group_ids(p[0], b"A", 0, p[1], p[2], p[3], 0, err, 256) == -1 and b"null argument" in err.value


def test_freeing_a_zeroed_table_does_nothing():
    L = _lib()
    t = fa.GroupTableC()
    L.freesasa_gpu_group_table_free(C.byref(t))
    L.freesasa_gpu_group_table_free(C.byref(t))
    L.freesasa_gpu_group_table_free(None)
    assert bytes(t) == bytes(C.sizeof(t))


def test_new_code_does_not_reference_the_oracle():
    """(tests/test_residue_sweep.py's scan, over the files this feature adds to)"""
    for rel in ("freesasa_amd/csrc/gpu_groups.hip", "freesasa_amd/csrc/gpu_sweep.hip", "freesasa_amd/csrc/group_kernels.h", "freesasa_amd/csrc/gpu_kernels.hip",
                "freesasa_amd/csrc/select.c", "freesasa_amd/__init__.py", "tools/sweep.py", "tools/groups_sweep_bench.py"):
        txt = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"#include\s+\"[^\"]*oracle|import\s+oracle|from\s+oracle|sasa_oracle|libsasa_emu", txt), rel


# ------------------------------------------------------------------------------------------------ the kernel's phase function on the CPU

@pytest.fixture(scope="module")
def batch():
    return ingest.load_files(FIXTURES, n_threads=4)


@pytest.mark.parametrize("kw", SPECS, ids=lambda kw: kw.get("spec") or "separate")
def test_emulated_ids_equal_the_host_functions(batch, kw):
    from emu import groups_emu
    want = batch.chain_groups(**kw)
    got = groups_emu.run(batch, **kw)
    for x, y, what in zip(want, got, ("group", "n_groups", "status")):
        assert np.array_equal(x, y), (kw, what, np.nonzero(x != y)[0][:8])
    # file by file too: a structure's ids do not depend on its neighbours in the batch
    for p in FIXTURES:
        b = ingest.load_files([p])
        for x, y, what in zip(b.chain_groups(**kw), groups_emu.run(b, **kw), ("group", "n_groups", "status")):
            assert np.array_equal(x, y), (os.path.basename(p), kw, what)


def test_the_fixtures_cover_both_outcomes_and_a_recurring_label(batch):
    """what the host loader gives for the fixtures: the ground the emulation test stands on"""
    names = [os.path.basename(p) for p in FIXTURES]
    g, n, st = batch.chain_groups(separate_chains=True)
    loaded = batch.status == 0
    assert int(((n >= 2) & (n <= 4)).sum()) == 12 and np.all(st == batch.status)
    k = names.index("3gnn.pdb")
    ids = g[batch.offsets[k]:batch.offsets[k + 1]]
    assert n[k] == 4 and np.bincount(ids).tolist() == [1960, 1773, 20, 20]
    for name in ("syn_basic.cif", "syn_altloc_icode_chain.pdb"):      # a label recurs and starts a group of its own
        k = names.index(name)
        labels = batch.res_chain[batch.res_offsets[k]:batch.res_offsets[k + 1]]
        runs = [l for i, l in enumerate(labels) if i == 0 or l != labels[i - 1]]
        assert runs == ["A", "B", "A"] and n[k] == 3, name
    for spec, ok, egroup in (("A+B", 9, 23), ("A", 31, 1)):
        _, n, st = batch.chain_groups(spec)
        assert int((st[loaded] == 0).sum()) == ok and int((st == ingest.EGROUP).sum()) == egroup, spec
