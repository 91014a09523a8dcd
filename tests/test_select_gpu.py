"""Selection areas on the device (freesasa_gpu_select_batch, freesasa_gpu_sweep_files_select, include/freesasa_gpu.h): a
compiled selection set (ingest.Selection) run per atom by a kernel, the per-atom areas summed under every mask by another.

The bars: freesasa_ingest_select (Batch.select; tests/test_select.py pins it to the real reference) for every mask bit, the
class-sum kernel with the mask as class for every area, bit for bit (the same chunks in the same order: equality is
derived, not measured), and the long way round - ingest.load_files -> calc_batch -> select_batch, file by file - for the
sweep, whoever parses, however the batches are cut and whichever worker takes them."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import freesasa_amd as fa
from freesasa_amd import ingest
from test_device_parser import MUST_PARSE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDB = os.path.join(ROOT, "tests", "golden", "pdb")
CIF = os.path.join(ROOT, "tests", "golden", "cif")
CFG = os.path.join(ROOT, "tests", "golden", "classifiers")
with open(os.path.join(ROOT, "tests", "golden", "select.json")) as fh:
    GOLD = json.load(fh)
DEV = ingest.PARSE_ON_DEVICE

EIGHT = ["bb, name n+ca+c+o", "hyd, resn ala+val+leu+ile+met+phe+trp+pro", "r, resi 10-20+30 and not symbol c",
         "open, resi -5 or resi 60-", "ch, chain A-B and not chain A", "ic, resi 52A", "het, symbol fe+zn+se+s", "w, name abcde"]
REFUSED = ["syn_crlf.pdb", "syn_basic.cif", "syn_reordered_columns.cif"]
SWEEP_FILES = sorted(MUST_PARSE) + REFUSED + ["empty.pdb", "does_not_exist.pdb"]


def fixture(name):
    return os.path.join(CIF if name.endswith(".cif") else PDB, name)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def masks_of(words, S):
    return ((words[None, :] >> np.arange(S, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(np.uint8)


def joined(batches):
    """one ingest.Batch holding the structures of several, in order (each may have been loaded with options of its own)"""
    b = object.__new__(ingest.Batch)
    cat = lambda name: np.concatenate([getattr(x, name) for x in batches])
    for name in ("xyz", "radii", "atom_class", "atom_backbone", "res_ref", "atom_name_raw", "atom_symbol_raw", "status",
                 "res_name_raw", "res_number_raw", "res_chain_raw"):
        setattr(b, name, np.ascontiguousarray(cat(name)))
    a0 = np.concatenate([[0], np.cumsum([x.n_atoms for x in batches])]).astype(np.int64)
    r0 = np.concatenate([[0], np.cumsum([x.n_residues for x in batches])]).astype(np.int64)
    b.offsets = np.concatenate([x.offsets[:-1] + a0[k] for k, x in enumerate(batches)] + [a0[-1:]]).astype(np.int64)
    b.res_offsets = np.concatenate([x.res_offsets[:-1] + r0[k] for k, x in enumerate(batches)] + [r0[-1:]]).astype(np.int64)
    b.res_first = np.concatenate([x.res_first[:-1] + a0[k] for k, x in enumerate(batches)] + [a0[-1:]]).astype(np.int64)
    b.n_structs, b.n_atoms, b.n_residues = sum(x.n_structs for x in batches), int(a0[-1]), int(r0[-1])
    return b


def test_select_batch_against_the_host_masks_and_the_class_sum_kernel():
    import torch
    parts = [ingest.load_pdb_files([fixture(g["file"])], options=g["options"]) for g in GOLD]
    parts.append(ingest.load_pdb_files([fixture("empty.pdb")]))
    b = joined(parts)
    ns = b.n_structs
    assert ns == 8 and b.offsets[-1] == b.n_atoms and b.offsets[8] == b.offsets[7]
    sasa, _, _ = fa.calc_batch(b.xyz, b.radii, b.offsets, fa.LEE_RICHARDS, resolution=20)
    commands = []
    for g in GOLD:
        for r in g["selections"]:
            if r["rc"] != -1 and r["command"] not in commands:
                commands.append(r["command"])
    assert len(commands) > 64
    dev = torch.device("cuda:0")
    d_sasa = torch.from_numpy(sasa).to(dev)
    d_out = torch.empty(3 * ns, dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0)
    worst = 0.0
    for lo in range(0, len(commands), 64):
        cmds = commands[lo:lo + 64]
        s = ingest.Selection(cmds)
        areas, counts, words = fa.select_batch(b, s, sasa, device=0, bits=True)
        m = masks_of(words, len(cmds))
        for q, cmd in enumerate(cmds):
            for k in range(ns):
                _, want, warned = b.select(k, cmd)
                sl = slice(int(b.offsets[k]), int(b.offsets[k + 1]))
                assert np.array_equal(m[q][sl], want), (cmd, k)
                assert counts[k, q] == int(want.sum()), (cmd, k)
                terms = sasa[sl][want == 1]
                host = float(np.cumsum(terms)[-1]) if terms.size else 0.0   # left to right, like src/selection.c:717-720
                bound = max(terms.size - 1, 0) * 2.0 ** -53 * float(np.abs(terms).sum())
                assert abs(areas[k, q] - host) <= bound, (cmd, k, areas[k, q], host, bound)
                worst = max(worst, abs(areas[k, q] - host))
                assert k == 7 or s.warned[q] == warned             # (nothing is evaluated, so nothing warns, on a structure without atoms)
            ctx.class_sums(d_sasa.data_ptr(), torch.from_numpy(m[q]).to(dev).data_ptr(), b.offsets, d_out.data_ptr())
            cls = d_out.cpu().numpy().reshape(ns, 3)
            assert np.array_equal(bits64(cls[:, 1]), bits64(areas[:, q])), cmd
        assert not counts[7].any() and not areas[7].any()         # empty.pdb
    ctx.close()
    print(f"worst |device - host sum| = {worst:.3e}")


@pytest.fixture(scope="module")
def long_way():
    """areas[n, S], counts[n, S] of EIGHT for every file of SWEEP_FILES: load_files -> calc_batch -> select_batch, file by file"""
    s = ingest.Selection(EIGHT)
    areas, counts = np.zeros((len(SWEEP_FILES), len(EIGHT))), np.zeros((len(SWEEP_FILES), len(EIGHT)), dtype=np.int64)
    for k, name in enumerate(SWEEP_FILES):
        b = ingest.load_files([fixture(name)])
        if b.n_atoms:
            sasa, _, _ = fa.calc_batch(b.xyz, b.radii, b.offsets, fa.LEE_RICHARDS, resolution=20)
            areas[k], counts[k] = (x[0] for x in fa.select_batch(b, s, sasa, device=0))
    return areas, counts


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["one", "three"])
@pytest.mark.parametrize("batch_atoms", [0, 3000])
@pytest.mark.parametrize("parser", ["host", "device"])
def test_sweep_files_select_equals_the_long_way(long_way, parser, batch_atoms, devices):
    paths = [fixture(n) for n in SWEEP_FILES]
    opt = DEV if parser == "device" else 0
    s = ingest.Selection(EIGHT)
    assert s.warned == [False] * 7 + [True]
    fa.sweep_parse_stats()
    got = fa.sweep_files_select(paths, s, ingest_options=opt, batch_atoms=batch_atoms, devices=devices, n_threads=4)
    on_device, by_host = fa.sweep_parse_stats()
    want = fa.sweep_files(paths, ingest_options=opt, batch_atoms=batch_atoms, devices=devices, n_threads=4)
    for x, y, what in zip(want, got[:4], ("totals", "class sums", "atoms", "status")):
        assert np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(x, y), what
    areas, counts = got[4], got[5]
    assert np.array_equal(counts, long_way[1])
    assert np.array_equal(bits64(areas), bits64(long_way[0]))
    if parser == "device":
        assert on_device >= len(MUST_PARSE) and by_host >= len(REFUSED)   # the device-built keys and residues were what was tested
    # the files the host parser read behind the device's atoms are at their own places, the failed ones are zero
    for name in REFUSED:
        k = SWEEP_FILES.index(name)
        assert got[3][k] == 0 and counts[k, 0] > 0 and counts[k, 0] == long_way[1][k, 0]
    for name in ("empty.pdb", "does_not_exist.pdb"):
        k = SWEEP_FILES.index(name)
        assert got[3][k] != 0 and not counts[k].any() and not areas[k].any()
    assert counts[:, 0].sum() > 3000 and counts[:, 3].sum() > 0 and counts[:, 4].sum() > 0 and counts[:, 6].sum() > 0


@pytest.mark.parametrize("parser", ["host", "device"])
def test_sweep_files_select_with_a_user_classifier(parser):
    nac = ingest.Classifier(path=os.path.join(CFG, "naccess.config"))
    names = ["1ubq.pdb", "3bkr.cif", "syn_crlf.pdb", "alt_model_twochain.pdb"]
    paths = [fixture(n) for n in names]
    s = ingest.Selection(EIGHT)
    opt = DEV if parser == "device" else 0
    got = fa.sweep_files_select(paths, s, ingest_options=opt, classifier=nac, batch_atoms=3000, devices=[0, 0])
    want = fa.sweep_files(paths, ingest_options=opt, classifier=nac, batch_atoms=3000, devices=[0, 0])
    for x, y in zip(want, got[:4]):
        assert np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(x, y)
    plain = fa.sweep_files_select(paths, s, ingest_options=opt, batch_atoms=3000, devices=[0, 0])
    assert not np.array_equal(plain[4], got[4])                    # other radii: other areas
    for k, p in enumerate(paths):
        b = ingest.load_files([p], classifier=nac)
        sasa, _, _ = fa.calc_batch(b.xyz, b.radii, b.offsets, fa.LEE_RICHARDS, resolution=20)
        areas, counts = fa.select_batch(b, s, sasa, device=0)
        assert np.array_equal(counts[0], got[5][k]) and np.array_equal(bits64(areas[0]), bits64(got[4][k])), names[k]


@pytest.mark.parametrize("parser", ["host", "device"])
def test_sweep_files_select_under_device_allocation_failures(parser):
    """The n-th device / page-locked allocation failing (freesasa_gpu_test_fail_after), n = 1, 2, ... walked upward ONCE until a
    call goes through: every failure is -1 with a message, and the next unarmed call gives the full result.  (Injected
    failures are reported errors; nothing here faults the GPU, and nothing is tried again.)"""
    L = fa._select_proto(fa.lib())
    paths = [fixture(n) for n in ("1ubq.pdb", "syn_crlf.pdb", "3bkr.cif")]
    s = ingest.Selection(EIGHT)
    opt = DEV if parser == "device" else 0

    def call():
        try:
            return fa.sweep_files_select(paths, s, ingest_options=opt, batch_atoms=1000, devices=[0, 0], n_threads=2)
        except RuntimeError as e:
            assert len(str(e)) > len("freesasa_gpu_sweep_files_select: "), "failure without a message"
            return None

    def same(a, b):
        for x, y in zip(a, b):
            assert np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(x, y)

    want = call()
    assert want is not None and want[5][:, 0].sum() > 300
    failures = 0
    try:
        for n in range(1, 2000):
            L.freesasa_gpu_release_pool()                          # fresh contexts: every buffer is allocated in this call
            L.freesasa_gpu_test_fail_after(n)
            got = call()
            L.freesasa_gpu_test_fail_after(0)
            again = call()
            assert again is not None
            same(again, want)
            if got is not None:
                same(got, want)
                break
            failures += 1
        else:
            raise AssertionError("the walk did not end")
    finally:
        L.freesasa_gpu_test_fail_after(0)
    assert failures >= 10, (parser, failures)


def test_select_batch_refuses_bad_arguments():
    L = fa._select_proto(fa.lib())
    b = ingest.load_files([fixture("icode.pdb")])
    s = ingest.Selection(["a, resi 1A"])
    with pytest.raises(ValueError):
        fa.select_batch(b, s, np.zeros(3))
    cb = b._as_c()
    err = C.create_string_buffer(256)
    out, cnt = (C.c_double * 1)(), (C.c_longlong * 1)()
    assert L.freesasa_gpu_select_batch(C.byref(cb), None, b.radii.ctypes.data_as(C.POINTER(C.c_double)), out, cnt, None, 0, err, 256) == -1
    assert b"null argument" in err.value
    areas, counts, words = fa.select_batch(b, s, b.radii, device=0, bits=True)
    assert counts.tolist() == [[1]] and words.tolist() == [0, 1, 0, 0, 0] and areas[0, 0] == b.radii[1]
