"""Chain groups in the file sweep on the device (freesasa_gpu_sweep_files_groups, freesasa_gpu_chain_group_ids,
include/freesasa_gpu.h): the group ids made by a kernel from residues and chain labels that are on the device
(csrc/group_kernels.h, k_gid_struct), the complex and its groups computed as one batch, a table of groups in file order.

The bars: freesasa_ingest_chain_groups (Batch.chain_groups; tests/test_chain_groups.py pins it to the real reference) for every
id, count and status, exactly; the long way round - ingest.load_files -> chain_groups -> calc_groups, file by file - for the
table, bit for bit (an atom's area does not depend on what else rides in its batch, and a group's totals are summed over the
same chunks in the same order: equality is derived, not measured); the plain sweep for the plain outputs, bit for bit; the
reference's own numbers (tests/golden/chain_groups.json) for the isolated areas."""
import ctypes as C
import glob
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
DEV = ingest.PARSE_ON_DEVICE
REFUSED = ["syn_crlf.pdb", "syn_basic.cif", "syn_reordered_columns.cif"]
SWEEP_FILES = sorted(MUST_PARSE) + REFUSED + ["empty.pdb", "does_not_exist.pdb"]       # (tests/test_select_gpu.py's list)
SPECS = [dict(separate_chains=True), dict(spec="H+L"), dict(spec="AB+CD"), dict(spec="A"), dict(spec="A+B"), dict(spec="A/B+C", long=True)]


def fixture(name):
    return os.path.join(CIF if name.endswith(".cif") else PDB, name)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_ids(b, **kw):
    want = b.chain_groups(kw.get("spec"), long=kw.get("long", False), separate_chains=kw.get("separate_chains", False))
    got = fa.chain_group_ids(b, kw.get("spec"), separate_chains=kw.get("separate_chains", False), long_syntax=kw.get("long", False), device=0)
    for x, y, what in zip(want, got, ("group", "n_groups", "status")):
        assert x.dtype == y.dtype and np.array_equal(x, y), (kw, what, np.nonzero(x != y)[0][:8])
    return want


# ------------------------------------------------------------------------------------------------ 1. the ids kernel

def test_ids_of_all_fixtures_in_one_batch():
    b = ingest.load_files(sorted(glob.glob(os.path.join(PDB, "*")) + glob.glob(os.path.join(CIF, "*"))), n_threads=4)
    assert b.n_structs == 40 and (b.status != 0).sum() >= 5
    for kw in SPECS:
        g, n, st = same_ids(b, **kw)
    assert (same_ids(b, separate_chains=True)[1] >= 2).sum() >= 12
    assert (same_ids(b, spec="A+B")[2] == ingest.EGROUP).sum() == 23


def pdb_text(chains):
    """one CA atom per residue; chains: the chain letter of every residue, in order"""
    lines = []
    for i, ch in enumerate(chains):
        x, y, z = 4.0 * (i % 40), 4.0 * ((i // 40) % 40), 4.0 * (i // 1600)
        lines.append("ATOM  %5d  CA  ALA %s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C" % (i % 100000, ch, i % 10000, x, y, z))
    return "\n".join(lines) + "\nEND\n"


def cif_text(chains, atoms_per_residue=2):
    head = "data_SYN\n#\nloop_\n" + "".join("_atom_site.%s\n" % c for c in (
        "group_PDB", "id", "type_symbol", "label_atom_id", "label_alt_id", "label_comp_id", "label_asym_id", "label_entity_id", "label_seq_id",
        "pdbx_PDB_ins_code", "Cartn_x", "Cartn_y", "Cartn_z", "occupancy", "B_iso_or_equiv", "pdbx_formal_charge", "auth_seq_id", "auth_comp_id",
        "auth_asym_id", "auth_atom_id", "pdbx_PDB_model_num"))
    rows, k = [], 0
    for i, ch in enumerate(chains):
        for name, sym in (("N", "N"), ("CA", "C"))[:atoms_per_residue]:
            k += 1
            rows.append(f"ATOM {k} {sym} {name} . ALA {ch} 1 {i + 1} ? {4.0 * (i % 40):.3f} {4.0 * (i // 40):.3f} {1.5 * (name == 'CA'):.3f} 1.00 10.00 ? {i + 1} ALA {ch} {name} 1")
    return head + "\n".join(rows) + "\n#\n"


def test_ids_at_the_shapes_where_a_wave_can_go_wrong():
    # structures of 1, 63, 64, 65, 129 residues, two chains each where there is room; an empty structure between two others;
    # a chain change exactly between residues 63|64 and 127|128; A,B,A; one-residue chains throughout
    texts = [pdb_text("A"), pdb_text("A" * 40 + "B" * 23), pdb_text("A" * 32 + "B" * 32), "", pdb_text("A" * 64 + "B"),
             pdb_text("A" * 64 + "B" * 64 + "C"), pdb_text("A" * 50 + "B" * 50 + "A" * 29), pdb_text("AB" * 100 + "A"),
             pdb_text("A" * 63 + "B" * 65 + "A"), pdb_text("ABCA" * 33)]
    b = ingest.load_texts(texts)
    assert b.n_structs == 10 and b.status[3] != 0 and np.diff(b.res_offsets).tolist() == [1, 63, 64, 0, 65, 129, 129, 201, 129, 132]
    g, n, st = same_ids(b, separate_chains=True)
    assert n.tolist() == [1, 2, 2, 0, 2, 3, 3, 201, 3, 100] and st[3] != 0     # ("ABCA" repeated: the A at the seam is one run)
    g, n, st = same_ids(b, spec="A")
    assert np.all(st == b.status) and n.tolist() == [1] * 10      # (the spec's count for every structure, as the host function gives it)
    for kw in (dict(spec="A+B"), dict(spec="AB+C"), dict(spec="B/A+C", long=True), dict(spec="C+A")):
        g, n, st = same_ids(b, **kw)
        assert (st == ingest.EGROUP).any() and (st == 0).any(), kw


def test_65535_chains_are_the_limit():
    ok, over = pdb_text("AB" * 32767 + "A"), pdb_text("AB" * 32768)
    b = ingest.load_texts([pdb_text("AAB"), ok, over, pdb_text("BA")])
    assert np.diff(b.res_offsets).tolist() == [3, 65535, 65536, 2]
    g, n, st = same_ids(b, separate_chains=True)
    assert n.tolist() == [2, 65535, 0, 2] and st.tolist() == [0, 0, ingest.EGROUP, 0]
    assert np.all(g[b.offsets[2]:b.offsets[3]] == -1) and g[b.offsets[2] - 1] == 65534
    same_ids(b, spec="A+B")


def test_mmcif_labels_that_differ_in_their_second_or_third_byte():
    b = ingest.load_texts([cif_text(["AA"] * 3 + ["AB"] * 2 + ["ABA"] * 2 + ["ABB"] * 3 + ["AB"] + ["A"] * 2), cif_text(["AB", "ABA"]), cif_text(["A", "AA", "AAA"])])
    assert np.all(b.status == 0) and sorted(set(b.res_chain)) == ["A", "AA", "AAA", "AB", "ABA", "ABB"]
    g, n, st = same_ids(b, separate_chains=True)
    assert n.tolist() == [6, 2, 3]
    E = ingest.EGROUP
    for spec, want in (("AA/AB+ABA/ABB+A", [0, E, E]), ("AB+ABA", [0, 0, E]), ("A+AA+AAA", [E, E, 0]), ("ABB", [0, E, E]), ("AAA/A", [E, E, 0])):
        g, n, st = same_ids(b, spec=spec, long=True)
        assert st.tolist() == want, spec


def test_a_long_spec_of_100_labels():
    labels = [a + c for a in "ABCDEFGHIJ" for c in "0123456789"]
    spec = "+".join("/".join(labels[k:k + 7]) for k in range(0, 100, 7))
    b = ingest.load_texts([cif_text(labels, 1), cif_text(labels[:-1], 1), cif_text(labels[::-1] * 2, 1)])
    g, n, st = same_ids(b, spec=spec, long=True)
    assert st.tolist() == [0, ingest.EGROUP, 0] and n.tolist() == [15, 15, 15] and np.all(g[b.offsets[1]:b.offsets[2]] == -1)
    assert sorted(set(g[:100].tolist())) == list(range(15))


# ------------------------------------------------------------------------------------------------ 2. the sweep against the long way

def long_way_of(paths, alg, res, kw, classifier=None):
    """per file: (group status, group_totals [G, 3], atoms per group, labels) from load_files -> chain_groups -> calc_groups"""
    out = []
    for p in paths:
        b = ingest.load_files([p], classifier=classifier)
        g, n, st = b.chain_groups(kw.get("spec"), separate_chains=kw.get("separate_chains", False))
        if st[0] != 0:
            out.append((int(st[0]), np.zeros((0, 3)), np.zeros(0, np.int32), []))
            continue
        gt = fa.calc_groups(b.xyz, b.radii, b.offsets, g, n, alg, resolution=res, device=0)[3]
        atoms = np.bincount(g[g >= 0], minlength=int(n[0])).astype(np.int32)
        if kw.get("separate_chains"):
            chain = b.res_chain
            first_res = [int(np.searchsorted(b.res_first, int(np.nonzero(g == k)[0][0]), side="right")) - 1 for k in range(int(n[0]))]
            labels = [chain[r] for r in first_res]
        else:
            labels = [grp[0] for grp in kw["spec"].split("+")]
        out.append((0, gt, atoms, labels))
    return out


_LONG = {}


def long_way(alg, res, key):
    kw = dict(separate_chains=True) if key == "separate" else dict(spec=key)
    if (alg, res, key) not in _LONG:
        _LONG[(alg, res, key)] = long_way_of([fixture(n) for n in SWEEP_FILES], alg, res, kw)
    return kw, _LONG[(alg, res, key)]


def same_as_the_long_way(got, want, names):
    gstatus, t = got[4], got[5]
    assert t.n_files == len(names) and t.group_offsets[0] == 0 and t.group_offsets[-1] == t.n_groups
    chain = t.chain
    for k, (st, gt, atoms, labels) in enumerate(want):
        s = t.file(k)
        assert gstatus[k] == st, (names[k], gstatus[k], st)
        assert s.stop - s.start == len(atoms), names[k]
        assert np.array_equal(t.group_atoms[s], atoms), names[k]
        assert np.array_equal(bits64(t.areas[s]), bits64(gt)), names[k]
        assert chain[s] == labels, (names[k], chain[s], labels)


@pytest.mark.parametrize("alg, res", [(fa.LEE_RICHARDS, 20), (fa.SHRAKE_RUPLEY, 100)], ids=["lr20", "sr100"])
@pytest.mark.parametrize("key", ["separate", "A+B"])
@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["one", "three"])
@pytest.mark.parametrize("batch_atoms", [0, 3000])
@pytest.mark.parametrize("parser", ["host", "device"])
def test_sweep_files_groups_equals_the_long_way(parser, batch_atoms, devices, key, alg, res):
    kw, want = long_way(alg, res, key)
    paths = [fixture(n) for n in SWEEP_FILES]
    opt = DEV if parser == "device" else 0
    fa.sweep_parse_stats()
    got = fa.sweep_files_groups(paths, kw.get("spec"), separate_chains=kw.get("separate_chains", False), alg=alg, resolution=res,
                                ingest_options=opt, batch_atoms=batch_atoms, devices=devices, n_threads=4)
    on_device, by_host = fa.sweep_parse_stats()
    plain = fa.sweep_files(paths, alg, resolution=res, ingest_options=opt, batch_atoms=batch_atoms, devices=devices, n_threads=4)
    for x, y, what in zip(plain, got[:4], ("totals", "class sums", "atoms", "status")):
        assert np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(x, y), what
    same_as_the_long_way(got, want, SWEEP_FILES)
    if parser == "device":
        assert on_device >= len(MUST_PARSE) and by_host >= len(REFUSED)   # the device-built residues and labels were what was tested
    gstatus, t = got[4], got[5]
    for name in ("empty.pdb", "does_not_exist.pdb"):
        k = SWEEP_FILES.index(name)
        assert gstatus[k] == got[3][k] != 0 and t.file(k).start == t.file(k).stop
    if key == "A+B":    # a file without its chains keeps its plain results and owns no rows
        k = SWEEP_FILES.index("1a0q.pdb")
        assert gstatus[k] == ingest.EGROUP and got[3][k] == 0 and got[0][k] > 0 and got[2][k] == 3183 and t.file(k).start == t.file(k).stop
        assert (gstatus == 0).sum() >= 5 and t.n_groups == 2 * (gstatus == 0).sum()
    else:
        k = SWEEP_FILES.index("3gnn.pdb")
        assert t.group_atoms[t.file(k)].tolist() == [1960, 1773, 20, 20] and np.all(gstatus == got[3])
    assert np.all(t.areas[:, 2] >= -1e-9)


# ------------------------------------------------------------------------------------------------ 3. the reference's numbers

@pytest.mark.parametrize("parser", ["host", "device"])
def test_the_references_numbers(parser):
    with open(os.path.join(ROOT, "tests", "golden", "chain_groups.json")) as fh:
        cases = json.load(fh)
    assert [c["file"] for c in cases] == ["1a0q.pdb", "2jo4.pdb", "3gnn.pdb"]
    for c in cases:
        for alg, res, key in ((fa.LEE_RICHARDS, 20, "lr20"), (fa.SHRAKE_RUPLEY, 100, "sr100")):
            tot, _, atoms, status, gstatus, t = fa.sweep_files_groups([fixture(c["file"])], c["spec"], separate_chains=c["spec"] is None, alg=alg,
                                                                      resolution=res, ingest_options=DEV if parser == "device" else 0)
            assert status[0] == 0 and gstatus[0] == 0 and t.n_groups == len(c["groups"]) and atoms[0] == c["complex"]["atoms"]
            want = c["complex"][key]
            assert abs(tot[0] - want) <= 1e-8 * atoms[0] + 1e-12 * want
            for k, wg in enumerate(c["groups"]):
                assert t.group_atoms[k] == wg["atoms"]
                assert abs(t.areas[k, 0] - wg[key]) <= 1e-8 * wg["atoms"] + 1e-12 * wg[key], (c["file"], k, t.areas[k, 0], wg[key])
                assert t.areas[k, 2] >= 0


# ------------------------------------------------------------------------------------------------ 4. a user classifier

@pytest.mark.parametrize("parser", ["host", "device"])
def test_with_a_user_classifier(parser):
    nac = ingest.Classifier(path=os.path.join(CFG, "naccess.config"))
    names = ["1a0q.pdb", "3bkr.cif", "syn_crlf.pdb", "alt_model_twochain.pdb", "2jo4.pdb", "empty.pdb"]
    paths = [fixture(n) for n in names]
    opt = DEV if parser == "device" else 0
    for kw in (dict(separate_chains=True), dict(spec="A+B")):
        want = long_way_of(paths, fa.LEE_RICHARDS, 20, kw, classifier=nac)
        got = fa.sweep_files_groups(paths, kw.get("spec"), separate_chains=kw.get("separate_chains", False), ingest_options=opt, classifier=nac,
                                    batch_atoms=3000, devices=[0, 0])
        plain = fa.sweep_files(paths, ingest_options=opt, classifier=nac, batch_atoms=3000, devices=[0, 0])
        for x, y in zip(plain, got[:4]):
            assert np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(x, y)
        same_as_the_long_way(got, want, names)
    other = fa.sweep_files_groups(paths, separate_chains=True, ingest_options=opt, batch_atoms=3000, devices=[0, 0])
    assert not np.array_equal(other[5].areas, got[5].areas) or kw.get("spec")       # other radii: other areas


# ------------------------------------------------------------------------------------------------ 5. fault walk

def _free_device_memory():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("parser", ["device", "host"])
@pytest.mark.parametrize("hook", ["gpu", "host"])
def test_fault_walk(parser, hook):
    """(tests/test_residue_sweep.py::test_fault_walk for this entry) The n-th device / page-locked allocation, the n-th host
    allocation or thread creation failing, n = 1, 2, ... until a call goes through: -1 with a message and a zeroed table, and
    the next call gives the full result.  (Injected failures are reported errors; nothing here faults the GPU.)"""
    L = fa._groups_proto(fa.lib())
    names = ["1a0q.pdb", "3bkr.cif", "empty.pdb", "syn_crlf.pdb", "2jo4.pdb", "does_not_exist.pdb", "1ubq.cif", "alt_model_twochain.pdb"]
    paths = [fixture(n) for n in names]
    opt = DEV if parser == "device" else 0
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    devs = (C.c_int * 2)(0, 0)

    def call():
        totals, status, gstatus = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        t = fa.GroupTableC()
        C.memset(C.byref(t), 0x5a, C.sizeof(t))
        err = C.create_string_buffer(512)
        ip = C.POINTER(C.c_int)
        rc = L.freesasa_gpu_sweep_files_groups(arr, n, opt, 4, 0, 1.4, 20, 1500, totals.ctypes.data_as(C.POINTER(C.c_double)), None, None,
                                               status.ctypes.data_as(ip), devs, 2, None, None, ingest.SEPARATE_CHAINS, gstatus.ctypes.data_as(ip),
                                               C.byref(t), err, 512)
        if rc:
            assert rc == -1 and err.value, "failure without a message"
            assert bytes(t) == bytes(C.sizeof(t)), "table not zeroed after a failure"
            return None
        out = (totals, status, gstatus, fa.GroupTable(t))
        L.freesasa_gpu_group_table_free(C.byref(t))
        assert bytes(t) == bytes(C.sizeof(t))
        return out

    def same(a, b):
        assert np.array_equal(bits64(a[0]), bits64(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        for f in ("group_offsets", "group_atoms", "chain_raw"):
            assert getattr(a[3], f).tobytes() == getattr(b[3], f).tobytes(), f
        assert bits64(a[3].areas).tobytes() == bits64(b[3].areas).tobytes()

    want = call()
    assert want is not None and want[3].n_groups >= 8
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
    same(call(), want)
    L.freesasa_gpu_release_pool()
    assert _free_device_memory() >= free0 - (8 << 20), (free0, _free_device_memory())
