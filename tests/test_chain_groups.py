"""Chain groups on the host (include/freesasa_ingest.h, freesasa_ingest_chain_groups): the spec syntax of the reference
CLI's --chain-groups / --chain-groups-long (src/main.cc:389-443), the atoms each group selects against the reference
library's freesasa_structure_get_chains_lcl / freesasa_structure_array(SEPARATE_CHAINS), EGROUP for a missing chain,
and the refusal of overlapping groups.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

PDB = os.path.join(GOLDEN, "pdb")
FILES = ["1a0q.pdb", "2jo4.pdb", "3gnn.pdb", "alt_model_twochain.pdb"]


@pytest.fixture(scope="module")
def batch():
    from freesasa_amd import ingest
    return ingest.load_pdb_files([os.path.join(PDB, f) for f in FILES])


class _ChainGroup(C.Structure):
    _fields_ = [("chains", C.POINTER(C.c_char_p)), ("n", C.c_size_t)]


class _Ref:
    """The reference library's structure functions through ctypes (oracle/_ref/libfreesasa_ref.so)."""

    def __init__(self):
        import oracle
        if not oracle.Reference.available():
            pytest.skip("oracle/_ref/libfreesasa_ref.so not built (needs the reference sources)")
        L = self.L = C.CDLL(oracle.REF_SO)
        self.libc = C.CDLL(None)
        self.libc.fopen.restype = C.c_void_p
        self.libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        self.libc.fclose.argtypes = [C.c_void_p]
        self.libc.free.argtypes = [C.c_void_p]
        L.freesasa_set_verbosity.argtypes = [C.c_int]
        L.freesasa_set_verbosity(2)
        L.freesasa_structure_from_pdb.restype = C.c_void_p
        L.freesasa_structure_from_pdb.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.freesasa_structure_array.restype = C.POINTER(C.c_void_p)
        L.freesasa_structure_array.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
        L.freesasa_structure_get_chains_lcl.restype = C.c_void_p
        L.freesasa_structure_get_chains_lcl.argtypes = [C.c_void_p, C.POINTER(_ChainGroup), C.c_void_p, C.c_int]
        L.freesasa_structure_n.argtypes = [C.c_void_p]
        L.freesasa_structure_coord_array.restype = C.POINTER(C.c_double)
        L.freesasa_structure_coord_array.argtypes = [C.c_void_p]
        L.freesasa_structure_free.argtypes = [C.c_void_p]

    def _xyz(self, s):
        n = self.L.freesasa_structure_n(s)
        return np.ctypeslib.as_array(self.L.freesasa_structure_coord_array(s), (3 * n,)).reshape(n, 3).copy()

    def groups(self, path, groups):
        """xyz of freesasa_structure_get_chains_lcl for each group (a list of labels), None where it refuses"""
        fh = self.libc.fopen(path.encode(), b"r")
        whole = self.L.freesasa_structure_from_pdb(fh, None, 0)
        self.libc.fclose(fh)
        assert whole
        out = []
        for labels in groups:
            arr = (C.c_char_p * len(labels))(*[x.encode() for x in labels])
            cg = _ChainGroup(arr, len(labels))
            s = self.L.freesasa_structure_get_chains_lcl(whole, C.byref(cg), None, 0)
            out.append(self._xyz(s) if s else None)
            if s:
                self.L.freesasa_structure_free(s)
        self.L.freesasa_structure_free(whole)
        return out

    def separate_chains(self, path):
        fh = self.libc.fopen(path.encode(), b"r")
        n = C.c_int(0)
        arr = self.L.freesasa_structure_array(fh, C.byref(n), None, 1 << 4)   # FREESASA_SEPARATE_CHAINS
        self.libc.fclose(fh)
        assert arr
        out = [self._xyz(arr[k]) for k in range(n.value)]
        for k in range(n.value):
            self.L.freesasa_structure_free(arr[k])
        self.libc.free(arr)
        return out


@pytest.fixture(scope="module")
def ref():
    return _Ref()


def _parse_like_the_reference(spec, long):
    """What src/main.cc:389-443 plus freesasa_structure_get_chains_lcl make of a spec: the groups, or None where the
    CLI ends with an error for every structure (bad character, label longer than 3, an empty group or label, a chain
    twice in one group)."""
    if not long and any(not (c == "+" or c.isascii() and c.isalnum()) for c in spec):
        return None
    toks = spec.split("+")
    if toks and toks[-1] == "":
        toks = toks[:-1]                         # std::sregex_token_iterator drops an empty last token
    groups = []
    for t in toks:
        if long:
            labels = t.split("/")
            if labels and labels[-1] == "":
                labels = labels[:-1]
        else:
            labels = list(t)
        if not labels or any(len(x) > 3 or x == "" for x in labels) or len(set(labels)) != len(labels):
            return None
        groups.append(labels)
    return groups


SPECS = [("A", False), ("AB+C", False), ("A+", False), ("", False), ("a1+Z", False), ("A+B+C+D", False),
         ("+A", False), ("A++B", False), ("A-B", False), ("A B", False), ("A/B", False), ("AA", False), ("+", False),
         ("A/B+C", True), ("ABC/D", True), ("ABCD", True), ("A//B", True), ("A/", True), ("A+", True), ("/A", True),
         ("A+/", True), ("H", True), ("A/A", True)]


@pytest.mark.parametrize("spec,long", SPECS)
def test_spec_parser_accepts_what_the_reference_accepts(batch, spec, long):
    want = _parse_like_the_reference(spec, long)
    if want is None:
        with pytest.raises(ValueError):
            batch.chain_groups(spec, long=long)
    else:
        g, n, st = batch.chain_groups(spec, long=long)
        assert np.all(n == len(want))


def test_overlapping_groups_are_refused(batch):
    for spec, long in (("A+A", False), ("AB+BC", False), ("A/B+B", True), ("H+HL", False)):
        with pytest.raises(ValueError, match="overlapping"):
            batch.chain_groups(spec, long=long)
    with pytest.raises(ValueError):
        batch.chain_groups("A", separate_chains=True)       # a spec and separate chains are exclusive
    with pytest.raises(ValueError):
        batch.chain_groups(None)


def test_missing_chain_gives_egroup(batch):
    from freesasa_amd import ingest
    g, n, st = batch.chain_groups("H+L")
    assert st.tolist() == [ingest.OK, ingest.EGROUP, ingest.EGROUP, ingest.EGROUP]
    assert np.all(n == 2)
    for s in (1, 2, 3):
        assert np.all(g[batch.offsets[s]:batch.offsets[s + 1]] == -1)
    # one chain present, the other not: still refused as a whole (ref: src/structure.c:1070)
    g, n, st = batch.chain_groups("A+H")
    assert np.all(st == ingest.EGROUP) and np.all(g == -1)


def _check_against(batch, s, g, n_groups, want_xyz):
    ids = g[batch.offsets[s]:batch.offsets[s + 1]]
    xyz = batch.xyz[batch.offsets[s]:batch.offsets[s + 1]]
    assert n_groups == len(want_xyz)
    for k, w in enumerate(want_xyz):
        assert w is not None
        assert np.array_equal(xyz[ids == k], w), (s, k)


@pytest.mark.parametrize("s,spec,long", [(0, "H+L", False), (0, "L+H", False), (0, "HL", False), (1, "AB+CD", False),
                                         (1, "A+C+D", False), (1, "D/A+B", True), (2, "AB+DE", False), (2, "E+B", False),
                                         (3, "A+B", False)])
def test_groups_select_the_references_atoms(batch, ref, s, spec, long):
    g, n, st = batch.chain_groups(spec, long=long)
    assert st[s] == 0
    groups = _parse_like_the_reference(spec, long)
    _check_against(batch, s, g, n[s], ref.groups(os.path.join(PDB, FILES[s]), groups))


def test_missing_chain_is_what_the_reference_refuses(batch, ref):
    for s, spec in ((0, "H+A"), (1, "AB+E"), (3, "C")):
        g, n, st = batch.chain_groups(spec)
        assert st[s] != 0
        assert any(x is None for x in ref.groups(os.path.join(PDB, FILES[s]), _parse_like_the_reference(spec, False)))


@pytest.mark.parametrize("s", range(len(FILES)))
def test_separate_chains_cut_like_the_reference(batch, ref, s):
    g, n, st = batch.chain_groups(separate_chains=True)
    assert st[s] == 0
    _check_against(batch, s, g, n[s], ref.separate_chains(os.path.join(PDB, FILES[s])))


def test_separate_chains_start_a_group_where_a_label_recurs():
    from freesasa_amd import ingest
    lines = []
    for k, ch in enumerate("AABBAA"):
        lines.append("ATOM  %5d  CA  ALA %s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n" % (k + 1, ch, k + 1, 3.0 * k, 0.0, 0.0))
    b = ingest.load_pdb_texts(["".join(lines)])
    g, n, st = b.chain_groups(separate_chains=True)
    assert g.tolist() == [0, 0, 1, 1, 2, 2] and n.tolist() == [3]
    g, n, st = b.chain_groups("A+B")
    assert g.tolist() == [0, 0, 1, 1, 0, 0] and n.tolist() == [2]
