"""User classifiers (freesasa_ingest_classifier_*, csrc/classifier.c) against the REAL reference library: its
configuration reader (freesasa_classifier_from_file, src/classifier.c:703-850) and lookup (find_atom, :739-779), live,
on the fixture configs and on a few hundred seeded mutations of them; and the host loader under every config against
the vectors tests/golden/make_ingest_classifier_golden.py minted from freesasa_structure_from_pdb / _from_cif."""
import ctypes as C
import hashlib
import json
import os
import random
import re
import struct

import numpy as np
import pytest

from freesasa_amd import ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(GOLD, "classifiers")
CONFIGS = ["protor", "naccess", "oons", "dssp", "synthetic"]
LOADABLE = ["protor", "naccess", "oons", "synthetic"]            # (dssp.config is rejected: its classes are not polar / apolar)
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libfreesasa_ref.so")
OPTION_SETS = [0, 1, 4, 5, 32, 128, 64, 129, 256, 37]               # make_ingest_golden.OPTION_SETS
CIF_OPTION_SETS = [0, 1, 4, 5, 32, 128, 64, 129, 37]                # make_ingest_golden.CIF_OPTION_SETS


def cfg_path(name):
    return os.path.join(CFG, name + ".config")


def cfg_text(name):
    with open(cfg_path(name), "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref not built (make oracle)")
    lib = C.CDLL(REF_SO)
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    lib.freesasa_classifier_from_file.restype = C.c_void_p
    lib.freesasa_classifier_from_file.argtypes = [C.c_void_p]
    lib.freesasa_classifier_free.argtypes = [C.c_void_p]
    lib.freesasa_classifier_radius.restype = C.c_double
    lib.freesasa_classifier_radius.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.freesasa_classifier_class.restype = C.c_int
    lib.freesasa_classifier_class.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.freesasa_classifier_name.restype = C.c_char_p
    lib.freesasa_classifier_name.argtypes = [C.c_void_p]
    lib.freesasa_set_verbosity(2)

    class Ref:
        def load(self, path):
            fp = libc.fopen(str(path).encode(), b"r")
            assert fp
            h = lib.freesasa_classifier_from_file(fp)
            libc.fclose(fp)
            return h

        free = staticmethod(lib.freesasa_classifier_free)

        @staticmethod
        def lookup(h, res, atom):
            return lib.freesasa_classifier_radius(h, res, atom), lib.freesasa_classifier_class(h, res, atom)

        @staticmethod
        def name(h):
            n = lib.freesasa_classifier_name(h)
            return n.decode() if n is not None else "no-name-given"   # (the reference keeps NULL and warns)
    return Ref()


def names_of(text):
    """every (first, second) token pair of the lines with at least three tokens"""
    res, atoms = set(), set()
    for line in text.split(b"\n"):
        t = line.split(b"#")[0].split()
        if len(t) >= 3:
            res.add(t[0])
            atoms.add(t[1])
    return res, atoms


def same_lookups(ref, h, ours, text):
    res, atoms = names_of(text)
    res |= {b"XYZ", b"ABCD", b"ANY", b"ALA", b"GLY", b" ALA ", b"ALANINE"}
    atoms |= {b"CA", b"XX", b" CB", b"OXT"}
    for r in sorted(res):
        for a in sorted(atoms):
            want = ref.lookup(h, r, a)
            got = ours.radius(r, a)
            assert struct.pack("<d", got[0]) == struct.pack("<d", want[0]) and got[1] == want[1], (r, a, got, want)


@pytest.mark.parametrize("name", CONFIGS)
def test_parser_and_lookup_match_the_reference(ref, name):
    h = ref.load(cfg_path(name))
    if name == "dssp":
        # (the reference's own DSSP file names its classes 'backbone' / 'sidechain': its reader rejects the file, and so
        # does this one)
        assert not h
        with pytest.raises(ValueError, match="class 'backbone'"):
            ingest.Classifier(path=cfg_path(name))
        return
    assert h
    try:
        for ours in (ingest.Classifier(path=cfg_path(name)), ingest.Classifier(text=cfg_text(name))):
            assert ours.name == ref.name(h)
            same_lookups(ref, h, ours, cfg_text(name))
    finally:
        ref.free(h)


def test_synthetic_config_rules():
    c = ingest.Classifier(path=cfg_path("synthetic"))
    assert c.name == "SYNTH-1"
    assert c.radius("ALA", "CB") == (1.70, ingest.APOLAR)        # the first (ALA, CB) wins
    assert c.radius("GLY", "CA") == (1.55, ingest.POLAR)         # a residue's own row before ANY's
    assert c.radius("TRP", "CA") == (1.70, ingest.APOLAR)        # residue not listed: ANY
    assert c.radius("ALA", "SG") == (1.80, ingest.APOLAR)        # listed without the atom: ANY
    assert c.radius("ABCD", "N") == (1.55, ingest.POLAR)         # longer than 3 characters: ANY
    assert c.radius("  LIG ", " C1  ") == (2.50, ingest.APOLAR)  # names are trimmed
    assert c.radius("LIG", "QQ") == (-1.0, ingest.UNKNOWN)
    assert c.radius("ZZZ", "Q") == (-1.0, ingest.UNKNOWN)        # commented out
    no_name = ingest.Classifier(text="types:\nC 1.5 apolar\natoms:\nANY CA C\n")
    assert no_name.name == "no-name-given"
    assert no_name.digest != c.digest
    # the digest is the resolved table's: comments, order and the name do not change it
    same = ingest.Classifier(text="name: other\natoms:\nANY CA C   # the sections in the other order\ntypes:\nC 1.5 apolar\n")
    assert same.digest == no_name.digest


# ------------------------------------------------------------------------------------------------ differential fuzz

def mutate(rng, text):
    lines = text.split(b"\n")
    for _ in range(rng.randint(1, 3)):
        k = rng.randrange(len(lines))
        op = rng.randrange(10)
        if op == 0:
            del lines[k]
        elif op == 1:
            lines.insert(k, lines[k])
        elif op == 2:
            lines.insert(k, b"ANY CA NO_SUCH_TYPE")
        elif op == 3:
            lines.insert(k, b"ALAX CA C_ALI")
        elif op == 4:
            lines.insert(k, b"ALA CAXYZ O")
        elif op == 5:
            lines.insert(k, b"XT 1.5 nonpolar")
        elif op == 6:
            lines.insert(k, rng.choice([b"# types: in a comment", b"# atoms: in a comment", b"  # name: in a comment"]))
        elif op == 7:
            lines.insert(k, b"ANY CA " + b"x" * rng.choice([200, 248, 249, 250, 260]))
        elif op == 8:
            lines.insert(k, rng.choice([b"ALA", b"ALA CB", b"\tC_X\t1.0\tPolar", b"C_Y 1.2", b"AB", b"1", b"GLY  CA\tC_CAR"]))
        else:
            lines.insert(k, rng.choice([b"ANY XX C_ALI", b"C_ALI 3.0 polar", b"HOH O O", b"NEW CZ S", b"types:", b"atoms:"]))
    return b"\n".join(lines)


def fuzz_cases(n=320, seed=2024):
    rng = random.Random(seed)
    bases = [cfg_text(c) for c in CONFIGS]
    out = []
    while len(out) < n:
        t = mutate(rng, rng.choice(bases))
        # (inputs on which the reference's reader ASSERTS and aborts are not inputs it defines: "name:" or "atoms:" run
        # into a following character)
        if re.search(rb"(name|atoms):[^\s]", t):
            continue
        out.append(t)
    return out


def test_differential_fuzz_against_the_reference(ref, tmp_path):
    accepted = rejected = 0
    for i, text in enumerate(fuzz_cases()):
        p = tmp_path / f"m{i}.config"
        p.write_bytes(text)
        h = ref.load(p)
        try:
            ours = ingest.Classifier(text=text)
        except ValueError as e:
            assert str(e)
            assert not h, f"case {i}: the reference accepts what this parser rejects ({e})\n{text.decode()}"
            rejected += 1
            continue
        try:
            assert h, f"case {i}: the reference rejects what this parser accepts\n{text.decode()}"
            assert ours.name == ref.name(h)
            same_lookups(ref, h, ours, text)
            assert ingest.Classifier(path=p).digest == ours.digest
            accepted += 1
        finally:
            ref.free(h)
    assert accepted > 40 and rejected > 40, (accepted, rejected)


def test_long_lines_and_comments(ref, tmp_path):
    base = b"name: L\ntypes:\nC 1.5 apolar\natoms:\n"
    for n in (254, 255, 256, 257):
        for tail in (b"\n", b""):
            text = base + b"ANY CA C #" + b"x" * (n - 10) + tail
            p = tmp_path / "l.config"
            p.write_bytes(text)
            h = ref.load(p)
            try:
                ok = ingest.Classifier(text=text)
            except ValueError:
                ok = None
            assert (ok is None) == (not h), (n, tail)
            if h:
                ref.free(h)


# ------------------------------------------------------------------------------------------------ the host loader

def short(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def fixture_path(name):
    if name.startswith("syn_any"):
        return os.path.join(CFG, name)
    return os.path.join(GOLD, "cif" if name.endswith(".cif") else "pdb", name)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(GOLD, "ingest_classifiers.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("cfg", LOADABLE)
def test_loader_matches_the_reference_under_every_config(vectors, cfg):
    c = ingest.Classifier(path=cfg_path(cfg))
    per = vectors["vectors"][cfg]
    checked = 0
    for kind, option_sets in (("pdb", OPTION_SETS), ("cif", CIF_OPTION_SETS)):
        names = [n for n in per if n.endswith(".cif") == (kind == "cif")]
        for o in option_sets:
            b = ingest.load_pdb_files([fixture_path(n) for n in names], options=o, classifier=c)
            assert (b.res_ref == -1).all()
            for s, n in enumerate(names):
                exp = per[n][str(o)]
                if exp.get("crash"):
                    continue
                a0, a1 = b.offsets[s], b.offsets[s + 1]
                if exp.get("fail"):
                    assert b.status[s] != 0 and a1 == a0, (n, o)
                    continue
                assert b.status[s] == 0, (n, o, b.status[s])
                r0, r1 = b.res_offsets[s], b.res_offsets[s + 1]
                got = {"n_atoms": int(a1 - a0), "n_residues": int(r1 - r0), "xyz": short(b.xyz[a0:a1]),
                       "radii": short(b.radii[a0:a1]), "classes": short(b.atom_class[a0:a1]),
                       "res_first": short(np.append(b.res_first[r0:r1] - a0, a1 - a0).astype(np.int64))}
                assert got == exp, (cfg, n, o)
                checked += 1
    assert checked > 200


def test_null_classifier_is_the_plain_entry_and_save_load_keeps_a_custom_batch(tmp_path):
    files = [fixture_path(n) for n in ("1ubq.pdb", "3bkr.cif", "syn_any.pdb", "syn_any.cif", "empty.pdb")]
    L = ingest._proto()
    for o in (0, 1, 128):
        plain = ingest.load_pdb_files(files, options=o)
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        cb = ingest._CBatch()
        ex = ingest._finish(L, L.freesasa_ingest_pdb_files_ex(arr, len(files), o, 0, None, C.byref(cb)), cb)
        texts = [open(f, "rb").read() for f in files]
        tx = ingest.load_pdb_texts(texts, options=o)
        raw = (C.c_char_p * len(texts))(*texts)
        lens = (C.c_size_t * len(texts))(*[len(t) for t in texts])
        cb = ingest._CBatch()
        ex_t = ingest._finish(L, L.freesasa_ingest_pdb_texts_ex(raw, lens, len(texts), o, 0, None, C.byref(cb)), cb)
        for a, b in ((plain, ex), (tx, ex_t), (plain, tx)):
            for name in ("xyz", "radii", "atom_class", "atom_backbone", "offsets", "res_first", "res_offsets", "res_ref", "status",
                         "atom_name_raw", "res_name_raw", "res_number_raw", "res_chain_raw"):
                assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    # ProtOr's own config file as a user classifier gives ProtOr's radii and classes (only res_ref differs)
    protor = ingest.load_pdb_files(files, classifier=ingest.Classifier(path=cfg_path("protor")))
    builtin = ingest.load_pdb_files(files)
    assert protor.radii.tobytes() == builtin.radii.tobytes() and protor.atom_class.tobytes() == builtin.atom_class.tobytes()
    assert (protor.res_ref == -1).all() and (builtin.res_ref >= 0).any()
    nac = ingest.load_pdb_files(files, classifier=ingest.Classifier(path=cfg_path("naccess")))
    p = str(tmp_path / "nac.cache")
    nac.save(p)
    back = ingest.load_cache(p)
    for name in ("xyz", "radii", "atom_class", "offsets", "res_first", "res_ref", "status", "res_name_raw"):
        assert getattr(nac, name).tobytes() == getattr(back, name).tobytes(), name
    assert (back.res_ref == -1).all()
    texts_nac = ingest.load_pdb_texts([open(f, "rb").read() for f in files], classifier=ingest.Classifier(path=cfg_path("naccess")))
    assert texts_nac.radii.tobytes() == nac.radii.tobytes() and texts_nac.atom_class.tobytes() == nac.atom_class.tobytes()


def test_failures_give_null_and_a_message(tmp_path):
    with pytest.raises(ValueError, match="cannot open"):
        ingest.Classifier(path=str(tmp_path / "missing.config"))
    for bad, what in ((b"name: X\natoms:\nANY CA C\n", "lacks"),
                      (b"types:\nC 1.5 apolar\natoms:\nANY CA D\n", "unknown atom type"),
                      (b"types:\nC 1.5 nonpolar\natoms:\nANY CA C\n", "class"),
                      (b"types:\nC 1.5 apolar\natoms:\nANYX CA C\n", "residue name"),
                      (b"types:\nC 1.5 apolar\natoms:\nANY CAXYZ C\n", "atom name"),
                      (b"types:\nC 1.5\natoms:\nANY CA C\n", "could not parse"),
                      (b"types:\nC 1.5 apolar\natoms:\nANY CA C\nANY CA C\n", "repeats"),
                      (b"types:\nC 1.5 apolar\natoms:\nANY CA C " + b"x" * 300 + b"\n", "longer than 256")):
        with pytest.raises(ValueError, match=what):
            ingest.Classifier(text=bad)
    with pytest.raises(TypeError):
        ingest.load_pdb_files([fixture_path("1ubq.pdb")], classifier="naccess")
