"""Allocation failures on the user classifier's creation paths (freesasa_ingest_classifier_from_file / _from_text) and
in the loader with one (freesasa_ingest_pdb_files_ex), walked n = 1, 2, ... with the library-local hook
(freesasa_host_test_fail_after, csrc/hostfault.h) as tests/test_hostfault.py walks the other host code: every call is a
clean NULL with a message or a success, and the call after the walk gives the un-faulted result.  `make asan-test` runs
this file under AddressSanitizer (leaks: the classifier is freed on every way out)."""
import os

import pytest

import freesasa_amd as fa
from freesasa_amd import ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "classifiers")
FILES = [os.path.join(ROOT, "tests", "golden", "pdb", "1ubq.pdb"), os.path.join(ROOT, "tests", "golden", "cif", "3bkr.cif"),
         os.path.join(CFG, "syn_any.pdb"), os.path.join(CFG, "syn_any.cif")]


def walk(call, limit=100000):
    """call() -> (ok, message); as tests/test_hostfault.py walk(): (faults that fired, calls that failed)"""
    fired = failed = 0
    n = 1
    while n <= limit:
        fa.host_test_fail_after(n)
        try:
            ok, msg = call()
        finally:
            left = fa.host_test_fail_after(0)
        if left > 0:
            assert ok, msg
            return fired, failed
        fired += 1
        if not ok:
            failed += 1
            assert msg, f"failure without a message at n = {n}"
        n += 1
    raise AssertionError("the walk did not end")


@pytest.mark.parametrize("name", ["naccess", "protor", "synthetic"])
def test_creation_under_allocation_failures(name):
    path = os.path.join(CFG, name + ".config")
    text = open(path, "rb").read()
    want = ingest.Classifier(path=path)

    def from_file():
        try:
            c = ingest.Classifier(path=path)
        except ValueError as e:
            return False, str(e)
        return c.digest == want.digest and c.name == want.name, "wrong classifier"

    def from_text():
        try:
            c = ingest.Classifier(text=text)
        except ValueError as e:
            return False, str(e)
        return c.digest == want.digest, "wrong classifier"
    for call in (from_file, from_text):
        fired, failed = walk(call)
        assert fired > 5 and failed == fired


def test_loader_with_a_classifier_under_allocation_failures():
    nac = ingest.Classifier(path=os.path.join(CFG, "naccess.config"))
    want = ingest.load_pdb_files(FILES, classifier=nac, n_threads=2)

    def load():
        try:
            b = ingest.load_pdb_files(FILES, classifier=nac, n_threads=2)
        except RuntimeError as e:
            return False, str(e)
        ok = b.status.tolist() == want.status.tolist() or any(s == ingest.ENOMEM for s in b.status)
        return ok, "unexpected status"
    fired, _ = walk(load)
    assert fired > 3
    again = ingest.load_pdb_files(FILES, classifier=nac, n_threads=2)
    assert again.radii.tobytes() == want.radii.tobytes() and again.atom_class.tobytes() == want.atom_class.tobytes()
