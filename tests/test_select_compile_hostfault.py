"""Allocation failures while a selection set is compiled (freesasa_ingest_selection_compile), walked n = 1, 2, ... with
the library-local hook (freesasa_host_test_fail_after, csrc/hostfault.h) as tests/test_classifier_hostfault.py walks the
classifier's creation: every call is a clean failure with a message or a success, and the set a call gives equals the
un-faulted one."""
import ctypes as C

import freesasa_amd as fa
from freesasa_amd import ingest

COMMANDS = ["bb, name n+ca+c+o", "r, resi 10-20+30 and not symbol c", "open, resi -5 or resi 60-",
            "deep, (resn ala or (chain A-B and not chain A)) and not (name abcde or resi 52A)"]


def program(s):
    L = ingest._selection_proto()
    nw, flags = C.c_int(0), C.c_int(0)
    p = L.freesasa_ingest_selection_program(s.handle, C.byref(nw), C.byref(flags))
    return C.string_at(p, 16 * nw.value), flags.value, s.names, s.warned


def test_compile_under_allocation_failures():
    want = program(ingest.Selection(COMMANDS))
    fired = failed = 0
    n = 1
    while True:
        assert n < 10000, "the walk did not end"
        fa.host_test_fail_after(n)
        try:
            try:
                got = program(ingest.Selection(COMMANDS))
            except (ValueError, MemoryError) as e:
                got = None
                assert str(e), f"failure without a message at n = {n}"
        finally:
            left = fa.host_test_fail_after(0)
        if left > 0:
            assert got == want
            break
        fired += 1
        if got is None:
            failed += 1
        else:
            assert got == want
        n += 1
    assert fired > 10 and failed == fired                          # one per node of the trees and the set itself
    assert program(ingest.Selection(COMMANDS)) == want
