"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the file sweep's interfaces
(freesasa_gpu_sweep_files_interfaces), as tests/test_groups_sweep_gpu.py::test_fault_walk does for the group sweep: the n-th host
allocation or thread creation fails, n = 1, 2, ... until a call goes through.  A failed call gives -1, a message and two zeroed
tables; the call after it gives the full result, bit for bit.  Host allocation failures only: they are reported errors, and
nothing here faults the GPU."""
import ctypes as C

import numpy as np
import pytest

import freesasa_amd as fa
from freesasa_amd import ingest
from test_groups_sweep_gpu import DEV, bits64, fixture, _free_device_memory

pytestmark = pytest.mark.gpu

FIELDS = ("pair_offsets", "pair_groups", "pair_atoms", "pair_chain_raw", "pair_areas", "pair_class_buried", "res_offsets", "res_index", "res_atoms",
          "res_areas", "res_name_raw", "res_number_raw", "res_chain_raw")


@pytest.mark.parametrize("parser", ["device", "host"])
def test_host_fault_walk(parser):
    L = fa._ifsweep_proto(fa.lib())
    names = ["1a0q.pdb", "3bkr.cif", "empty.pdb", "syn_crlf.pdb", "2jo4.pdb", "does_not_exist.pdb", "1ubq.cif", "alt_model_twochain.pdb"]
    paths = [fixture(n) for n in names]
    opt = DEV if parser == "device" else 0
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    devs = (C.c_int * 2)(0, 0)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def call():
        totals, status, gstatus, istatus = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        g, t = fa.GroupTableC(), fa.InterfaceTableC()
        C.memset(C.byref(g), 0x5a, C.sizeof(g))
        C.memset(C.byref(t), 0x5a, C.sizeof(t))
        err = C.create_string_buffer(512)
        rc = L.freesasa_gpu_sweep_files_interfaces(arr, n, opt, 4, 0, 1.4, 20, 1500, totals.ctypes.data_as(dp), None, None, status.ctypes.data_as(ip),
                                                   devs, 2, None, None, ingest.SEPARATE_CHAINS, gstatus.ctypes.data_as(ip), C.byref(g), 1, 0.0,
                                                   istatus.ctypes.data_as(ip), C.byref(t), err, 512)
        if rc:
            assert rc == -1 and err.value, "failure without a message"
            assert bytes(g) == bytes(C.sizeof(g)) and bytes(t) == bytes(C.sizeof(t)), "tables not zeroed after a failure"
            return None
        out = (totals, status, gstatus, istatus, fa.GroupTable(g), fa.InterfaceTable(t, True))
        L.freesasa_gpu_group_table_free(C.byref(g))
        L.freesasa_gpu_interface_table_free(C.byref(t))
        assert bytes(g) == bytes(C.sizeof(g)) and bytes(t) == bytes(C.sizeof(t))
        return out

    def same(a, b):
        assert np.array_equal(bits64(a[0]), bits64(b[0])) and all(np.array_equal(a[k], b[k]) for k in (1, 2, 3))
        assert bits64(a[4].areas).tobytes() == bits64(b[4].areas).tobytes() and a[4].chain_raw.tobytes() == b[4].chain_raw.tobytes()
        for f in FIELDS:
            assert getattr(a[5], f).tobytes() == getattr(b[5], f).tobytes(), f

    want = call()
    assert want is not None and want[5].n_pairs >= 7 and want[5].n_res_rows >= 50
    failures = fired = 0
    try:
        k = 1
        while k <= 100000:
            fa.host_test_fail_after(k)
            try:
                got = call()
            finally:
                left = fa.host_test_fail_after(0)
            if got is None:
                failures += 1           # (a call may also go through with a file's status ENOMEM: the loader's report)
            again = call()              # the next call succeeds with the full result
            assert again is not None
            same(again, want)
            if left > 0:
                break
            fired += 1
            k += 1 if k < 48 else max(1, k // 6)         # (tests/test_hostfault.py: steps grow once k is large)
        else:
            raise AssertionError("the walk did not end")
    finally:
        fa.host_test_fail_after(0)
    assert failures >= 10, (parser, failures, fired)
    same(call(), want)
    L.freesasa_gpu_release_pool()
    free0 = _free_device_memory()
    same(call(), want)
    L.freesasa_gpu_release_pool()
    assert _free_device_memory() >= free0 - (8 << 20), (free0, _free_device_memory())
