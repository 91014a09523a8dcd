"""freesasa_amd — thin ctypes front-end of libfreesasa_amd.so (the MI355X SASA engine).

The product is the C library (include/freesasa_amd.h = the reference's calculation API,
include/freesasa_gpu.h = the additive batch API).  This module only loads it and wraps the
C entry points for the tests, the bench and Python callers; it contains no SASA arithmetic
and no CPU fallback — if the library or a HIP device is missing, calls fail loudly.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("FREESASA_AMD_LIB") or os.path.join(HERE, "lib", "libfreesasa_amd.so")

LEE_RICHARDS, SHRAKE_RUPLEY = 0, 1
SUCCESS, FAIL, WARN = 0, -1, -2
V_NORMAL, V_NOWARNINGS, V_SILENT, V_DEBUG = 0, 1, 2, 3

_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64)
_u32p = C.POINTER(C.c_uint32)


class Parameters(C.Structure):
    """freesasa_parameters (include/freesasa_amd.h; reference src/freesasa.h:232-238)."""
    _fields_ = [("alg", C.c_int), ("probe_radius", C.c_double),
                ("shrake_rupley_n_points", C.c_int), ("lee_richards_n_slices", C.c_int),
                ("n_threads", C.c_int)]


class Result(C.Structure):
    """freesasa_result (reference src/freesasa.h:267-272)."""
    _fields_ = [("total", C.c_double), ("sasa", _dp), ("n_atoms", C.c_int),
                ("parameters", Parameters)]


class CoordT(C.Structure):
    """coord_t (reference src/coord.h:26-38)."""
    _fields_ = [("n", C.c_int), ("is_linked", C.c_int), ("xyz", _dp)]


class Stats(C.Structure):
    _fields_ = [("n_atoms", C.c_longlong), ("n_cells", C.c_longlong), ("n_structs", C.c_int),
                ("max_neighbors", C.c_int), ("fallback_tiles", C.c_int), ("tile_atoms", C.c_int),
                ("block_threads", C.c_int), ("lds_bytes", C.c_int), ("ms_prep", C.c_double),
                ("ms_kernel", C.c_double), ("ms_total", C.c_double)]


class _OccupancyTable(C.Structure):
    """freesasa_gpu_contact_occupancy_table_t (include/freesasa_gpu.h): the library's arrays of a run table's snapshot."""
    _fields_ = [("n_frames", C.c_longlong), ("n_rows", C.c_longlong), ("keys", C.POINTER(C.c_int32)), ("frames", _lp), ("frames_either", _lp),
                ("counts", _lp), ("area", _dp), ("span", _lp), ("reverse", C.POINTER(C.c_int32))]


_lib = None


def build():
    """Compile the library in-tree (hipcc --offload-arch=gfx950; works without a GPU)."""
    subprocess.run(["make", "-C", ROOT, "all"], check=True, stdout=subprocess.DEVNULL)


def _preload_torch_hip_runtime():
    """libfreesasa_amd.so needs libamdhip64.so.7.  PyTorch-ROCm wheels bundle their own copy under
    the same soname; a process must not end up with ROCm's copy loaded first and torch's other
    runtime libraries later ("No HIP GPUs are available").  If torch is installed and not yet
    imported, load ITS libamdhip64 first so that both this library and a later `import torch`
    share one runtime.  Pure C callers are unaffected (no torch in the process)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("FREESASA_AMD_NO_TORCH_PRELOAD"):
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} is not built (run `make` or __graft_entry__.build()); "
                          "freesasa_amd has no pure-Python or CPU path")
        _preload_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.freesasa_calc_coord.argtypes = [_dp, _dp, C.c_int, C.POINTER(Parameters)]
        L.freesasa_calc_coord.restype = C.POINTER(Result)
        L.freesasa_calc.argtypes = [C.POINTER(CoordT), _dp, C.POINTER(Parameters)]
        L.freesasa_calc.restype = C.POINTER(Result)
        L.freesasa_calc_structure.argtypes = [C.c_void_p, C.POINTER(Parameters)]
        L.freesasa_calc_structure.restype = C.POINTER(Result)
        L.freesasa_result_free.argtypes = [C.POINTER(Result)]
        L.freesasa_result_free.restype = None
        L.freesasa_lee_richards.argtypes = [_dp, C.POINTER(CoordT), _dp, C.POINTER(Parameters)]
        L.freesasa_shrake_rupley.argtypes = [_dp, C.POINTER(CoordT), _dp, C.POINTER(Parameters)]
        L.freesasa_set_verbosity.argtypes = [C.c_int]
        L.freesasa_get_verbosity.restype = C.c_int
        L.freesasa_gpu_device_count.restype = C.c_int
        L.freesasa_gpu_ctx_create.argtypes = [C.c_int, C.c_void_p]
        L.freesasa_gpu_ctx_create.restype = C.c_void_p
        L.freesasa_gpu_ctx_destroy.argtypes = [C.c_void_p]
        L.freesasa_gpu_ctx_destroy.restype = None
        L.freesasa_gpu_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.freesasa_gpu_ctx_set_timing.restype = None
        L.freesasa_gpu_ctx_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.freesasa_gpu_ctx_get_stats.restype = None
        L.freesasa_gpu_ctx_last_error.argtypes = [C.c_void_p]
        L.freesasa_gpu_ctx_last_error.restype = C.c_char_p
        L.freesasa_gpu_lr_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int,
                                                C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_lr_batch_dev_async.argtypes = L.freesasa_gpu_lr_batch_dev.argtypes
        L.freesasa_gpu_wait.argtypes = [C.c_void_p]
        L.freesasa_gpu_sr_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int,
                                                C.c_double, C.c_int, _dp, C.c_void_p, C.c_void_p,
                                                C.c_void_p]
        L.freesasa_gpu_segment_sums_dev.argtypes = [C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p]
        L.freesasa_gpu_class_sums_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p]
        L.freesasa_gpu_residue_areas_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int,
                                                     C.POINTER(C.c_short), _dp, C.c_int, C.c_void_p, C.c_void_p]
        _i32p = C.POINTER(C.c_int32)
        L.freesasa_gpu_groups_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p, _i32p,
                                              C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_calc_groups.argtypes = [_dp, _dp, _lp, C.c_int, _i32p, _i32p, C.c_int, C.c_double, C.c_int,
                                               _dp, _dp, _dp, _dp, C.c_int, C.c_char_p, C.c_int]
        _llp = C.POINTER(C.c_longlong)
        L.freesasa_gpu_interface_pairs_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p, _i32p,
                                                       C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_longlong, _llp, _llp, _i32p, _i32p, _llp]
        L.freesasa_gpu_interfaces_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p, _i32p,
                                                  C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_longlong, C.c_longlong, _llp, _llp, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_calc_interface_pairs.argtypes = [_dp, _dp, _lp, C.c_int, _i32p, _i32p, C.c_int, C.c_double, C.c_int,
                                                        C.c_longlong, _llp, _llp, _i32p, _i32p, _llp, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_calc_interfaces.argtypes = [_dp, _dp, _lp, C.c_int, _i32p, _i32p, C.c_int, C.c_double, C.c_int,
                                                   _dp, _dp, _dp, _dp, C.c_longlong, C.c_longlong, _llp, _llp, _i32p, _i32p, _dp,
                                                   _lp, _i32p, _dp, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_interface_residues_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p, _i32p,
                                                          _lp, C.c_int, C.c_double, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, _llp, _llp,
                                                          _llp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_calc_interface_residues.argtypes = [_dp, _dp, _lp, C.c_int, _i32p, _i32p, _lp, C.c_int, C.c_int, C.c_double,
                                                           C.c_int, C.c_double, _dp, _dp, _dp, _dp, C.c_longlong, C.c_longlong,
                                                           C.c_longlong, _llp, _llp, _llp, _i32p, _i32p, _dp, _lp, _i32p, _dp, _lp,
                                                           _i32p, _i32p, _dp, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_interface_contacts_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p, _i32p,
                                                          C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _llp, _llp, _llp, _llp,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_calc_interface_contacts.argtypes = [_dp, _dp, _lp, C.c_int, _i32p, _i32p, C.c_int, C.c_double, C.c_int,
                                                           _dp, _dp, _dp, _dp, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong,
                                                           _llp, _llp, _llp, _llp, _i32p, _i32p, _dp, _lp, _i32p, _dp, _lp, _i32p, _i32p,
                                                           _dp, C.POINTER(C.c_uint32), _i32p, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_interface_residue_contacts_dev.argtypes = L.freesasa_gpu_interface_contacts_dev.argtypes + [
            _lp, C.c_int, C.c_longlong, _llp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_calc_interface_residue_contacts.argtypes = L.freesasa_gpu_calc_interface_contacts.argtypes[:-3] + [
            _lp, C.c_int, C.c_longlong, _llp, _lp, _i32p, _i32p, _dp, _i32p, C.c_int, C.c_char_p, C.c_int]
        _otp = C.POINTER(_OccupancyTable)
        L.freesasa_gpu_contact_occupancy_open.argtypes = [_dp, C.c_int, _i32p, C.c_int, _lp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                                          C.c_char_p, C.c_int]
        L.freesasa_gpu_contact_occupancy_open.restype = C.c_void_p
        L.freesasa_gpu_contact_occupancy_add_frames.argtypes = [C.c_void_p, _dp, C.c_int, _lp]
        L.freesasa_gpu_contact_occupancy_add_rows.argtypes = [C.c_void_p, C.c_int, _lp, _i32p, _i32p, _dp]
        L.freesasa_gpu_contact_occupancy_table.argtypes = [C.c_void_p, _otp]
        L.freesasa_gpu_contact_occupancy_table_free.argtypes = [_otp]
        L.freesasa_gpu_contact_occupancy_table_free.restype = None
        L.freesasa_gpu_contact_occupancy_close.argtypes = [C.c_void_p]
        L.freesasa_gpu_contact_occupancy_close.restype = None
        L.freesasa_gpu_contact_occupancy_error.argtypes = [C.c_void_p]
        L.freesasa_gpu_contact_occupancy_error.restype = C.c_char_p
        L.freesasa_gpu_calc_contact_occupancy.argtypes = [_dp, C.c_int, _dp, C.c_int, _i32p, C.c_int, _lp, C.c_int, C.c_double, C.c_int, C.c_int,
                                                          _lp, _otp, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_sr_volume_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_double, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_calc_volume.argtypes = [_dp, _dp, _lp, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp, _dp, _dp, _dp,
                                               C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_sr_masks_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_double, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_dots_count_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
        L.freesasa_gpu_dots_expand_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_calc_masks.argtypes = [_dp, _dp, _lp, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp, _u32p, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_masks_count.argtypes = [_u32p, C.c_longlong, C.c_int, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
        L.freesasa_gpu_dots_from_masks.argtypes = [_dp, _dp, C.c_longlong, C.c_double, C.c_int, _u32p, C.c_longlong, _lp, _dp, _ip, _ip,
                                                   C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_periodic_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_int, _dp, C.c_double, C.c_int,
                                                C.c_void_p, C.c_void_p, _lp]
        L.freesasa_gpu_calc_periodic.argtypes = [_dp, _dp, _lp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp, _dp, _lp,
                                                 C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_periodic_triclinic_dev.argtypes = L.freesasa_gpu_periodic_dev.argtypes
        L.freesasa_gpu_calc_periodic_triclinic.argtypes = L.freesasa_gpu_calc_periodic.argtypes
        L.freesasa_gpu_groups_periodic_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_void_p, _i32p, _dp,
                                                       C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _lp]
        L.freesasa_gpu_groups_periodic_triclinic_dev.argtypes = L.freesasa_gpu_groups_periodic_dev.argtypes
        L.freesasa_gpu_calc_groups_periodic.argtypes = [_dp, _dp, _lp, C.c_int, _i32p, _i32p, _dp, C.c_int, C.c_double, C.c_int,
                                                        _dp, _dp, _dp, _dp, _lp, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_calc_groups_periodic_triclinic.argtypes = L.freesasa_gpu_calc_groups_periodic.argtypes
        L.freesasa_gpu_cell_widths.argtypes = [_dp, _dp]
        L.freesasa_gpu_cell_from_dcd.argtypes = [_dp, _dp, C.c_char_p, C.c_int]
        L.freesasa_gpu_cell_from_lengths_angles.argtypes = [_dp, _dp, _dp, C.c_char_p, C.c_int]
        L.freesasa_gpu_test_points.argtypes = [C.c_int, _dp]
        L.freesasa_gpu_test_points.restype = None
        L.freesasa_gpu_calc_batch.argtypes = [_dp, _dp, _lp, C.c_int, C.c_int, C.c_double, C.c_int,
                                              _dp, _ip, _dp, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_calc_batch_devices.argtypes = [_dp, _dp, _lp, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp,
                                                      _ip, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_calc_batch_pipelined.argtypes = [_dp, _dp, _lp, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp,
                                                        C.c_int, C.c_int, C.c_longlong, C.c_char_p, C.c_int]
        L.freesasa_gpu_lr_neighbors_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
        L.freesasa_gpu_arc_union_dev.argtypes = [C.c_void_p, _dp, _ip, C.c_int, _dp]
        L.freesasa_gpu_kat_elementwise_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_double,
                                                       C.c_void_p, C.c_void_p]
        L.freesasa_gpu_kat_wave_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.freesasa_gpu_xtc_decode_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.freesasa_gpu_cell_sort_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _lp, C.c_int, C.c_double, C.c_int, C.c_longlong, C.c_longlong, C.c_int] + [C.c_void_p] * 9
        L.freesasa_gpu_cell_sort_cap.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_longlong]
        L.freesasa_gpu_cell_sort_cap.restype = C.c_longlong
        L.freesasa_gpu_xtc_decode_check.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        L.freesasa_gpu_release_pool.argtypes = []
        L.freesasa_gpu_release_pool.restype = None
        L.freesasa_gpu_test_fail_after.argtypes = [C.c_int]
        L.freesasa_gpu_test_fail_after.restype = None
        L.freesasa_host_test_fail_after.argtypes = [C.c_int]
        L.freesasa_host_test_fail_after.restype = C.c_int
        L.freesasa_gpu_shard_cuts.argtypes = [_lp, C.c_int, C.c_int, _ip]
        L.freesasa_gpu_shard_cuts.restype = None
        L.freesasa_gpu_sweep_files.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                               C.c_longlong, _dp, _dp, _lp, _ip, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_sweep_files_resumable.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                         C.c_longlong, _dp, _dp, _lp, _ip, C.c_char_p, C.c_longlong, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_trajectory.argtypes = [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                              C.c_int, _dp, _dp, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_trajectory_file.argtypes = [C.c_char_p, C.c_int, C.c_longlong, _dp, C.c_int, C.c_longlong, C.c_int, C.c_double,
                                                   C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_longlong, C.c_int,
                                                   C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
        L.freesasa_gpu_sweep_files_devices.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                       C.c_longlong, _dp, _dp, _lp, _ip, C.c_char_p, C.c_longlong, _ip, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_sweep_files_classified.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                          C.c_longlong, _dp, _dp, _lp, _ip, C.c_char_p, C.c_longlong, _ip, C.c_int,
                                                          C.c_void_p, C.c_char_p, C.c_int]
        L.freesasa_gpu_sweep_cache_devices.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_longlong, _dp, _dp, _lp, _ip, C.c_int,
                                                       _ip, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_trajectory_devices.argtypes = [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                      C.c_int, _dp, _dp, _ip, C.c_int, C.c_char_p, C.c_int]
        L.freesasa_gpu_trajectory_file_devices.argtypes = [C.c_char_p, C.c_int, C.c_longlong, _dp, C.c_int, C.c_longlong, C.c_int, C.c_double,
                                                           C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_longlong, _ip, C.c_int,
                                                           C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
        _lib = L
    return _lib


def _devs(devices, device):
    """the device list of a driver call: `devices` (a list; entries may repeat) or the single `device`"""
    d = np.ascontiguousarray([device] if devices is None else list(devices), dtype=np.int32)
    return d, d.ctypes.data_as(_ip), int(d.size)


def device_count():
    return lib().freesasa_gpu_device_count()


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def calc_coord(xyz, radii, alg=LEE_RICHARDS, probe=1.4, n_points=100, n_slices=20, n_threads=1):
    """freesasa_calc_coord(): returns (per-atom sasa, total) or raises on NULL."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    p = Parameters(alg, probe, n_points, n_slices, n_threads)
    res = lib().freesasa_calc_coord(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp),
                                    radii.size, C.byref(p))
    if not res:
        raise RuntimeError("freesasa_calc_coord returned NULL (see the library's error output)")
    sasa = np.ctypeslib.as_array(res.contents.sasa, (radii.size,)).copy()
    total = res.contents.total
    lib().freesasa_result_free(res)
    return sasa, total


def calc_batch(xyz, radii, offsets, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1):
    """freesasa_gpu_calc_batch() on host arrays: (sasa, counts-or-None, totals)."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, ns = radii.size, offsets.size - 1
    sasa, totals = np.empty(n), np.empty(ns)
    counts = np.empty(n, dtype=np.int32) if alg == SHRAKE_RUPLEY else None
    err = C.create_string_buffer(512)
    ret = lib().freesasa_gpu_calc_batch(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp),
                                        offsets.ctypes.data_as(_lp), ns, alg, probe, resolution,
                                        sasa.ctypes.data_as(_dp),
                                        counts.ctypes.data_as(_ip) if counts is not None else None,
                                        totals.ctypes.data_as(_dp), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_batch: " + err.value.decode())
    return sasa, counts, totals


def calc_groups(xyz, radii, offsets, group, n_groups, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1):
    """freesasa_gpu_calc_groups() on host arrays: (sasa, iso, totals, group_totals[G, 3]).  group: an int32 id per atom,
    local to its structure (-1: in no group); n_groups: groups per structure.  iso - sasa is each atom's buried area;
    group_totals rows are (isolated, complex, buried) per group, structure-major."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    group = np.ascontiguousarray(group, dtype=np.int32)
    n_groups = np.ascontiguousarray(n_groups, dtype=np.int32)
    n, ns = radii.size, offsets.size - 1
    if group.size != n or n_groups.size != ns:
        raise ValueError("group needs one id per atom and n_groups one count per structure")
    G = int(n_groups.astype(np.int64).sum())
    sasa, iso, totals, gt = np.empty(n), np.empty(n), np.empty(ns), np.empty((max(G, 0), 3))
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    ret = lib().freesasa_gpu_calc_groups(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                         group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32), alg, probe, resolution,
                                         sasa.ctypes.data_as(_dp), iso.ctypes.data_as(_dp), totals.ctypes.data_as(_dp),
                                         gt.ctypes.data_as(_dp), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_groups: " + err.value.decode())
    return sasa, iso, totals, gt


def _group_batch(xyz, radii, offsets, group, n_groups):
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    group = np.ascontiguousarray(group, dtype=np.int32)
    n_groups = np.ascontiguousarray(n_groups, dtype=np.int32)
    if group.size != radii.size or n_groups.size != offsets.size - 1:
        raise ValueError("group needs one id per atom and n_groups one count per structure")
    return xyz, radii, offsets, group, n_groups


class InterfacePairs:
    """The groups of a batch that touch: n_pairs, n_pair_atoms (the atoms of all pair structures), pair_struct [P] and
    pair_groups [P, 2] (int32; structure-major, then g, then h ascending), n_tests and n_candidates (the pairs the screen
    tested and those whose boxes came close)."""

    def __init__(self, n_pairs, n_pair_atoms, pair_struct, pair_groups, n_tests, n_candidates):
        self.n_pairs, self.n_pair_atoms = n_pairs, n_pair_atoms
        self.pair_struct, self.pair_groups = pair_struct, pair_groups
        self.n_tests, self.n_candidates = n_tests, n_candidates


class Interfaces:
    """calc_interfaces()'s result: sasa, iso [n], totals [n_structs], group_totals [G, 3] as calc_groups gives them; pair_struct
    [P], pair_groups [P, 2], pair_areas [P, 6] = (iso_g, iso_h, in_pair_g, in_pair_h, buried_g, buried_h); with per_atom
    side_offsets [2P + 1], pair_atom [M], pair_buried [M] (else None); with res_first the per-residue table: res_offsets [2P + 1]
    (the row range of every side), res_index [R] (the batch-wide residue), res_atoms [R], res_areas [R, 3] = (iso_res,
    in_pair_res, buried_res) and n_res_rows = R (else None)."""

    def __init__(self, sasa, iso, totals, group_totals, pair_struct, pair_groups, pair_areas, side_offsets, pair_atom, pair_buried,
                 res_offsets=None, res_index=None, res_atoms=None, res_areas=None):
        self.sasa, self.iso, self.totals, self.group_totals = sasa, iso, totals, group_totals
        self.pair_struct, self.pair_groups, self.pair_areas = pair_struct, pair_groups, pair_areas
        self.side_offsets, self.pair_atom, self.pair_buried = side_offsets, pair_atom, pair_buried
        self.n_pairs = int(pair_struct.size)
        self.res_offsets, self.res_index, self.res_atoms, self.res_areas = res_offsets, res_index, res_atoms, res_areas
        self.n_res_rows = None if res_areas is None else int(res_areas.shape[0])

    def side_rows(self, p, side):
        """the rows of side 0 (group g) or 1 (group h) of pair p, as a slice into res_index, res_atoms and res_areas"""
        if self.res_offsets is None:
            raise ValueError("no per-residue table: calc_interfaces() was called without res_first")
        return slice(int(self.res_offsets[2 * p + side]), int(self.res_offsets[2 * p + side + 1]))


def interface_pairs(xyz, radii, offsets, group, n_groups, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1):
    """freesasa_gpu_calc_interface_pairs() on host arrays: which groups of every structure are in contact (the reference's
    neighbour test between their atoms; include/freesasa_gpu.h) -> InterfacePairs.  Two calls: the counts, then the list."""
    xyz, radii, offsets, group, n_groups = _group_batch(xyz, radii, offsets, group, n_groups)
    i32 = C.POINTER(C.c_int32)
    P, M, err = C.c_longlong(0), C.c_longlong(0), C.create_string_buffer(512)
    stats = (C.c_longlong * 2)()

    def call(cap, ps, pg):
        if lib().freesasa_gpu_calc_interface_pairs(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp),
                                                   offsets.size - 1, group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32), alg,
                                                   probe, resolution, cap, C.byref(P), C.byref(M),
                                                   None if ps is None else ps.ctypes.data_as(i32),
                                                   None if pg is None else pg.ctypes.data_as(i32), stats, device, err, 512):
            raise RuntimeError("freesasa_gpu_calc_interface_pairs: " + err.value.decode())

    call(0, None, None)
    ps, pg = np.empty(P.value, dtype=np.int32), np.empty((P.value, 2), dtype=np.int32)
    if P.value:
        call(P.value, ps, pg)
    return InterfacePairs(int(P.value), int(M.value), ps, pg, int(stats[0]), int(stats[1]))


def calc_interfaces(xyz, radii, offsets, group, n_groups, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1, per_atom=False,
                    res_first=None, min_buried=0.0):
    """freesasa_gpu_calc_interfaces() on host arrays -> Interfaces: calc_groups()'s results and a row for every pair of groups of
    a structure that are in contact, with each side's isolated area, its area in the pair taken on its own, and the
    difference: the interface area.  The arrays are sized by a first interface_pairs() call.
    res_first (the batch's residue boundaries [n_res + 1], as ingest.Batch.res_first): freesasa_gpu_calc_interface_residues()
    instead, which adds the per-residue table - a row for every residue of a side that loses more than min_buried; it has at
    most as many rows as the pair structures have atoms, so its arrays are sized by the same first call and trimmed."""
    xyz, radii, offsets, group, n_groups = _group_batch(xyz, radii, offsets, group, n_groups)
    n, ns = radii.size, offsets.size - 1
    pairs = interface_pairs(xyz, radii, offsets, group, n_groups, alg, probe, resolution, device)
    P, M = pairs.n_pairs, pairs.n_pair_atoms
    G = int(n_groups.astype(np.int64).sum())
    sasa, iso, totals, gt = np.empty(n), np.empty(n), np.empty(ns), np.empty((max(G, 0), 3))
    ps, pg, areas = np.empty(P, dtype=np.int32), np.empty((P, 2), dtype=np.int32), np.empty((P, 6))
    so, pa, pb = (np.empty(2 * P + 1, dtype=np.int64), np.empty(M, dtype=np.int32), np.empty(M)) if per_atom else (None, None, None)
    i32 = C.POINTER(C.c_int32)
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    Pc, Mc, err = C.c_longlong(0), C.c_longlong(0), C.create_string_buffer(512)
    if res_first is not None:
        res_first = np.ascontiguousarray(res_first, dtype=np.int64)
        if res_first.ndim != 1 or res_first.size < 2:
            raise ValueError("res_first must be a one-dimensional array of n_res + 1 >= 2 boundaries")
        ro, ri, ra, rar = np.empty(2 * P + 1, dtype=np.int64), np.empty(M, dtype=np.int32), np.empty(M, dtype=np.int32), np.empty((M, 3))
        Rc = C.c_longlong(0)
        ret = lib().freesasa_gpu_calc_interface_residues(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                                         group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32),
                                                         res_first.ctypes.data_as(_lp), res_first.size - 1, alg, probe, resolution,
                                                         min_buried, sasa.ctypes.data_as(_dp), iso.ctypes.data_as(_dp),
                                                         totals.ctypes.data_as(_dp), gt.ctypes.data_as(_dp), P, M, M, C.byref(Pc),
                                                         C.byref(Mc), C.byref(Rc), ps.ctypes.data_as(i32), pg.ctypes.data_as(i32),
                                                         areas.ctypes.data_as(_dp), opt(so, _lp), opt(pa, i32), opt(pb, _dp),
                                                         ro.ctypes.data_as(_lp), ri.ctypes.data_as(i32), ra.ctypes.data_as(i32),
                                                         rar.ctypes.data_as(_dp), device, err, 512)
        if ret:
            raise RuntimeError("freesasa_gpu_calc_interface_residues: " + err.value.decode())
        R = int(Rc.value)
        return Interfaces(sasa, iso, totals, gt, ps, pg, areas, so, pa, pb, ro, ri[:R].copy(), ra[:R].copy(), rar[:R].copy())
    ret = lib().freesasa_gpu_calc_interfaces(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                             group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32), alg, probe, resolution,
                                             sasa.ctypes.data_as(_dp), iso.ctypes.data_as(_dp), totals.ctypes.data_as(_dp),
                                             gt.ctypes.data_as(_dp), P, M, C.byref(Pc), C.byref(Mc), ps.ctypes.data_as(i32),
                                             pg.ctypes.data_as(i32), areas.ctypes.data_as(_dp), opt(so, _lp), opt(pa, i32), opt(pb, _dp),
                                             device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_interfaces: " + err.value.decode())
    return Interfaces(sasa, iso, totals, gt, ps, pg, areas, so, pa, pb)


class InterfaceContacts(Interfaces):
    """calc_interface_contacts()'s result: everything calc_interfaces(per_atom=True) gives, and the directed atom-atom contact
    table over the M pair-structure atoms: contact_first [M + 1] (int64, the row range of every atom), contact_partner [C]
    (int32, a pair-structure atom: pair_atom[j] is the input atom), contact_points [C] (int32), contact_area [C], buried_masks
    [M, 4] (uint32: the test points the partner buries), n_contacts = C, n_buried_dots = D_b; with res_first the rows folded per
    pair of residues: rescontact_offsets [2P + 1] (int64, the row range of every source side), rescontact_residues [Q, 2] (int32,
    the batch-wide residue of source and partner), rescontact_counts [Q, 2] (int32: contact rows folded, points), rescontact_area
    [Q], rescontact_reverse [Q] (int32: the row that runs the other way, or -1) and n_rescontacts = Q (else None)."""

    def __init__(self, base, contact_first, contact_partner, contact_points, contact_area, buried_masks, n_buried_dots, rescontacts=None):
        Interfaces.__init__(self, *base)
        self.contact_first, self.contact_partner, self.contact_points = contact_first, contact_partner, contact_points
        self.contact_area, self.buried_masks = contact_area, buried_masks
        self.n_contacts, self.n_buried_dots = int(contact_partner.size), int(n_buried_dots)
        (self.rescontact_offsets, self.rescontact_residues, self.rescontact_counts, self.rescontact_area,
         self.rescontact_reverse) = rescontacts if rescontacts is not None else (None,) * 5
        self.n_rescontacts = None if rescontacts is None else int(self.rescontact_area.size)

    def residue_side_rows(self, p, side):
        """the folded rows whose source is side 0 (group g) or 1 (group h) of pair p, as a range over the rescontact arrays"""
        if self.rescontact_offsets is None:
            raise ValueError("no residue-residue contact table: calc_interface_contacts() was called without res_first")
        return range(int(self.rescontact_offsets[2 * p + side]), int(self.rescontact_offsets[2 * p + side + 1]))

    def atom_rows(self, i):
        """the rows of pair-structure atom i, as a slice into contact_partner, contact_points and contact_area"""
        return slice(int(self.contact_first[i]), int(self.contact_first[i + 1]))

    def side_rows(self, p, side):
        """the rows of all atoms of side 0 (group g) or 1 (group h) of pair p, as a slice into the same arrays"""
        q = 2 * p + side
        return slice(int(self.contact_first[self.side_offsets[q]]), int(self.contact_first[self.side_offsets[q + 1]]))


def calc_interface_contacts(xyz, radii, offsets, group, n_groups, probe=1.4, n_points=100, device=-1, res_first=None):
    """freesasa_gpu_calc_interface_contacts() on host arrays -> InterfaceContacts: calc_interfaces() with Shrake-Rupley and, for
    every pair-structure atom, which atoms of the partner bury its test points, how many, and the area they stand for
    (include/freesasa_gpu.h).  Two calls: the counts, then the arrays.
    res_first (the batch's residue boundaries [n_res + 1], as ingest.Batch.res_first): the second call is
    freesasa_gpu_calc_interface_residue_contacts(), which adds the rows folded per pair of residues and their reverse rows; the
    folded table has at most as many rows as the contact table, so its arrays are sized by the same first call and trimmed."""
    xyz, radii, offsets, group, n_groups = _group_batch(xyz, radii, offsets, group, n_groups)
    n, ns = radii.size, offsets.size - 1
    G = int(n_groups.astype(np.int64).sum())
    i32, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    Pc, Mc, Cc, Dc, err = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.create_string_buffer(512)
    sasa, iso, totals, gt = np.empty(n), np.empty(n), np.empty(ns), np.empty((max(G, 0), 3))

    def call(P, M, Cn, arrays):
        ps, pg, areas, so, pa, pb, cf, cp, cn, ca, bm = arrays
        opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return lib().freesasa_gpu_calc_interface_contacts(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                                          group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32), SHRAKE_RUPLEY, probe,
                                                          n_points, sasa.ctypes.data_as(_dp), iso.ctypes.data_as(_dp),
                                                          totals.ctypes.data_as(_dp), gt.ctypes.data_as(_dp), P, M, Cn, 0, C.byref(Pc),
                                                          C.byref(Mc), C.byref(Cc), C.byref(Dc), opt(ps, i32), opt(pg, i32),
                                                          areas.ctypes.data_as(_dp), opt(so, _lp), opt(pa, i32), opt(pb, _dp), opt(cf, _lp),
                                                          opt(cp, i32), opt(cn, i32), opt(ca, _dp), opt(bm, u32), None, device, err, 512)

    pairs = interface_pairs(xyz, radii, offsets, group, n_groups, SHRAKE_RUPLEY, probe, n_points, device)
    P, M = pairs.n_pairs, pairs.n_pair_atoms
    areas = np.empty((P, 6))
    if call(P, M, 0, (None, None, areas, None, None, None, None, None, None, None, None)):      # the counts: no contact array is asked for
        raise RuntimeError("freesasa_gpu_calc_interface_contacts: " + err.value.decode())
    Cn = int(Cc.value)
    arrays = (np.empty(P, dtype=np.int32), np.empty((P, 2), dtype=np.int32), areas, np.empty(2 * P + 1, dtype=np.int64),
              np.empty(M, dtype=np.int32), np.empty(M), np.empty(M + 1, dtype=np.int64), np.empty(Cn, dtype=np.int32),
              np.empty(Cn, dtype=np.int32), np.empty(Cn), np.empty((M, 4), dtype=np.uint32))
    if res_first is not None:
        res_first = np.ascontiguousarray(res_first, dtype=np.int64)
        if res_first.ndim != 1 or res_first.size < 2:
            raise ValueError("res_first must be a one-dimensional array of n_res + 1 >= 2 boundaries")
        ps, pg, areas, so, pa, pb, cf, cp, cn, ca, bm = arrays
        qo, qr, qc = np.empty(2 * P + 1, dtype=np.int64), np.empty((Cn, 2), dtype=np.int32), np.empty((Cn, 2), dtype=np.int32)
        qa, qv, Qc = np.empty(Cn), np.empty(Cn, dtype=np.int32), C.c_longlong(0)
        if lib().freesasa_gpu_calc_interface_residue_contacts(
                xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns, group.ctypes.data_as(i32),
                n_groups.ctypes.data_as(i32), SHRAKE_RUPLEY, probe, n_points, sasa.ctypes.data_as(_dp), iso.ctypes.data_as(_dp),
                totals.ctypes.data_as(_dp), gt.ctypes.data_as(_dp), P, M, Cn, 0, C.byref(Pc), C.byref(Mc), C.byref(Cc), C.byref(Dc),
                ps.ctypes.data_as(i32), pg.ctypes.data_as(i32), areas.ctypes.data_as(_dp), so.ctypes.data_as(_lp), pa.ctypes.data_as(i32),
                pb.ctypes.data_as(_dp), cf.ctypes.data_as(_lp), cp.ctypes.data_as(i32), cn.ctypes.data_as(i32), ca.ctypes.data_as(_dp),
                bm.ctypes.data_as(u32), None, res_first.ctypes.data_as(_lp), res_first.size - 1, Cn, C.byref(Qc), qo.ctypes.data_as(_lp),
                qr.ctypes.data_as(i32), qc.ctypes.data_as(i32), qa.ctypes.data_as(_dp), qv.ctypes.data_as(i32), device, err, 512):
            raise RuntimeError("freesasa_gpu_calc_interface_residue_contacts: " + err.value.decode())
        Q = int(Qc.value)
        return InterfaceContacts((sasa, iso, totals, gt, ps, pg, areas, so, pa, pb), cf, cp, cn, ca, bm, Dc.value,
                                 (qo, qr[:Q].copy(), qc[:Q].copy(), qa[:Q].copy(), qv[:Q].copy()))
    if call(P, M, Cn, arrays):
        raise RuntimeError("freesasa_gpu_calc_interface_contacts: " + err.value.decode())
    ps, pg, areas, so, pa, pb, cf, cp, cn, ca, bm = arrays
    return InterfaceContacts((sasa, iso, totals, gt, ps, pg, areas, so, pa, pb), cf, cp, cn, ca, bm, Dc.value)


class ContactOccupancyTable:
    """A snapshot of the run table of a ContactOccupancy (include/freesasa_gpu.h has the definitions), copied out of the library's
    arrays: one row per distinct key (g, h, side, res_a, res_b), ascending - keys [U, 5] (int32), frames [U] and frames_either [U]
    (int64: the frames that hold the key / the key or its reversed key), counts [U, 2] (int64: the sums of n_rows and n_points),
    area [U, 3] (sum, min, max over the frames that hold the key), span [U, 2] (int64: the first and the last such frame), reverse
    [U] (int32: the row of the reversed key, or -1) - and n_frames, the frames the run had when it was taken."""

    def __init__(self, n_frames, keys, frames, frames_either, counts, area, span, reverse):
        self.n_frames = int(n_frames)
        self.keys, self.frames, self.frames_either, self.counts = keys, frames, frames_either, counts
        self.area, self.span, self.reverse = area, span, reverse
        self.n_rows = int(frames.size)

    def occupancy(self):
        """frames / n_frames: the share of the run's frames in which the key has a row"""
        return self.frames / float(self.n_frames) if self.n_frames else np.zeros(self.n_rows)

    def occupancy_either(self):
        """frames_either / n_frames: ... in which the key or its reversed key has one - what a contact map plots"""
        return self.frames_either / float(self.n_frames) if self.n_frames else np.zeros(self.n_rows)

    def mean_area(self):
        """area[:, 0] / frames: the mean area over the frames in which the key is present"""
        return self.area[:, 0] / self.frames

    def pair_rows(self, g, h, side):
        """the rows of pair (g, h) whose source is side 0 (group g) or 1 (group h), as a range over the arrays"""
        k = self.keys
        at = np.nonzero((k[:, 0] == g) & (k[:, 1] == h) & (k[:, 2] == side))[0]
        return range(int(at[0]), int(at[-1]) + 1) if at.size else range(0, 0)


def _occupancy_table(t):
    """the arrays of a filled _OccupancyTable, copied; the library's blocks are given back"""
    U = int(t.n_rows)
    try:
        take = lambda p, shape, dtype: np.ctypeslib.as_array(p, shape=shape).astype(dtype, copy=True) if U else np.zeros(shape, dtype)
        return ContactOccupancyTable(t.n_frames, take(t.keys, (U, 5), np.int32), take(t.frames, (U,), np.int64), take(t.frames_either, (U,), np.int64),
                                     take(t.counts, (U, 2), np.int64), take(t.area, (U, 3), np.float64), take(t.span, (U, 2), np.int64),
                                     take(t.reverse, (U,), np.int32))
    finally:
        lib().freesasa_gpu_contact_occupancy_table_free(C.byref(t))


def _occupancy_system(radii, group, res_first):
    radii, group = _f64(radii).reshape(-1), np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
    res_first = np.ascontiguousarray(res_first, dtype=np.int64).reshape(-1)
    if group.size != radii.size:
        raise ValueError("group must have one id per atom")
    if res_first.size < 1:
        raise ValueError("res_first must hold n_res + 1 boundaries")
    return radii, group, res_first


class ContactOccupancy:
    """freesasa_gpu_contact_occupancy_open(): a streaming accumulator of the residue contact occupancy map of ONE system over the
    frames of a run (include/freesasa_gpu.h has the definitions): radii [n], group [n] (int32, -1: in no group), n_groups and
    res_first [n_res + 1] are constant over the run; Shrake-Rupley with n_points <= 128.  add(frames) takes the run's next frames
    [f, n, 3] and returns frame_counts [f, 2] = (pairs, folded rows) per frame; add_rows() takes frames whose folded rows the
    caller has already; table() is a snapshot (the accumulator goes on).  The table does not depend on how the frames were cut
    over the calls or on frames_per_batch.  radii=None: an accumulator for add_rows() only.  A failed add poisons the accumulator:
    every later call raises with the first failure's message.  Use as a context manager, or close()."""

    def __init__(self, radii, group=None, n_groups=0, res_first=None, probe=1.4, n_points=100, frames_per_batch=0, device=-1):
        err = C.create_string_buffer(512)
        i32 = C.POINTER(C.c_int32)
        self.n_atoms = 0
        if radii is None:
            self._h = lib().freesasa_gpu_contact_occupancy_open(None, 0, None, 0, None, 0, probe, n_points, frames_per_batch, device, err, 512)
        else:
            radii, group, res_first = _occupancy_system(radii, group, res_first)
            self.n_atoms = int(radii.size)
            self._h = lib().freesasa_gpu_contact_occupancy_open(radii.ctypes.data_as(_dp), radii.size, group.ctypes.data_as(i32), n_groups,
                                                               res_first.ctypes.data_as(_lp), res_first.size - 1, probe, n_points,
                                                               frames_per_batch, device, err, 512)
        if not self._h:
            raise RuntimeError("freesasa_gpu_contact_occupancy_open: " + err.value.decode())

    def _error(self, what):
        return RuntimeError(what + ": " + lib().freesasa_gpu_contact_occupancy_error(self._h).decode())

    def _handle(self):
        if not self._h:
            raise ValueError("the accumulator is closed")
        return self._h

    def add(self, frames):
        """freesasa_gpu_contact_occupancy_add_frames(): frames [f, n, 3] (or [n, 3]: one frame) -> frame_counts [f, 2] int64"""
        h = self._handle()
        frames = _f64(frames)
        if self.n_atoms and frames.size % (3 * self.n_atoms):
            raise ValueError("frames must be [f, n_atoms, 3]")
        f = frames.size // (3 * self.n_atoms) if self.n_atoms else 0
        counts = np.zeros((f, 2), dtype=np.int64)
        if lib().freesasa_gpu_contact_occupancy_add_frames(h, frames.reshape(-1).ctypes.data_as(_dp), f, counts.ctypes.data_as(_lp)):
            raise self._error("freesasa_gpu_contact_occupancy_add_frames")
        return counts

    def add_rows(self, frame_first, keys, counts, area):
        """freesasa_gpu_contact_occupancy_add_rows(): frame_first [f + 1], keys [q, 5], counts [q, 2], area [q]"""
        h = self._handle()
        i32 = C.POINTER(C.c_int32)
        frame_first = np.ascontiguousarray(frame_first, dtype=np.int64).reshape(-1)
        keys, counts = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1), np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        area = _f64(area).reshape(-1)
        if frame_first.size < 1:
            raise ValueError("frame_first must hold f + 1 boundaries")
        q = int(frame_first[-1])
        if q > 0 and (keys.size < 5 * q or counts.size < 2 * q or area.size < q):
            raise ValueError("keys, counts and area must hold frame_first[-1] rows")
        if lib().freesasa_gpu_contact_occupancy_add_rows(h, frame_first.size - 1, frame_first.ctypes.data_as(_lp), keys.ctypes.data_as(i32),
                                                         counts.ctypes.data_as(i32), area.ctypes.data_as(_dp)):
            raise self._error("freesasa_gpu_contact_occupancy_add_rows")

    def table(self):
        """freesasa_gpu_contact_occupancy_table() -> ContactOccupancyTable"""
        t = _OccupancyTable()
        if lib().freesasa_gpu_contact_occupancy_table(self._handle(), C.byref(t)):
            raise self._error("freesasa_gpu_contact_occupancy_table")
        return _occupancy_table(t)

    def close(self):
        if self._h:
            lib().freesasa_gpu_contact_occupancy_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def contact_occupancy(frames, radii, group, n_groups, res_first, probe=1.4, n_points=100, frames_per_batch=0, device=-1, frame_counts=False):
    """freesasa_gpu_calc_contact_occupancy() on host arrays -> ContactOccupancyTable: the one-shot form of ContactOccupancy over
    frames [f, n, 3]; with frame_counts=True (table, frame_counts [f, 2])."""
    radii, group, res_first = _occupancy_system(radii, group, res_first)
    frames = _f64(frames)
    if frames.size % (3 * max(radii.size, 1)):
        raise ValueError("frames must be [f, n_atoms, 3]")
    f = frames.size // (3 * max(radii.size, 1))
    counts = np.zeros((f, 2), dtype=np.int64)
    t, err = _OccupancyTable(), C.create_string_buffer(512)
    if lib().freesasa_gpu_calc_contact_occupancy(frames.reshape(-1).ctypes.data_as(_dp), f, radii.ctypes.data_as(_dp), radii.size,
                                                 group.ctypes.data_as(C.POINTER(C.c_int32)), n_groups, res_first.ctypes.data_as(_lp),
                                                 res_first.size - 1, probe, n_points, frames_per_batch, counts.ctypes.data_as(_lp), C.byref(t),
                                                 device, err, 512):
        raise RuntimeError("freesasa_gpu_calc_contact_occupancy: " + err.value.decode())
    table = _occupancy_table(t)
    return (table, counts) if frame_counts else table


def calc_volume(xyz, radii, offsets, probe=1.4, n_points=100, device=-1, per_atom=False):
    """freesasa_gpu_calc_volume() on host arrays: (sasa, counts, totals, volumes) - the Shrake-Rupley areas, exposed-point
    counts and totals of calc_batch, bit for bit, and the volume the solvent-accessible surface of every structure encloses
    (what `gmx sasa -tv` gives; include/freesasa_gpu.h has the definition) - and with per_atom=True behind them evec [n, 3],
    every atom's sum of its exposed unit points, and vol [n], its term of the volume.  Up to 128 test points."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, ns = radii.size, offsets.size - 1
    sasa, totals, volumes = np.empty(n), np.empty(ns), np.empty(ns)
    counts = np.empty(n, dtype=np.int32)
    evec, vol = (np.empty((n, 3)), np.empty(n)) if per_atom else (None, None)
    err = C.create_string_buffer(512)
    opt = lambda a: None if a is None else a.ctypes.data_as(_dp)
    ret = lib().freesasa_gpu_calc_volume(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                         probe, n_points, sasa.ctypes.data_as(_dp), counts.ctypes.data_as(_ip), opt(evec), opt(vol),
                                         totals.ctypes.data_as(_dp), volumes.ctypes.data_as(_dp), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_volume: " + err.value.decode())
    return (sasa, counts, totals, volumes, evec, vol) if per_atom else (sasa, counts, totals, volumes)


def calc_masks(xyz, radii, offsets, probe=1.4, n_points=100, device=-1):
    """freesasa_gpu_calc_masks() on host arrays: (sasa, counts, totals, masks) - the Shrake-Rupley areas, exposed-point counts and
    totals of calc_batch, bit for bit, and masks [n, 4] uint32: bit k & 31 of word k >> 5 of atom i is set iff test point k of
    atom i is exposed (include/freesasa_gpu.h has the definitions).  Up to 128 test points."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, ns = radii.size, offsets.size - 1
    sasa, totals = np.empty(n), np.empty(ns)
    counts, masks = np.empty(n, dtype=np.int32), np.empty((n, 4), dtype=np.uint32)
    err = C.create_string_buffer(512)
    ret = lib().freesasa_gpu_calc_masks(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns, probe, n_points,
                                        sasa.ctypes.data_as(_dp), counts.ctypes.data_as(_ip), totals.ctypes.data_as(_dp),
                                        masks.ctypes.data_as(_u32p), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_masks: " + err.value.decode())
    return sasa, counts, totals, masks


def masks_count(masks, n_points=100):
    """freesasa_gpu_masks_count(): the number of dots the masks [n, 4] hold (on the host; refused if a bit at or above n_points is set)"""
    masks = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
    D, err = C.c_longlong(0), C.create_string_buffer(512)
    if lib().freesasa_gpu_masks_count(masks.ctypes.data_as(_u32p), masks.size // 4, n_points, C.byref(D), err, 512):
        raise RuntimeError("freesasa_gpu_masks_count: " + err.value.decode())
    return int(D.value)


def dots_from_masks(xyz, radii, masks, n_dots, probe=1.4, n_points=100, device=-1, with_index=False):
    """freesasa_gpu_dots_from_masks() on host arrays: the surface dots of stored masks [n, 4] -> (dots [n_dots, 3], dot_first
    [n + 1] int64), with with_index=True behind them dot_atom [n_dots] and dot_point [n_dots] (int32).  n_dots: what the masks
    are held to have (the sum of `counts`); refused if their popcount is another number or a bit at or above n_points is set."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    masks = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
    n, D = radii.size, int(n_dots)
    if xyz.size != 3 * n or masks.size != 4 * n:
        raise ValueError("xyz [n, 3], radii [n] and masks [n, 4] must agree")
    dots, first = np.empty((max(D, 0), 3)), np.empty(n + 1, dtype=np.int64)
    atom, point = (np.empty(max(D, 0), dtype=np.int32), np.empty(max(D, 0), dtype=np.int32)) if with_index else (None, None)
    err = C.create_string_buffer(512)
    opt = lambda a: None if a is None else a.ctypes.data_as(_ip)
    ret = lib().freesasa_gpu_dots_from_masks(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), n, probe, n_points, masks.ctypes.data_as(_u32p),
                                             D, first.ctypes.data_as(_lp), dots.ctypes.data_as(_dp), opt(atom), opt(point), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_dots_from_masks: " + err.value.decode())
    return (dots, first, atom, point) if with_index else (dots, first)


def calc_dots(xyz, radii, offsets, probe=1.4, n_points=100, device=-1, with_index=False):
    """calc_masks() and dots_from_masks() behind it: (sasa, counts, totals, dots [D, 3], dot_offsets [n_structs + 1]) - the dots of
    structure s are dots[dot_offsets[s]:dot_offsets[s + 1]], atom by atom, within an atom by ascending test point: what
    `gmx sasa -q` writes - and with with_index=True behind them dot_atom [D] and dot_point [D].  A dot's outward normal is
    test_points(n_points)[dot_point], the area it stands for 4 pi (r + probe)^2 / n_points.  (The arrays are sized by
    masks_count(): the loader does no arithmetic of its own.)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    sasa, counts, totals, masks = calc_masks(xyz, radii, offsets, probe, n_points, device)
    got = dots_from_masks(xyz, radii, masks, masks_count(masks, n_points), probe, n_points, device, with_index)
    dot_offsets = got[1][offsets]
    return (sasa, counts, totals, got[0], dot_offsets) + tuple(got[2:])


def calc_periodic(xyz, radii, offsets, cells, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1):
    """freesasa_gpu_calc_periodic() on host arrays: (sasa, totals, images).  cells [n_structs, 3]: the orthorhombic cell of
    every structure; each edge must be finite and at least 2 (max radius of the structure + probe).  sasa: every atom's area
    among the periodic images of its structure; totals: per structure over its own atoms; images [n_structs] int64: the image
    atoms the device added to every structure."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    cells = _f64(cells).reshape(-1)
    n, ns = radii.size, offsets.size - 1
    if cells.size != 3 * ns:
        raise ValueError("cells needs three edges per structure")
    sasa, totals, images = np.empty(n), np.empty(ns), np.zeros(ns, dtype=np.int64)
    err = C.create_string_buffer(512)
    ret = lib().freesasa_gpu_calc_periodic(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                           cells.ctypes.data_as(_dp), alg, probe, resolution, sasa.ctypes.data_as(_dp),
                                           totals.ctypes.data_as(_dp), images.ctypes.data_as(_lp), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_periodic: " + err.value.decode())
    return sasa, totals, images


def calc_periodic_triclinic(xyz, radii, offsets, cells6, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1):
    """freesasa_gpu_calc_periodic_triclinic() on host arrays: (sasa, totals, images) as calc_periodic.  cells6 [n_structs, 6]:
    every structure's cell as (ax, bx, by, cx, cy, cz), the lower-triangular box matrix with rows a, b, c; all finite, ax, by,
    cz > 0 and every width (cell_widths) at least 2 (max radius of the structure + probe)."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    cells6 = _f64(cells6).reshape(-1)
    n, ns = radii.size, offsets.size - 1
    if cells6.size != 6 * ns:
        raise ValueError("cells6 needs six numbers per structure")
    sasa, totals, images = np.empty(n), np.empty(ns), np.zeros(ns, dtype=np.int64)
    err = C.create_string_buffer(512)
    ret = lib().freesasa_gpu_calc_periodic_triclinic(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                                     cells6.ctypes.data_as(_dp), alg, probe, resolution, sasa.ctypes.data_as(_dp),
                                                     totals.ctypes.data_as(_dp), images.ctypes.data_as(_lp), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_periodic_triclinic: " + err.value.decode())
    return sasa, totals, images


def _calc_groups_periodic(name, W, xyz, radii, offsets, group, n_groups, cells, alg, probe, resolution, device):
    xyz, radii, offsets, group, n_groups = _group_batch(xyz, radii, offsets, group, n_groups)
    cells = _f64(cells).reshape(-1)
    n, ns = radii.size, offsets.size - 1
    if cells.size != W * ns:
        raise ValueError("cells needs three edges per structure" if W == 3 else "cells6 needs six numbers per structure")
    G = int(n_groups.astype(np.int64).sum())
    sasa, iso, totals, gt = np.empty(n), np.empty(n), np.empty(ns), np.empty((max(G, 0), 3))
    images = np.zeros(ns, dtype=np.int64)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    ret = getattr(lib(), name)(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                               group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32), cells.ctypes.data_as(_dp), alg, probe,
                               resolution, sasa.ctypes.data_as(_dp), iso.ctypes.data_as(_dp), totals.ctypes.data_as(_dp),
                               gt.ctypes.data_as(_dp), images.ctypes.data_as(_lp), device, err, 512)
    if ret:
        raise RuntimeError(name + ": " + err.value.decode())
    return sasa, iso, totals, gt, images


def calc_groups_periodic(xyz, radii, offsets, group, n_groups, cells, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1):
    """freesasa_gpu_calc_groups_periodic() on host arrays: (sasa, iso, totals, group_totals[G, 3], images) - calc_groups with every
    structure among the periodic images of its orthorhombic cell (cells [n_structs, 3], see calc_periodic) and every group,
    taken on its own, among ITS images in the same cell: chains that lie in different images of the box bury what they bury."""
    return _calc_groups_periodic("freesasa_gpu_calc_groups_periodic", 3, xyz, radii, offsets, group, n_groups, cells, alg, probe,
                                 resolution, device)


def calc_groups_periodic_triclinic(xyz, radii, offsets, group, n_groups, cells6, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1):
    """freesasa_gpu_calc_groups_periodic_triclinic(): calc_groups_periodic for triclinic cells (cells6 [n_structs, 6], see
    calc_periodic_triclinic)."""
    return _calc_groups_periodic("freesasa_gpu_calc_groups_periodic_triclinic", 6, xyz, radii, offsets, group, n_groups, cells6, alg,
                                 probe, resolution, device)


def cell_widths(cell6):
    """freesasa_gpu_cell_widths(): the distances (d_a, d_b, d_c) between the opposite faces of the cell (ax, bx, by, cx, cy, cz);
    ValueError for an entry that is not finite or a diagonal entry that is not positive."""
    cell6, out = _f64(cell6).reshape(-1), np.empty(3)
    if cell6.size != 6:
        raise ValueError("a cell is six numbers")
    if lib().freesasa_gpu_cell_widths(cell6.ctypes.data_as(_dp), out.ctypes.data_as(_dp)):
        raise ValueError("freesasa_gpu_cell_widths: the entries must be finite and ax, by, cz > 0")
    return out


def cell_from_dcd(rec):
    """freesasa_gpu_cell_from_dcd(): a DCD unit-cell record (A, gamma, B, beta, alpha, C; the angles as cosines or degrees) ->
    the cell (ax, bx, by, cx, cy, cz); ValueError with the library's reason for a record that spans no cell."""
    rec, out = _f64(rec).reshape(-1), np.empty(6)
    if rec.size != 6:
        raise ValueError("a cell record is six numbers")
    why = C.create_string_buffer(256)
    if lib().freesasa_gpu_cell_from_dcd(rec.ctypes.data_as(_dp), out.ctypes.data_as(_dp), why, 256):
        raise ValueError("freesasa_gpu_cell_from_dcd: " + why.value.decode())
    return out


def cell_from_lengths_angles(lengths, angles):
    """freesasa_gpu_cell_from_lengths_angles(): the edges (a, b, c) and the angles (alpha, beta, gamma) in degrees, as AMBER NetCDF
    files hold them -> the cell (ax, bx, by, cx, cy, cz), bit for bit what cell_from_dcd gives for the same numbers in degrees;
    ValueError with the library's reason for an angle outside (0, 180) or angles that span no cell."""
    lengths, angles, out = _f64(lengths).reshape(-1), _f64(angles).reshape(-1), np.empty(6)
    if lengths.size != 3 or angles.size != 3:
        raise ValueError("a cell is three lengths and three angles")
    why = C.create_string_buffer(256)
    if lib().freesasa_gpu_cell_from_lengths_angles(lengths.ctypes.data_as(_dp), angles.ctypes.data_as(_dp), out.ctypes.data_as(_dp), why, 256):
        raise ValueError("freesasa_gpu_cell_from_lengths_angles: " + why.value.decode())
    return out


def calc_batch_devices(xyz, radii, offsets, devices, alg=LEE_RICHARDS, probe=1.4, resolution=20):
    """freesasa_gpu_calc_batch_devices(): (sasa, counts-or-None, totals); contiguous runs of structures of
    about equal atom count go to the listed devices (one host thread each; a device may repeat)."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    devs = np.ascontiguousarray(devices, dtype=np.int32)
    n, ns = radii.size, offsets.size - 1
    sasa, totals = np.zeros(n), np.zeros(ns)
    counts = np.zeros(n, dtype=np.int32) if alg == SHRAKE_RUPLEY else None
    err = C.create_string_buffer(512)
    ret = lib().freesasa_gpu_calc_batch_devices(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                                alg, probe, resolution, sasa.ctypes.data_as(_dp),
                                                counts.ctypes.data_as(_ip) if counts is not None else None,
                                                totals.ctypes.data_as(_dp), devs.ctypes.data_as(_ip), devs.size, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_batch_devices: " + err.value.decode())
    return sasa, counts, totals


def calc_batch_pipelined(xyz, radii, offsets, alg=LEE_RICHARDS, probe=1.4, resolution=20, device=-1, lanes=0,
                         chunk_atoms=0, out=None):
    """freesasa_gpu_calc_batch_pipelined() on host arrays (numpy, or anything with .ctypes / data_ptr() such as a
    pinned torch tensor via its numpy view): (sasa, counts-or-None, totals).  `out` = (sasa, counts, totals) arrays
    to write into (e.g. page-locked ones); by default fresh numpy arrays."""
    xyz, radii = _f64(xyz).reshape(-1), _f64(radii)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, ns = radii.size, offsets.size - 1
    if out is None:
        sasa, totals = np.empty(n), np.empty(ns)
        counts = np.empty(n, dtype=np.int32) if alg == SHRAKE_RUPLEY else None
    else:
        sasa, counts, totals = out
    err = C.create_string_buffer(512)
    ret = lib().freesasa_gpu_calc_batch_pipelined(xyz.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), offsets.ctypes.data_as(_lp), ns,
                                                  alg, probe, resolution, sasa.ctypes.data_as(_dp),
                                                  counts.ctypes.data_as(_ip) if counts is not None else None,
                                                  totals.ctypes.data_as(_dp) if totals is not None else None,
                                                  device, lanes, chunk_atoms, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_calc_batch_pipelined: " + err.value.decode())
    return sasa, counts, totals


def shard_cuts(offsets, n_parts):
    """freesasa_gpu_shard_cuts(): first structure of each of n_parts contiguous, atom-balanced runs (+ the end)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    cuts = np.zeros(n_parts + 1, dtype=np.int32)
    lib().freesasa_gpu_shard_cuts(offsets.ctypes.data_as(_lp), offsets.size - 1, n_parts, cuts.ctypes.data_as(_ip))
    return cuts


def sweep_files(paths, alg=LEE_RICHARDS, probe=1.4, resolution=20, ingest_options=0, n_threads=0, batch_atoms=0,
                class_sums=True, device=-1, devices=None, classifier=None):
    """freesasa_gpu_sweep_files[_devices](): PDB / mmCIF files -> (totals[n], class_sums[n,3] or None, n_atoms[n],
    status[n]); loading of the next batch overlaps the GPU work on the current one.  devices: a list of devices
    (entries may repeat) that share the batches, largest first.  classifier: an ingest.Classifier in place of ProtOr
    (freesasa_gpu_sweep_files_classified), for the host and the device parser alike."""
    n = len(paths)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    totals, atoms, status = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    cls = np.zeros((n, 3)) if class_sums else None
    err = C.create_string_buffer(512)
    if classifier is not None:
        from . import ingest
        keep, dp_, nd = _devs(devices, device)
        ret = lib().freesasa_gpu_sweep_files_classified(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                                        totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp) if cls is not None else None,
                                                        atoms.ctypes.data_as(_lp), status.ctypes.data_as(_ip), None, 0, dp_, nd,
                                                        ingest._handle(classifier), err, 512)
    elif devices is None:
        ret = lib().freesasa_gpu_sweep_files(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                             totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp) if cls is not None else None,
                                             atoms.ctypes.data_as(_lp), status.ctypes.data_as(_ip), device, err, 512)
    else:
        keep, dp_, nd = _devs(devices, device)
        ret = lib().freesasa_gpu_sweep_files_devices(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                                     totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp) if cls is not None else None,
                                                     atoms.ctypes.data_as(_lp), status.ctypes.data_as(_ip), None, 0, dp_, nd, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_sweep_files: " + err.value.decode())
    return totals, cls, atoms, status


class ResidueTableC(C.Structure):
    """freesasa_gpu_residue_table (include/freesasa_gpu.h)."""
    _fields_ = [("n_files", C.c_int32), ("n_residues", C.c_int64), ("res_offsets", _lp), ("res_atoms", C.POINTER(C.c_int32)),
                ("res_ref", C.POINTER(C.c_int16)), ("abs", _dp), ("rel", _dp), ("res_name", C.POINTER(C.c_char)),
                ("res_number", C.POINTER(C.c_char)), ("res_chain", C.POINTER(C.c_char))]


class ResidueTable:
    """numpy copy of a freesasa_gpu_residue_table: file k owns residues [res_offsets[k], res_offsets[k + 1]); abs columns are
    total, main chain, side chain, polar, apolar, unknown, rel columns the first five over the reference areas (NaN: none);
    the labels are decoded like ingest.Batch decodes them."""

    def __init__(self, ct):
        n, nr = int(ct.n_files), int(ct.n_residues)

        def arr(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            nbytes = count * np.dtype(dtype).itemsize    # (one copy: a view of the C block, copied before the block is freed)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_ubyte)), (nbytes,)).view(dtype).copy()
        self.n_files, self.n_residues = n, nr
        self.res_offsets = arr(ct.res_offsets, n + 1, np.int64)
        self.res_atoms = arr(ct.res_atoms, nr, np.int32)
        self.res_ref = arr(ct.res_ref, nr, np.int16)
        self.abs = arr(ct.abs, 6 * nr, np.float64).reshape(nr, 6)
        self.rel = arr(ct.rel, 5 * nr, np.float64).reshape(nr, 5)
        self.res_name_raw = arr(ct.res_name, nr, "S4")
        self.res_number_raw = arr(ct.res_number, nr, "S6")
        self.res_chain_raw = arr(ct.res_chain, nr, "S4")

    @property
    def res_name(self):
        return [v.decode() for v in self.res_name_raw.tolist()]

    @property
    def res_number(self):
        return [v.decode() for v in self.res_number_raw.tolist()]

    @property
    def res_chain(self):
        return [v.decode() for v in self.res_chain_raw.tolist()]

    def file(self, k):
        """the slice of file k's residues"""
        return slice(int(self.res_offsets[k]), int(self.res_offsets[k + 1]))


def _residue_proto(L):
    L.freesasa_gpu_sweep_files_residues.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                    C.c_longlong, _dp, _dp, _lp, _ip, _ip, C.c_int, C.c_void_p,
                                                    C.POINTER(ResidueTableC), C.c_char_p, C.c_int]
    L.freesasa_gpu_residue_table_free.argtypes = [C.POINTER(ResidueTableC)]
    L.freesasa_gpu_residue_table_free.restype = None
    return L


def sweep_files_residues(paths, alg=LEE_RICHARDS, probe=1.4, resolution=20, ingest_options=0, n_threads=0, batch_atoms=0,
                         device=-1, devices=None, classifier=None):
    """freesasa_gpu_sweep_files_residues(): sweep_files plus the per-residue table of all files -> (totals[n],
    class_sums[n,3], n_atoms[n], status[n], table: a ResidueTable).  The per-atom areas stay on the device; with
    ingest.PARSE_ON_DEVICE the residues are built there too.  classifier: an ingest.Classifier in place of ProtOr (the
    relative areas are then NaN throughout)."""
    from . import ingest
    L = _residue_proto(lib())
    n = len(paths)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    totals, atoms, status = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    cls = np.zeros((n, 3))
    err = C.create_string_buffer(512)
    keep, dp_, nd = _devs(devices, device)
    ct = ResidueTableC()
    ret = L.freesasa_gpu_sweep_files_residues(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                              totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp), atoms.ctypes.data_as(_lp),
                                              status.ctypes.data_as(_ip), dp_, nd, ingest._handle(classifier), C.byref(ct), err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_sweep_files_residues: " + err.value.decode())
    try:
        table = ResidueTable(ct)
    finally:
        L.freesasa_gpu_residue_table_free(C.byref(ct))
    return totals, cls, atoms, status, table


def _select_proto(L):
    L.freesasa_gpu_select_batch.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong),
                                            C.c_int, C.c_char_p, C.c_int]
    L.freesasa_gpu_sweep_files_select.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                  C.c_longlong, _dp, _dp, _lp, _ip, _ip, C.c_int, C.c_void_p, C.c_void_p,
                                                  _dp, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    return L


def select_batch(batch, selection, sasa, device=-1, bits=False):
    """freesasa_gpu_select_batch(): the areas of an ingest.Selection set on a loaded ingest.Batch, from per-atom areas on
    the host (e.g. calc_batch's) -> (areas[n_structs, S], counts[n_structs, S]) or, bits=True, (areas, counts,
    bits[n_atoms] uint64: bit k = selection k holds the atom).  The masks and the sums are made on the device."""
    L = _select_proto(lib())
    S, ns = len(selection), batch.n_structs
    sasa = _f64(sasa)
    if sasa.size != batch.n_atoms:
        raise ValueError("sasa needs one area per atom of the batch")
    areas, counts = np.zeros((ns, S)), np.zeros((ns, S), dtype=np.int64)
    words = np.zeros(batch.n_atoms, dtype=np.uint64) if bits else None
    err = C.create_string_buffer(512)
    cb = batch._as_c()
    ret = L.freesasa_gpu_select_batch(C.byref(cb), selection.handle, sasa.ctypes.data_as(_dp), areas.ctypes.data_as(_dp),
                                      counts.ctypes.data_as(C.POINTER(C.c_longlong)),
                                      words.ctypes.data_as(C.POINTER(C.c_ulonglong)) if bits else None, device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_select_batch: " + err.value.decode())
    return (areas, counts, words) if bits else (areas, counts)


def sweep_files_select(paths, selection, alg=LEE_RICHARDS, probe=1.4, resolution=20, ingest_options=0, n_threads=0, batch_atoms=0,
                       device=-1, devices=None, classifier=None):
    """freesasa_gpu_sweep_files_select(): sweep_files plus the areas of an ingest.Selection set for every file ->
    (totals[n], class_sums[n,3], n_atoms[n], status[n], areas[n, S], counts[n, S]); a file that failed to load has zeros.
    The per-atom areas stay on the device; with ingest.PARSE_ON_DEVICE the atoms' names, symbols and residues are built
    there too.  classifier: an ingest.Classifier in place of ProtOr."""
    from . import ingest
    L = _select_proto(lib())
    n, S = len(paths), len(selection)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    totals, atoms, status = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    cls = np.zeros((n, 3))
    areas, counts = np.zeros((n, S)), np.zeros((n, S), dtype=np.int64)
    err = C.create_string_buffer(512)
    keep, dp_, nd = _devs(devices, device)
    ret = L.freesasa_gpu_sweep_files_select(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                            totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp), atoms.ctypes.data_as(_lp),
                                            status.ctypes.data_as(_ip), dp_, nd, ingest._handle(classifier), selection.handle,
                                            areas.ctypes.data_as(_dp), counts.ctypes.data_as(C.POINTER(C.c_longlong)), err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_sweep_files_select: " + err.value.decode())
    return totals, cls, atoms, status, areas, counts


class GroupTableC(C.Structure):
    """freesasa_gpu_group_table (include/freesasa_gpu.h)."""
    _fields_ = [("n_files", C.c_int32), ("n_groups", C.c_int64), ("group_offsets", _lp), ("group_atoms", C.POINTER(C.c_int32)),
                ("areas", _dp), ("chain", C.POINTER(C.c_char))]


class GroupTable:
    """numpy copy of a freesasa_gpu_group_table: file k owns groups [group_offsets[k], group_offsets[k + 1]); areas columns are
    isolated, complex, buried; chain: the group's label (separate chains: the run's; a spec: the first the spec names)."""

    def __init__(self, ct):
        n, ng = int(ct.n_files), int(ct.n_groups)

        def arr(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            nbytes = count * np.dtype(dtype).itemsize    # (one copy: a view of the C block, copied before the block is freed)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_ubyte)), (nbytes,)).view(dtype).copy()
        self.n_files, self.n_groups = n, ng
        self.group_offsets = arr(ct.group_offsets, n + 1, np.int64)
        self.group_atoms = arr(ct.group_atoms, ng, np.int32)
        self.areas = arr(ct.areas, 3 * ng, np.float64).reshape(ng, 3)
        self.chain_raw = arr(ct.chain, ng, "S4")

    @property
    def chain(self):
        return [v.decode() for v in self.chain_raw.tolist()]

    def file(self, k):
        """the slice of file k's groups"""
        return slice(int(self.group_offsets[k]), int(self.group_offsets[k + 1]))


def _groups_proto(L):
    i32 = C.POINTER(C.c_int32)
    L.freesasa_gpu_sweep_files_groups.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                  C.c_longlong, _dp, _dp, _lp, _ip, _ip, C.c_int, C.c_void_p, C.c_char_p, C.c_int,
                                                  _ip, C.POINTER(GroupTableC), C.c_char_p, C.c_int]
    L.freesasa_gpu_group_table_free.argtypes = [C.POINTER(GroupTableC)]
    L.freesasa_gpu_group_table_free.restype = None
    L.freesasa_gpu_chain_group_ids.argtypes = [C.c_void_p, C.c_char_p, C.c_int, i32, i32, i32, C.c_int, C.c_char_p, C.c_int]
    return L


def _group_flags(long_syntax, separate_chains):
    from . import ingest
    return (ingest.GROUPS_LONG if long_syntax else 0) | (ingest.SEPARATE_CHAINS if separate_chains else 0)


def chain_group_ids(batch, spec=None, separate_chains=False, long_syntax=False, device=0):
    """freesasa_gpu_chain_group_ids(): Batch.chain_groups made by the device's kernel -> (group[n_atoms] int32,
    n_groups[n_structs], status[n_structs]).  A bad spec raises RuntimeError with freesasa_ingest_chain_groups's message."""
    L = _groups_proto(lib())
    group = np.empty(batch.n_atoms, dtype=np.int32)
    n_groups = np.empty(batch.n_structs, dtype=np.int32)
    status = np.empty(batch.n_structs, dtype=np.int32)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    cb = batch._as_c()
    ret = L.freesasa_gpu_chain_group_ids(C.byref(cb), spec.encode() if spec is not None else None, _group_flags(long_syntax, separate_chains),
                                         group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32), status.ctypes.data_as(i32), device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_chain_group_ids: " + err.value.decode())
    return group, n_groups, status


def sweep_files_groups(paths, spec=None, separate_chains=False, long_syntax=False, alg=LEE_RICHARDS, probe=1.4, resolution=20,
                       ingest_options=0, n_threads=0, batch_atoms=0, device=-1, devices=None, classifier=None):
    """freesasa_gpu_sweep_files_groups(): sweep_files plus the chain groups of every file (the reference's --chain-groups SPEC,
    long_syntax=True: --chain-groups-long, or --separate-chains) -> (totals[n], class_sums[n,3], n_atoms[n], status[n],
    group_status[n], table: a GroupTable).  The group ids are made on the device and stay there with the per-atom areas; a
    file whose group_status is not 0 (its load failed, or ingest.EGROUP: a chain the spec names is missing) owns no rows."""
    from . import ingest
    L = _groups_proto(lib())
    n = len(paths)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    totals, atoms, status = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    gstatus = np.zeros(n, dtype=np.int32)
    cls = np.zeros((n, 3))
    err = C.create_string_buffer(512)
    keep, dp_, nd = _devs(devices, device)
    ct = GroupTableC()
    ret = L.freesasa_gpu_sweep_files_groups(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                            totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp), atoms.ctypes.data_as(_lp),
                                            status.ctypes.data_as(_ip), dp_, nd, ingest._handle(classifier),
                                            spec.encode() if spec is not None else None, _group_flags(long_syntax, separate_chains),
                                            gstatus.ctypes.data_as(_ip), C.byref(ct), err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_sweep_files_groups: " + err.value.decode())
    try:
        table = GroupTable(ct)
    finally:
        L.freesasa_gpu_group_table_free(C.byref(ct))
    return totals, cls, atoms, status, gstatus, table


EIFACE_GROUPS = 100    # FREESASA_GPU_EIFACE_GROUPS: a file with more than 4096 groups owns no interface rows


class InterfaceTableC(C.Structure):
    """freesasa_gpu_interface_table (include/freesasa_gpu.h)."""
    _fields_ = [("n_files", C.c_int32), ("n_pairs", C.c_int64), ("n_res_rows", C.c_int64), ("pair_offsets", _lp),
                ("pair_groups", C.POINTER(C.c_int32)), ("pair_atoms", C.POINTER(C.c_int32)), ("pair_chain", C.POINTER(C.c_char)),
                ("pair_areas", _dp), ("pair_class_buried", _dp), ("res_offsets", _lp), ("res_index", C.POINTER(C.c_int32)),
                ("res_atoms", C.POINTER(C.c_int32)), ("res_areas", _dp), ("res_name", C.POINTER(C.c_char)),
                ("res_number", C.POINTER(C.c_char)), ("res_chain", C.POINTER(C.c_char))]


class InterfaceTable:
    """numpy copy of a freesasa_gpu_interface_table: file k owns pairs [pair_offsets[k], pair_offsets[k + 1]); per pair
    pair_groups[p] (rows of the file's block of the GroupTable), pair_atoms[p] (per side), pair_areas[p] (calc_interfaces'
    six columns), pair_class_buried[p, side] (apolar, polar, unknown) and the two groups' labels.  residues: the per-residue
    rows of side q = 2 p + side are [res_offsets[q], res_offsets[q + 1]): res_index (the residue's place among the residues of
    its file), res_atoms, res_areas (isolated, in the pair, buried) and the residue's labels, decoded like ResidueTable's."""

    def __init__(self, ct, residues):
        n, P, R = int(ct.n_files), int(ct.n_pairs), int(ct.n_res_rows)

        def arr(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            nbytes = count * np.dtype(dtype).itemsize    # (one copy: a view of the C block, copied before the block is freed)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_ubyte)), (nbytes,)).view(dtype).copy()
        self.n_files, self.n_pairs, self.n_res_rows, self.residues = n, P, R, bool(residues)
        self.pair_offsets = arr(ct.pair_offsets, n + 1, np.int64)
        self.pair_groups = arr(ct.pair_groups, 2 * P, np.int32).reshape(P, 2)
        self.pair_atoms = arr(ct.pair_atoms, 2 * P, np.int32).reshape(P, 2)
        self.pair_chain_raw = arr(ct.pair_chain, 2 * P, "S4").reshape(P, 2)
        self.pair_areas = arr(ct.pair_areas, 6 * P, np.float64).reshape(P, 6)
        self.pair_class_buried = arr(ct.pair_class_buried, 6 * P, np.float64).reshape(P, 2, 3)
        self.res_offsets = arr(ct.res_offsets, 2 * P + 1, np.int64) if residues else np.zeros(2 * P + 1, dtype=np.int64)
        self.res_index = arr(ct.res_index, R, np.int32)
        self.res_atoms = arr(ct.res_atoms, R, np.int32)
        self.res_areas = arr(ct.res_areas, 3 * R, np.float64).reshape(R, 3)
        self.res_name_raw = arr(ct.res_name, R, "S4")
        self.res_number_raw = arr(ct.res_number, R, "S6")
        self.res_chain_raw = arr(ct.res_chain, R, "S4")

    @property
    def pair_chain(self):
        return [(g.decode(), h.decode()) for g, h in self.pair_chain_raw.tolist()]

    @property
    def res_name(self):
        return [v.decode() for v in self.res_name_raw.tolist()]

    @property
    def res_number(self):
        return [v.decode() for v in self.res_number_raw.tolist()]

    @property
    def res_chain(self):
        return [v.decode() for v in self.res_chain_raw.tolist()]

    def file(self, k):
        """the slice of file k's pairs"""
        return slice(int(self.pair_offsets[k]), int(self.pair_offsets[k + 1]))

    def side_rows(self, p, side):
        """the slice of the residue rows of side 0 / 1 of pair p"""
        q = 2 * int(p) + int(side)
        return slice(int(self.res_offsets[q]), int(self.res_offsets[q + 1]))


def _ifsweep_proto(L):
    L.freesasa_gpu_sweep_files_interfaces.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                      C.c_longlong, _dp, _dp, _lp, _ip, _ip, C.c_int, C.c_void_p, C.c_char_p, C.c_int,
                                                      _ip, C.POINTER(GroupTableC), C.c_int, C.c_double, _ip,
                                                      C.POINTER(InterfaceTableC), C.c_char_p, C.c_int]
    L.freesasa_gpu_interface_table_free.argtypes = [C.POINTER(InterfaceTableC)]
    L.freesasa_gpu_interface_table_free.restype = None
    L.freesasa_gpu_group_table_free.argtypes = [C.POINTER(GroupTableC)]
    L.freesasa_gpu_group_table_free.restype = None
    return L


def sweep_files_interfaces(paths, spec=None, separate_chains=False, long_syntax=False, alg=LEE_RICHARDS, probe=1.4, resolution=20,
                           ingest_options=0, n_threads=0, batch_atoms=0, device=-1, devices=None, classifier=None,
                           residues=False, min_buried=0.0):
    """freesasa_gpu_sweep_files_interfaces(): sweep_files_groups plus the interfaces between the chain groups of every file ->
    (totals[n], class_sums[n,3], n_atoms[n], status[n], group_status[n], iface_status[n], groups: a GroupTable, interfaces:
    an InterfaceTable).  The first five and the group table are sweep_files_groups'.  iface_status: the group status, or
    EIFACE_GROUPS (more than 4096 groups), or 0; a file whose iface_status is not 0 owns no interface rows.  residues=True:
    the per-residue rows of every side whose buried area is > min_buried.  Nothing per atom leaves the device."""
    from . import ingest
    L = _ifsweep_proto(lib())
    n = len(paths)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    totals, atoms, status = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    gstatus, istatus = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    cls = np.zeros((n, 3))
    err = C.create_string_buffer(512)
    keep, dp_, nd = _devs(devices, device)
    gt, it = GroupTableC(), InterfaceTableC()
    ret = L.freesasa_gpu_sweep_files_interfaces(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                                totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp), atoms.ctypes.data_as(_lp),
                                                status.ctypes.data_as(_ip), dp_, nd, ingest._handle(classifier),
                                                spec.encode() if spec is not None else None, _group_flags(long_syntax, separate_chains),
                                                gstatus.ctypes.data_as(_ip), C.byref(gt), 1 if residues else 0, float(min_buried),
                                                istatus.ctypes.data_as(_ip), C.byref(it), err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_sweep_files_interfaces: " + err.value.decode())
    try:
        groups, table = GroupTable(gt), InterfaceTable(it, residues)
    finally:
        L.freesasa_gpu_group_table_free(C.byref(gt))
        L.freesasa_gpu_interface_table_free(C.byref(it))
    return totals, cls, atoms, status, gstatus, istatus, groups, table


def sweep_files_resumable(paths, done_path, alg=LEE_RICHARDS, probe=1.4, resolution=20, ingest_options=0, n_threads=0,
                          batch_atoms=0, max_new_batches=0, device=-1, devices=None, classifier=None):
    """freesasa_gpu_sweep_files_resumable(): like sweep_files with a done-list at done_path (+ done_path.bin):
    returns (complete, totals, class_sums, n_atoms, status); batches listed there are not computed again.  A done-list
    written under one classifier (or none) is refused by a call with another."""
    n = len(paths)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    totals, atoms, status = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    cls = np.zeros((n, 3))
    err = C.create_string_buffer(512)
    if classifier is not None:
        from . import ingest
        keep, dp_, nd = _devs(devices, device)
        ret = lib().freesasa_gpu_sweep_files_classified(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                                        totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp), atoms.ctypes.data_as(_lp),
                                                        status.ctypes.data_as(_ip), str(done_path).encode(), max_new_batches, dp_, nd,
                                                        ingest._handle(classifier), err, 512)
    elif devices is None:
        ret = lib().freesasa_gpu_sweep_files_resumable(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                                       totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp), atoms.ctypes.data_as(_lp),
                                                       status.ctypes.data_as(_ip), str(done_path).encode(), max_new_batches, device, err, 512)
    else:
        keep, dp_, nd = _devs(devices, device)
        ret = lib().freesasa_gpu_sweep_files_devices(arr, n, ingest_options, n_threads, alg, probe, resolution, batch_atoms,
                                                     totals.ctypes.data_as(_dp), cls.ctypes.data_as(_dp), atoms.ctypes.data_as(_lp),
                                                     status.ctypes.data_as(_ip), str(done_path).encode(), max_new_batches, dp_, nd, err, 512)
    if ret < 0:
        raise RuntimeError("freesasa_gpu_sweep_files_resumable: " + err.value.decode())
    return ret == 0, totals, cls, atoms, status


def sweep_cache(cache_path, alg=LEE_RICHARDS, probe=1.4, resolution=20, batch_atoms=0, class_sums=True, device=-1, devices=None,
                lanes_per_device=0):
    """freesasa_gpu_sweep_cache_devices(): the sweep of a binary cache file (ingest.Batch.save) -> (totals[n],
    class_sums[n,3] or None, n_atoms[n], status[n]): only coordinates, radii and classes are read, verified piece by
    piece, by a few lanes per device."""
    from . import ingest
    c = ingest.Cache(cache_path)
    n = c.n_structs
    c.close()
    totals, atoms, status = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    cls = np.zeros((n, 3)) if class_sums else None
    err = C.create_string_buffer(512)
    keep, dp_, nd = _devs(devices, device)
    ret = lib().freesasa_gpu_sweep_cache_devices(str(cache_path).encode(), alg, probe, resolution, batch_atoms, totals.ctypes.data_as(_dp),
                                                 cls.ctypes.data_as(_dp) if cls is not None else None, atoms.ctypes.data_as(_lp),
                                                 status.ctypes.data_as(_ip), n, dp_, nd, lanes_per_device, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_sweep_cache_devices: " + err.value.decode())
    return totals, cls, atoms, status


# run statistics (include/freesasa_gpu.h, FREESASA_GPU_STATS_*): the outputs in the order of a partial's columns
STATS_BITS = {"totals": 1, "atoms": 2, "isolated": 4, "classes": 8, "residues": 16, "selections": 32, "groups": 64}
# ... and the two more that the interface-residue entries alone accept (FREESASA_GPU_STATS_PAIRS, _PAIR_RESIDUES), behind the groups
PAIR_STATS_BITS = {"pairs": 128, "pair_residues": 256}


# The trajectory entries with a topology (include/freesasa_gpu.h): their argument lists from named pieces.  A piece is a list of
# (argument, ctype); _OUT is an output - the caller's array of doubles in the memory form, a result file's path in the file form -
# and "head" and "tail" are (the memory form's, the file form's).
_i32p, _llp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
_OUT = (_dp, C.c_char_p)
_TRAJ_PIECES = {
    "head": ([("frames", _dp), ("n_frames", C.c_int)],
             [("frames_path", C.c_char_p), ("frames_f32", C.c_int), ("header_bytes", C.c_longlong), ("n_frames", C.c_longlong)]),
    "topology": [("batch", C.c_void_p), ("structure", C.c_int), ("frame_atoms", C.c_int), ("atom_index", _i32p), ("selection", C.c_void_p)],
    "groups": [("group", _i32p), ("n_groups", C.c_int)],
    "parameters": [("alg", C.c_int), ("probe", C.c_double), ("resolution", C.c_int), ("frames_per_batch", C.c_int)],
    "outputs": [("totals", _OUT), ("sasa", _OUT), ("class_sums", _OUT), ("residues", _OUT), ("sel_area", _OUT), ("sel_atoms", _llp)],
    "group_outputs": [("group_areas", _OUT), ("isolated", _OUT)],
    "volumes": [("volumes", _OUT)],
    "masks": [("masks", (_u32p, C.c_char_p))],
    "tail": ([("devices", _ip), ("n_devices", C.c_int)],
             [("done_path", C.c_char_p), ("max_new_shards", C.c_longlong), ("devices", _ip), ("n_devices", C.c_int), ("frames_total", _llp)]),
    "statistics": [("stats", C.c_int), ("stats_to", _OUT), ("partials_to", _OUT)],
    "pairs": [("pairs", _i32p), ("n_pairs", C.c_int), ("pair_areas", _OUT)],
    "pair_residues": [("min_buried", C.c_double), ("pair_residues", _OUT)],
    "err": [("err", C.c_char_p), ("err_len", C.c_int)],
}
# entry -> its pieces: freesasa_gpu_trajectory_<entry> has them in the memory form, freesasa_gpu_trajectory_file_<entry> in the file form
_GROUPS = "head topology groups parameters outputs group_outputs tail"
_TRAJ_ENTRIES = {
    "topology": "head topology parameters outputs tail err",
    "volume": "head topology parameters outputs volumes tail err",
    "masks": "head topology parameters outputs masks tail err",
    "groups": _GROUPS + " err",
    "groups_stats": _GROUPS + " statistics err",
    "interfaces": _GROUPS + " statistics pairs err",
    "interface_residues": _GROUPS + " statistics pairs pair_residues err",
}
# ... and the file entries among periodic images, which have their siblings' arguments
_TRAJ_PERIODIC = {"file_groups_periodic": "groups_stats", "file_interfaces_periodic": "interfaces", "file_interface_residues_periodic": "interface_residues"}


def _traj_entry_args(name):
    """[(argument, ctype)] of freesasa_gpu_trajectory_<name>, err and err_len included"""
    form = int(name.startswith("file_"))
    pieces = _TRAJ_ENTRIES[_TRAJ_PERIODIC.get(name) or name[5 * form:]].split()
    args = [a for p in pieces for a in (_TRAJ_PIECES[p][form] if p in ("head", "tail") else _TRAJ_PIECES[p])]
    return [(arg, t[form] if isinstance(t, tuple) else t) for arg, t in args]


def _traj_protos(L):
    for name in list(_TRAJ_ENTRIES) + ["file_" + k for k in _TRAJ_ENTRIES] + list(_TRAJ_PERIODIC):
        getattr(L, "freesasa_gpu_trajectory_" + name).argtypes = [t for _, t in _traj_entry_args(name)]
    return L


def _traj_call(name, batch, selection, devices, device, **values):
    """Calls freesasa_gpu_trajectory_<name> with the arguments its pieces name, taken from `values` - which may hold more: the
    arguments of the entry's siblings; arrays go as they are, paths as str() of what they are - and returns its code; a refusal
    is a RuntimeError that begins with the entry's name."""
    cb = batch._as_c()
    keep, dp_, nd = _devs(devices, device)
    values.update(batch=C.byref(cb), selection=selection.handle if selection is not None else None, devices=dp_, n_devices=nd)
    args = []
    for arg, ctype in _traj_entry_args(name)[:-2]:
        v = values[arg]
        if isinstance(v, np.ndarray):
            v = v.ctypes.data_as(ctype)
        elif ctype is C.c_char_p and v is not None:
            v = str(v).encode()
        args.append(v)
    err = C.create_string_buffer(512)
    ret = getattr(_traj_protos(lib()), "freesasa_gpu_trajectory_" + name)(*args, err, 512)
    if ret < 0:
        raise RuntimeError("freesasa_gpu_trajectory_" + name + ": " + err.value.decode())
    return ret


def _stats_proto(L):
    L.freesasa_gpu_traj_stats_width.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _llp]
    L.freesasa_gpu_traj_stats_width.restype = C.c_longlong
    L.freesasa_gpu_traj_stats_merge.argtypes = [_dp, _llp, C.c_longlong, C.c_longlong, _dp, _llp]
    L.freesasa_gpu_trajectory_stats.argtypes = [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int,
                                                C.c_int, _dp, _dp, C.c_char_p, C.c_int]
    L.freesasa_gpu_trajectory_file_stats.argtypes = [C.c_char_p, C.c_int, C.c_longlong, _dp, C.c_int, C.c_longlong, C.c_int, C.c_double,
                                                     C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_longlong, _ip, C.c_int,
                                                     _llp, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.freesasa_gpu_trajectory_interface_segments.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int, _i32p, C.c_int, C.c_longlong, _llp, _llp, _i32p,
                                                             _i32p, C.c_char_p, C.c_int]
    L.freesasa_gpu_traj_stats_width_pairs.argtypes = [C.c_int] + 6 * [C.c_longlong] + [_llp]
    L.freesasa_gpu_traj_stats_width_pairs.restype = C.c_longlong
    return _traj_protos(L)


def stats_word(stats, pairs=False):
    """the FREESASA_GPU_STATS_* word of stats=("atoms", "residues", ...); None or () is 0.  pairs: the names of PAIR_STATS_BITS
    are known too (the interface-residue runs)"""
    word, known = 0, dict(STATS_BITS, **PAIR_STATS_BITS) if pairs else STATS_BITS
    for name in ([stats] if isinstance(stats, str) else stats or ()):
        if name not in known:
            raise ValueError(f"unknown statistics output {name!r}: one of {', '.join(known)}")
        word |= known[name]
    return word


def traj_stats_width(stats, n_atoms, n_res=0, n_sel=0, n_groups=0):
    """(W, first column of every output [7], -1: not asked for) of a statistics word or tuple of names"""
    word = stats if isinstance(stats, int) else stats_word(stats)
    first = np.zeros(7, dtype=np.int64)
    W = _stats_proto(lib()).freesasa_gpu_traj_stats_width(word, n_atoms, n_res, n_sel, n_groups, first.ctypes.data_as(C.POINTER(C.c_longlong)))
    if W < 0:
        raise ValueError("bad statistics word or counts")
    return int(W), first


def traj_stats_width_pairs(stats, n_atoms, n_res=0, n_sel=0, n_groups=0, n_pairs=0, n_segments=0):
    """(W, first column of every output [9], -1: not asked for) of a statistics word or tuple of names of an interface-residue
    run: the seven of traj_stats_width, then the pairs [6 K] and the interface residues [4 S]"""
    word = stats if isinstance(stats, int) else stats_word(stats, pairs=True)
    first = np.zeros(9, dtype=np.int64)
    W = _stats_proto(lib()).freesasa_gpu_traj_stats_width_pairs(word, n_atoms, n_res, n_sel, n_groups, n_pairs, n_segments,
                                                                first.ctypes.data_as(C.POINTER(C.c_longlong)))
    if W < 0:
        raise ValueError("bad statistics word or counts")
    return int(W), first


class RunStats(dict):
    """Run statistics of a trajectory: a dict of the outputs asked for, each [4, ...] - mean, std (population), min, max over
    the frames: totals [4], atoms [4, n], isolated [4, n], classes [4, 3], residues [4, R, 6], selections [4, S], groups
    [4, G, 3].  raw: the same as the library delivers it, [4, W]; partials [n_shards, 4, W] (rows mean, M2, min, max of every
    shard) and frames [n_shards] where they were asked for, else None: traj_stats_merge(partials, frames, a, b) gives the
    statistics of shards [a, b) - block averages."""

    def __init__(self, raw, stats, n_atoms, n_res=0, n_sel=0, n_groups=0, partials=None, frames=None, n_pairs=None, n_segments=0):
        """n_pairs not None: the statistics of an interface-residue run, which may hold pairs [4, K, 6] and pair_residues [4, S, 4]
        (pair_residues[0, :, 3] is the occupancy of every segment)"""
        if n_pairs is None:
            W, first = traj_stats_width(stats, n_atoms, n_res, n_sel, n_groups)
        else:
            W, first = traj_stats_width_pairs(stats, n_atoms, n_res, n_sel, n_groups, n_pairs, n_segments)
        raw = np.asarray(raw, dtype=np.float64).reshape(4, W)
        shapes = [(), (n_atoms,), (n_atoms,), (3,), (n_res, 6), (n_sel,), (n_groups, 3), (n_pairs or 0, 6), (n_segments, 4)]
        for name, at, shape in zip(list(STATS_BITS) + list(PAIR_STATS_BITS), first, shapes):
            if at >= 0:
                self[name] = raw[:, at:at + int(np.prod(shape, dtype=np.int64))].reshape((4,) + shape)
        self.raw, self.partials, self.frames = raw, partials, frames


def traj_stats_merge(parts, frames, first=0, last=None):
    """freesasa_gpu_traj_stats_merge(): the statistics [4, W] (mean, std, min, max) of the consecutive shards [first, last) of
    parts [n_shards, 4, W] (a partials file or RunStats.partials) with frames [n_shards] frames each."""
    parts = np.ascontiguousarray(parts, dtype=np.float64)
    frames = np.ascontiguousarray(frames, dtype=np.int64)
    if parts.ndim != 3 or parts.shape[1] != 4 or frames.shape != (parts.shape[0],):
        raise ValueError("parts must be [n_shards, 4, W] and frames [n_shards]")
    last = parts.shape[0] if last is None else last
    if not 0 <= first < last <= parts.shape[0]:
        raise ValueError("bad range of shards")
    cut, nf = np.ascontiguousarray(parts[first:last]), np.ascontiguousarray(frames[first:last])
    out = np.empty((4, parts.shape[2]))
    if _stats_proto(lib()).freesasa_gpu_traj_stats_merge(cut.ctypes.data_as(_dp), nf.ctypes.data_as(C.POINTER(C.c_longlong)), cut.shape[0],
                                                         cut.shape[2], out.ctypes.data_as(_dp), None):
        raise ValueError("freesasa_gpu_traj_stats_merge: zero parts, a part without frames or a width below 1")
    return out


def traj_stats_read(path, stats, n_atoms, n_res=0, n_sel=0, n_groups=0, partials_path=None, frames=None, n_pairs=None, n_segments=0):
    """The statistics file of a file run (raw fp64 [4, W]) as a RunStats; with partials_path and frames [n_shards] (the frames
    of every shard: frames_per_batch each, the last one the rest) its partials too.  n_pairs, n_segments: of an interface-residue
    run (RunStats)."""
    if n_pairs is None:
        W, _ = traj_stats_width(stats, n_atoms, n_res, n_sel, n_groups)
    else:
        W, _ = traj_stats_width_pairs(stats, n_atoms, n_res, n_sel, n_groups, n_pairs, n_segments)
    raw = np.fromfile(path, dtype=np.float64)
    if raw.size != 4 * W:
        raise ValueError("the statistics file does not have 4 x W values")
    parts = None if partials_path is None else np.fromfile(partials_path, dtype=np.float64).reshape(-1, 4, W)
    return RunStats(raw, stats, n_atoms, n_res, n_sel, n_groups, parts, None if frames is None else np.asarray(frames, dtype=np.int64),
                    n_pairs=n_pairs, n_segments=n_segments)


def _shard_frames(n_frames, frames_per_batch):
    """frames of every shard of a run whose frames_per_batch was given; None when the library chooses it"""
    if frames_per_batch <= 0:
        return None
    fpb = min(int(frames_per_batch), n_frames)
    return np.array([min(fpb, n_frames - f0) for f0 in range(0, n_frames, fpb)], dtype=np.int64)


def trajectory(xyz_frames, radii, alg=LEE_RICHARDS, probe=1.4, resolution=20, frames_per_batch=0,
               per_atom=True, device=-1, devices=None, stats=None):
    """freesasa_gpu_trajectory() on host arrays: xyz_frames [n_frames, n_atoms, 3] -> (totals
    [n_frames], per-atom [n_frames, n_atoms] or None).
    stats=("totals", "atoms"): freesasa_gpu_trajectory_stats() - a third element, the RunStats of those outputs over the run,
    reduced on the device (with per_atom=False the per-atom areas never leave it); its partials come with a frames_per_batch > 0."""
    if stats:
        return _trajectory_stats(xyz_frames, radii, alg, probe, resolution, frames_per_batch, per_atom, device, devices, stats)
    xyz_frames = np.ascontiguousarray(xyz_frames, dtype=np.float64)
    radii = _f64(radii)
    n_frames, n_atoms = xyz_frames.shape[0], radii.size
    assert xyz_frames.size == n_frames * n_atoms * 3
    totals = np.empty(n_frames)
    sasa = np.empty((n_frames, n_atoms)) if per_atom else None
    err = C.create_string_buffer(512)
    if devices is None:
        ret = lib().freesasa_gpu_trajectory(xyz_frames.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), n_atoms,
                                            n_frames, alg, probe, resolution, frames_per_batch,
                                            totals.ctypes.data_as(_dp),
                                            sasa.ctypes.data_as(_dp) if sasa is not None else None,
                                            device, err, 512)
    else:
        keep, dp_, nd = _devs(devices, device)
        ret = lib().freesasa_gpu_trajectory_devices(xyz_frames.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), n_atoms,
                                                    n_frames, alg, probe, resolution, frames_per_batch, totals.ctypes.data_as(_dp),
                                                    sasa.ctypes.data_as(_dp) if sasa is not None else None, dp_, nd, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_trajectory: " + err.value.decode())
    return totals, sasa


def _trajectory_stats(xyz_frames, radii, alg, probe, resolution, frames_per_batch, per_atom, device, devices, stats):
    L = _stats_proto(lib())
    xyz_frames = np.ascontiguousarray(xyz_frames, dtype=np.float64)
    radii = _f64(radii)
    n_frames, n_atoms = xyz_frames.shape[0], radii.size
    assert xyz_frames.size == n_frames * n_atoms * 3
    word = stats_word(stats)
    W, _ = traj_stats_width(word, n_atoms)
    totals = np.empty(n_frames)
    sasa = np.empty((n_frames, n_atoms)) if per_atom else None
    raw = np.empty((4, W))
    nf = _shard_frames(n_frames, frames_per_batch)
    parts = None if nf is None else np.empty((nf.size, 4, W))
    err = C.create_string_buffer(512)
    keep, dp_, nd = _devs(devices, device)
    ret = L.freesasa_gpu_trajectory_stats(xyz_frames.ctypes.data_as(_dp), radii.ctypes.data_as(_dp), n_atoms, n_frames, alg, probe, resolution,
                                          frames_per_batch, totals.ctypes.data_as(_dp), sasa.ctypes.data_as(_dp) if sasa is not None else None,
                                          dp_, nd, word, raw.ctypes.data_as(_dp), parts.ctypes.data_as(_dp) if parts is not None else None, err, 512)
    if ret:
        raise RuntimeError("freesasa_gpu_trajectory_stats: " + err.value.decode())
    return totals, sasa, RunStats(raw, word, n_atoms, partials=parts, frames=nf)


FRAMES_F32, FRAMES_OUT_F32, FRAMES_DCD, FRAMES_PBC, FRAMES_TRICLINIC, FRAMES_NETCDF, FRAMES_XTC, FRAMES_TRR = 1, 2, 4, 8, 16, 32, 64, 128   # the bits of frames_f32 (include/freesasa_gpu.h)


class DcdInfoC(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("n_frames", C.c_int64), ("n_frames_header", C.c_int64), ("first_frame", C.c_int64),
                ("frame_bytes", C.c_int64), ("x_off", C.c_int32), ("plane_bytes", C.c_int32), ("big_endian", C.c_int32),
                ("has_cell", C.c_int32), ("has_4d", C.c_int32), ("charmm_version", C.c_int32)]


class DcdInfo:
    """What dcd_info() returns: the fields of freesasa_gpu_dcd_info (include/freesasa_gpu.h) - n_atoms, n_frames (whole
    frames by file size), n_frames_header (as the header claims), first_frame, frame_bytes, x_off, plane_bytes (bytes), and
    the flags big_endian, has_cell, has_4d as bools, charmm_version."""

    def __init__(self, c):
        for name, _ in DcdInfoC._fields_:
            v = int(getattr(c, name))
            setattr(self, name, bool(v) if name in ("big_endian", "has_cell", "has_4d") else v)

    def __repr__(self):
        return "DcdInfo(" + ", ".join(f"{name}={getattr(self, name)}" for name, _ in DcdInfoC._fields_) + ")"


def dcd_info(path):
    """freesasa_gpu_dcd_info_read(): the header of a DCD trajectory -> DcdInfo; ValueError with the library's message for
    a file that is no DCD, is damaged, or is a DCD the drivers do not read (fixed atoms, 64-bit record markers)."""
    L = lib()
    L.freesasa_gpu_dcd_info_read.argtypes = [C.c_char_p, C.POINTER(DcdInfoC), C.c_char_p, C.c_int]
    c = DcdInfoC()
    err = C.create_string_buffer(512)
    if L.freesasa_gpu_dcd_info_read(str(path).encode(), C.byref(c), err, 512):
        raise ValueError("freesasa_gpu_dcd_info_read: " + err.value.decode())
    return DcdInfo(c)


class NcInfoC(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("n_frames", C.c_int64), ("n_frames_header", C.c_int64), ("first_record", C.c_int64),
                ("record_bytes", C.c_int64), ("coord_off", C.c_int64), ("lengths_off", C.c_int64), ("angles_off", C.c_int64),
                ("version", C.c_int32), ("has_cell", C.c_int32), ("has_time", C.c_int32), ("has_velocities", C.c_int32)]


class NcInfo:
    """What nc_info() returns: the fields of freesasa_gpu_nc_info (include/freesasa_gpu.h) - n_atoms, n_frames (whole records
    by file size), n_frames_header (numrecs as the header claims, -1: streaming), first_record, record_bytes, coord_off,
    lengths_off, angles_off (bytes; -1 without a cell), version, and the flags has_cell, has_time, has_velocities as bools."""

    def __init__(self, c):
        for name, _ in NcInfoC._fields_:
            v = int(getattr(c, name))
            setattr(self, name, bool(v) if name.startswith("has_") else v)

    def __repr__(self):
        return "NcInfo(" + ", ".join(f"{name}={getattr(self, name)}" for name, _ in NcInfoC._fields_) + ")"


def nc_info(path):
    """freesasa_gpu_nc_info_read(): the header of an AMBER NetCDF trajectory -> NcInfo; ValueError with the library's message
    for a file that is no NetCDF classic file, is damaged, or is one the drivers do not read (NetCDF-4 / HDF5, CDF-5, a restart
    file, a scale_factor other than 1)."""
    L = lib()
    L.freesasa_gpu_nc_info_read.argtypes = [C.c_char_p, C.POINTER(NcInfoC), C.c_char_p, C.c_int]
    c = NcInfoC()
    err = C.create_string_buffer(512)
    if L.freesasa_gpu_nc_info_read(str(path).encode(), C.byref(c), err, 512):
        raise ValueError("freesasa_gpu_nc_info_read: " + err.value.decode())
    return NcInfo(c)


class XtcInfoC(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("n_frames", C.c_int64), ("max_frame_bytes", C.c_int64), ("precision", C.c_float), ("has_box", C.c_int32)]


class XtcInfo:
    """What xtc_info() returns: the fields of freesasa_gpu_xtc_info (include/freesasa_gpu.h) - n_atoms, n_frames (by one pass
    over the frames' headers), max_frame_bytes (the longest frame, header and padding included), precision (frame 0's) and
    has_box (frame 0's box has a non-zero element) as a bool."""

    def __init__(self, c):
        self.n_atoms, self.n_frames, self.max_frame_bytes = int(c.n_atoms), int(c.n_frames), int(c.max_frame_bytes)
        self.precision, self.has_box = float(c.precision), bool(c.has_box)

    def __repr__(self):
        return "XtcInfo(" + ", ".join(f"{name}={getattr(self, name)}" for name, _ in XtcInfoC._fields_) + ")"


def xtc_info(path):
    """freesasa_gpu_xtc_info_read(): one pass over the headers of a GROMACS XTC trajectory -> XtcInfo; ValueError with the
    library's message, which names the frame, for a file that is no XTC file, is damaged, or is one the drivers do not read
    (magic 2023, frames of 9 atoms or fewer)."""
    L = lib()
    L.freesasa_gpu_xtc_info_read.argtypes = [C.c_char_p, C.POINTER(XtcInfoC), C.c_char_p, C.c_int]
    c = XtcInfoC()
    err = C.create_string_buffer(512)
    if L.freesasa_gpu_xtc_info_read(str(path).encode(), C.byref(c), err, 512):
        raise ValueError("freesasa_gpu_xtc_info_read: " + err.value.decode())
    return XtcInfo(c)


class TrrInfoC(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("n_frames", C.c_int64), ("n_records", C.c_int64), ("max_frame_bytes", C.c_int64),
                ("real_bytes", C.c_int32), ("has_box", C.c_int32), ("has_velocities", C.c_int32), ("has_forces", C.c_int32)]


class TrrInfo:
    """What trr_info() returns: the fields of freesasa_gpu_trr_info (include/freesasa_gpu.h) - n_atoms, n_frames (the records
    WITH coordinates, by one pass over the records' headers), n_records (all records), max_frame_bytes (the longest stretch from
    one frame's first byte to the next frame's), real_bytes (4: single, 8: double precision) and the flags has_box (the first
    frame has a box with a non-zero element), has_velocities, has_forces (some record has them) as bools."""

    def __init__(self, c):
        for name, _ in TrrInfoC._fields_:
            v = int(getattr(c, name))
            setattr(self, name, bool(v) if name.startswith("has_") else v)

    def __repr__(self):
        return "TrrInfo(" + ", ".join(f"{name}={getattr(self, name)}" for name, _ in TrrInfoC._fields_) + ")"


def trr_info(path):
    """freesasa_gpu_trr_info_read(): one pass over the headers of a GROMACS TRR trajectory -> TrrInfo; ValueError with the
    library's message, which names the record, for a file that is no TRR file, is damaged, or is one the drivers do not read
    (records that change atom count or precision, no record with coordinates)."""
    L = lib()
    L.freesasa_gpu_trr_info_read.argtypes = [C.c_char_p, C.POINTER(TrrInfoC), C.c_char_p, C.c_int]
    c = TrrInfoC()
    err = C.create_string_buffer(512)
    if L.freesasa_gpu_trr_info_read(str(path).encode(), C.byref(c), err, 512):
        raise ValueError("freesasa_gpu_trr_info_read: " + err.value.decode())
    return TrrInfo(c)


def _frames_bits(f32, out_f32, dcd, header_bytes, pbc=False, triclinic=False, netcdf=False, xtc=False, trr=False):
    if dcd and (f32 or header_bytes):
        raise ValueError("dcd=True excludes f32=True and a non-zero header_bytes: a DCD file says for itself where its frames are")
    if netcdf and (dcd or f32 or header_bytes):
        raise ValueError("netcdf=True excludes dcd=True, f32=True and a non-zero header_bytes: an AMBER NetCDF file says for itself where its frames are")
    if xtc and (dcd or netcdf or f32 or header_bytes):
        raise ValueError("xtc=True excludes dcd=True, netcdf=True, f32=True and a non-zero header_bytes: an XTC file's frames are found by their headers")
    if trr and (dcd or netcdf or xtc or f32 or header_bytes):
        raise ValueError("trr=True excludes dcd=True, netcdf=True, xtc=True, f32=True and a non-zero header_bytes: a TRR file's frames are found by "
                         "their headers, which say their precision")
    return (FRAMES_F32 if f32 else 0) | (FRAMES_OUT_F32 if out_f32 else 0) | (FRAMES_DCD if dcd else 0) | (FRAMES_PBC if pbc else 0) | \
        (FRAMES_TRICLINIC if triclinic else 0) | (FRAMES_NETCDF if netcdf else 0) | (FRAMES_XTC if xtc else 0) | (FRAMES_TRR if trr else 0)


def trajectory_file(frames_path, radii, totals_path, sasa_path=None, done_path=None, f32=False, header_bytes=0,
                    n_frames=0, alg=LEE_RICHARDS, probe=1.4, resolution=20, frames_per_batch=0, max_new_shards=0, device=-1,
                    devices=None, out_f32=False, dcd=False, pbc=False, triclinic=False, netcdf=False, xtc=False,
                    stats=None, stats_path=None, partials_path=None, trr=False):
    """freesasa_gpu_trajectory_file(): raw frame file -> totals file (+ per-atom file), resumable through the
    done-list at done_path.  Returns (complete, n_frames): complete is False when max_new_shards stopped the run.
    f32: the frames are floats (an input format); out_f32: the per-atom file holds floats (an output format);
    dcd: frames_path is a DCD trajectory whose NATOM is len(radii) (no f32, no header_bytes with it);
    pbc: (with dcd) every frame among the periodic images its unit-cell record implies, as calc_periodic defines them;
    triclinic: (with dcd and pbc) the record decoded by cell_from_dcd, the frame as calc_periodic_triclinic defines it;
    netcdf: frames_path is an AMBER NetCDF trajectory whose atom count is len(radii) (no dcd, no f32, no header_bytes with
    it); pbc and triclinic go with it as with dcd: the cell is the frame's cell_lengths and cell_angles (cell_from_lengths_angles);
    xtc: frames_path is a GROMACS XTC trajectory whose atom count is len(radii) (no dcd, no netcdf, no f32, no header_bytes with
    it), decoded on the device; pbc and triclinic go with it as with dcd: the cell is the frame's box, nm * 10.
    trr: frames_path is a GROMACS TRR trajectory, single or double precision, whose atom count is len(radii) (no dcd, no netcdf,
    no xtc, no f32, no header_bytes with it); records without coordinates are no frames of the run; results are those of a raw
    fp64 file of float64(x_nm) * 10; pbc and triclinic go with it as with xtc.
    stats=("totals", "atoms") with stats_path and partials_path: freesasa_gpu_trajectory_file_stats() - the run statistics of those
    outputs; the shards' partials go to partials_path as they finish, the call that finds the run complete writes stats_path
    (traj_stats_read reads it).  With out_f32 the statistics are still those of the fp64 areas."""
    radii = _f64(radii)
    f32 = _frames_bits(f32, out_f32, dcd, header_bytes, pbc, triclinic, netcdf, xtc, trr)
    err = C.create_string_buffer(512)
    total = C.c_longlong(0)
    enc = lambda p: None if p is None else str(p).encode()
    if stats:
        keep, dp_, nd = _devs(devices, device)
        ret = _stats_proto(lib()).freesasa_gpu_trajectory_file_stats(
            enc(frames_path), f32, header_bytes, radii.ctypes.data_as(_dp), radii.size, n_frames, alg, probe, resolution, frames_per_batch,
            enc(totals_path), enc(sasa_path), enc(done_path), max_new_shards, dp_, nd, C.byref(total), stats_word(stats), enc(stats_path),
            enc(partials_path), err, 512)
        if ret < 0:
            raise RuntimeError("freesasa_gpu_trajectory_file_stats: " + err.value.decode())
        return ret == 0, int(total.value)
    if devices is None:
        ret = lib().freesasa_gpu_trajectory_file(enc(frames_path), f32, header_bytes, radii.ctypes.data_as(_dp), radii.size,
                                                 n_frames, alg, probe, resolution, frames_per_batch, enc(totals_path), enc(sasa_path),
                                                 enc(done_path), max_new_shards, device, C.byref(total), err, 512)
    else:
        keep, dp_, nd = _devs(devices, device)
        ret = lib().freesasa_gpu_trajectory_file_devices(enc(frames_path), f32, header_bytes, radii.ctypes.data_as(_dp), radii.size,
                                                         n_frames, alg, probe, resolution, frames_per_batch, enc(totals_path), enc(sasa_path),
                                                         enc(done_path), max_new_shards, dp_, nd, C.byref(total), err, 512)
    if ret < 0:
        raise RuntimeError("freesasa_gpu_trajectory_file: " + err.value.decode())
    return ret == 0, int(total.value)


def _topology_proto(L):
    return _traj_protos(L)


class TopologyResult:
    """What trajectory_topology() returns: totals [F], class_sums [F, 3] (apolar, polar, unknown), residues [F, R, 6] (total,
    main chain, side chain, polar, apolar, unknown), selection_areas [F, S] and selection_atoms [S] (None without a
    selection set), sasa [F, n] or None, and res_ref [R]: rows of ingest.residue_reference_table() - the relative areas are
    100 * residues[..., :5] / table[res_ref] where res_ref >= 0.  With chain groups (None without): group_areas [F, G, 3]
    (isolated, complex, buried per frame and group), group_atoms [G], and with per_atom isolated [F, n], every atom's area in
    its group taken on its own (isolated - sasa: what the atom buries in the complex).  stats: the RunStats of the outputs
    named in stats=, None without.  With per_frame=False only totals (and selection_atoms) are delivered per frame: the others
    are None.  volumes [F]: with volumes=True, the volume every frame's solvent-accessible surface encloses; None without.
    masks [F, n, 4] uint32: with masks=True, every atom's exposure mask in every frame (calc_masks); None without.
    pair_areas [F, K, 6] and pair_groups [K, 2]: with interface_pairs=, per frame and pair (g, h) of groups (iso_g, iso_h,
    in_pair_g, in_pair_h, buried_g, buried_h) as calc_interfaces orders them; None without.
    With interface_residues=True: pair_residues [F, S, 4] - per frame and segment (iso_res, in_pair_res, buried_res, in_interface) -
    and the segments, which are the same for every frame: pair_res_offsets [2 K + 1] (side q of pair k owns the segments
    side_segments(k, q)), pair_res_index [S] (the residue within the structure) and pair_res_atoms [S]; None without."""

    def __init__(self, totals, class_sums, residues, selection_areas, selection_atoms, sasa, res_ref, group_areas=None,
                 group_atoms=None, isolated=None, stats=None, volumes=None, masks=None, pair_areas=None, pair_groups=None,
                 pair_residues=None, pair_res_offsets=None, pair_res_index=None, pair_res_atoms=None):
        self.stats, self.volumes, self.masks = stats, volumes, masks
        self.pair_areas, self.pair_groups = pair_areas, pair_groups
        self.pair_residues, self.pair_res_offsets = pair_residues, pair_res_offsets
        self.pair_res_index, self.pair_res_atoms = pair_res_index, pair_res_atoms
        self.totals, self.class_sums, self.residues = totals, class_sums, residues
        self.selection_areas, self.selection_atoms, self.sasa, self.res_ref = selection_areas, selection_atoms, sasa, res_ref
        self.group_areas, self.group_atoms, self.isolated = group_areas, group_atoms, isolated

    def side_segments(self, k, side):
        """the segments of side `side` (0: g, 1: h) of pair k, as a slice of the second axis of pair_residues"""
        j = 2 * int(k) + int(side)
        return slice(int(self.pair_res_offsets[j]), int(self.pair_res_offsets[j + 1]))


def _topology_args(batch, structure, atom_index, frame_atoms):
    """(n, R, res_ref, index array or None, frame_atoms) of a topology; the library checks them"""
    ok = 0 <= structure < batch.n_structs
    n = int(batch.offsets[structure + 1] - batch.offsets[structure]) if ok else 0
    r0, r1 = (int(batch.res_offsets[structure]), int(batch.res_offsets[structure + 1])) if ok else (0, 0)
    idx = None if atom_index is None else np.ascontiguousarray(atom_index, dtype=np.int32)
    if idx is not None and idx.size != n and ok:
        raise ValueError("atom_index needs one entry per atom of the structure")
    return n, r1 - r0, batch.res_ref[r0:r1].copy(), idx, int(n if frame_atoms is None else frame_atoms)


def _topology_groups(batch, structure, n, chain_groups, separate_chains, long, group, n_groups):
    """(ids [n] int32, G, atoms per group [G]) of the topology's structure, or (None, 0, None): from a spec / separate chains
    through Batch.chain_groups (the structure's slice of the batch's ids), or from ids given directly; the library checks
    the ids"""
    if chain_groups is not None or separate_chains:
        if group is not None:
            raise ValueError("give chain_groups / separate_chains or group, not both")
        from . import ingest
        ids, ng, status = batch.chain_groups(chain_groups, long=long, separate_chains=separate_chains)
        if not 0 <= structure < batch.n_structs:
            raise ValueError("structure out of range")
        if status[structure] == ingest.EGROUP:
            raise ValueError("the topology's structure lacks a chain the groups name (EGROUP)")
        group, n_groups = ids[batch.offsets[structure]:batch.offsets[structure + 1]], int(ng[structure])
    if group is None:
        if n_groups is not None:
            raise ValueError("n_groups needs group")
        return None, 0, None
    group = np.ascontiguousarray(group, dtype=np.int32)
    if n_groups is None:
        raise ValueError("group needs n_groups")
    if group.size != n:
        raise ValueError("group needs one id per atom of the structure")
    G = int(n_groups)
    return group, G, np.bincount(group[(group >= 0) & (group < G)], minlength=max(G, 0)).astype(np.int64)


def _interface_pairs(interface_pairs, ids, G):
    """pairs [K, 2] int32 of interface_pairs= ("all": every g < h, g-major - the order of calc_interfaces' table), or None; the
    library checks the pairs"""
    if interface_pairs is None:
        return None
    if ids is None:
        raise ValueError("interface_pairs needs chain groups: chain_groups=, separate_chains=True or group= with n_groups=")
    if isinstance(interface_pairs, str):
        if interface_pairs != "all":
            raise ValueError('interface_pairs is None, "all" or a list of (g, h)')
        return np.array([(g, h) for g in range(G) for h in range(g + 1, G)], dtype=np.int32).reshape(-1, 2)
    pairs = np.ascontiguousarray(interface_pairs, dtype=np.int32)
    if pairs.size and (pairs.ndim != 2 or pairs.shape[1] != 2):
        raise ValueError("interface_pairs must be [K, 2]: one (g, h) per pair")
    return pairs.reshape(-1, 2)


def traj_pair_segments(batch, group, n_groups, pairs, structure=0):
    """freesasa_gpu_trajectory_interface_segments(): the segments of an interface-residue run over structure `structure` of the
    batch with these group ids and pairs, without a device -> (offsets [2 K + 1], residue [S], atoms [S])"""
    L = _stats_proto(lib())
    group = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    pairs = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    K = 0 if pairs is None else pairs.shape[0]
    cb = batch._as_c()
    i32 = C.POINTER(C.c_int32)
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    S, err = C.c_longlong(0), C.create_string_buffer(512)
    args = (C.byref(cb), structure, opt(group, i32), n_groups, opt(pairs, i32), K)
    if L.freesasa_gpu_trajectory_interface_segments(*args, 1 << 62, C.byref(S), None, None, None, err, 512):
        raise RuntimeError("freesasa_gpu_trajectory_interface_segments: " + err.value.decode())
    offs, res, atoms = np.zeros(2 * K + 1, dtype=np.int64), np.zeros(S.value, dtype=np.int32), np.zeros(S.value, dtype=np.int32)
    if L.freesasa_gpu_trajectory_interface_segments(*args, S.value, C.byref(S), offs.ctypes.data_as(C.POINTER(C.c_longlong)), opt(res, i32),
                                                    opt(atoms, i32), err, 512):
        raise RuntimeError("freesasa_gpu_trajectory_interface_segments: " + err.value.decode())
    return offs, res, atoms


def trajectory_topology(frames, batch, structure=0, atom_index=None, selection=None, per_atom=False, alg=LEE_RICHARDS, probe=1.4,
                        resolution=20, frames_per_batch=0, device=-1, devices=None, chain_groups=None, separate_chains=False,
                        long=False, group=None, n_groups=None, stats=None, per_frame=True, volumes=False, masks=False,
                        interface_pairs=None, interface_residues=False, min_buried=0.0):
    """freesasa_gpu_trajectory_topology(): frames [F, frame_atoms, 3] of a (solvated) system whose solute is structure
    `structure` of the ingest.Batch - topology atom i is frame atom atom_index[i] (None: the frames hold exactly the
    structure's atoms) - -> a TopologyResult.  The gather, the per-residue, per-class and per-selection sums run on the
    device; the per-atom areas come back only with per_atom=True.
    Chain groups (freesasa_gpu_trajectory_groups): chain_groups="AB+C" (long=True: the long syntax) or separate_chains=True
    as Batch.chain_groups takes them, or group=ids [n] (-1: in no group) with n_groups=G - the result then has group_areas,
    group_atoms and, with per_atom, isolated.
    stats=("atoms", "residues", ...) (the names of STATS_BITS; freesasa_gpu_trajectory_groups_stats): the result's stats holds the
    RunStats of those outputs over the run, reduced on the device shard by shard.  An output named there is computed whether or not
    it is delivered: with per_atom=False the per-atom areas never leave the device, and with per_frame=False neither do the class
    sums, residues, selection and group areas.
    volumes=True (freesasa_gpu_trajectory_volume; Shrake-Rupley, up to 128 points, no chain groups, no statistics): the
    result's volumes [F] holds the volume every frame's surface encloses, as calc_volume gives it for the frame.
    masks=True (freesasa_gpu_trajectory_masks; Shrake-Rupley, up to 128 points, no chain groups, no statistics, no volumes): the
    result's masks [F, n, 4] holds every atom's exposure mask in every frame, as calc_masks gives it for the frame; the dots of any
    frame follow from it with dots_from_masks.
    interface_pairs="all" or [(g, h), ...] (freesasa_gpu_trajectory_interfaces; needs chain groups; no volumes, no masks): the
    result's pair_areas [F, K, 6] holds, per frame and pair of groups g < h, (iso_g, iso_h, in_pair_g, in_pair_h, buried_g,
    buried_h) - which partner buries how much; pair_groups [K, 2] the pairs ("all": every g < h, g-major).  There is no contact
    screen: a pair that does not touch in a frame has buried areas of 0 or rounding noise.
    interface_residues=True with interface_pairs (freesasa_gpu_trajectory_interface_residues): the result's pair_residues [F, S, 4]
    holds, per frame and segment - the atoms of one side of a pair that lie in one residue - (iso_res, in_pair_res, buried_res,
    in_interface = buried_res > min_buried); pair_res_offsets, pair_res_index, pair_res_atoms and side_segments(k, side) say which
    segment is which.  stats= then also takes "pairs" and "pair_residues" (PAIR_STATS_BITS): stats["pair_residues"][0, :, 3] is
    every segment's occupancy over the run; with per_frame=False an output named there is not delivered."""
    if interface_pairs is not None and (volumes or masks):
        raise ValueError("interface_pairs is not offered with volumes=True or masks=True")
    if interface_residues and interface_pairs is None:
        raise ValueError("interface_residues=True needs interface_pairs")
    if volumes and (stats or not per_frame or chain_groups is not None or separate_chains or group is not None):
        raise ValueError("volumes=True is not offered with chain groups, stats= or per_frame=False")
    if masks and (volumes or stats or not per_frame or chain_groups is not None or separate_chains or group is not None):
        raise ValueError("masks=True is not offered with chain groups, stats=, per_frame=False or volumes=True")
    return _trajectory_topology_stats(frames, batch, structure, atom_index, selection, per_atom, alg, probe, resolution, frames_per_batch,
                                      device, devices, chain_groups, separate_chains, long, group, n_groups, stats, per_frame, interface_pairs,
                                      interface_residues, min_buried, volumes, masks)


def _trajectory_topology_stats(frames, batch, structure, atom_index, selection, per_atom, alg, probe, resolution, frames_per_batch,
                               device, devices, chain_groups, separate_chains, long, group, n_groups, stats, per_frame, interface_pairs=None,
                               interface_residues=False, min_buried=0.0, volumes=False, masks=False):
    """the memory form of every entry with a topology: the arrays once, and the entry by what is asked for"""
    L = _stats_proto(lib())
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    if frames.ndim != 3 or frames.shape[2] != 3:
        raise ValueError("frames must be [n_frames, frame_atoms, 3]")
    F = frames.shape[0]
    n, R, res_ref, idx, fa_ = _topology_args(batch, structure, atom_index, frames.shape[1])
    S = len(selection) if selection is not None else 0
    ids, G, g_atoms = _topology_groups(batch, structure, n, chain_groups, separate_chains, long, group, n_groups)
    pairs = _interface_pairs(interface_pairs, ids, G)
    with_res = pairs is not None and bool(interface_residues)
    word = stats_word(stats, pairs=bool(interface_residues))
    K, NS, segments = 0 if pairs is None else pairs.shape[0], 0, (None, None, None)
    if with_res:
        # (the library's refusals of the topology, the ids and the pairs come from the segments entry first, with its messages)
        segments = traj_pair_segments(batch, ids, G, pairs, structure)
        NS = segments[1].size
    name = "interface_residues" if with_res else "interfaces" if pairs is not None else "volume" if volumes else "masks" if masks else \
        "groups_stats" if stats or not per_frame else "topology" if ids is None else "groups"
    out = dict(totals=np.zeros(F), sasa=np.zeros((F, n)) if per_atom else None,
               class_sums=np.zeros((F, 3)) if per_frame else None, residues=np.zeros((F, R, 6)) if per_frame else None,
               sel_area=np.zeros((F, S)) if selection is not None and per_frame else None,
               sel_atoms=np.zeros(S, dtype=np.int64) if selection is not None else None,
               group_areas=np.zeros((F, max(G, 0), 3)) if ids is not None and per_frame else None,
               isolated=np.zeros((F, n)) if ids is not None and per_atom else None,
               volumes=np.zeros(F) if volumes else None, masks=np.zeros((F, n, 4), dtype=np.uint32) if masks else None,
               pair_areas=np.zeros((F, K, 6)) if pairs is not None and (per_frame or not with_res or not word & PAIR_STATS_BITS["pairs"]) else None,
               pair_residues=np.zeros((F, NS, 4)) if with_res and (per_frame or not word & PAIR_STATS_BITS["pair_residues"]) else None)
    W = L.freesasa_gpu_traj_stats_width_pairs(word, n, R, S, max(G, 0), K, NS, None) if with_res else \
        L.freesasa_gpu_traj_stats_width(word, n, R, S, max(G, 0), None)
    raw = np.empty((4, max(W, 0)))
    nf = _shard_frames(F, frames_per_batch)
    parts = None if nf is None or not word else np.empty((nf.size, 4, max(W, 0)))
    _traj_call(name, batch, selection, devices, device, frames=frames, n_frames=F, structure=structure, frame_atoms=fa_, atom_index=idx,
               group=ids, n_groups=G, alg=alg, probe=probe, resolution=resolution, frames_per_batch=frames_per_batch, stats=word,
               stats_to=raw if word else None, partials_to=parts, pairs=pairs, n_pairs=K, min_buried=float(min_buried) if with_res else 0.0, **out)
    run = None
    if word:
        run = RunStats(raw, word, n, R, S, max(G, 0), parts, nf, **(dict(n_pairs=K, n_segments=NS) if with_res else {}))
    return TopologyResult(out["totals"], out["class_sums"], out["residues"], out["sel_area"], out["sel_atoms"], out["sasa"], res_ref,
                          out["group_areas"], g_atoms, out["isolated"], run, out["volumes"], out["masks"], out["pair_areas"], pairs,
                          out["pair_residues"], *segments)


def trajectory_file_topology(frames_path, batch, totals_path, structure=0, atom_index=None, frame_atoms=None, selection=None,
                             sasa_path=None, class_sums_path=None, residues_path=None, selections_path=None, done_path=None,
                             f32=False, header_bytes=0, n_frames=0, alg=LEE_RICHARDS, probe=1.4, resolution=20, frames_per_batch=0,
                             max_new_shards=0, device=-1, devices=None, out_f32=False, chain_groups=None, separate_chains=False,
                             long=False, group=None, n_groups=None, group_areas_path=None, isolated_path=None, dcd=False, pbc=False,
                             triclinic=False, netcdf=False, xtc=False, stats=None, stats_path=None, partials_path=None, trr=False,
                             volumes_path=None, masks_path=None, interface_pairs=None, pair_areas_path=None, pair_residues_path=None,
                             min_buried=None):
    """freesasa_gpu_trajectory_file_topology(): trajectory_file() with a topology (see trajectory_topology; frame_atoms:
    atoms per frame of the file, None: the structure's) and one raw fp64 result file per output asked for: class sums
    [F, 3], residues [F, R, 6], selection areas [F, S].  Returns (complete, n_frames, selection_atoms [S] or None).
    Chain groups (the keywords of trajectory_topology; freesasa_gpu_trajectory_file_groups): group_areas_path receives
    [F, G, 3] fp64, isolated_path [F, n] fp64 (fp32 with out_f32).
    dcd: frames_path is a DCD trajectory; frame_atoms None is then the file's NATOM.
    pbc: (with dcd) the atoms the index keeps among their periodic images, frame by frame (with chain groups:
    trajectory_file_groups_periodic);
    triclinic: (with dcd and pbc) the cell records decoded as triclinic cells, see trajectory_file;
    netcdf: frames_path is an AMBER NetCDF trajectory; frame_atoms None is then the file's atom count; pbc and triclinic as with dcd;
    xtc: frames_path is a GROMACS XTC trajectory; frame_atoms None is then the file's atom count; pbc and triclinic as with dcd.
    trr: frames_path is a GROMACS TRR trajectory; frame_atoms None is then the file's atom count; pbc and triclinic as with dcd.
    stats=("atoms", "residues", ...) with stats_path and partials_path (freesasa_gpu_trajectory_file_groups_stats): the run statistics of
    those outputs, as trajectory_file describes them; an output named there needs no result file of its own.
    volumes_path (freesasa_gpu_trajectory_file_volume; Shrake-Rupley, up to 128 points, no chain groups, no statistics, no pbc):
    receives the frames' volumes [F] fp64, as trajectory_topology(volumes=True) gives them.
    masks_path (freesasa_gpu_trajectory_file_masks; Shrake-Rupley, up to 128 points, no chain groups, no statistics, no pbc, no
    volumes): receives the frames' exposure masks [F, n, 4] uint32, as trajectory_topology(masks=True) gives them.
    interface_pairs="all" or [(g, h), ...] with pair_areas_path (freesasa_gpu_trajectory_file_interfaces; needs chain groups; no
    pbc, no volumes, no masks): pair_areas_path receives [F, K, 6] fp64, as trajectory_topology(interface_pairs=...) gives them.
    pair_residues_path and / or min_buried with interface_pairs (freesasa_gpu_trajectory_file_interface_residues): pair_residues_path
    receives [F, S, 4] fp64, as trajectory_topology(interface_residues=True) gives them (traj_pair_segments says which segment is
    which); stats= then also takes "pairs" and "pair_residues", and pair_areas_path may be None; min_buried None is 0.0."""
    return _trajectory_file_topology(periodic=False, **locals())


def _trajectory_file_topology(periodic, frames_path, batch, totals_path, structure, atom_index, frame_atoms, selection, sasa_path, class_sums_path,
                              residues_path, selections_path, done_path, f32, header_bytes, n_frames, alg, probe, resolution, frames_per_batch,
                              max_new_shards, device, devices, out_f32, chain_groups, separate_chains, long, group, n_groups, group_areas_path,
                              isolated_path, dcd, pbc, triclinic, netcdf, xtc, stats, stats_path, partials_path, trr, volumes_path, masks_path,
                              interface_pairs, pair_areas_path, pair_residues_path, min_buried):
    """the file form of every entry with a topology, under the keywords of trajectory_file_topology: the entry by what is asked for;
    periodic: the entries among periodic images (trajectory_file_groups_periodic)"""
    with_res = pair_residues_path is not None or min_buried is not None
    if with_res and interface_pairs is None:
        raise ValueError("pair_residues_path and min_buried need interface_pairs")
    if not with_res and (interface_pairs is None) != (pair_areas_path is None):
        raise ValueError("interface_pairs and pair_areas_path go together")
    if interface_pairs is not None and (volumes_path is not None or masks_path is not None):
        raise ValueError("interface_pairs is not offered with volumes_path or masks_path")
    if volumes_path is not None and (stats or chain_groups is not None or separate_chains or group is not None or
                                     group_areas_path is not None or isolated_path is not None):
        raise ValueError("volumes_path is not offered with chain groups or stats=")
    if masks_path is not None and (volumes_path is not None or stats or chain_groups is not None or separate_chains or group is not None or
                                   group_areas_path is not None or isolated_path is not None):
        raise ValueError("masks_path is not offered with chain groups, stats= or volumes_path")
    bits = _frames_bits(f32, out_f32, dcd, header_bytes, pbc, triclinic, netcdf, xtc, trr)
    if frame_atoms is None:   # (a container says for itself how many atoms a frame has)
        info = dcd_info if dcd else nc_info if netcdf else xtc_info if xtc else trr_info if trr else None
        if info is not None:
            frame_atoms = info(frames_path).n_atoms
    n, R, res_ref, idx, fa_ = _topology_args(batch, structure, atom_index, frame_atoms)
    S = len(selection) if selection is not None else 0
    sel_atoms = np.zeros(S, dtype=np.int64) if selection is not None else None
    total = C.c_longlong(0)
    ids, G, _ = _topology_groups(batch, structure, n, chain_groups, separate_chains, long, group, n_groups)
    pairs = _interface_pairs(interface_pairs, ids, G)
    if pairs is not None:
        name = "file_interface_residues" if with_res else "file_interfaces"
    elif periodic:
        name = "file_groups"
    else:
        name = "file_volume" if volumes_path is not None else "file_masks" if masks_path is not None else "file_groups_stats" if stats else \
            "file_groups" if ids is not None or group_areas_path is not None or isolated_path is not None else "file_topology"
    ret = _traj_call(name + "_periodic" * periodic, batch, selection, devices, device, frames_path=frames_path, frames_f32=bits,
                     header_bytes=header_bytes, n_frames=n_frames, structure=structure, frame_atoms=fa_, atom_index=idx, group=ids, n_groups=G,
                     alg=alg, probe=probe, resolution=resolution, frames_per_batch=frames_per_batch, totals=totals_path, sasa=sasa_path,
                     class_sums=class_sums_path, residues=residues_path, sel_area=selections_path, sel_atoms=sel_atoms,
                     group_areas=group_areas_path, isolated=isolated_path, volumes=volumes_path, masks=masks_path, done_path=done_path,
                     max_new_shards=max_new_shards, frames_total=C.byref(total),
                     stats=stats_word(stats, pairs=pairs is not None and with_res) if stats else 0, stats_to=stats_path, partials_to=partials_path,
                     pairs=pairs, n_pairs=0 if pairs is None else pairs.shape[0], pair_areas=pair_areas_path,
                     min_buried=0.0 if min_buried is None else float(min_buried), pair_residues=pair_residues_path)
    return ret == 0, int(total.value), sel_atoms


def trajectory_file_groups_periodic(frames_path, batch, totals_path, structure=0, atom_index=None, frame_atoms=None, selection=None,
                                    sasa_path=None, class_sums_path=None, residues_path=None, selections_path=None, done_path=None,
                                    n_frames=0, alg=LEE_RICHARDS, probe=1.4, resolution=20, frames_per_batch=0,
                                    max_new_shards=0, device=-1, devices=None, out_f32=False, chain_groups=None, separate_chains=False,
                                    long=False, group=None, n_groups=None, group_areas_path=None, isolated_path=None, dcd=False,
                                    triclinic=False, netcdf=False, xtc=False, stats=None, stats_path=None, partials_path=None, trr=False,
                                    interface_pairs=None, pair_areas_path=None, pair_residues_path=None, min_buried=None):
    """freesasa_gpu_trajectory_file_groups_periodic(): trajectory_file_topology() with chain groups and every frame among the
    periodic images of its own cell (pbc is implied; dcd, netcdf, xtc or trr names the container, triclinic how its cell is read):
    per frame the totals, the per-atom areas, the per-atom isolated areas and the group table are those of calc_groups_periodic
    (calc_groups_periodic_triclinic) on that frame - chains that lie in different images of the box bury what they bury.  The
    keywords, outputs, statistics and the done-list are trajectory_file_topology's.  Returns (complete, n_frames,
    selection_atoms [S] or None).
    interface_pairs="all" or [(g, h), ...] with pair_areas_path (freesasa_gpu_trajectory_file_interfaces_periodic): the interfaces
    between the groups among periodic images - every pair structure in the frame's cell among its own images; pair_areas_path
    receives [F, K, 6] fp64, the columns of trajectory_file_topology(interface_pairs=...).  pair_residues_path and / or min_buried
    with interface_pairs (freesasa_gpu_trajectory_file_interface_residues_periodic): pair_residues_path receives [F, S, 4] fp64
    (traj_pair_segments says which segment is which); stats= then also takes "pairs" and "pair_residues", and pair_areas_path
    may be None; min_buried None is 0.0.  The argument checks are trajectory_file_topology's."""
    return _trajectory_file_topology(periodic=True, f32=False, header_bytes=0, pbc=True, volumes_path=None, masks_path=None, **locals())


def parse_files_dev(paths, ingest_options=0, n_threads=0, device=0, classifier=None):
    """freesasa_gpu_parse_files(): the device-side PDB / mmCIF parser on its own -> (xyz [atoms, 3], radii, classes,
    offsets [n + 1], status [n], refused [n]); a refused file (the sweep hands it to the host parser) contributes no atoms.
    classifier: an ingest.Classifier in place of ProtOr (freesasa_gpu_parse_files_classified)."""
    L = lib()
    L.freesasa_gpu_parse_files.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(C.c_ubyte),
                                           C.c_longlong, _lp, _ip, _ip, C.c_char_p, C.c_int]
    L.freesasa_gpu_parse_files.restype = C.c_longlong
    L.freesasa_gpu_parse_files_classified.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                                      C.POINTER(C.c_ubyte), C.c_longlong, _lp, _ip, _ip, C.c_void_p, C.c_char_p, C.c_int]
    L.freesasa_gpu_parse_files_classified.restype = C.c_longlong
    from . import ingest
    handle = ingest._handle(classifier)
    n = len(paths)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    offs, status, host = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    err = C.create_string_buffer(512)
    cap = 1 << 16
    while True:
        xyz, r, cls = np.empty(3 * cap), np.empty(cap), np.empty(cap, dtype=np.uint8)
        args = (arr, n, ingest_options, n_threads, device, xyz.ctypes.data_as(_dp), r.ctypes.data_as(_dp),
                cls.ctypes.data_as(C.POINTER(C.c_ubyte)), cap, offs.ctypes.data_as(_lp), status.ctypes.data_as(_ip), host.ctypes.data_as(_ip))
        if classifier is None:
            got = L.freesasa_gpu_parse_files(*args, err, 512)
        else:
            got = L.freesasa_gpu_parse_files_classified(*args, handle, err, 512)
        if got == -2:
            cap = int(offs[-1]) + 16
            continue
        if got < 0:
            raise RuntimeError("freesasa_gpu_parse_files: " + err.value.decode())
        return xyz[:3 * got].reshape(-1, 3).copy(), r[:got].copy(), cls[:got].copy(), offs, status, host


def sweep_parse_stats():
    """(files parsed on the device, files left to the host parser) by this process's sweeps since the last call."""
    a, b = C.c_longlong(0), C.c_longlong(0)
    lib().freesasa_gpu_sweep_parse_stats(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def host_test_fail_after(n):
    """freesasa_host_test_fail_after(): the n-th host allocation / thread creation of the library's own code fails
    (n <= 0: off); returns what was left of the previous countdown (tests/test_hostfault.py)."""
    return int(lib().freesasa_host_test_fail_after(int(n)))


def test_points(n_points):
    tp = np.empty(3 * n_points)
    lib().freesasa_gpu_test_points(n_points, tp.ctypes.data_as(_dp))
    return tp.reshape(n_points, 3)


# the records of the test hook GpuContext.cell_sort (include/freesasa_gpu.h, freesasa_gpu_cell_sort_dev)
CELL_SORT_STATUS_WORDS = 142
CELL_SORT_GRID = np.dtype([("x0", "<f8"), ("y0", "<f8"), ("z0", "<f8"), ("d", "<f8"), ("nx", "<i4"), ("ny", "<i4"), ("nz", "<i4"), ("cell_base", "<i4")])
CELL_SORT_IDX = np.dtype([("cell", "<i8"), ("orig", "<i4"), ("strct", "<i4")])


class GpuContext:
    """Device-resident batches: pointers are raw device addresses (e.g. tensor.data_ptr())."""

    def __init__(self, device=0, stream=None, timing=False):
        self._h = lib().freesasa_gpu_ctx_create(device, C.c_void_p(stream) if stream else None)
        if not self._h:
            raise RuntimeError("freesasa_gpu_ctx_create failed: no usable HIP device "
                               "(libfreesasa_amd has no CPU path)")
        if timing:
            lib().freesasa_gpu_ctx_set_timing(self._h, 1)
        self._tp = {}

    def set_timing(self, on):
        """freesasa_gpu_ctx_set_timing(): HIP events around the cell sort and the tile kernel of every batch (stats():
        ms_prep, ms_kernel, ms_total); off by default - the four event records cost a small batch ~35 us of its step."""
        lib().freesasa_gpu_ctx_set_timing(self._h, 1 if on else 0)

    def close(self):
        if self._h:
            lib().freesasa_gpu_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self):
        return lib().freesasa_gpu_ctx_last_error(self._h).decode()

    def stats(self):
        s = Stats()
        lib().freesasa_gpu_ctx_get_stats(self._h, C.byref(s))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def lee_richards(self, d_xyz, d_radii, offsets, d_sasa, d_totals=0, probe=1.4, n_slices=20):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ret = lib().freesasa_gpu_lr_batch_dev(self._h, d_xyz, d_radii, offsets.ctypes.data_as(_lp),
                                              offsets.size - 1, probe, n_slices, d_sasa,
                                              d_totals or None)
        if ret:
            raise RuntimeError("freesasa_gpu_lr_batch_dev: " + self.error())

    def lee_richards_async(self, d_xyz, d_radii, offsets, d_sasa, d_totals=0, probe=1.4, n_slices=20):
        """Enqueue the batch and return (freesasa_gpu_lr_batch_dev_async): up to two in flight; wait() collects them."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if lib().freesasa_gpu_lr_batch_dev_async(self._h, d_xyz, d_radii, offsets.ctypes.data_as(_lp),
                                                 offsets.size - 1, probe, n_slices, d_sasa, d_totals or None):
            raise RuntimeError("freesasa_gpu_lr_batch_dev_async: " + self.error())

    def wait(self):
        if lib().freesasa_gpu_wait(self._h):
            raise RuntimeError("freesasa_gpu_wait: " + self.error())

    def lr_neighbors(self, d_xyz, d_radii, offsets, d_nn, d_nb=0, nb_cap=0, probe=1.4):
        """Test hook: the neighbor sets the L&R kernel finds (counts, optionally the first nb_cap neighbors per atom)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if lib().freesasa_gpu_lr_neighbors_dev(self._h, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1,
                                               probe, d_nn, d_nb or None, nb_cap):
            raise RuntimeError("freesasa_gpu_lr_neighbors_dev: " + self.error())

    def arc_union(self, sets):
        """Test hook: exposed arc length of every set of (start, end) arcs through the kernel's arc union."""
        first = np.concatenate([[0], np.cumsum([len(x) // 2 for x in sets])]).astype(np.int32)
        arcs = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in sets]))
        out = np.empty(len(sets))
        if lib().freesasa_gpu_arc_union_dev(self._h, arcs.ctypes.data_as(_dp), first.ctypes.data_as(_ip), len(sets),
                                            out.ctypes.data_as(_dp)):
            raise RuntimeError("freesasa_gpu_arc_union_dev: " + self.error())
        return out

    def kat_elementwise(self, op, a=None, b=None, c=None, k=0.0, n=None, outputs=2):
        """Test hook: the device-only arithmetic, one thread per operand (csrc/kat_kernels.h numbers the ops and says which of
        the float64 arrays a, b, c and the scalar k each reads).  Returns (out0, out1), NaN where the op writes nothing;
        `n` and `outputs` (how many output arrays are handed over) default to what the arrays say.  ValueError for
        arguments that are refused."""
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (a, b, c)]
        if n is None:
            n = max([x.size for x in arrs if x is not None] or [0])
        if any(x is not None and x.size < min(max(int(n), 0), 1 << 20) for x in arrs):
            raise ValueError("kat_elementwise: an array is shorter than n")
        outs = [np.full(max(int(n), 0), np.nan) if j < outputs else None for j in range(2)]
        ptr = lambda x: x.ctypes.data if x is not None else None
        if lib().freesasa_gpu_kat_elementwise_dev(self._h, int(op), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), int(n), float(k),
                                                  ptr(outs[0]), ptr(outs[1])):
            raise ValueError("freesasa_gpu_kat_elementwise_dev: " + self.error())
        return outs[0], outs[1]

    def kat_wave(self, op, words, rows=None):
        """Test hook: the lane primitives, `words` (uint64 [rows, 64]) through one full wave (csrc/kat_kernels.h numbers the ops).
        Returns uint64 [rows, 64]; words=None hands over no arrays.  ValueError for arguments that are refused."""
        w = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 64)
        if rows is None:
            rows = 0 if w is None else w.shape[0]
        if w is not None and w.shape[0] < min(max(int(rows), 0), 4096):
            raise ValueError("kat_wave: fewer rows than said")
        out = None if w is None else np.zeros_like(w)
        if lib().freesasa_gpu_kat_wave_dev(self._h, int(op), None if w is None else w.ctypes.data, int(rows),
                                           None if out is None else out.ctypes.data):
            raise ValueError("freesasa_gpu_kat_wave_dev: " + self.error())
        return out

    def xtc_decode(self, file_bytes, n_frames, n_atoms):
        """Test hook: the XTC decode kernels over n_frames whole frames at the beginning of file_bytes -> (records: per frame the
        [groups, 4] int32 array of (bit, atom, run, smallidx), status [n_frames], xyz [n_frames, n_atoms, 3] float32 in Angstrom,
        NaN where no thread wrote).  ValueError for an argument or a header that is refused."""
        n_frames, n_atoms = int(n_frames), int(n_atoms)
        slots = max(n_frames, 0) * max(n_atoms, 0)
        rec = np.zeros((slots, 4), dtype=np.int32)
        count = np.full((max(n_frames, 0), 2), -1, dtype=np.int32)
        out = np.full((slots, 3), np.nan, dtype=np.float32)
        data = bytes(file_bytes)
        if lib().freesasa_gpu_xtc_decode_dev(self._h, data, len(data), n_frames, n_atoms, rec.ctypes.data, count.ctypes.data, out.ctypes.data):
            raise ValueError("freesasa_gpu_xtc_decode_dev: " + self.error())
        rec = rec.reshape(n_frames, n_atoms, 4)
        return [rec[f, :max(int(count[f, 0]), 0)] for f in range(n_frames)], count[:, 1].copy(), out.reshape(n_frames, n_atoms, 3)

    def cell_sort(self, d_xyz, d_radii, offsets, probe=1.4, arrangement=0, cells_cap=0, shared_radii=False):
        """Test hook: ONE pass of the cell sort on its own (freesasa_gpu_cell_sort_dev), forced into `arrangement` - 0 the general
        pipeline, 1 k_sort_struct with the dense table, 2 k_sort_struct with the compact table - with a table of cells_cap cells
        (0: the engine's sizing of a first batch).  Nothing is redone and the context learns nothing.  Returns a dict: status
        (int32 [CELL_SORT_STATUS_WORDS]), error, retry, occ_sum, occ_n, cells (the named status words), occ_stride, cells_cap
        (the capacity used), grid (records x0, y0, z0, d, nx, ny, nz, cell_base), ncells, sq [n, 4], s_idx (records cell, orig,
        strct), and cell_start [cells_cap + 2] or cell_tbl [(cells_cap >> 5) + 2] with cell_first [n + n_structs + 2]; what no
        kernel wrote is all-ones bytes.  ValueError for arguments that are refused."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ns = offsets.size - 1
        n = int(offsets[-1]) if ns >= 1 else 0
        cap = lib().freesasa_gpu_cell_sort_cap(self._h, n, ns, int(cells_cap))
        dense = arrangement != 2
        status = np.full(CELL_SORT_STATUS_WORDS, -1, dtype=np.int32)
        stride = np.full(1, -1, dtype=np.int32)
        nn, nss, capn = max(n, 0), max(ns, 0), max(cap, 0)
        grid = np.full(nss, -1, dtype=np.int64).repeat(6).view(CELL_SORT_GRID)
        ncells = np.full(nss, -1, dtype=np.int64)
        sq = np.full(4 * nn, -1, dtype=np.int64).view(np.float64)
        s_idx = np.full(2 * nn, -1, dtype=np.int64).view(CELL_SORT_IDX)
        cell_start = np.full(capn + 2, -1, dtype=np.int32) if dense else None
        cell_tbl = None if dense else np.full((capn >> 5) + 2, -1, dtype=np.int64).view(np.uint64)
        cell_first = None if dense else np.full(nn + nss + 2, -1, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None else None
        if lib().freesasa_gpu_cell_sort_dev(self._h, d_xyz, d_radii, offsets.ctypes.data_as(_lp), ns, probe, int(arrangement), int(cells_cap),
                                            int(cap), 1 if shared_radii else 0, ptr(status), ptr(stride), ptr(grid), ptr(ncells), ptr(sq), ptr(s_idx),
                                            ptr(cell_start), ptr(cell_tbl), ptr(cell_first)):
            raise ValueError("freesasa_gpu_cell_sort_dev: " + self.error())
        out = {"status": status, "error": int(status[0]), "occ_sum": int(status[4]), "occ_n": int(status[5]), "retry": int(status[7]),
               "cells": int(status[140:142].view(np.int64)[0]), "occ_stride": int(stride[0]), "cells_cap": int(cap), "grid": grid,
               "ncells": ncells, "sq": sq.reshape(-1, 4), "s_idx": s_idx}
        out.update({"cell_start": cell_start} if dense else {"cell_tbl": cell_tbl, "cell_first": cell_first})
        return out

    def segment_sums(self, d_sasa, seg_offsets, d_out):
        seg = np.ascontiguousarray(seg_offsets, dtype=np.int64)
        if lib().freesasa_gpu_segment_sums_dev(self._h, d_sasa, seg.ctypes.data_as(_lp), seg.size - 1, d_out):
            raise RuntimeError("freesasa_gpu_segment_sums_dev: " + self.error())

    def class_sums(self, d_sasa, d_class, offsets, d_out):
        """d_out[3*s + c] <- sum of d_sasa over structure s's atoms of class c (0 apolar, 1 polar, 2 unknown)."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if lib().freesasa_gpu_class_sums_dev(self._h, d_sasa, d_class, offs.ctypes.data_as(_lp), offs.size - 1, d_out):
            raise RuntimeError("freesasa_gpu_class_sums_dev: " + self.error())

    def residue_areas(self, d_sasa, d_class, d_backbone, res_first, d_abs, res_ref=None, ref_table=None, d_rel=0):
        """Per-residue node areas (d_abs[6*r+..]) and, given res_ref / ref_table, relative areas (d_rel[5*r+..])."""
        rf = np.ascontiguousarray(res_first, dtype=np.int64)
        rr = np.ascontiguousarray(res_ref, dtype=np.int16) if res_ref is not None else None
        rt = np.ascontiguousarray(ref_table, dtype=np.float64).reshape(-1) if ref_table is not None else None
        ret = lib().freesasa_gpu_residue_areas_dev(
            self._h, d_sasa, d_class, d_backbone, rf.ctypes.data_as(_lp), rf.size - 1,
            rr.ctypes.data_as(C.POINTER(C.c_short)) if rr is not None else None,
            rt.ctypes.data_as(_dp) if rt is not None else None, (rt.size // 5) if rt is not None else 0, d_abs, d_rel)
        if ret:
            raise RuntimeError("freesasa_gpu_residue_areas_dev: " + self.error())

    def groups(self, d_xyz, d_radii, offsets, d_group, n_groups, d_sasa, d_iso, d_totals=0, d_group_totals=0,
               alg=LEE_RICHARDS, probe=1.4, resolution=20):
        """freesasa_gpu_groups_dev(): complex areas (d_sasa), areas of every atom in its isolated group (d_iso), totals
        and per-group (isolated, complex, buried) totals (d_group_totals [3 G]); d_group is a device int32 array,
        n_groups a host array of groups per structure."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ng = np.ascontiguousarray(n_groups, dtype=np.int32)
        ret = lib().freesasa_gpu_groups_dev(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1,
                                            d_group, ng.ctypes.data_as(C.POINTER(C.c_int32)), probe, resolution, d_sasa,
                                            d_iso, d_totals or None, d_group_totals or None)
        if ret:
            raise RuntimeError("freesasa_gpu_groups_dev: " + self.error())

    def interface_pairs(self, d_xyz, d_radii, offsets, d_group, n_groups, pair_capacity=0, pair_struct=None, pair_groups=None,
                        d_sasa=0, d_iso=0, d_totals=0, d_group_totals=0, alg=LEE_RICHARDS, probe=1.4, resolution=20):
        """freesasa_gpu_interface_pairs_dev(): the contact screen behind groups() -> (n_pairs, n_pair_atoms, n_tests,
        n_candidates); pair_struct [pair_capacity] and pair_groups [pair_capacity, 2]: host int32 arrays (None: the counts only)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ng = np.ascontiguousarray(n_groups, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        P, M, stats = C.c_longlong(0), C.c_longlong(0), (C.c_longlong * 2)()
        if lib().freesasa_gpu_interface_pairs_dev(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, d_group,
                                                  ng.ctypes.data_as(i32), probe, resolution, d_sasa or None, d_iso or None,
                                                  d_totals or None, d_group_totals or None, pair_capacity, C.byref(P), C.byref(M),
                                                  None if pair_struct is None else pair_struct.ctypes.data_as(i32),
                                                  None if pair_groups is None else pair_groups.ctypes.data_as(i32), stats):
            raise RuntimeError("freesasa_gpu_interface_pairs_dev: " + self.error())
        return int(P.value), int(M.value), int(stats[0]), int(stats[1])

    def interfaces(self, d_xyz, d_radii, offsets, d_group, n_groups, d_sasa, d_iso, pair_capacity, d_pair_areas, d_pair_struct=0,
                   d_pair_groups=0, atom_capacity=0, d_side_offsets=0, d_pair_atom=0, d_pair_buried=0, d_totals=0, d_group_totals=0,
                   alg=LEE_RICHARDS, probe=1.4, resolution=20):
        """freesasa_gpu_interfaces_dev(): groups() and the pair table into device arrays that hold pair_capacity rows
        (d_pair_areas [6 P], d_pair_struct [P], d_pair_groups [2 P], d_side_offsets [2 P + 1]) and atom_capacity atoms
        (d_pair_atom, d_pair_buried [M]) -> (n_pairs, n_pair_atoms); a capacity that is too small: RuntimeError naming the number."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ng = np.ascontiguousarray(n_groups, dtype=np.int32)
        P, M = C.c_longlong(0), C.c_longlong(0)
        if lib().freesasa_gpu_interfaces_dev(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, d_group,
                                             ng.ctypes.data_as(C.POINTER(C.c_int32)), probe, resolution, d_sasa or None, d_iso or None,
                                             d_totals or None, d_group_totals or None, pair_capacity, atom_capacity, C.byref(P),
                                             C.byref(M), d_pair_struct or None, d_pair_groups or None, d_pair_areas or None,
                                             d_side_offsets or None, d_pair_atom or None, d_pair_buried or None):
            raise RuntimeError("freesasa_gpu_interfaces_dev: " + self.error())
        return int(P.value), int(M.value)

    def interface_residues(self, d_xyz, d_radii, offsets, d_group, n_groups, res_first, d_sasa, d_iso, pair_capacity, d_pair_areas,
                           res_capacity, d_res_areas, d_res_offsets=0, d_res_index=0, d_res_atoms=0, d_pair_struct=0, d_pair_groups=0,
                           atom_capacity=0, d_side_offsets=0, d_pair_atom=0, d_pair_buried=0, d_totals=0, d_group_totals=0,
                           alg=LEE_RICHARDS, probe=1.4, resolution=20, min_buried=0.0):
        """freesasa_gpu_interface_residues_dev(): interfaces() and the per-residue table of every side - res_first: a host
        array of the batch's residue boundaries [n_res + 1]; d_res_areas [3 R], d_res_index [R], d_res_atoms [R]: device arrays
        that hold res_capacity rows, d_res_offsets [2 P + 1] one that holds pair_capacity rows - a row for every residue of a
        side that loses more than min_buried -> (n_pairs, n_pair_atoms, n_res_rows); a capacity that is too small: RuntimeError
        naming the number."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ng = np.ascontiguousarray(n_groups, dtype=np.int32)
        res_first = np.ascontiguousarray(res_first, dtype=np.int64)
        P, M, R = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        if lib().freesasa_gpu_interface_residues_dev(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, d_group,
                                                     ng.ctypes.data_as(C.POINTER(C.c_int32)), res_first.ctypes.data_as(_lp),
                                                     res_first.size - 1, probe, resolution, min_buried, d_sasa or None, d_iso or None,
                                                     d_totals or None, d_group_totals or None, pair_capacity, atom_capacity,
                                                     res_capacity, C.byref(P), C.byref(M), C.byref(R), d_pair_struct or None,
                                                     d_pair_groups or None, d_pair_areas or None, d_side_offsets or None,
                                                     d_pair_atom or None, d_pair_buried or None, d_res_offsets or None,
                                                     d_res_index or None, d_res_atoms or None, d_res_areas or None):
            raise RuntimeError("freesasa_gpu_interface_residues_dev: " + self.error())
        return int(P.value), int(M.value), int(R.value)

    def interface_contacts(self, d_xyz, d_radii, offsets, d_group, n_groups, d_sasa, d_iso, pair_capacity, d_pair_areas,
                           contact_capacity=0, d_contact_first=0, d_contact_partner=0, d_contact_points=0, d_contact_area=0,
                           d_buried_masks=0, dot_capacity=0, d_dot_partner=0, d_pair_struct=0, d_pair_groups=0, atom_capacity=0,
                           d_side_offsets=0, d_pair_atom=0, d_pair_buried=0, d_totals=0, d_group_totals=0, alg=SHRAKE_RUPLEY, probe=1.4,
                           n_points=100):
        """freesasa_gpu_interface_contacts_dev(): interfaces() with Shrake-Rupley and the atom-atom contact table -
        d_contact_first [M + 1] and d_buried_masks [4 M] (device arrays that hold atom_capacity atoms), d_contact_partner,
        d_contact_points, d_contact_area [C] (contact_capacity rows), d_dot_partner [D_b] (dot_capacity dots) ->
        (n_pairs, n_pair_atoms, n_contacts, n_buried_dots); a capacity that is too small: RuntimeError naming the number."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ng = np.ascontiguousarray(n_groups, dtype=np.int32)
        P, M, Cn, D = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        if lib().freesasa_gpu_interface_contacts_dev(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, d_group,
                                                     ng.ctypes.data_as(C.POINTER(C.c_int32)), probe, n_points, d_sasa or None, d_iso or None,
                                                     d_totals or None, d_group_totals or None, pair_capacity, atom_capacity,
                                                     contact_capacity, dot_capacity, C.byref(P), C.byref(M), C.byref(Cn), C.byref(D),
                                                     d_pair_struct or None, d_pair_groups or None, d_pair_areas or None,
                                                     d_side_offsets or None, d_pair_atom or None, d_pair_buried or None,
                                                     d_contact_first or None, d_contact_partner or None, d_contact_points or None,
                                                     d_contact_area or None, d_buried_masks or None, d_dot_partner or None):
            raise RuntimeError("freesasa_gpu_interface_contacts_dev: " + self.error())
        return int(P.value), int(M.value), int(Cn.value), int(D.value)

    def interface_residue_contacts(self, d_xyz, d_radii, offsets, d_group, n_groups, res_first, d_sasa, d_iso, pair_capacity, d_pair_areas,
                                   rescontact_capacity, d_rescontact_area, d_rescontact_offsets=0, d_rescontact_residues=0,
                                   d_rescontact_counts=0, d_rescontact_reverse=0, contact_capacity=0, d_contact_first=0,
                                   d_contact_partner=0, d_contact_points=0, d_contact_area=0, d_buried_masks=0, dot_capacity=0,
                                   d_dot_partner=0, d_pair_struct=0, d_pair_groups=0, atom_capacity=0, d_side_offsets=0, d_pair_atom=0,
                                   d_pair_buried=0, d_totals=0, d_group_totals=0, alg=SHRAKE_RUPLEY, probe=1.4, n_points=100):
        """freesasa_gpu_interface_residue_contacts_dev(): interface_contacts() and the contact rows folded per pair of residues
        - res_first: a host array of the batch's residue boundaries [n_res + 1]; d_rescontact_area [Q], d_rescontact_residues
        [2 Q], d_rescontact_counts [2 Q], d_rescontact_reverse [Q]: device arrays that hold rescontact_capacity rows,
        d_rescontact_offsets [2 P + 1] one that holds pair_capacity rows -> (n_pairs, n_pair_atoms, n_contacts, n_buried_dots,
        n_rescontacts); a capacity that is too small: RuntimeError naming the number."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ng = np.ascontiguousarray(n_groups, dtype=np.int32)
        res_first = np.ascontiguousarray(res_first, dtype=np.int64)
        P, M, Cn, D, Q = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        if lib().freesasa_gpu_interface_residue_contacts_dev(
                self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, d_group, ng.ctypes.data_as(C.POINTER(C.c_int32)),
                probe, n_points, d_sasa or None, d_iso or None, d_totals or None, d_group_totals or None, pair_capacity, atom_capacity,
                contact_capacity, dot_capacity, C.byref(P), C.byref(M), C.byref(Cn), C.byref(D), d_pair_struct or None, d_pair_groups or None,
                d_pair_areas or None, d_side_offsets or None, d_pair_atom or None, d_pair_buried or None, d_contact_first or None,
                d_contact_partner or None, d_contact_points or None, d_contact_area or None, d_buried_masks or None, d_dot_partner or None,
                res_first.ctypes.data_as(_lp), res_first.size - 1, rescontact_capacity, C.byref(Q), d_rescontact_offsets or None,
                d_rescontact_residues or None, d_rescontact_counts or None, d_rescontact_area or None, d_rescontact_reverse or None):
            raise RuntimeError("freesasa_gpu_interface_residue_contacts_dev: " + self.error())
        return int(P.value), int(M.value), int(Cn.value), int(D.value), int(Q.value)

    def periodic(self, d_xyz, d_radii, offsets, cells, d_sasa, d_totals=0, alg=LEE_RICHARDS, probe=1.4, resolution=20):
        """freesasa_gpu_periodic_dev(): every atom's area among the periodic images of its structure's cell (cells: a host
        array [n_structs, 3], see calc_periodic) into d_sasa, per-structure totals over the real atoms into d_totals; returns
        the image count of every structure (a host int64 array)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        cells = _f64(cells).reshape(-1)
        if cells.size != 3 * (offsets.size - 1):
            raise ValueError("cells needs three edges per structure")
        images = np.zeros(offsets.size - 1, dtype=np.int64)
        ret = lib().freesasa_gpu_periodic_dev(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1,
                                              cells.ctypes.data_as(_dp), probe, resolution, d_sasa, d_totals or None,
                                              images.ctypes.data_as(_lp))
        if ret:
            raise RuntimeError("freesasa_gpu_periodic_dev: " + self.error())
        return images

    def periodic_triclinic(self, d_xyz, d_radii, offsets, cells6, d_sasa, d_totals=0, alg=LEE_RICHARDS, probe=1.4, resolution=20):
        """freesasa_gpu_periodic_triclinic_dev(): periodic() for triclinic cells (cells6: a host array [n_structs, 6], see
        calc_periodic_triclinic)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        cells6 = _f64(cells6).reshape(-1)
        if cells6.size != 6 * (offsets.size - 1):
            raise ValueError("cells6 needs six numbers per structure")
        images = np.zeros(offsets.size - 1, dtype=np.int64)
        ret = lib().freesasa_gpu_periodic_triclinic_dev(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1,
                                                        cells6.ctypes.data_as(_dp), probe, resolution, d_sasa, d_totals or None,
                                                        images.ctypes.data_as(_lp))
        if ret:
            raise RuntimeError("freesasa_gpu_periodic_triclinic_dev: " + self.error())
        return images

    def _groups_periodic(self, name, W, d_xyz, d_radii, offsets, d_group, n_groups, cells, d_sasa, d_iso, d_totals, d_group_totals,
                         alg, probe, resolution):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ng = np.ascontiguousarray(n_groups, dtype=np.int32)
        cells = _f64(cells).reshape(-1)
        if cells.size != W * (offsets.size - 1):
            raise ValueError("cells needs three edges per structure" if W == 3 else "cells6 needs six numbers per structure")
        images = np.zeros(offsets.size - 1, dtype=np.int64)
        ret = getattr(lib(), name)(self._h, alg, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, d_group,
                                   ng.ctypes.data_as(C.POINTER(C.c_int32)), cells.ctypes.data_as(_dp), probe, resolution, d_sasa, d_iso,
                                   d_totals or None, d_group_totals or None, images.ctypes.data_as(_lp))
        if ret:
            raise RuntimeError(name + ": " + self.error())
        return images

    def groups_periodic(self, d_xyz, d_radii, offsets, d_group, n_groups, cells, d_sasa, d_iso, d_totals=0, d_group_totals=0,
                        alg=LEE_RICHARDS, probe=1.4, resolution=20):
        """freesasa_gpu_groups_periodic_dev(): groups() with every structure, and every group taken on its own, among the
        periodic images of the structure's cell (cells: a host array [n_structs, 3], see calc_periodic); returns the image count
        of every complex (a host int64 array)."""
        return self._groups_periodic("freesasa_gpu_groups_periodic_dev", 3, d_xyz, d_radii, offsets, d_group, n_groups, cells, d_sasa,
                                     d_iso, d_totals, d_group_totals, alg, probe, resolution)

    def groups_periodic_triclinic(self, d_xyz, d_radii, offsets, d_group, n_groups, cells6, d_sasa, d_iso, d_totals=0, d_group_totals=0,
                                  alg=LEE_RICHARDS, probe=1.4, resolution=20):
        """freesasa_gpu_groups_periodic_triclinic_dev(): groups_periodic() for triclinic cells (cells6: a host array
        [n_structs, 6], see calc_periodic_triclinic)."""
        return self._groups_periodic("freesasa_gpu_groups_periodic_triclinic_dev", 6, d_xyz, d_radii, offsets, d_group, n_groups, cells6,
                                     d_sasa, d_iso, d_totals, d_group_totals, alg, probe, resolution)

    def volume(self, d_xyz, d_radii, offsets, d_sasa, d_volumes, d_counts=0, d_evec=0, d_vol=0, d_totals=0, probe=1.4, n_points=100):
        """freesasa_gpu_sr_volume_dev(): shrake_rupley() and, into d_volumes [n_structs], the volume every structure's
        solvent-accessible surface encloses (device pointers; d_counts [n], d_evec [3 n], d_vol [n], d_totals optional)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ret = lib().freesasa_gpu_sr_volume_dev(self._h, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, probe, n_points,
                                               d_sasa, d_counts or None, d_evec or None, d_vol or None, d_totals or None, d_volumes or None)
        if ret:
            raise RuntimeError("freesasa_gpu_sr_volume_dev: " + self.error())

    def masks(self, d_xyz, d_radii, offsets, d_sasa, d_masks, d_counts=0, d_totals=0, probe=1.4, n_points=100):
        """freesasa_gpu_sr_masks_dev(): shrake_rupley() and, into d_masks [n, 4] uint32, every atom's exposure mask (device
        pointers; d_counts [n] and d_totals [n_structs] optional)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ret = lib().freesasa_gpu_sr_masks_dev(self._h, d_xyz, d_radii, offsets.ctypes.data_as(_lp), offsets.size - 1, probe, n_points,
                                              d_sasa, d_counts or None, d_totals or None, d_masks or None)
        if ret:
            raise RuntimeError("freesasa_gpu_sr_masks_dev: " + self.error())

    def dots_count(self, d_masks, n_atoms, d_dot_first, n_points=100):
        """freesasa_gpu_dots_count_dev(): d_dot_first [n_atoms + 1] int64, the exclusive prefix sum of the masks' popcounts -> D"""
        D = C.c_longlong(0)
        if lib().freesasa_gpu_dots_count_dev(self._h, d_masks or None, n_atoms, n_points, d_dot_first or None, C.byref(D)):
            raise RuntimeError("freesasa_gpu_dots_count_dev: " + self.error())
        return int(D.value)

    def dots_expand(self, d_xyz, d_radii, n_atoms, d_masks, d_dot_first, capacity, d_dot_xyz, d_dot_atom=0, d_dot_point=0, probe=1.4,
                    n_points=100):
        """freesasa_gpu_dots_expand_dev(): the dots of the masks into d_dot_xyz [capacity, 3] (d_dot_atom, d_dot_point [capacity]
        int32 optional); nothing is written at or beyond slot `capacity`"""
        if lib().freesasa_gpu_dots_expand_dev(self._h, d_xyz or None, d_radii or None, n_atoms, probe, n_points, d_masks or None,
                                              d_dot_first or None, capacity, d_dot_xyz or None, d_dot_atom or None, d_dot_point or None):
            raise RuntimeError("freesasa_gpu_dots_expand_dev: " + self.error())

    def shrake_rupley(self, d_xyz, d_radii, offsets, d_sasa, d_counts=0, d_totals=0, probe=1.4,
                      n_points=100):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if n_points not in self._tp:
            self._tp[n_points] = np.ascontiguousarray(test_points(n_points).reshape(-1))
        tp = self._tp[n_points]
        ret = lib().freesasa_gpu_sr_batch_dev(self._h, d_xyz, d_radii, offsets.ctypes.data_as(_lp),
                                              offsets.size - 1, probe, n_points,
                                              tp.ctypes.data_as(_dp), d_sasa, d_counts or None,
                                              d_totals or None)
        if ret:
            raise RuntimeError("freesasa_gpu_sr_batch_dev: " + self.error())
