/*
 * freesasa_gpu.h — ADDITIVE C-ABI of the MI355X engine (nothing here exists in the
 * reference; freesasa_amd.h stays byte-compatible with the reference's freesasa.h).
 *
 * The reference computes one structure per call (src/freesasa.c:76-120) and parallelises
 * with <= 16 pthreads inside it (src/sasa_lr.c:219-253).  A GPU needs many structures per
 * launch, so the engine's native unit is a BATCH of independent structures in CSR form.
 * Plain pointers and sizes only; no torch / HIP types in any signature (a stream is passed
 * as void*).
 *
 * NUMERIC DOMAIN (what the parity tests prove; north_star's contract is 1e-4 A^2 per atom against the reference).
 * Inputs: finite coordinates and radii (anything else is FREESASA_FAIL with a message, never garbage), radius + probe
 * > 0, at most 2^30 atoms per batch and 2^30 cells (cell edge 2 max(R + probe), ref: src/nb.c:543).
 *   Shrake-Rupley: test-point counts and areas are the reference's bit for bit, for any coordinates and any number of
 *   points (tests/test_gpu_parity.py, tests/test_deep_parity.py: no atom of 1e6 differs).
 *   Lee-Richards, |coordinate| <= 1e5 A (tested to 5e4 A), radii 0.1 .. 30 A, probe 0 .. 5 A, 1 .. 20000 slices:
 *   per-atom |dSASA| <= 1e-8 A^2 on ordinary structures (asserted; measured <= 1e-9 over 6e6 atoms) - slice planes in
 *   closed form for atoms with |z| <= 1024 A, walked exactly as the reference walks them (src/sasa_lr.c:304-307)
 *   beyond, so the accuracy does not depend on the distance from the origin.  Inputs CONSTRUCTED so that two slice
 *   circles are tangent to the last bits - where the reference's own three comparisons and its acos argument disagree
 *   and it returns NaN or a full circle for a covered one (src/sasa_lr.c:324-351) - get the value of the reference
 *   just outside that band: <= 3e-5 A^2 for |z| <= 1024 A, <= 1e-6 beyond (tests/test_adversarial.py).
 *   Two atoms at the same position with equal radii: NaN, as the reference (0 / 0 in its acos argument).
 */
#ifndef FREESASA_GPU_H
#define FREESASA_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct freesasa_gpu_ctx freesasa_gpu_ctx;
struct freesasa_ingest_classifier; /* include/freesasa_ingest.h */

/* Per-call statistics of the last batch run on a context. */
typedef struct freesasa_gpu_stats {
    long long n_atoms;      /* atoms processed */
    long long n_cells;      /* cells of the batch-wide cell list */
    int n_structs;
    int max_neighbors;      /* largest neighbor count of any atom */
    int fallback_tiles;     /* tiles re-done by the large-capacity fallback launch */
    int tile_atoms;         /* launch configuration of the fused kernel */
    int block_threads;
    int lds_bytes;
    double ms_prep;         /* HIP-event time of the cell-sort pipeline (0 unless timing on) */
    double ms_kernel;       /* HIP-event time of the fused L&R / S&R kernel */
    double ms_total;        /* HIP-event time of the whole call on the stream */
} freesasa_gpu_stats;

/* Number of usable HIP devices (0 when there is none; never fails). */
int freesasa_gpu_device_count(void);

/* A context owns one device's workspace.  stream: a hipStream_t to launch on (e.g. torch's
   current stream) or NULL for a private non-blocking stream.  Work is ordered only with respect
   to THAT stream: device inputs produced asynchronously on another stream must be complete
   (synchronise, or create the context on the producing stream).  Returns NULL on failure. */
freesasa_gpu_ctx *freesasa_gpu_ctx_create(int device, void *stream);
void freesasa_gpu_ctx_destroy(freesasa_gpu_ctx *ctx);
/* Record HIP events around the pipeline stages (adds two syncs per call). */
void freesasa_gpu_ctx_set_timing(freesasa_gpu_ctx *ctx, int enable);
void freesasa_gpu_ctx_get_stats(const freesasa_gpu_ctx *ctx, freesasa_gpu_stats *out);
/* Text of the last error on this context ("" if none). */
const char *freesasa_gpu_ctx_last_error(const freesasa_gpu_ctx *ctx);

/* Device-resident batch.  d_* are DEVICE pointers, offsets is a HOST array [n_structs+1]
   (first atom of each structure; offsets[0] == 0).  d_xyz: x1,y1,z1,... (3 * n_atoms),
   d_radii without probe.  d_sasa [n_atoms] per-atom areas in input order; d_totals
   [n_structs] per-structure sums in atom order (may be NULL).  Work is enqueued on the
   context's stream; the call returns after the results are complete on that stream
   (it synchronises the stream once to size the cell list and once to read the status).
   Returns FREESASA_SUCCESS (0) or FREESASA_FAIL (-1). */
int freesasa_gpu_lr_batch_dev(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii,
                              const int64_t *offsets, int n_structs, double probe_radius,
                              int n_slices, double *d_sasa, double *d_totals);
/* The same batch, enqueued only: the call returns as soon as the batch is on the context's stream, so that the host
   side of the next batch (argument checks, launches; and on the device its cell sort) follows the tile kernel of
   this one without a gap.  Up to two batches may be in flight on a context; a third call first collects the oldest.
   The inputs of a batch and its offsets' VALUES must stay valid, and its outputs are complete, only after
   freesasa_gpu_wait (or the call that collects it) has returned 0; a failed batch is reported there, with the
   context's error text.  A batch whose cell table turns out too small (a first, very sparse batch) is redone by the
   collecting call, synchronously.  Results are bit-identical to freesasa_gpu_lr_batch_dev's.  Every synchronous
   entry point of the context collects what is in flight first.  Returns 0 (enqueued) / -1. */
int freesasa_gpu_lr_batch_dev_async(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii,
                                    const int64_t *offsets, int n_structs, double probe_radius,
                                    int n_slices, double *d_sasa, double *d_totals);
/* Collect every batch in flight on the context.  Returns 0, or -1 if one of them failed. */
int freesasa_gpu_wait(freesasa_gpu_ctx *ctx);
/* unit_points: HOST array [3*n_points] of unit test points (generate with
   freesasa_gpu_test_points for bit-exact parity with the reference).  d_counts [n_atoms]
   exposed points per atom (may be NULL).
   Any number of points is accepted (ref: src/sasa_sr.c:56-90, :168-224).  Up to 128 points that are unit vectors (to
   4e-15 in |u|^2: what freesasa_gpu_test_points produces) run the round-6 arrangement: when a context first sees a set of
   points it builds a table of cap masks for them (1.5 MB, a few milliseconds of host time, once per point set), the points
   a neighbor covers are looked up, and only the doubtful (neighbor, point) pairs are put to the reference's test,
   operand for operand (freesasa_amd/csrc/sr_caps.h: counts and areas identical by construction; checked against the
   reference).  Other point sets run the arrangement that tests every point.  The choice changes no result. */
int freesasa_gpu_sr_batch_dev(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii,
                              const int64_t *offsets, int n_structs, double probe_radius,
                              int n_points, const double *unit_points, double *d_sasa,
                              int *d_counts, double *d_totals);

/* Segmented sums of per-atom areas on the device: out[k] = sum of d_sasa[seg[k] .. seg[k+1]) in
   atom order, for k < n_segs.  seg is a HOST array [n_segs+1] of atom offsets (residues, chains
   or structures: the per-residue / per-chain totals that the reference's result tree computes on
   the host, src/node.c:150-176).  d_out [n_segs] is a device pointer.  Returns 0 / -1. */
int freesasa_gpu_segment_sums_dev(freesasa_gpu_ctx *ctx, const double *d_sasa, const int64_t *seg,
                                  int n_segs, double *d_out);

/* Per-structure sums by atom class: d_out[3*s + c] = sum of d_sasa over the atoms of structure s
   whose d_class byte is c (0 apolar, 1 polar, 2 unknown — the reference's freesasa_atom_class,
   src/freesasa.h:163-167; what freesasa_result_classes adds up on the host,
   src/classifier.c:830-866, and the CLI prints as Apolar / Polar).  offsets is a HOST array
   [n_structs+1]; d_class [n_atoms] and d_out [3*n_structs] are device pointers.  Returns 0 / -1. */
int freesasa_gpu_class_sums_dev(freesasa_gpu_ctx *ctx, const double *d_sasa, const unsigned char *d_class,
                                const int64_t *offsets, int n_structs, double *d_out);

/* Per-residue areas as the reference's result tree holds them (freesasa_nodearea of a residue node,
   src/node.c:717-764): d_abs[6*r + {0..5}] = total, main chain, side chain, polar, apolar, unknown,
   summed in atom order over residue r = atoms [res_first[r], res_first[r+1]); and, if d_rel is not
   NULL, the relative areas of the RSA output (src/rsa.c:14-25): d_rel[5*r + {0..4}] =
   100 * {total, main chain, side chain, polar, apolar} / reference, NaN where the residue has no
   reference values (ref_row[r] < 0; the reference prints N/A).  d_class / d_backbone [n_atoms] are
   device byte arrays (freesasa_ingest_batch.atom_class / .atom_backbone); res_first [n_res+1],
   ref_row [n_res] (freesasa_ingest_batch.res_ref) and ref_table [5*ref_rows]
   (freesasa_ingest_residue_reference_table) are HOST arrays.  Returns 0 / -1. */
int freesasa_gpu_residue_areas_dev(freesasa_gpu_ctx *ctx, const double *d_sasa, const unsigned char *d_class,
                                   const unsigned char *d_backbone, const int64_t *res_first, int n_res,
                                   const short *ref_row, const double *ref_table, int ref_rows,
                                   double *d_abs, double *d_rel);

/* Golden-spiral unit test points on the host, host libm (src/sasa_sr.c:56-90). */
void freesasa_gpu_test_points(int n_points, double *unit_points);

/* The same over several GPUs of the node from one process: the structures are cut into contiguous runs
   of about equal atom count (freesasa_gpu_shard_cuts), one per entry of devices[] — a device may
   appear more than once, its runs then overlap their copies and kernels — each run on its own host
   thread, context and stream; no exchange between devices (independent structures).  Arrays as in
   freesasa_gpu_calc_batch.  _multi takes a bit mask instead (bit d = device d).  Return 0 / -1. */
int freesasa_gpu_calc_batch_devices(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                    int alg, double probe_radius, int resolution, double *sasa_out, int *counts_out,
                                    double *totals_out, const int *devices, int n_devices, char *err, int err_len);
int freesasa_gpu_calc_batch_multi(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                  int alg, double probe_radius, int resolution, double *sasa_out, int *counts_out,
                                  double *totals_out, unsigned device_mask, char *err, int err_len);
/* Host arrays in, host arrays out, with the PCIe copies under the kernels: the batch is cut into chunks of whole
   structures (about chunk_atoms atoms, <= 0: 1.25e6) that n_lanes host threads (<= 0: 3 for page-locked arrays, 4 for
   pageable ones; at most 8) take from a
   shared counter, each lane on its own pooled context and stream, so that the upload of one chunk, the kernels of
   another and the download of a third overlap.  Page-locked caller arrays (hipHostMalloc / hipHostRegister, a
   pinned tensor) are copied by DMA in place; pageable ones go through page-locked staging buffers of the lanes.
   Arrays and results as in freesasa_gpu_calc_batch (bit-identical: chunks are independent structures).
   Return 0 / -1. */
int freesasa_gpu_calc_batch_pipelined(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                      int alg, double probe_radius, int resolution, double *sasa_out, int *counts_out,
                                      double *totals_out, int device, int n_lanes, long long chunk_atoms,
                                      char *err, int err_len);
int freesasa_gpu_trajectory_file(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                                 int n_atoms, long long n_frames, int alg, double probe_radius, int resolution,
                                 int frames_per_batch, const char *totals_path, const char *sasa_path, const char *done_path,
                                 long long max_new_shards, int device, long long *frames_total_out, char *err, int err_len);

/* The host-pointer entries (freesasa_calc_coord, freesasa_gpu_calc_batch*, _trajectory, _sweep_files) keep their
   contexts — stream, device workspace, staging buffers — in a pool between calls.  This destroys the idle ones and
   returns their device memory. */
void freesasa_gpu_release_pool(void);

/* Test hook: fault injection.  The n-th device or page-locked-host allocation made by this library from now on
   fails (n <= 0: off), the way the reference's test suite makes its n-th malloc fail (tests/tools.c:10-48,
   tests/test_freesasa.c:475-514): every entry point must then return its failure value with a message, leave
   nothing running on its stream, and work again on the next call. */
void freesasa_gpu_test_fail_after(int n);
/* ... and its HOST-side twin: the n-th allocation (malloc / calloc / realloc of the C sources, operator new of the C++
   sources) or thread creation of the library's own host code from now on fails - the loaders (freesasa_ingest_*), the
   cache reader, the selection parser, freesasa_calc / result_new and every driver below.  n <= 0: off.  Returns what
   was left of the previous countdown (0: it fired, or was not armed).  Every extern "C" entry point catches what its
   C++ code throws (std::bad_alloc, std::system_error from a thread that does not start) and returns its failure value
   with a message: no exception crosses this boundary (ref: src/util.c:89-113, "never exit()"). */
int freesasa_host_test_fail_after(int n);
/* Test hook: the mapping behind the drivers' NUMA placement (a lane, its page-locked staging and its loader threads run on
   the CPUs of the socket its GPU hangs off; FREESASA_AMD_NO_AFFINITY=1 turns it off): the CPUs of the NUMA node of the PCI
   device `pci_address` ("0000:c1:00.0", as hipDeviceGetPCIBusId names it) under the sysfs tree `sysfs_root` ("/sys"; a
   made-up tree in the tests).  Returns how many CPUs the node has (the first `cap` are stored in cpus_out), 0 when the
   platform names no node for the device (numa_node -1), -1 when the tree cannot be read. */
int freesasa_gpu_test_node_cpus(const char *sysfs_root, const char *pci_address, int *cpus_out, int cap);

/* Test hooks: the integer / exact parts of the Lee-Richards kernel, run on the device on their own.
   _lr_neighbors_dev: the neighbor sets it finds (what freesasa_nb_new builds, src/nb.c:524-557; the reference's
   tests/test_nb.c): d_nn[n] = neighbors per atom, d_nb[n * nb_cap] (may be NULL) = the first nb_cap neighbors of
   every atom (original indices); device pointers, original atom order.
   _arc_union_dev: exposed arc length of n_sets (<= 64) sets of arcs given as (start, end) pairs in [0, 2 pi]
   (set k = pairs first[k] .. first[k+1]), through the kernel's arc union and sweep (exposed_arc_length,
   src/sasa_lr.c:389-408; its KATs :455-475); host arrays.  Return 0 / -1. */
int freesasa_gpu_lr_neighbors_dev(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                                  int n_structs, double probe_radius, int *d_nn, int *d_nb, int nb_cap);
int freesasa_gpu_arc_union_dev(freesasa_gpu_ctx *ctx, const double *arcs, const int *first, int n_sets, double *out);
/* Test hooks: the arithmetic and the lane primitives that are defined one way for the device and another for the CPU
   emulation of the kernels (hardware seeds, inline assembly, data-parallel scans, mbcnt, ballot, readlane, 24-bit products)
   and the functions built on the seeds, run on the device on their own: known-answer kernels that call the product's own
   macros and functions (csrc/kat_kernels.h, which numbers the ops and says what each reads and writes).  Host arrays.
   _kat_elementwise_dev: n operands (1 .. 2^20), a thread each in workgroups of 256: thread i reads a[i], b[i], c[i] - those the
   op takes; the others may be NULL - and the scalar k (a kernel argument: it sits in scalar registers), writes out0[i] and
   out1[i] - those the op gives.
   _kat_wave_dev: `rows` (1 .. 4096) rows of 64 64-bit words through ONE full wave, every lane active in every cross-lane
   operation; lane l of row r reads in[64 r + l] and writes out[64 r + l].
   Return 0, or -1 with the context's error text; refused before any device call: "unknown op ...", "n must be ...", "rows
   must be ...", "null argument", a shuffle's source lane beyond 63, an operand beyond the range of lr2_div9 / lr2_div3, an
   odd number of rows for the 64-bit shuffle.  tests/test_device_arith_gpu.py holds every op to exact or extended-precision
   references through them (tests/device_arith_ref.py), tests/test_device_arith.py the CPU definitions to the same. */
int freesasa_gpu_kat_elementwise_dev(freesasa_gpu_ctx *ctx, int op, const double *a, const double *b, const double *c, long long n, double k,
                                     double *out0, double *out1);
int freesasa_gpu_kat_wave_dev(freesasa_gpu_ctx *ctx, int op, const uint64_t *in, int rows, uint64_t *out);
/* Test hook: the two XTC decode kernels (xtc_scan, xtc_unpack: "GROMACS XTC input" below) run on the device on their own, by the
   launches the file drivers make for a shard.  Host arrays: `bytes` is n_frames whole frames of n_atoms atoms, one behind the
   other, as a file holds them (len bytes); their descriptors are made as the drivers make them (freesasa_gpu_xtc_frame_desc, the
   stream at the frame's byte + FREESASA_GPU_XTC_HEADER).  rec [n_frames * n_atoms * 4]: per frame and group (bit offset, first
   atom, run, smallidx), zero where the scan wrote none; count [n_frames * 2]: per frame (groups, status; 0 is good, the bits are
   xtc_kernels.h's XTC_ST_*); out [n_frames * n_atoms * 3]: fp32 Angstrom, all-ones bytes (NaN) where no thread wrote.  Returns 0,
   or -1 with the context's error text: "frame K of the XTC bytes: <the host's reason>" for a header the host refuses, and - before
   any device call; freesasa_gpu_xtc_decode_check is that part alone, host only, the message in err - "xtc_decode: ..." for a null
   pointer, n_frames, n_atoms or len below 1, or n_frames * n_atoms beyond an int.  Device and page-locked memory are the
   context's workspace (freesasa_gpu_test_fail_after reaches them).  Through it tests/test_xtc_decode_gpu.py pins the device
   decode group by group to the pure-Python codec: every path of the format (runs 0 to 8, forced flags, inherited runs, smallidx
   held at 9 and at 72, bitsize 0 with runs) alone and as the frames of one shard, every padding, the scan's window as it moves
   (a group that ends on the window's last bit, a hop by every excess of 1 to 6 bits, flags at bit 0 and bit 31 of a word), 600
   frames in one launch, integers beyond 2^24 at four precisions and the widest dimensions a header may hold, and the status
   word of damaged streams. */
int freesasa_gpu_xtc_decode_dev(freesasa_gpu_ctx *ctx, const void *bytes, long long len, int n_frames, int n_atoms, int32_t *rec,
                                int32_t *count, float *out);
int freesasa_gpu_xtc_decode_check(const void *bytes, long long len, int n_frames, int n_atoms, const int32_t *rec, const int32_t *count,
                                  const float *out, char *err, int err_len);
/* Test hook: the cell sort - the first stage of every batch - run on the device on its own, by the engine's own launches.
   d_xyz, d_radii (device), offsets (host), n_structs and probe_radius as freesasa_gpu_lr_batch_dev takes them.
   arrangement: 0 the general pipeline (k_prep_general, k_count, k_scan, k_scatter) with the dense table, 1 k_sort_struct (one
   workgroup per structure) with the dense table, 2 k_sort_struct with the compact table.  It is forced: what the engine would
   choose for the batch (structure sizes, n_structs, the environment switches, what the context has learnt) is not consulted,
   so the kernels' own refusals can be seen.  cells_cap: the cells the table has room for; 0: the engine's sizing of a first
   batch (10 n + 256 n_structs, raised to what the context has seen) - freesasa_gpu_cell_sort_cap says which number that is (it
   returns cells_cap itself when that is positive, -1 for arguments the hook refuses; it collects batches in flight first, as
   the hook does, since collecting one raises what the context has seen): the table arrays below are sized with it, and the
   caller says so in table_cells - a pass that would take another number of cells is refused ("the table arrays are sized for
   ...") and copies nothing.  shared_radii (0 / 1): d_radii holds ONE structure's radii, used by every structure (the trajectory path's addressing).
   ONE pass: whatever the status words say - an error, "redo with a larger table" (ST_RETRY bit 0), "not a batch for
   k_sort_struct" (bit 1) - nothing is redone, and the context's learnt state (the choice of the sort, the table sizing, the
   launch-shape hints) stays as it was; what a pass with ST_ERROR or ST_RETRY set leaves in the arrays is not a result.
   Before the first launch grid, ncells, sq, s_idx and the table are filled with all-ones bytes: an entry no kernel wrote reads
   as -1 (NaN in sq).  Host arrays out:
     status [FREESASA_GPU_CELL_SORT_STATUS_WORDS] the batch's status words (sasa_kernels.h ST_*: ST_ERROR 0, ST_OCC_SUM 4,
                 ST_OCC_N 5, ST_RETRY 7, the 64-bit cell total ST_CELLS at words 140-141);
     occ_stride  every occ_stride-th atom is a density sample (n / 256, at least 1);
     grid [n_structs] records of 48 bytes: x0, y0, z0, d (doubles), nx, ny, nz, cell_base (int32);
     ncells [n_structs] int64;
     sq [4 n] x, y, z, radius + probe of the atoms in cell-sorted order;
     s_idx [n] records of 16 bytes: cell (int64: batch-wide cell | (border flags | cell_pack_grid) << 32), orig, strct (int32);
     arrangements 0 and 1: cell_start [cells_cap + 2] (cell_tbl, cell_first may be NULL);
     arrangement 2: cell_tbl [(cells_cap >> 5) + 2] and cell_first [n + n_structs + 2] (cell_start may be NULL).
   Returns 0, or -1 with the context's error text; refused before any device call, with run_batch's wording where the condition is
   the same: "null argument", "n_structs must be > 0", "offsets[0] must be 0", "offsets must be non-decreasing", "empty batch",
   "unknown arrangement ...", "cells_cap must not be negative".  Batches in flight are collected first; device memory is the
   context's workspace (freesasa_gpu_test_fail_after reaches it).  tests/test_cell_sort_gpu.py holds all three arrangements to
   a numpy reference through it (tests/cell_sort_ref.py). */
#define FREESASA_GPU_CELL_SORT_STATUS_WORDS 142
int freesasa_gpu_cell_sort_dev(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                               double probe_radius, int arrangement, long long cells_cap, long long table_cells, int shared_radii, int32_t *status,
                               int32_t *occ_stride, void *grid, int64_t *ncells, double *sq, void *s_idx, int32_t *cell_start,
                               uint64_t *cell_tbl, int32_t *cell_first);
long long freesasa_gpu_cell_sort_cap(freesasa_gpu_ctx *ctx, long long n_atoms, int n_structs, long long cells_cap);
/* cuts[0..n_parts]: first structure of every run for the partition above (host-only helper) */
void freesasa_gpu_shard_cuts(const int64_t *offsets, int n_structs, int n_parts, int *cuts);

/* Structure sweep (BASELINE configs[3]): PDB / mmCIF files -> per-structure totals.  The files are
   read in batches of about batch_atoms atoms (<= 0: 1e6) by n_threads host threads
   (include/freesasa_ingest.h; ingest_options are its option bits) while the previous batch is on
   the GPU.  totals_out[n_paths]; class_sums_out[3*n_paths] (apolar, polar, unknown) and
   atoms_out[n_paths] may be NULL; status_out[n_paths] receives the loader's per-input status
   (non-zero: the input contributed nothing and its total is 0).  alg: 0 Lee-Richards (resolution =
   slices), 1 Shrake-Rupley (test points).  Returns 0, or -1 on a GPU error (message in err). */
int freesasa_gpu_sweep_files(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                             int alg, double probe_radius, int resolution, long long batch_atoms,
                             double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                             int device, char *err, int err_len);

/* The same sweep with a done-list (see freesasa_gpu_trajectory_file): done_path holds a first line with the sweep's
   parameters and one line "shard <batch> <first file> <files>" per finished batch; <done_path>.bin holds the
   results of the finished batches (per file a 48-byte record: total, three class sums, atoms, status), written
   before the batch is listed.  A later call with the same files and parameters takes the listed batches' results
   from there and computes only the others.  max_new_batches > 0: stop after that many batches.
   Returns 0 done, 1 stopped early, -1 error. */
int freesasa_gpu_sweep_files_resumable(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                       int alg, double probe_radius, int resolution, long long batch_atoms,
                                       double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                       const char *done_path, long long max_new_batches, int device, char *err, int err_len);

/* The drivers over a LIST of devices of the node (BASELINE configs[3] "sharded across 8 x MI355X", configs[4] "frames
   sharded 8 x MI355X with per-frame stream-out"), from one process.  Work units — batches of files, shards of frames —
   are independent, so there is no exchange between devices: the workers of all devices take units from one shared
   list (the file sweep: largest batch first, LPT on the file sizes), every result lands at its own place (the caller's
   arrays; pwrite at the unit's offset of the result files) and ONE done-list serves all devices, so a run interrupted
   on eight devices can be finished on one (or the other way round) with the same files byte for byte.  devices[]: 1 to
   64 entries, each an existing device, repeats allowed (the entries of one device overlap their copies and kernels; a
   one-GPU box runs [0, 0, 0]).  The host threads the CGROUP grants (freesasa_ingest_usable_cpus) are divided among the
   devices' loaders / lanes.  Results are bit-identical to the single-device drivers', which are these with one entry.
   _sweep_files_devices: as freesasa_gpu_sweep_files_resumable (done_path may be NULL, max_new_batches <= 0: all).
   _sweep_cache_devices: the sweep of a binary cache (freesasa_ingest_save): lanes_per_device threads per device
   (<= 0: the granted CPUs divided by the devices, 2 .. 8; batch_atoms <= 0: 1e6) read, VERIFY (1 MiB piece checksums) and upload exactly the
   coordinates, radii and classes of their batch through page-locked staging; n_out = length of the output arrays
   (>= the cache's structure count); class_sums_out / atoms_out / status_out may be NULL.  Returns 0 / -1.
   _trajectory_devices, _trajectory_file_devices: as freesasa_gpu_trajectory / _trajectory_file. */
/* ingest_options | FREESASA_INGEST_PARSE_ON_DEVICE (include/freesasa_ingest.h): the files' text is parsed ON THE DEVICE (round 6;
   the host reads bytes, kernels do what src/structure.c:644-722, src/pdb.c:176-283, src/cif.cc:113-240, src/classifier.c:781-796
   do); results are those of the host parser bit for bit, files the device refuses are read by it.  _sweep_parse_stats: files
   parsed on the device / by the host in this process's sweeps since the last call. */
void freesasa_gpu_sweep_parse_stats(long long *device_files, long long *host_files);
/* The device-side parser on its own: n files -> coordinates [3 * atoms], radii, classes of the atoms it keeps (host arrays with
   room for `cap` atoms; each may be NULL), offsets_out [n + 1], status_out [n] (FREESASA_INGEST_* codes), host_out [n] (1: the
   device refuses the file, which then contributes nothing here; the sweep hands such a file to the host parser).  Returns the
   atoms written, -1 on error, -2 when cap is too small (offsets_out[n] = atoms needed). */
long long freesasa_gpu_parse_files(const char *const *paths, int n_paths, int ingest_options, int n_threads, int device,
                                   double *xyz_out, double *radii_out, unsigned char *class_out, long long cap,
                                   long long *offsets_out, int *status_out, int *host_out, char *err, int err_len);
int freesasa_gpu_sweep_files_devices(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                     int alg, double probe_radius, int resolution, long long batch_atoms,
                                     double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                     const char *done_path, long long max_new_batches, const int *devices, int n_devices,
                                     char *err, int err_len);
/* The file sweep and the device-side parser with a user classifier (include/freesasa_ingest.h,
   freesasa_ingest_classifier_from_file: the reference's -c configuration files) in place of ProtOr: the arguments of
   freesasa_gpu_sweep_files_devices / freesasa_gpu_parse_files and the classifier; classifier NULL: exactly those entries.
   The host parser (the loader threads, and the files the device refuses) and the device parser (its table uploaded with
   every batch into the context's own buffer; a table of more than 16384 rows is not taken: the batch's files then go to
   the host parser and count as such in freesasa_gpu_sweep_parse_stats) both classify with it.  Radii and classes - and
   so totals and class sums - are those of the reference under that classifier; the done-list's first line names it
   (" classifier=<digest>", freesasa_ingest_classifier_digest): a done-list written under another classifier, or under
   none, belongs to other parameters and is refused, and one written without a classifier keeps its old first line. */
int freesasa_gpu_sweep_files_classified(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                        int alg, double probe_radius, int resolution, long long batch_atoms,
                                        double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                        const char *done_path, long long max_new_batches, const int *devices, int n_devices,
                                        const struct freesasa_ingest_classifier *classifier, char *err, int err_len);
long long freesasa_gpu_parse_files_classified(const char *const *paths, int n_paths, int ingest_options, int n_threads, int device,
                                              double *xyz_out, double *radii_out, unsigned char *class_out, long long cap,
                                              long long *offsets_out, int *status_out, int *host_out,
                                              const struct freesasa_ingest_classifier *classifier, char *err, int err_len);
/* The file sweep with a PER-RESIDUE table: what the reference prints with --format=rsa / --format=seq (src/rsa.c:14-25,
   src/node.c:717-764), for all files of a sweep in one call.  The arguments of freesasa_gpu_sweep_files_classified without
   done_path and max_new_batches; totals, class sums, atom counts and status come back exactly as that entry gives them, and
   table_out receives one table for all files: file k owns residues [res_offsets[k], res_offsets[k + 1]) - none if it failed -
   in the file's order, whatever the devices, workers or the batch cut.  Per residue: its atoms, the row of the reference-area
   table (freesasa_ingest_residue_reference_table; -1: none), abs[6 r + ..] = total, main chain, side chain, polar, apolar,
   unknown and rel[5 r + ..] = 100 * abs / reference (NaN where res_ref < 0) as freesasa_gpu_residue_areas_dev computes them,
   and the labels in the byte layout of freesasa_ingest_batch.  classifier NULL: ProtOr; a user classifier: res_ref -1 and rel
   NaN throughout (a configuration file has no reference areas; the reference's CLI drops its REL columns under -c,
   src/main.cc:729-730).  The per-atom areas never leave the device: the residue sums are taken there, and with
   FREESASA_INGEST_PARSE_ON_DEVICE the residues themselves - boundaries, labels, reference rows, backbone flags - are built on
   the device by the host loader's rules (csrc/gpu_parse.hip); files the device refuses are read by the host parser as in
   every sweep.  The table's arrays are ONE block, released by freesasa_gpu_residue_table_free only (which zeroes the struct;
   a zeroed struct is a no-op); on any failure (-1, message in err) the struct is zeroed and nothing is kept.
   Not offered: a done-list / resumable form (records of variable length need a file format of their own), the cache sweep
   (a cache read brings coordinates, radii and classes, no residue arrays).  (Per-residue output of the trajectory drivers:
   freesasa_gpu_trajectory_topology below.) */
typedef struct freesasa_gpu_residue_table {
    int32_t n_files;
    int64_t n_residues;
    int64_t *res_offsets;  /* [n_files + 1] */
    int32_t *res_atoms;    /* [n_residues] atoms of the residue */
    int16_t *res_ref;      /* [n_residues] row of the reference-area table, -1: none */
    double *abs;           /* [6 * n_residues] */
    double *rel;           /* [5 * n_residues] */
    char *res_name, *res_number, *res_chain; /* [4 | 6 | 4 bytes per residue], as in freesasa_ingest_batch */
} freesasa_gpu_residue_table;
int freesasa_gpu_sweep_files_residues(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                      int alg, double probe_radius, int resolution, long long batch_atoms,
                                      double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                      const int *devices, int n_devices, const struct freesasa_ingest_classifier *classifier,
                                      freesasa_gpu_residue_table *table_out, char *err, int err_len);
void freesasa_gpu_residue_table_free(freesasa_gpu_residue_table *table);
/* SELECTION AREAS on the device: the reference's --select (src/selection.c:683-742) for a set of up to 64 selections compiled
   once (freesasa_ingest_selection_compile, include/freesasa_ingest.h).  A kernel runs the set's program for every atom - its
   name and element symbol, the number, chain and name labels of its residue (the residue's first atom's, as
   freesasa_ingest_select reads them), its structure's first and last residue number for the open ranges - and leaves one
   64-bit word per atom, bit k = selection k holds it; a second kernel sums the per-atom areas under every mask per
   structure, in the order of the class sums: an area equals element [1] of freesasa_gpu_class_sums_dev with the
   selection's 0/1 mask as class, bit for bit.
   _select_batch: a LOADED batch and per-atom areas the caller holds on the host (e.g. from freesasa_gpu_calc_batch) ->
   area_out / atoms_out [n_structs * n_sel] (structure-major: the area and the number of selected atoms; 0 for a structure
   without atoms, as freesasa_ingest_select returns 0 for it) and, unless NULL, bits_out [n_atoms], the mask words.
   Labels, keys and areas go up, the kernels run, the results come back; on a pooled context of `device` (-1: any).
   _sweep_files_select: the file sweep with selections - the arguments of freesasa_gpu_sweep_files_residues with a selection
   set in place of the table.  Totals, class sums, atom counts and status are exactly freesasa_gpu_sweep_files_classified's;
   sel_area_out / sel_atoms_out [n_paths * n_sel] are file-major, 0 for a file that failed to load or kept no atoms.  The
   per-atom areas never leave the device: the two kernels run behind the batch's tile kernels on its stream and their
   results ride in front of the batch's one synchronisation.  With FREESASA_INGEST_PARSE_ON_DEVICE the atoms' keys and the
   residues are built on the device (csrc/gpu_parse.hip: kp_atom_keys, kp_res_*); files the host parser read - all of them
   without that option, the refused ones with it - have theirs uploaded (8 bytes per atom, 22 per residue).
   Both return 0 / -1 with the message in err.
   Not offered: a done-list / resumable form, the cache sweep (a cache read brings no names or residue arrays).  (Selections
   in the trajectory drivers: freesasa_gpu_trajectory_topology below.) */
struct freesasa_ingest_selection;
struct freesasa_ingest_batch;
int freesasa_gpu_select_batch(const struct freesasa_ingest_batch *batch, const struct freesasa_ingest_selection *sel,
                              const double *sasa, double *area_out, long long *atoms_out, unsigned long long *bits_out,
                              int device, char *err, int err_len);
int freesasa_gpu_sweep_files_select(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                    int alg, double probe_radius, int resolution, long long batch_atoms,
                                    double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                    const int *devices, int n_devices, const struct freesasa_ingest_classifier *classifier,
                                    const struct freesasa_ingest_selection *sel,
                                    double *sel_area_out, long long *sel_atoms_out, char *err, int err_len);
/* CHAIN GROUPS in the file sweep: the reference's --chain-groups / --separate-chains (src/main.cc:261-312) for all files of a
   sweep in one call - how much area every group of chains of every file exposes on its own, in its complex, and buries.
   _sweep_files_groups: the arguments of freesasa_gpu_sweep_files_select up to `classifier`, then spec and group_flags as
   freesasa_ingest_chain_groups takes them (include/freesasa_ingest.h: the short or the long syntax, or spec NULL with
   FREESASA_INGEST_SEPARATE_CHAINS).  A bad character, an empty group, overlapping groups, both or neither of spec and
   separate chains, unknown flags are call errors with that function's messages (its own code parses the spec), reported
   before a device is touched or a file read.  Totals, class sums, atom counts and status are exactly
   freesasa_gpu_sweep_files_classified's.  group_status_out [n_paths]: the loader's status, or FREESASA_INGEST_EGROUP (a chain
   the spec names is missing, or more than 65535 separate chains); a file whose group status is not 0 owns no rows of the
   table - an EGROUP file keeps its total, class sums and atom count.  table_out: file k owns groups [group_offsets[k],
   group_offsets[k + 1]) in the spec's order (separate chains: in the file's); per group its atoms, areas[3 g + ..] = isolated,
   complex, buried (the columns of freesasa_gpu_groups_dev's d_group_totals) and chain[4 g ..], 4 bytes as res_chain holds
   them: the run's label with separate chains, else the first label the spec names for the group.
   The per-atom group ids are made ON THE DEVICE (csrc/group_kernels.h, k_gid_struct: one wave per structure over its
   residues) from residue boundaries and chain labels that are there - with FREESASA_INGEST_PARSE_ON_DEVICE the device
   parser's, the host parser's files' uploaded behind them (12 bytes per residue) - and neither they nor any per-atom area
   leave it: per batch the structures' group counts and status and the groups' atom counts come back (they size the combined
   batch of freesasa_gpu_groups_dev's pipeline), then 24 bytes per group and, with separate chains, its label.
   The table's arrays are ONE block, released by freesasa_gpu_group_table_free only (which zeroes the struct; a zeroed struct
   is a no-op); on any failure (-1, message in err) the struct is zeroed and nothing is kept.
   _chain_group_ids: the ids kernel alone on a LOADED batch, the twin of freesasa_ingest_chain_groups with the same outputs
   (group_out [n_atoms], n_groups_out and status_out [n_structs]): offsets, residue boundaries, chain labels and status go up,
   the three arrays come back; on a pooled context of `device` (-1: any).  0 / -1 with the message in err.
   Not offered: a done-list / resumable form (records of variable length), the cache sweep (a cache read brings no residue
   arrays).  (Chain groups in the trajectory drivers: freesasa_gpu_trajectory_groups below.) */
typedef struct freesasa_gpu_group_table {
    int32_t n_files;
    int64_t n_groups;
    int64_t *group_offsets; /* [n_files + 1]: file k owns groups [group_offsets[k], group_offsets[k + 1]) */
    int32_t *group_atoms;   /* [n_groups] */
    double *areas;          /* [3 * n_groups]: isolated, complex, buried */
    char *chain;            /* [4 * n_groups] */
} freesasa_gpu_group_table;
int freesasa_gpu_sweep_files_groups(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                    int alg, double probe_radius, int resolution, long long batch_atoms,
                                    double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                    const int *devices, int n_devices, const struct freesasa_ingest_classifier *classifier,
                                    const char *spec, int group_flags, int *group_status_out,
                                    freesasa_gpu_group_table *table_out, char *err, int err_len);
void freesasa_gpu_group_table_free(freesasa_gpu_group_table *table);
/* INTERFACES BETWEEN CHAIN GROUPS in the file sweep: every interface of every file of a sweep in one call - which groups of
   chains bury each other, by how much, of which polar / apolar make-up, through which residues (the batch entries:
   freesasa_gpu_interfaces_dev and freesasa_gpu_interface_residues_dev below).
   _sweep_files_interfaces: the arguments of freesasa_gpu_sweep_files_groups up to group_status_out and table_out (the group
   table may be NULL here), then residue_rows, min_buried, iface_status_out [n_paths] and itable_out.
   Totals, class sums, atom counts, status, group status and the group table are byte for byte those of
   freesasa_gpu_sweep_files_groups with the same arguments.
   iface_status_out[k]: the group status of the file where that is not 0; else FREESASA_GPU_EIFACE_GROUPS for a file with more
   than 4096 groups (the interface entries' limit: such a file keeps its totals and its rows of the group table, and the other
   files of its batch are not affected); else 0.  A file whose interface status is not 0 owns no rows of the interface table.
   itable_out: file k owns pairs [pair_offsets[k], pair_offsets[k + 1]), in file order and within a file in the pair order of
   freesasa_gpu_interfaces_dev (g < h, the tests' order), whatever the devices, the workers or the batch cut.  Per pair p:
   pair_groups[2 p ..] indices into the file's rows of the group table, pair_atoms[2 p ..] the atoms of the two sides,
   pair_chain[8 p ..] both groups' 4-byte labels as the group table holds them, pair_areas[6 p ..] the six areas of
   freesasa_gpu_interfaces_dev, pair_class_buried[6 p ..] per side the buried area split as apolar, polar, unknown (the class
   order of freesasa_gpu_class_sums_dev).  With residue_rows != 0 also the per-residue table of
   freesasa_gpu_interface_residues_dev (else those pointers are NULL and n_res_rows is 0): res_offsets [2 n_pairs + 1] rows per
   side, and per row res_index, res_atoms, res_areas[3 r ..] and the residue's labels res_name / res_number / res_chain at
   4 | 6 | 4 bytes; a row exists for a residue segment of a side whose buried area is > min_buried.  res_index is the residue's
   place among the residues of ITS FILE: the row of the file's block in freesasa_gpu_sweep_files_residues' table.
   Every area equals, bit for bit, what freesasa_gpu_calc_interface_residues gives on that file alone, loaded with
   freesasa_ingest_pdb_files_ex and cut with freesasa_ingest_chain_groups (the engine's results do not depend on the batch, and
   the residue sums are taken in strict atom order); pair_class_buried of side q is freesasa_gpu_class_sums_dev over pair_buried
   with the class atom_class[pair_atom[m]] and side_offsets as the structures' offsets, bit for bit.
   Refused before a device is touched or a file read: what freesasa_gpu_sweep_files_groups refuses, with its messages;
   min_buried not finite or < 0 (the per-residue entry's message); a NULL itable_out or iface_status_out.  The call fails
   when ONE BATCH needs more than 2^27 pair tests or more than 2^30 atoms (the batch, its groups and its pair structures
   together): the message names the batch's first and last file and says to lower batch_atoms; when the call succeeds its
   results never depend on the batch cut.
   The pipeline is the batch entries' (csrc/gpu_interfaces.hip), run ONCE per batch with capacities that hold anything: P, M
   and R size the batch's block afterwards.  Residue boundaries are the ones the sweep holds on the device; nothing per atom
   leaves it.  Two kernels of its own (csrc/ifsweep_kernels.h): the classes of the pair structures' atoms, and the rows' place
   in their file with their labels.
   The table's arrays are ONE block, released by freesasa_gpu_interface_table_free only (which zeroes the struct; a zeroed struct
   is a no-op); on any failure (-1, message in err) both tables are zeroed and nothing is kept.
   Not offered: a done-list / resumable form, the cache sweep, contact tables in the sweep, interfaces among periodic images
   (interfaces per frame of a trajectory: freesasa_gpu_trajectory_interfaces below). */
#define FREESASA_GPU_EIFACE_GROUPS 100 /* (no FREESASA_INGEST_* status: those are 0 .. 8) */
typedef struct freesasa_gpu_interface_table {
    int32_t n_files;
    int64_t n_pairs, n_res_rows;
    int64_t *pair_offsets;     /* [n_files + 1] */
    int32_t *pair_groups;      /* [2 * n_pairs] */
    int32_t *pair_atoms;       /* [2 * n_pairs] */
    char *pair_chain;          /* [8 * n_pairs] */
    double *pair_areas;        /* [6 * n_pairs] */
    double *pair_class_buried; /* [6 * n_pairs] */
    int64_t *res_offsets;      /* [2 * n_pairs + 1] */
    int32_t *res_index;        /* [n_res_rows] */
    int32_t *res_atoms;        /* [n_res_rows] */
    double *res_areas;         /* [3 * n_res_rows]: isolated, in the pair, buried */
    char *res_name, *res_number, *res_chain; /* [4 | 6 | 4 per row] */
} freesasa_gpu_interface_table;
int freesasa_gpu_sweep_files_interfaces(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                        int alg, double probe_radius, int resolution, long long batch_atoms,
                                        double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                        const int *devices, int n_devices, const struct freesasa_ingest_classifier *classifier,
                                        const char *spec, int group_flags, int *group_status_out,
                                        freesasa_gpu_group_table *table_out, int residue_rows, double min_buried,
                                        int *iface_status_out, freesasa_gpu_interface_table *itable_out, char *err, int err_len);
void freesasa_gpu_interface_table_free(freesasa_gpu_interface_table *table);
int freesasa_gpu_chain_group_ids(const struct freesasa_ingest_batch *batch, const char *spec, int flags, int32_t *group_out,
                                 int32_t *n_groups_out, int32_t *status_out, int device, char *err, int err_len);
int freesasa_gpu_sweep_cache_devices(const char *cache_path, int alg, double probe_radius, int resolution, long long batch_atoms,
                                     double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out, int n_out,
                                     const int *devices, int n_devices, int lanes_per_device, char *err, int err_len);
int freesasa_gpu_trajectory_devices(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                                    int alg, double probe_radius, int resolution, int frames_per_batch,
                                    double *totals_out, double *sasa_out, const int *devices, int n_devices,
                                    char *err_out, int err_len);
int freesasa_gpu_trajectory_file_devices(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                                         int n_atoms, long long n_frames, int alg, double probe_radius, int resolution,
                                         int frames_per_batch, const char *totals_path, const char *sasa_path, const char *done_path,
                                         long long max_new_shards, const int *devices, int n_devices,
                                         long long *frames_total_out, char *err, int err_len);

/* Host-pointer batch on a pooled per-thread context of `device` (-1: current default).
   alg/probe/resolution as in freesasa_parameters; counts_out may be NULL (S&R only);
   totals_out may be NULL.  Thread-safe.  Returns 0 / -1; message via err_out (>= len 1). */
int freesasa_gpu_calc_batch(const double *xyz, const double *radii, const int64_t *offsets,
                            int n_structs, int alg, double probe_radius, int resolution,
                            double *sasa_out, int *counts_out, double *totals_out,
                            int device, char *err_out, int err_len);

/* Periodic images: every structure s has an orthorhombic cell L = cells[3 s .. 3 s + 2] of its own.  With
   c = 2 (max radius of the structure + probe_radius), the largest distance at which two of its atoms can be neighbours:
     requirement   L finite and L[a] >= c on every axis (first-shell images then suffice); anything else is refused (-1 with a
                   message that names the structure and the edge), never approximated
     wrap          w[i][a] = x[i][a] - L[a] * floor(x[i][a] / L[a]), fp64
     images        on axis a atom i admits shift 0 always, +1 when w[i][a] < c, -1 when w[i][a] > L[a] - c; its images are the
                   admitted (sx, sy, sz) != (0, 0, 0) at w[i] + s L with radius r[i]: 0 to 26 per atom
     expanded      the wrapped atoms in input order, then the images by atom and, within an atom, by 9 (sx+1) + 3 (sy+1) + (sz+1)
     result        atom i's area is the engine's area of atom i of the expanded structure; a structure's total is the sum over
                   its real atoms, formed like every total of the engine (fixed order, no float atomics)
   Coordinates in [0, L) further than c from every face give the areas and totals of the batch entries bit for bit.  A
   structure without atoms passes (total 0).  The expansion is made on the device (pbc_kernels.h) and the expanded batch
   goes through the engine as any batch: its 2^30-atom limit applies to atoms and images together.  images_out (host,
   [n_structs], may be NULL) receives the image count of every structure.
   freesasa_gpu_periodic_dev: d_xyz, d_radii, d_sasa [offsets[n_structs]], d_totals [n_structs] (may be NULL) on the device,
   offsets and cells on the host; synchronous.  freesasa_gpu_calc_periodic: host arrays, pooled context (device -1: the
   current one); the cells are checked against the radii before a device is touched.  Returns 0 / -1.
   Not offered: cells smaller than c, skipping the area computation of the image atoms (their areas are
   computed and dropped), periodic images in the file or cache sweeps (a PDB CRYST1 record is a crystallographic cell with
   symmetry).  Triclinic cells: the two entries below these.  Trajectories: FREESASA_GPU_FRAMES_PBC below.  Chain groups among the
   images (isolated, complex and buried areas of chains that lie in different images): freesasa_gpu_groups_periodic_dev, below. */
int freesasa_gpu_periodic_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                              const int64_t *offsets, int n_structs, const double *cells /* host, [3 n_structs] */,
                              double probe_radius, int resolution, double *d_sasa, double *d_totals,
                              int64_t *images_out /* host, [n_structs], may be NULL */);
int freesasa_gpu_calc_periodic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                               const double *cells, int alg, double probe_radius, int resolution,
                               double *sasa_out, double *totals_out, int64_t *images_out,
                               int device, char *err_out, int err_len);

/* Periodic images in a TRICLINIC cell: every structure s has a cell of six numbers h = cells6[6 s .. 6 s + 5] =
   (ax, bx, by, cx, cy, cz), the lower-triangular box matrix with rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz) - the
   form GROMACS, LAMMPS and OpenMM hold (truncated octahedra, rhombic dodecahedra, hexagonal prisms, crystals).  Everything is
   fp64, every operation rounded on its own, in exactly the order written.  With c = 2 (max radius of the structure +
   probe_radius):
     widths        d_c = cz;  d_b = by * (cz / sqrt(cy*cy + cz*cz));  t = bx*cy - by*cx;
                   d_a = ax * ((by*cz) / sqrt(((by*cz)*(by*cz) + (bx*cz)*(bx*cz)) + t*t))
                   (the distances between opposite faces; made once per structure on the host, freesasa_gpu_cell_widths; for a
                   right-angled cell the edges exactly)
     requirement   all six numbers finite, ax, by, cz > 0 and every width >= c.  Shifts in {-1, 0, 1}^3 then suffice: two points
                   whose k-th fractional coordinates differ by D are at least |D| d_k apart, and the neighbour predicate is
                   strict.  Anything else is refused (-1 with a message that names the structure and the entry or width), never
                   approximated.  The cell need not be reduced.
     fractional    of a point p:  fc = p_z / cz;  fb = (p_y - fc*cy) / by;  fa = ((p_x - fc*cx) - fb*bx) / ax
     wrap          with n = floor(f) of the input atom:
                   w_x = ((x - nc*cx) - nb*bx) - na*ax;  w_y = (y - nc*cy) - nb*by;  w_z = z - nc*cz
     images        g = the fractional coordinates of w, recomputed with the same formulas (not f - n).  Axis k admits shift 0
                   always, +1 when g_k * d_k < c, -1 when (1.0 - g_k) * d_k < c; an atom's images are the admitted
                   (sa, sb, sc) != (0, 0, 0), 0 to 26 per atom, with the atom's radius, at
                   x = ((w_x + sc*cx) + sb*bx) + sa*ax;  y = (w_y + sc*cy) + sb*by;  z = w_z + sc*cz
     expanded      the wrapped atoms in input order, then the images by atom and, within an atom, by 9 (sa+1) + 3 (sb+1) + (sc+1)
     result        as for orthorhombic cells: atom i's area is the engine's area of atom i of the expanded structure, totals over
                   the real atoms formed like every total of the engine
   On cells (Lx, 0, Ly, 0, 0, Lz) this is the definition above (the tests hold both entries to the same bytes).  Arguments,
   limits, images_out and return values are those of freesasa_gpu_periodic_dev / freesasa_gpu_calc_periodic, whose behaviour,
   messages and refusals do not change; the expansion is made on the device (pbc_tri_kernels.h).
   Not offered: cells with a width below c, skipping the area computation of the image atoms, a
   PDB CRYST1 record.  Chain groups among the images: freesasa_gpu_groups_periodic_triclinic_dev, below. */
int freesasa_gpu_periodic_triclinic_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                        const int64_t *offsets, int n_structs, const double *cells6 /* host, [6 n_structs] */,
                                        double probe_radius, int resolution, double *d_sasa, double *d_totals,
                                        int64_t *images_out /* host, [n_structs], may be NULL */);
int freesasa_gpu_calc_periodic_triclinic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                         const double *cells6, int alg, double probe_radius, int resolution,
                                         double *sasa_out, double *totals_out, int64_t *images_out,
                                         int device, char *err_out, int err_len);
/* The three widths (d_a, d_b, d_c) of a cell as defined above.  Returns 0, or -1 (widths_out then holds NaN) when an entry is
   not finite or ax, by or cz is not positive.  Touches no device. */
int freesasa_gpu_cell_widths(const double cell6[6], double widths_out[3]);
/* A CHARMM / NAMD / OpenMM unit-cell record as DCD files hold it - rec = A, gamma, B, beta, alpha, C - to the six numbers.
   An angle field v with |v| <= 1 is a cosine; otherwise it is degrees and must lie in (0, 180).  |v| <= 1e-6 and
   |v - 90| <= 1e-4 give cosine 0 EXACTLY (the two cases the orthorhombic decoder of FREESASA_GPU_FRAMES_PBC accepts); any other
   degree value gives cos(v pi / 180).  Then ax = A, bx = B cosg, by = B sqrt(1 - cosg cosg), cx = C cosb,
   cy = C ((cosa - cosb cosg) / sqrt(1 - cosg cosg)), cz = sqrt((C*C - cx*cx) - cy*cy); right angles give (A, 0, B, 0, 0, C)
   exactly.  Returns 0, or -1 with the reason in why (may be NULL): an edge that is not finite, an angle field that is neither,
   angles that span no cell (cz^2 <= 0 or not a number).  Touches no device. */
int freesasa_gpu_cell_from_dcd(const double rec[6], double cell6_out[6], char *why, int why_len);
/* The same from three edge lengths (a, b, c) and three angles (alpha, beta, gamma) as AMBER NetCDF files hold them.  The
   angles are ALWAYS degrees, each in (0, 180): there is no cosine reading.  The operations and their order are those of the
   degree branch of freesasa_gpu_cell_from_dcd, so a DCD record (len[0], deg[2], len[1], deg[1], deg[0], len[2]) in degrees gives
   the same six doubles bit for bit.  Returns 0, or -1 with the reason in why (may be NULL).  Touches no device. */
int freesasa_gpu_cell_from_lengths_angles(const double len[3], const double deg[3], double cell6_out[6], char *why, int why_len);

/* Trajectory drivers (BASELINE configs[4]): frames of the SAME n_atoms atoms, radii constant.
   Frames are independent structures; a SHARD = frames_per_batch frames (<= 0: about 1.25e6 atoms) goes through the
   engine as one batch.  A few host lanes take shards from a shared counter, each on its own pooled context and
   stream, so that reading / uploading one shard, the kernels of another and the download / writing of a third
   overlap.  The radii are stored ONCE per device context, not once per frame.

   freesasa_gpu_trajectory: frames in HOST memory (frame f at xyz_frames + f*3*n_atoms; DMA in place when the
   array is page-locked), totals_out [n_frames], sasa_out NULL or [n_frames*n_atoms].  Returns 0 / -1.

   freesasa_gpu_trajectory_file: frames from a file of raw little-endian frames (3*n_atoms doubles, or floats when
   bit 0 of frames_f32 is set — an input format: they are widened on the device and all arithmetic is fp64 — at byte
   header_bytes + f * frame size), results to files: totals_path (one double per frame at byte 8*f) and, unless
   NULL, sasa_path (n_atoms doubles per frame; n_atoms FLOATS per frame when bit 1 of frames_f32 is set — an output
   format, round 6: the areas are computed in fp64 and narrowed on the device, half the bytes over PCIe and on disk).
   done_path (may be NULL) is the done-list: a text file whose first
   line holds the run's parameters, followed by one line "shard <k> <first frame> <frames>" per finished shard,
   appended after that shard's results are on disk.  A call that finds the done-list of the same run skips the
   shards listed there, so an interrupted run (crash, kill, max_new_shards) resumes where it stopped and ends
   with the same files, bit for bit, as an uninterrupted one; a done-list with other parameters is an error.
   n_frames <= 0: all whole frames of the file; *frames_total_out (may be NULL) receives the count.
   max_new_shards > 0: stop after that many shards.  Returns 0 all done, 1 stopped early, -1 error.

   DCD input (all four file entries: freesasa_gpu_trajectory_file, _file_devices, _file_topology, _file_groups): with bit 2
   of frames_f32 set (FREESASA_GPU_FRAMES_DCD) frames_path is a DCD trajectory as CHARMM, NAMD, OpenMM and LAMMPS write it -
   uncompressed fp32, either byte order, with or without a unit-cell record and a 4th-dimension record per frame, every
   frame at the same byte stride (freesasa_gpu_dcd_info_read below has the layout).  header_bytes must be 0 and bit 0
   clear; bit 1 (fp32 output) keeps its meaning.  The frame count, the byte of frame 0 and the stride come from the file's
   header and its SIZE (never from the header's frame count); the file's NATOM must equal n_atoms (with a topology:
   frame_atoms) - a mismatch, a non-zero header_bytes or bit 0 is -1 with a message before a device is touched or an output
   file opened.  A shard is still one read and one host-to-device copy of contiguous bytes, exactly as they lie in the
   file; ONE kernel (traj_kernels.h, traj_gather_dcd) makes of the planar x[] | y[] | z[] records the compact fp64 frames
   the engine reads - byte-swapped when the file is big-endian, through the atom index when there is a topology - which
   is the work the gather and the widening do for raw frames.  The unit cell and the 4th dimension are never read.  On the
   host every record marker of every frame of a shard is checked before the shard goes up: a mismatch ends the run like a
   failed read ("frame K of the DCD file is damaged"; the shard is not listed).  The done-list's f32= word carries bit 2
   and its header_bytes= the byte of frame 0: a raw run's list is refused by a DCD run and the other way round; a raw run's
   line is what it was.  Without bit 3 SASA is computed WITHOUT periodic images: a solute that the writer wrapped across the
   box must be made whole beforehand.  Not offered: DCD files with fixed atoms or 64-bit record markers, a memory form.

   AMBER NetCDF input (all four file entries): with bit 5 of frames_f32 set (FREESASA_GPU_FRAMES_NETCDF) frames_path is an
   AMBER NetCDF trajectory (convention 1.0, `.nc` as sander, pmemd, cpptraj, OpenMM and MDAnalysis write it): NetCDF classic,
   version 1 or 2, big-endian, every frame one record at the same byte stride (freesasa_gpu_nc_info_read below has the
   layout).  header_bytes must be 0, bits 0 and 2 clear; bit 1 keeps its meaning.  The frame count comes from the file's SIZE
   (never from the header's numrecs), the byte of record 0 and the stride from its header; the file's atom count must equal
   n_atoms (with a topology: frame_atoms) - a mismatch, a non-zero header_bytes, bit 0 or bit 2 is -1 with a message before a
   device is touched or an output file opened.  A shard is one read and one host-to-device copy of whole records exactly as
   they lie in the file - the time, the cell, velocities and forces of a record go up with it and are never read on the
   device; ONE kernel (traj_kernels.h, traj_gather_nc) makes of the big-endian fp32 coordinates the compact fp64 frames the
   engine reads, through the atom index when there is a topology.  There are no record markers to check.  The done-list's
   f32= word carries bit 5 and its header_bytes= the byte of record 0: raw, DCD and NetCDF runs refuse each other's lists.
   Periodic images: bits 3 and 4 may stand beside bit 5 as they stand beside bit 2, for a file with the variables
   cell_lengths and cell_angles (fp64, in the same record).  Every frame's cell is decoded on the host from the staged bytes:
   without bit 4 every angle v must satisfy |v - 90| <= 1e-4 (the angles are degrees: a 0 is not a right angle here) and every
   edge must be finite and >= c; with bit 4 the cell goes through freesasa_gpu_cell_from_lengths_angles and the checks of a
   DCD record.  A frame that fails ends the run ("frame K of the NetCDF file: ..." with the reason; the shard is not listed).
   Refused up front: bit 3 on a file without the cell variables, freesasa_gpu_trajectory_file_groups with bit 3.
   Not offered: NetCDF-4 (HDF5) and CDF-5 files, AMBER restart files, a scale_factor other than 1, a memory form.

   GROMACS XTC input (all four file entries): with bit 6 of frames_f32 set (FREESASA_GPU_FRAMES_XTC) frames_path is an XTC
   trajectory (magic 1995, more than 9 atoms: compressed coordinates; freesasa_gpu_xtc_info_read below has the layout).
   header_bytes must be 0, bits 0, 2 and 5 clear; bit 1 keeps its meaning.  Frames are compressed and of unequal length: one
   pass over the file's headers before a device is touched or an output file opened builds the INDEX, the byte offset of every
   frame, checks every header and counts the frames; the file's atom count must equal n_atoms (with a topology: frame_atoms).
   A shard is the bytes offset[f0] .. offset[f0 + nf], still one read and one host-to-device copy; behind the bytes ride (the
   cells of a periodic run and) one descriptor of 64 bytes per frame, made on the host from the frame's header
   (freesasa_gpu_xtc_frame).  Two kernels decode on the device (xtc_kernels.h): xtc_scan, one wavefront per frame, walks the
   stream's groups and notes where each begins; xtc_unpack, one thread per group, unpacks the integers and writes fp32
   Angstrom coordinates, (float) integer * (float)(1 / (double) precision) * 10.0f in two fp32 products, as raw interleaved
   frames - from where the raw fp32 path goes on unchanged (the gather through a topology's index, or the widening): an XTC
   run's results are those of a raw fp32 file of the decoded values, byte for byte.  A stream that runs out of bits, runs past
   its atoms, leaves smallidx's range 9 .. 72 or unpacks a value outside its range gives its frame a non-zero status, which
   the host reads before the engine runs: the run ends ("frame K of the XTC file is damaged: ..."), nothing of the shard is
   written and it is not listed.  The done-list's f32= word carries bit 6: raw, DCD, NetCDF and XTC runs refuse each other's
   lists.  Periodic images: bits 3 and 4 may stand beside bit 6 as beside bit 2; the cell is every frame's box, each element
   (double) float * 10.0, GROMACS' lower triangle (ax, bx, by, cx, cy, cz) = box[0][0], box[1][0], box[1][1], box[2][0],
   box[2][1], box[2][2].  A non-zero upper element, an off-diagonal element without bit 4 or an all-zero box ends the run
   ("frame K of the XTC file: ..."); the rest are the checks of a DCD cell.  Refused up front: bit 3 on a file whose first
   frame has an all-zero box, freesasa_gpu_trajectory_file_groups with bit 3.
   Not offered: magic 2023 (64-bit byte counts), frames of 9 atoms or fewer (uncompressed), streams of 2^28 bytes and
   more, a memory form, double-precision XTC (chain groups with periodic images: freesasa_gpu_trajectory_file_groups_periodic).  No GROMACS-written file was at hand when
   this was written: conformance rests on the format's description; compare one frame against `gmx dump` first.

   GROMACS TRR input (all four file entries): with bit 7 of frames_f32 set (FREESASA_GPU_FRAMES_TRR) frames_path is a TRR
   trajectory, the full-precision file GROMACS writes with nstxout, in single or double precision
   (freesasa_gpu_trr_info_read below has the layout).  header_bytes must be 0, bits 0, 2, 5 and 6 clear; bit 1 keeps its
   meaning.  Records are uncompressed but of unequal length - nstvout and nstfout differ from nstxout - and need not hold
   coordinates: one pass over the file's headers before a device is touched or an output file opened builds the INDEX, the
   byte offset of every record WITH coordinates, checks every header and counts the frames; the records without coordinates
   are no frames of the run: they lie between the frames and go up unread.  The file's atom count must equal n_atoms (with a
   topology: frame_atoms).  A shard is the bytes offset[f0] .. offset[f0 + nf], still one read and one host-to-device copy;
   behind the bytes ride (the cells of a periodic run and) one int64 per frame, the byte of its x[0] within the shard.  Every
   header of the shard is checked again as it lies in the staging before anything goes up: a failure ends the run ("frame K
   of the TRR file is damaged: ..."), nothing of the shard is written and it is not listed.  ONE kernel (traj_kernels.h,
   traj_gather_trr) makes of the big-endian reals the compact fp64 frames the engine reads, through the atom index when
   there is a topology: 4-byte loads only (a double is two words, high word first: x[0] of a double record with a box lies at
   byte 164), (double) real * 10.0 (nm to Angstrom) - exact for a float, one rounding for a double.  BOTH precisions land in
   the fp64 frames directly: a TRR run's results are those of a raw fp64 frame file that holds (double) x_nm * 10.0, byte for
   byte.  The done-list's f32= word carries bit 7: raw, DCD, NetCDF, XTC and TRR runs refuse each other's lists.  Periodic
   images: bits 3 and 4 may stand beside bit 7 as beside bit 6; the cell is every frame's box, each element
   (double) real * 10.0, GROMACS' lower triangle as in an XTC frame, and the checks are those of an XTC box, a frame without
   a box failing like one whose box is all zero ("frame K of the TRR file: ...").  Refused up front: bit 3 on a file whose
   first coordinate frame has no box or an all-zero one, freesasa_gpu_trajectory_file_groups with bit 3.
   Chain groups with periodic images: freesasa_gpu_trajectory_file_groups_periodic.
   Not offered: a memory form, a TRR whose records change atom count or precision, a read
   of velocities or forces, records with an ir, e, top or sym part.  No GROMACS-written file was at hand when this was
   written: conformance rests on the format's description; compare one frame against `gmx dump` first.

   Periodic images (freesasa_gpu_trajectory_file, _file_devices, _file_topology): with bit 3 (FREESASA_GPU_FRAMES_PBC) beside
   bit 2 (beside bit 5: above) every frame is computed among the periodic images its own unit-cell record implies, as freesasa_gpu_calc_periodic
   below defines them - the atoms the engine sees (with a topology: the atoms the index keeps) wrapped into the cell, the
   first-shell images that can touch them added on the device in front of the engine, the areas and the total of the real
   atoms collected behind it; residues, class sums, selections, fp32 output and the files are what they are without the bit.
   On the host every frame's cell record is decoded beside the marker check (6 doubles in the file's byte order, CHARMM's A,
   gamma, B, beta, alpha, C: the angles as cosines or as degrees): an angle field v with neither |v| <= 1e-6 nor
   |v - 90| <= 1e-4, or an edge that is not finite or shorter than c = 2 (max radius + probe), ends the run like a damaged
   frame ("frame K of the DCD file: ..." with the reason; the shard is not listed).  A shard's edges go up behind its bytes,
   24 bytes per frame.  Refused with a message before a device is touched or an output file opened: bit 3 without bit 2, a
   DCD file without a cell record, freesasa_gpu_trajectory_file_groups (an isolated group among periodic images is not
   defined).  The done-list's f32= word carries bit 3: a periodic run's list is refused by a run without the bit and the other
   way round.  A cell no atom comes within c of changes nothing: such a run's files are those of the run without the bit,
   byte for byte.  Without bit 4 a cell that is not orthorhombic is refused as said above.

   Triclinic cells: with bit 4 (FREESASA_GPU_FRAMES_TRICLINIC) beside bits 2 and 3 every frame's record is decoded by
   freesasa_gpu_cell_from_dcd and the frame computed as freesasa_gpu_calc_periodic_triclinic defines it.  A record that
   decodes to no cell, an edge that is not positive or a width below the run's c ends the run like a damaged frame
   ("frame K of the DCD file: ..."; the shard is not listed).  A shard's cells and widths go up behind its bytes, 72 bytes
   per frame instead of 24, still one copy.  Bit 4 without bits 2 and 3, and freesasa_gpu_trajectory_file_groups with it,
   are refused before a device is touched or an output file opened.  The done-list's f32= word carries bit 4: runs with and
   without it refuse each other's lists.  A right-angled file gives the files of the run without bit 4, byte for byte.
   Chain groups with periodic images: freesasa_gpu_trajectory_file_groups_periodic (the other entries refuse them and name it).
   Not offered: cells smaller than c, a cell for raw frame files or the memory entries. */
#define FREESASA_GPU_FRAMES_F32 1     /* frames_f32 bit 0: raw fp32 frames (input format) */
#define FREESASA_GPU_FRAMES_OUT_F32 2 /* bit 1: per-atom (and isolated) areas written as fp32 (output format) */
#define FREESASA_GPU_FRAMES_DCD 4     /* bit 2: frames_path is a DCD trajectory */
#define FREESASA_GPU_FRAMES_PBC 8     /* bit 3: with bit 2, 5, 6 or 7, every frame among the periodic images of its cell */
#define FREESASA_GPU_FRAMES_TRICLINIC 16 /* bit 4: with bit 3, the cell decoded as a triclinic cell */
#define FREESASA_GPU_FRAMES_NETCDF 32 /* bit 5: frames_path is an AMBER NetCDF trajectory */
#define FREESASA_GPU_FRAMES_XTC 64    /* bit 6: frames_path is a GROMACS XTC trajectory */
#define FREESASA_GPU_FRAMES_TRR 128   /* bit 7: frames_path is a GROMACS TRR trajectory, single or double precision */

/* The header of a DCD file.  Every integer of the file is an int32 in the file's byte order; records lie between two equal
   byte counts:  [84 | "CORD" | 20 control words | 84]  [m | NTITLE | 80 NTITLE bytes | m]  [4 | NATOM | 4], then per frame
   [48 | 6 doubles | 48] when there is a unit cell, [4N | N floats | 4N] for x, for y and for z, and once more when there is a
   4th dimension.  Control words: 0 the frame count as the writer claims it, 8 fixed atoms, 10 / 11 non-zero: a unit-cell /
   4th-dimension record per frame, 19 the CHARMM version (0: X-PLOR, which has neither record - words 10 and 11 are ignored).
   Returns 0, or -1 with a message in err that says which check failed: the first word is neither 84 nor 84 byte-swapped,
   "CORD" is missing, 64-bit record markers, fixed atoms, NATOM <= 0, a header marker that does not match, a file shorter
   than the header, a file that holds no whole frame.  A tail that is not a whole frame is ignored.  Allocates nothing. */
typedef struct freesasa_gpu_dcd_info {
    int32_t n_atoms;          /* NATOM */
    int64_t n_frames;         /* whole frames by FILE SIZE */
    int64_t n_frames_header;  /* NSET as the header claims (often 0 or stale: reported, never trusted) */
    int64_t first_frame;      /* byte of frame 0 */
    int64_t frame_bytes;      /* constant stride */
    int32_t x_off;            /* byte of x[0] within a frame (4, or 60 with a cell record) */
    int32_t plane_bytes;      /* 4 * n_atoms + 8: x -> y -> z */
    int32_t big_endian, has_cell, has_4d, charmm_version;
} freesasa_gpu_dcd_info;
int freesasa_gpu_dcd_info_read(const char *path, freesasa_gpu_dcd_info *out, char *err, int err_len); /* 0 / -1 */

/* The header of an AMBER NetCDF trajectory.  The file is NetCDF classic, every integer big-endian and 32 bits wide unless said
   otherwise:  'C' 'D' 'F' version (1, or 2: a variable's begin is 8 bytes) | numrecs (0xFFFFFFFF: streaming) | dim_list |
   gatt_list | var_list, each list ABSENT (two zero words) or [tag | nelems | elements] with the tags 0x0A dimensions, 0x0C
   attributes, 0x0B variables.  name = length, bytes, padded to 4; dim = name, length (0: the record dimension); attr = name,
   nc_type, nelems, values padded to 4; var = name, ndims, dimid[ndims], its attribute list, nc_type, vsize, begin; nc_type and
   bytes: BYTE 1/1, CHAR 2/1, SHORT 3/2, INT 4/4, FLOAT 5/4, DOUBLE 6/8.  A record variable is one whose first dimension is the
   record dimension; the record size is the sum of the record variables' vsize (each padded to 4; with exactly one record
   variable its unpadded size); record 0 begins at the smallest begin among them, and variable v of frame f lies at
   begin_v + f * record size.
   What must hold: the global CHAR attribute Conventions has AMBER among its tokens (split on ',' and ' '; AMBERRESTART is
   a restart file, not a trajectory); `coordinates` is NC_FLOAT over (record dimension, `atom`, a dimension of length 3) and
   has no scale_factor other than 1; 0 < atoms, 12 atoms < 2^31; cell_lengths and cell_angles, where present, are NC_DOUBLE
   record variables over (record dimension, a dimension of length 3): has_cell when both are.
   Returns 0, or -1 with a message in err that says which check failed: those above, a NetCDF-4 (HDF5) or CDF-5 file, a file
   that is not CDF, a header that ends before its grammar or is longer than 64 KiB, a count, name length, dimid or begin that
   points outside the header or the file, a record layout that is not made of 32-bit words or does not hold its variables, a
   file that holds no whole record.  A tail that is not a whole record is ignored.  Reads the first 64 KiB of the file into a
   buffer of its own and nothing outside it; allocates nothing. */
typedef struct freesasa_gpu_nc_info {
    int32_t n_atoms;          /* the dimension `atom` */
    int64_t n_frames;         /* whole records by FILE SIZE */
    int64_t n_frames_header;  /* numrecs as the header claims, -1: streaming (reported, never trusted) */
    int64_t first_record;     /* byte of record 0 */
    int64_t record_bytes;     /* constant stride */
    int64_t coord_off;        /* byte of `coordinates` within a record */
    int64_t lengths_off, angles_off; /* of cell_lengths and cell_angles; -1 without a cell */
    int32_t version;          /* 1 or 2 */
    int32_t has_cell, has_time, has_velocities;
} freesasa_gpu_nc_info;
int freesasa_gpu_nc_info_read(const char *path, freesasa_gpu_nc_info *out, char *err, int err_len); /* 0 / -1 */
/* The cell of frame f of the records at `records` (frame 0's first byte; info->has_cell): three edge lengths and alpha, beta,
   gamma in degrees, in the host's byte order.  The offsets are multiples of 4, not of 8: copied byte by byte. */
void freesasa_gpu_nc_cell_record(const freesasa_gpu_nc_info *info, const void *records, long long f, double lengths_out[3], double angles_out[3]);

/* A GROMACS XTC trajectory.  Every value of the file is XDR: big-endian, 4 bytes.  A frame:
       int magic = 1995 | int natoms | int step | float time | float box[3][3] (nm, row-major) | int natoms | float precision |
       int minint[3] | int maxint[3] | int smallidx | int bytecount | bytecount bytes, padded to a multiple of 4
   The bit stream starts FREESASA_GPU_XTC_HEADER = 92 bytes into the frame, the next frame follows the padding; every offset is
   a multiple of 4.  freesasa_gpu_xtc_index_read makes ONE pass over the file, one read of 92 bytes per frame: it checks every
   header, counts the frames (the count comes from this pass, not from the file's size) and, with offsets_out, returns the
   byte offset of every frame, [n_frames + 1] with the end of the last one behind them, in an array the caller frees with
   freesasa_gpu_xtc_index_free; without offsets_out (freesasa_gpu_xtc_info_read) it allocates nothing.  Returns 0, or -1 with
   "frame K of the XTC file: <reason>" in err - each its own reason: magic 2023 (the variant with 64-bit byte counts), any
   other magic, 9 atoms or fewer (such frames hold uncompressed floats), two atom counts that differ from each other or from
   frame 0's, a precision that is not finite or <= 0, minint > maxint in a dimension (or a dimension that spans all 2^32
   integers), smallidx outside 9 .. 72, a byte count that is negative, 2^28 or more, or runs past the end of the file, a file
   that ends inside a header. */
#define FREESASA_GPU_XTC_HEADER 92
typedef struct freesasa_gpu_xtc_info {
    int32_t n_atoms;          /* of frame 0, and so of every frame */
    int64_t n_frames;         /* by the pass over the headers */
    int64_t max_frame_bytes;  /* the longest frame, header and padding included */
    float precision;          /* of frame 0 (every frame carries its own) */
    int32_t has_box;          /* frame 0's box has a non-zero element */
} freesasa_gpu_xtc_info;
int freesasa_gpu_xtc_info_read(const char *path, freesasa_gpu_xtc_info *out, char *err, int err_len); /* 0 / -1 */
int freesasa_gpu_xtc_index_read(const char *path, freesasa_gpu_xtc_info *out, int64_t **offsets_out, char *err, int err_len);
void freesasa_gpu_xtc_index_free(int64_t *offsets);
/* What the device needs to decode one frame, made from its header; 64 bytes, one per frame of a shard behind the shard's bytes.
   sizeint = maxint - minint + 1.  bitsize: 0 when (sizeint[0] | sizeint[1] | sizeint[2]) > 0xffffff - a "big" triple is then
   three fields of bitsizeint[k] = the smallest b <= 32 with 2^b > sizeint[k] bits - else the bit length of the product of the
   three sizes: a big triple is one field of that many bits. */
typedef struct freesasa_gpu_xtc_frame {
    int64_t stream_off;       /* byte of the stream's first byte within the shard (a multiple of 4) */
    int32_t bytecount;        /* bytes of the stream, < 2^28 */
    int32_t minint[3];
    uint32_t sizeint[3];
    int32_t bitsize, bitsizeint[3];
    int32_t smallidx;         /* of the frame's first group, 9 .. 72 */
    float inv_precision;      /* (float)(1.0 / (double) precision) */
    int32_t pad_;
} freesasa_gpu_xtc_frame;
/* The checks of one header (`avail` bytes of the file lie from its first byte on; n_atoms > 0: the count it must hold) and its
   descriptor, the stream at byte stream_off; *frame_bytes_out: header + stream + padding.  0, or -1 with the reason in why. */
int freesasa_gpu_xtc_frame_desc(const void *header, long long avail, int n_atoms, long long stream_off, freesasa_gpu_xtc_frame *out,
                                long long *frame_bytes_out, char *why, int why_len);
/* the nine floats of a header's box, in the host's byte order (nm) */
void freesasa_gpu_xtc_frame_box(const void *header, float box_out[9]);

/* A GROMACS TRR trajectory.  Every value of the file is XDR: big-endian, 4-byte units.  A record:
       int magic = 1993 | int 13 | int 12 | 12 bytes "GMX_trn_file" |
       int ir_size, e_size, box_size, vir_size, pres_size, top_size, sym_size, x_size, v_size, f_size, natoms, step, nre |
       real t | real lambda | box[9] | vir[9] | pres[9] | x[3 natoms] | v[3 natoms] | f[3 natoms]
   each part of the body present only when its size is not 0; real is 4 or 8 bytes for the whole record: box_size / 9 when
   box_size != 0, else the first non-zero of x_size, v_size, f_size divided by 3 natoms.  The header is
   FREESASA_GPU_TRR_HEADER_MIN + 2 reals = 84 or 92 bytes; units are nm; the box rows are a, b, c, the lower triangle of an
   XTC box.  freesasa_gpu_trr_index_read makes ONE pass over the file, one read of at most 92 bytes per record: it checks every
   header, counts the records and those WITH coordinates (the frames) and, with offsets_out, returns the byte at which every
   frame begins, [n_frames + 1] with the end of the file behind them, in an array the caller frees with
   freesasa_gpu_trr_index_free; without offsets_out (freesasa_gpu_trr_info_read) it allocates nothing.  Returns 0, or -1 with
   "record K of the TRR file: <reason>" in err - each its own reason: a magic number other than 1993, a version string other
   than 13, 12, "GMX_trn_file", a non-zero ir_size, e_size, top_size or sym_size, natoms <= 0, a real width that is neither 4
   nor 8, a size that disagrees with natoms and that width, an atom count or a precision other than record 0's, a file that
   ends inside a header or inside a body - or "the TRR file holds no coordinate frame".  A file cut exactly between two
   records is a shorter file. */
#define FREESASA_GPU_TRR_HEADER_MIN 76
typedef struct freesasa_gpu_trr_info {
    int32_t n_atoms;          /* of record 0, and so of every record */
    int64_t n_frames;         /* records WITH coordinates, by the pass over the headers */
    int64_t n_records;        /* all records */
    int64_t max_frame_bytes;  /* the longest stretch from a frame's first byte to the next frame's (the file's end) */
    int32_t real_bytes;       /* 4 or 8: of record 0, and so of every record */
    int32_t has_box;          /* the first frame has a box with a non-zero element */
    int32_t has_velocities, has_forces; /* some record has them (never read) */
} freesasa_gpu_trr_info;
int freesasa_gpu_trr_info_read(const char *path, freesasa_gpu_trr_info *out, char *err, int err_len); /* 0 / -1 */
int freesasa_gpu_trr_index_read(const char *path, freesasa_gpu_trr_info *out, int64_t **offsets_out, char *err, int err_len);
void freesasa_gpu_trr_index_free(int64_t *offsets);
/* What one record's header says, and where its parts lie when the record begins at byte `base` (of a shard, of the file) */
typedef struct freesasa_gpu_trr_record {
    int32_t n_atoms, real_bytes;
    int32_t has_box, has_x, has_v, has_f;
    int64_t record_bytes;     /* header and body */
    int64_t box_off, x_off;   /* byte of box[0] and of x[0]; -1: the record has none (multiples of 4, not of 8 in general) */
} freesasa_gpu_trr_record;
/* The checks of one header (`avail` bytes of the file lie from its first byte on, of which at most 92 are read; n_atoms > 0 and
   real_bytes > 0: what it must hold) and what it says.  0, or -1 with the reason in why. */
int freesasa_gpu_trr_frame_desc(const void *header, long long avail, int n_atoms, int real_bytes, long long base,
                                freesasa_gpu_trr_record *out, char *why, int why_len);
/* the nine reals of a box, as doubles in the host's byte order (nm) */
void freesasa_gpu_trr_box(const void *box, int real_bytes, double box_out[9]);

int freesasa_gpu_trajectory(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                            int alg, double probe_radius, int resolution, int frames_per_batch,
                            double *totals_out, double *sasa_out, int device,
                            char *err_out, int err_len);

/* Trajectory drivers with a TOPOLOGY: the solute of a solvated system, its residues, its classes and a set of selections,
   per frame.  The arguments of freesasa_gpu_trajectory_devices / freesasa_gpu_trajectory_file_devices with the pair
   (radii, n_atoms) replaced by
     batch, structure   structure `structure` of a loaded batch (include/freesasa_ingest.h) supplies what the kernels read:
                        its n atoms with their radii, classes, backbone flags, names and symbols, and its residues
                        (boundaries rebased to the structure, labels).  Its coordinates are not used.
     frame_atoms, atom_index   every input frame holds frame_atoms >= n atoms (3 * frame_atoms numbers); topology atom i
                        is frame atom atom_index[i] - any order, every index in [0, frame_atoms), none twice (two atoms
                        at one place give NaN).  atom_index NULL: the identity, and frame_atoms must be n.  The other
                        atoms of a frame - the solvent - go up with it and are dropped on the device by one gather
                        kernel (fp32 frames are widened by the same kernel); no index: the plain drivers' path.
     sel                a compiled set of up to 64 selections (freesasa_ingest_selection_compile) or NULL.
   Outputs, all fp64 and in frame order; each may be NULL (not wanted) except the totals.  Memory form: arrays; file form:
   paths of files whose offsets the frame number fixes, written by pwrite per shard like the totals file:
     totals      1 per frame          (8 f)            what the plain drivers give for the topology's atoms
     per-atom    n per frame          (8 n f)          likewise (file form: fp32 when bit 1 of frames_f32 is set)
     class sums  3 per frame          (8 * 3 f)        apolar, polar, unknown: freesasa_gpu_class_sums_dev on the frame
     residues    6 R per frame        (8 * 6 R f)      total, main chain, side chain, polar, apolar, unknown of the
                                                       structure's R residues: d_abs of freesasa_gpu_residue_areas_dev
     selections  S per frame          (8 S f)          area_out of freesasa_gpu_select_batch
   each bit for bit what the named entry gives on the frame taken as a structure of its own.  sel_atoms_out [S] (may be
   NULL): the atoms every selection holds - they do not depend on the frame and come back once, with the first shard a
   call computes (a resumed call that finds every shard done leaves the array as it is).  RELATIVE areas are not written:
   they are the residue columns divided by constants - 100 * column / freesasa_ingest_residue_reference_table()[5 *
   res_ref[r] + column] for the first five columns, where the structure's res_ref[r] >= 0.
   The residue boundaries, classes, backbone flags, the index and the selections' mask words (the set's program run once
   over the topology; open ranges take the structure's first and last residue) are made once per lane and stay on the
   device; per shard a gather and three kinds of ordered sums run on the lane's stream behind the tile kernels, and their
   results ride in front of the shard's one stream synchronisation.  Per-atom areas leave the device only when asked for.
   frames_per_batch <= 0: 1250000 / frame_atoms + 1.
   The done-list's first line also names the index, frame_atoms, the structure's residue boundaries, classes and backbone
   flags, the selection set's program and which outputs are written: a done-list that differs in any of these - or one
   of the plain drivers - is refused; every result file is flushed before its shard is listed.
   Argument errors - NULL batch, structure out of range, a structure that failed to load or has no atoms, a bad index,
   frame_atoms < n - return -1 with a message before a device is touched or a file opened.
   Returns as the plain drivers: 0 / -1, the file form 1 when max_new_shards stopped it.
   Not offered: relative areas in files, trajectory container formats other than DCD and AMBER NetCDF.  (Chain groups: freesasa_gpu_trajectory_groups below.) */
int freesasa_gpu_trajectory_topology(const double *xyz_frames, int n_frames, const struct freesasa_ingest_batch *batch, int structure,
                                     int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                     int alg, double probe_radius, int resolution, int frames_per_batch,
                                     double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                     double *sel_area_out, long long *sel_atoms_out,
                                     const int *devices, int n_devices, char *err, int err_len);
int freesasa_gpu_trajectory_file_topology(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                          const struct freesasa_ingest_batch *batch, int structure,
                                          int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                          int alg, double probe_radius, int resolution, int frames_per_batch,
                                          const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                          const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                          const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                          long long *frames_total_out, char *err, int err_len);

/* CHAIN GROUPS in the trajectory drivers: the reference's --chain-groups / --separate-chains as a time series of an interface
   - per frame the area every group of chains has on its own, the area it has in the complex, and the area it buries.  The two
   entries above are these with group = NULL; the arguments are theirs, with behind `sel`
     group, n_groups    group [n]: one int32 id per atom of the topology's structure, -1 = in no group - the slice
                        [offsets[structure], offsets[structure + 1]) of what freesasa_ingest_chain_groups or
                        freesasa_gpu_chain_group_ids gives for the batch; 1 <= n_groups <= 65535.  An empty group is allowed
                        (its totals are 0).  group NULL: no groups, and both outputs below must be NULL.
   and behind sel_atoms_out the outputs (memory form: arrays; file form: paths, offsets fixed by the frame number)
     group areas  3 G per frame       (8 * 3 G f)      isolated, complex, buried of every group: required with group
     isolated     n per frame         (8 n f)          every atom's area in its group taken on its own (= its complex area
                                                       for an atom in no group); may be NULL (file form: fp32, 4 n f, when
                                                       bit 1 of frames_f32 is set)
   group_areas_out[f] is bit for bit d_group_totals, and iso_out[f] d_iso, of freesasa_gpu_groups_dev (below) on frame f taken
   as a structure of its own; every other output is bit for bit what the entries above give without groups.
   The topology does not change over the run, so neither does its cut into groups: the host makes it once (the atoms of every
   group in input order), a lane uploads it once and writes the radii of its shards once; per shard ONE batch goes through
   the engine - the frames where they are without groups, behind them every group of every frame as a structure of its own
   (one gather kernel) - and behind the tile kernels the groups' complex areas are summed with the chunks of their isolated
   totals (csrc/traj_kernels.h).  The engine therefore sees up to TWICE the atoms of a shard: n + (atoms with an id >= 0)
   per frame; frames_per_batch <= 0 is still 1250000 / frame_atoms + 1, and frames_per_batch times that sum, and times
   1 + n_groups, must not exceed 2^30 (-1 with a message).  A run without groups takes exactly the copies and kernels it took.
   The done-list's first line names the outputs (groups 16, isolated 32) and ends in groups=<digest of n_groups and the ids>;
   a list that differs is refused; both files are flushed before their shard is listed.
   Argument errors, -1 with a message before a device is touched or a file opened: an id < -1 or >= n_groups (the message
   names the atom and the id), n_groups out of range, group given without group areas or either output without group.
   Not offered: a buried area per residue, group ids made on the device for a trajectory (make them once with
   freesasa_gpu_chain_group_ids), trajectory container formats other than DCD and AMBER NetCDF. */
int freesasa_gpu_trajectory_groups(const double *xyz_frames, int n_frames, const struct freesasa_ingest_batch *batch, int structure,
                                   int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                   const int32_t *group, int n_groups,
                                   int alg, double probe_radius, int resolution, int frames_per_batch,
                                   double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                   double *sel_area_out, long long *sel_atoms_out,
                                   double *group_areas_out /* [F, G, 3] */, double *iso_out /* [F, n] or NULL */,
                                   const int *devices, int n_devices, char *err, int err_len);
int freesasa_gpu_trajectory_file_groups(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                        const struct freesasa_ingest_batch *batch, int structure,
                                        int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                        const int32_t *group, int n_groups,
                                        int alg, double probe_radius, int resolution, int frames_per_batch,
                                        const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                        const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                        const char *group_areas_path, const char *iso_path,
                                        const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                        long long *frames_total_out, char *err, int err_len);

/* RUN STATISTICS of the trajectory drivers: mean, standard deviation, minimum and maximum over the frames of a run, of any
   per-frame output, reduced on the device - the per-frame values need not leave it (what `gmx sasa -or / -oa` prints; the
   per-atom stream-out is n_frames x n_atoms values, the statistics are 4 x n_atoms).
   stats: a word of FREESASA_GPU_STATS_* bits, one per output.  An output with its bit set is COMPUTED for every frame whether
   or not its array / its path is given; without array or path it is neither downloaded nor written.  W = the sum of the widths
   of the outputs asked for, in the order totals [1] | per-atom [n] | isolated [n] | class sums [3] | residues [6 R] |
   selections [S] | groups [3 G] (freesasa_gpu_traj_stats_width gives W and every output's first column).
   The definition (the tests hold the device to it bit for bit; fp64, every operation rounded on its own, no fma).  Per shard -
   frames [f0, f0 + nf) - and per column j of its block a[nf][w] of fp64 values (never the fp32 copies of an out-f32 run):
       s = 0; for f = 0 .. nf-1: s += a[f][j];     mean = s / nf;     lo, hi = the smallest and largest a[f][j];
       M2 = 0; for f = 0 .. nf-1: d = a[f][j] - mean; M2 += d * d
   the shard's PARTIAL is [4][W]: mean, M2, lo, hi.  The partials of a run are merged in shard order, left to right, starting
   from shard 0's; with n frames so far and nb of the next shard:
       t = n + nb;  d = mean_b - mean;  mean += d * (nb / t);  M2 = (M2 + M2_b) + (d * d) * (n * (nb / t));  lo = min, hi = max;  n = t
   and the result is [4][W]: mean, std = sqrt(M2 / n) (the population's, numpy's default), min, max.
   A run's statistics depend on the frames and on frames_per_batch - not on the device list, the lanes or on how often the run
   was interrupted and resumed.  Runs with different frames_per_batch agree to rounding, NOT to the bit.
   Memory forms: stats_out [4][W]; partials_out [n_shards][4][W] or NULL.  File forms: partials_path receives the partials as
   the shards finish (raw fp64, shard k at byte k * 4 W * 8; flushed with the result files before the shard is listed);
   a call that finds every shard done merges them and writes stats_path, raw fp64 [4][W]; a call stopped by max_new_shards writes
   none, a run that is not resumed removes a stale one at its start, a repeated call on a complete run writes the same bytes.
   With statistics the done-list's first line ends in stats=<word>; a list written with another word is refused; without
   statistics the line is what it was.  With stats == 0 every entry below is its parent.
   Argument errors, -1 with a message that names the output, before a device is touched or a file opened: class sums, residues
   or selections without a topology (the two plain entries), selections without a selection set, groups or isolated areas
   without chain groups, an unknown bit, statistics without stats_out / without stats_path and partials_path.
   Not offered: medians and quantiles, time correlation, statistics independent of frames_per_batch to the bit, weights per frame. */
#define FREESASA_GPU_STATS_TOTALS 1
#define FREESASA_GPU_STATS_ATOMS 2
#define FREESASA_GPU_STATS_ISOLATED 4
#define FREESASA_GPU_STATS_CLASSES 8
#define FREESASA_GPU_STATS_RESIDUES 16
#define FREESASA_GPU_STATS_SELECTIONS 32
#define FREESASA_GPU_STATS_GROUPS 64
#define FREESASA_GPU_STATS_PAIRS 128          /* (freesasa_gpu_trajectory_interface_residues and its file form only, below) */
#define FREESASA_GPU_STATS_PAIR_RESIDUES 256  /* (the same two entries only) */
int freesasa_gpu_trajectory_stats(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                                  int alg, double probe_radius, int resolution, int frames_per_batch,
                                  double *totals_out, double *sasa_out, const int *devices, int n_devices,
                                  int stats, double *stats_out, double *partials_out, char *err_out, int err_len);
int freesasa_gpu_trajectory_groups_stats(const double *xyz_frames, int n_frames, const struct freesasa_ingest_batch *batch, int structure,
                                         int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                         const int32_t *group, int n_groups,
                                         int alg, double probe_radius, int resolution, int frames_per_batch,
                                         double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                         double *sel_area_out, long long *sel_atoms_out, double *group_areas_out, double *iso_out,
                                         const int *devices, int n_devices,
                                         int stats, double *stats_out, double *partials_out, char *err, int err_len);
int freesasa_gpu_trajectory_file_stats(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                                       int n_atoms, long long n_frames, int alg, double probe_radius, int resolution,
                                       int frames_per_batch, const char *totals_path, const char *sasa_path,
                                       const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                       long long *frames_total_out,
                                       int stats, const char *stats_path, const char *partials_path, char *err_out, int err_len);
int freesasa_gpu_trajectory_file_groups_stats(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                              const struct freesasa_ingest_batch *batch, int structure,
                                              int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                              const int32_t *group, int n_groups,
                                              int alg, double probe_radius, int resolution, int frames_per_batch,
                                              const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                              const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                              const char *group_areas_path, const char *iso_path,
                                              const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                              long long *frames_total_out,
                                              int stats, const char *stats_path, const char *partials_path, char *err, int err_len);
/* CHAIN GROUPS AMONG PERIODIC IMAGES over a trajectory: freesasa_gpu_trajectory_file_groups_stats with every frame - and every
   group of it, taken on its own - among the periodic images of the frame's own cell: the buried area of a complex over a wrapped
   trajectory, whichever images of the box its chains lie in.  The signature is that entry's.  Bit 3 of frames_f32
   (FREESASA_GPU_FRAMES_PBC) and group are REQUIRED (-1 with a message before a file is opened: without either the run is
   another entry's), bit 4 (triclinic cells) is optional; the containers are those that carry a cell: DCD, AMBER NetCDF, XTC,
   TRR.  Per frame f the totals, the per-atom areas, the isolated areas and the group table are bit for bit
   freesasa_gpu_groups_periodic_dev (with bit 4: _triclinic_dev; below) on frame f taken as a structure with its cell: ONE engine
   run per shard holds the frames, their groups and the images of both.  Class sums, residues, selections, fp32 output, the
   statistics word and the done-list work as in the non-periodic groups run; the done-list's first line carries bit 3 (and 4)
   in its f32= word and the groups' digest, so the lists of this run, of the plain periodic run and of the non-periodic groups
   run refuse each other.  The other entries keep refusing chain groups with bit 3 or bit 4, and name this one.
   Interfaces between the groups among periodic images: freesasa_gpu_trajectory_file_interfaces_periodic (below).
   Not offered: the memory form (it has no cells), exposure masks or volume among periodic images. */
int freesasa_gpu_trajectory_file_groups_periodic(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                                 const struct freesasa_ingest_batch *batch, int structure,
                                                 int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                                 const int32_t *group, int n_groups,
                                                 int alg, double probe_radius, int resolution, int frames_per_batch,
                                                 const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                                 const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                                 const char *group_areas_path, const char *iso_path,
                                                 const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                 long long *frames_total_out,
                                                 int stats, const char *stats_path, const char *partials_path, char *err, int err_len);
/* INTERFACES BETWEEN CHAIN GROUPS over a trajectory: with three or more groups a group's buried area in the groups' run is the
   sum over all its partners; these entries say which partner buries how much, per frame.  They are
   freesasa_gpu_trajectory_groups_stats / _file_groups_stats - the arguments, the outputs, the statistics word, the done-list -
   with, in front of err,
     pairs, n_pairs     pairs [K, 2] int32: the pairs (g, h) of group numbers, 0 <= g < h < n_groups, every pair at most once,
                        K >= 1; constant over the run.  A pair may name an empty group.
     pair areas         6 K per frame (8 * 6 K f): per pair (iso_g, iso_h, in_pair_g, in_pair_h, buried_g, buried_h), the six
                        doubles and the order of freesasa_gpu_interfaces_dev's pair_areas (below).  Required.
   group is required; the group areas may be NULL here.  Per frame f and pair k:
     iso_*      column 0 of the frame's group areas of that group, bit for bit.
     in_pair_*  the PAIR STRUCTURE of (g, h) is group g's atoms in input order, then group h's; every atom's area in it is the
                plain entry's (freesasa_gpu_calc_batch) on that structure cut on the host, bit for bit; a side's in_pair is the
                sum of its atoms' areas in the order of the per-structure totals kernel: 256 contiguous runs of
                ceil(len / 256) atoms, each added in atom order from 0, then the runs added in order from 0 - whatever the
                side's size, so a row does not depend on what else is in the shard.
     buried_*   iso_* - in_pair_*, one subtraction.
   There is NO CONTACT SCREEN: a pair that does not touch in a frame still has its row.  Its in_pair is then the same terms as
   its iso added in possibly another order: buried is 0 or rounding noise, |buried| <= N * 2^-53 * iso with N the side's atom
   count.  An empty side's three columns are 0.
   Per shard ONE batch goes through the engine: behind the frames and their isolated groups every pair structure of every frame
   (csrc/traj_kernels.h has the layout): n + n_iso + n_pair atoms and 1 + G + K structures per frame, n_pair the sum over the
   pairs of |g| + |h|.  frames_per_batch <= 0 goes by that sum where it exceeds frame_atoms: 1250000 / max + 1; frames_per_batch
   times that sum, and times 1 + G + K, must not exceed 2^30.  Every output these entries share with the groups' run is bit for
   bit what that run gives; the run statistics of the other outputs work beside the pairs.
   The done-list's first line carries bit 256 in outputs= and, behind groups=, pairs=<digest of K and the pairs>: a list written
   for other pairs, or without them, is refused.
   Argument errors, -1 with a message before a device is touched or a file opened: group NULL, n_pairs < 1, pairs or the pair
   areas NULL, a pair with g >= h or an id out of [0, n_groups) (the message names the pair's index), a pair named twice (it names
   both indices), bit 3 or bit 4 of frames_f32 (interfaces among periodic images are another entry's:
   freesasa_gpu_trajectory_file_interfaces_periodic, below; the message names it).
   Not offered: a contact screen per frame, per-atom buried areas per pair, contact tables,
   group ids made on the device, more than two groups per interface.  Per-residue buried areas per pair and the run statistics
   of the pair columns: freesasa_gpu_trajectory_interface_residues below. */
int freesasa_gpu_trajectory_interfaces(const double *xyz_frames, int n_frames, const struct freesasa_ingest_batch *batch, int structure,
                                       int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                       const int32_t *group, int n_groups,
                                       int alg, double probe_radius, int resolution, int frames_per_batch,
                                       double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                       double *sel_area_out, long long *sel_atoms_out, double *group_areas_out, double *iso_out,
                                       const int *devices, int n_devices,
                                       int stats, double *stats_out, double *partials_out,
                                       const int32_t *pairs, int n_pairs, double *pair_areas_out /* [F, K, 6] */, char *err, int err_len);
int freesasa_gpu_trajectory_file_interfaces(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                            const struct freesasa_ingest_batch *batch, int structure,
                                            int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                            const int32_t *group, int n_groups,
                                            int alg, double probe_radius, int resolution, int frames_per_batch,
                                            const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                            const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                            const char *group_areas_path, const char *iso_path,
                                            const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                            long long *frames_total_out,
                                            int stats, const char *stats_path, const char *partials_path,
                                            const int32_t *pairs, int n_pairs, const char *pair_areas_path, char *err, int err_len);
/* PER-RESIDUE INTERFACE TABLES over a trajectory, with OCCUPANCY: where on each partner an interface lies, frame by frame, and in
   what fraction of the frames a residue is part of it.  These entries are freesasa_gpu_trajectory_interfaces / _file_interfaces
   with, in front of err,
     min_buried            a finite double, in A^2
     pair residues         4 S per frame (8 * 4 S f): the DENSE table below; an array [F, S, 4] / a path of raw fp64
   The pair part of a frame is the n_pair atoms of its pair structures: for every pair, side g's atoms in input order, then side
   h's.  A SEGMENT is a maximal run of consecutive atoms of ONE side whose topology atoms lie in one residue of the topology's
   structure: a head at every side's begin and wherever the residue changes.  Empty residues are never found; a residue split
   over two groups gives a segment on each side it occurs on; atoms in no group are in no side; an empty side has no segment; a
   group named in several pairs has its residues once per pair.  The segments are the same for every frame: S of them, S <=
   n_pair (freesasa_gpu_trajectory_interface_segments gives them without a device).  Per frame f and segment s, four doubles:
     iso_res       the sum of its atoms' areas in their ISOLATED group of frame f (the run's isolated output for those atoms)
     in_pair_res   the sum of its atoms' areas in the pair structure of frame f (the plain entry's on that structure)
     buried_res    iso_res - in_pair_res, one subtraction
     in_interface  1.0 if buried_res > min_buried (strict, fp64), else 0.0
   Both sums are taken one addition at a time in atom order, from 0.0; there is no fma.  The table is DENSE, not compacted, and
   there is no contact screen: the frames of a run line up column by column.  Taking the frames as a batch,
   freesasa_gpu_interface_residues_dev with the same res_first and min_buried lists rows that equal, in all three areas and bit
   for bit, the dense row of the same (frame, pair, side, residue); every dense row it does not list has in_interface == 0 or
   belongs to a pair that entry screened out.
   Statistics: two more bits of the word, accepted by THESE TWO entries only (every other entry refuses them as unknown):
   FREESASA_GPU_STATS_PAIRS - the 6 K pair columns - and FREESASA_GPU_STATS_PAIR_RESIDUES - the 4 S columns; they lie behind
   the groups: ... | groups [3 G] | pairs [6 K] | interface residues [4 S] (freesasa_gpu_traj_stats_width_pairs).  The mean of
   an in_interface column is the residue's OCCUPANCY: the fraction of the frames in which it is in the interface.
   Here the pair areas may be NULL, and an output whose statistics bit is set need not be delivered.  The engine's batch of a
   shard is the interfaces run's, atom for atom: every output shared with that run is bit for bit what it gives.
   The done-list's first line carries bit 512 in outputs= when the table is written and, behind pairs=,
   minburied=<the double's 16 hex digits> when it is computed: a list written with another min_buried, for other pairs, or by
   the plain interfaces run is refused.
   Argument errors, -1 with a message before a device is touched or a file opened: everything the interface entries refuse
   (bit 3 and bit 4 of frames_f32 included) but NULL pair areas; neither pair areas nor pair residues delivered nor named in the
   statistics word (nowhere to go); a min_buried that is not finite.
   Not offered: a compacted per-frame table, contact tables per frame (the run's residue-residue contacts as one table with
   occupancies: freesasa_gpu_contact_occupancy_open), class splits of the buried area, a contact screen per
   frame, medians, statistics of the volume column.  (Among periodic images: freesasa_gpu_trajectory_file_interface_residues_periodic
   below.) */
int freesasa_gpu_trajectory_interface_residues(const double *xyz_frames, int n_frames, const struct freesasa_ingest_batch *batch, int structure,
                                               int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                               const int32_t *group, int n_groups,
                                               int alg, double probe_radius, int resolution, int frames_per_batch,
                                               double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                               double *sel_area_out, long long *sel_atoms_out, double *group_areas_out, double *iso_out,
                                               const int *devices, int n_devices,
                                               int stats, double *stats_out, double *partials_out,
                                               const int32_t *pairs, int n_pairs, double *pair_areas_out /* [F, K, 6] or NULL */,
                                               double min_buried, double *pair_res_out /* [F, S, 4] or NULL */, char *err, int err_len);
int freesasa_gpu_trajectory_file_interface_residues(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                                    const struct freesasa_ingest_batch *batch, int structure,
                                                    int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                                    const int32_t *group, int n_groups,
                                                    int alg, double probe_radius, int resolution, int frames_per_batch,
                                                    const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                                    const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                                    const char *group_areas_path, const char *iso_path,
                                                    const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                    long long *frames_total_out,
                                                    int stats, const char *stats_path, const char *partials_path,
                                                    const int32_t *pairs, int n_pairs, const char *pair_areas_path,
                                                    double min_buried, const char *pair_res_path, char *err, int err_len);
/* INTERFACES BETWEEN CHAIN GROUPS AMONG PERIODIC IMAGES over a trajectory: the two file entries above for the frames an MD engine
   writes - wrapped into the box, the partners of a complex regularly in different images of it, where the run without cells
   reports a buried area of 0 for the pair.  freesasa_gpu_trajectory_file_interfaces_periodic has the signature of
   freesasa_gpu_trajectory_file_interfaces, freesasa_gpu_trajectory_file_interface_residues_periodic that of
   freesasa_gpu_trajectory_file_interface_residues.  Bit 3 of frames_f32 (FREESASA_GPU_FRAMES_PBC) is REQUIRED (-1 with a message
   that names the non-periodic entry), bit 4 (triclinic cells) is optional; the containers are those that carry a cell: DCD,
   AMBER NetCDF, XTC, TRR.  The run composes freesasa_gpu_trajectory_file_groups_periodic and the interfaces run.  Per frame f, in
   frame f's cell:
     complex          the periodic entry's structure (freesasa_gpu_periodic_dev; with bit 4: _triclinic_dev) of frame f
     isolated group   the periodic entry's structure of the group's atoms alone, among its own images
     pair structure   for pair (g, h): g's atoms in input order, then h's, as the run without cells cuts it - taken as the periodic
                      entry's structure in the same cell, among its OWN images, with the cutoff c of its OWN atoms
   and per frame and pair the six doubles (iso_g, iso_h, in_pair_g, in_pair_h, buried_g, buried_h):
     iso_*      column 0 of the frame's periodic group areas (freesasa_gpu_trajectory_file_groups_periodic), bit for bit
     in_pair_*  the side's areas in the periodic pair structure, summed in the order of the per-structure totals kernel, as above
     buried_*   iso_* - in_pair_*, one subtraction
   The dense per-residue table [F, S, 4], its segments, min_buried, the strict > of in_interface and the statistics bits
   FREESASA_GPU_STATS_PAIRS / _PAIR_RESIDUES are those of the entries above; the table reads the periodic isolated and pair areas.
   Every output shared with freesasa_gpu_trajectory_file_groups_periodic is bit for bit what that run gives, and in cells that give
   no structure an image the pair outputs are bit for bit those of the run without cells.
   Per shard ONE batch goes through the periodic stage and the engine: frames | isolated groups | pair structures, 1 + G + K
   structures and n + n_iso + n_pair atoms per frame, and the images of all of them (csrc/pbc_kernels.h has the layout); the
   expanded batch must not exceed 2^30 atoms and images.  The cell is checked for the COMPLEXES alone: a pair structure's largest
   radius never exceeds its complex's, so its c is no larger and a cell that suffices for the frame suffices for its pairs.
   Class sums, residues, selections, fp32 per-atom output, the statistics word (bits 128 / 256 of it in the _residues_ entry), the
   done-list and device lists work as in the groups' periodic run.  The done-list's first line carries bit 3 (and 4) in its f32=
   word beside pairs= (and minburied=): the lists of this run and of the interfaces run without cells refuse each other, as do
   those of an orthorhombic and a triclinic reading, of other pairs and of another min_buried.
   Argument errors, -1 with a message before a device is touched or a file opened: bit 3 missing; then everything the entries
   above refuse but bit 3 and bit 4.
   Not offered: a memory form (it has no cells); the batch interface entries among periodic images (freesasa_gpu_interfaces_dev:
   its contact screen would have to look among images); contact tables per frame, contact occupancy, exposure masks and volume
   among periodic images. */
int freesasa_gpu_trajectory_file_interfaces_periodic(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                                     const struct freesasa_ingest_batch *batch, int structure,
                                                     int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                                     const int32_t *group, int n_groups,
                                                     int alg, double probe_radius, int resolution, int frames_per_batch,
                                                     const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                                     const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                                     const char *group_areas_path, const char *iso_path,
                                                     const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                     long long *frames_total_out,
                                                     int stats, const char *stats_path, const char *partials_path,
                                                     const int32_t *pairs, int n_pairs, const char *pair_areas_path, char *err, int err_len);
int freesasa_gpu_trajectory_file_interface_residues_periodic(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                                             const struct freesasa_ingest_batch *batch, int structure,
                                                             int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                                             const int32_t *group, int n_groups,
                                                             int alg, double probe_radius, int resolution, int frames_per_batch,
                                                             const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                                             const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                                             const char *group_areas_path, const char *iso_path,
                                                             const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                             long long *frames_total_out,
                                                             int stats, const char *stats_path, const char *partials_path,
                                                             const int32_t *pairs, int n_pairs, const char *pair_areas_path,
                                                             double min_buried, const char *pair_res_path, char *err, int err_len);
/* The segments of such a run, on the host: no device is needed.  *n_segments_out = S is set first; then, when seg_capacity >= S,
   seg_offsets_out [2 K + 1] (the prefix of the segments per side: side j = 2 k + q of pair k owns segments
   [seg_offsets[j], seg_offsets[j + 1])), seg_res_out [S] (the residue of every segment, counted within the structure) and
   seg_atoms_out [S] (its atom count); each may be NULL.  seg_capacity < S: -1, nothing written, the message names S.  The
   refusals of the topology, the group ids and the pairs are the run's, with their messages. */
int freesasa_gpu_trajectory_interface_segments(const struct freesasa_ingest_batch *batch, int structure, const int32_t *group, int n_groups,
                                               const int32_t *pairs, int n_pairs, long long seg_capacity, long long *n_segments_out,
                                               long long *seg_offsets_out, int32_t *seg_res_out, int32_t *seg_atoms_out, char *err, int err_len);
/* W of a statistics word for a system of n_atoms atoms, n_res residues, n_sel selections and n_groups groups; first_out (may be
   NULL) [7] receives the first column of every output in the order above, -1 for one whose bit is not set.  -1: an unknown bit
   or a negative count.  (csrc/trajstats.c: plain C, no allocation, no GPU call.) */
long long freesasa_gpu_traj_stats_width(int stats, long long n_atoms, long long n_res, long long n_sel, long long n_groups,
                                        long long *first_out);
/* ... of the two interface-residue entries: n_pairs pairs and n_segments segments more, first_out [9] (pairs, interface residues
   behind the seven); bits above 256 or a negative count: -1.  With stats <= 127 it is the function above. */
long long freesasa_gpu_traj_stats_width_pairs(int stats, long long n_atoms, long long n_res, long long n_sel, long long n_groups,
                                              long long n_pairs, long long n_segments, long long *first_out);
/* The merge above over n_parts consecutive partials parts [n_parts][4][width] of frames_per_part [n_parts] frames each:
   out [4][width] = mean, std, min, max; frames_total_out (may be NULL) their frames.  Exported so that a caller can merge ANY
   run of consecutive shards of a partials file: block averages, the error estimate of an MD average.  No allocation, no GPU
   call.  -1 (out untouched): a NULL argument, n_parts < 1, a part with fewer than 1 frame, width < 1. */
int freesasa_gpu_traj_stats_merge(const double *parts, const long long *frames_per_part, long long n_parts, long long width,
                                  double *out, long long *frames_total_out);

/* Chain groups: the area of every atom in its complex AND in its group taken on its own (the reference's
   --chain-groups / --separate-chains: freesasa_structure_get_chains_lcl, src/structure.c:1026-1080, minus the
   re-classification), so that iso - sasa is the area an atom buries in the complex.
   d_group [n_atoms] (DEVICE): an int32 group id per atom, local to its structure, -1 = in no group; n_groups
   [n_structs] (HOST): structure s has groups 0 .. n_groups[s] - 1 (0 <= n_groups[s] <= 65535).  Groups are a partition:
   the isolated structure of group (s, g) is the atoms of s with id g, in their order, with the caller's coordinates and
   radii.  An empty group is allowed (totals 0).  alg, probe_radius and resolution as in freesasa_gpu_calc_batch (S&R:
   the points of freesasa_gpu_test_points(resolution)).
   Results (device): d_sasa [n_atoms] the complex areas, bit-identical to freesasa_gpu_lr_batch_dev / _sr_batch_dev on
   the same batch; d_iso [n_atoms] each atom's area in its isolated group, bit-identical to the engine's result for that
   group given as a structure of its own (= d_sasa for atoms with id -1); d_totals [n_structs] (may be NULL) as there;
   d_group_totals [3 G] (may be NULL; G = sum of n_groups, groups k in structure-major order): [3k] the isolated total,
   bit-identical to the engine's d_totals for the isolated structure, [3k + 1] the complex area of the group's atoms,
   summed the same way over them in order, [3k + 2] = [3k] - [3k + 1], the buried area.
   The groups and the complex go through ONE batch (gpu_groups.hip).  Synchronous; batches in flight on the context
   are collected first.  It makes TWO stream synchronizations more than freesasa_gpu_lr_batch_dev: one to read the
   per-group atom counts (they size the combined batch), one at the end.  A group id < -1 or >= n_groups[s] (found on
   the device), a bad n_groups or a NULL argument: -1 with the context's error text, the context stays usable. */
int freesasa_gpu_groups_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                            const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                            double probe_radius, int resolution,
                            double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals);
/* The same on host arrays (group in host memory too), on a pooled per-thread context like freesasa_gpu_calc_batch.
   totals_out, group_totals_out may be NULL.  Returns 0 / -1 with err_out. */
int freesasa_gpu_calc_groups(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                             const int32_t *group, const int32_t *n_groups, int alg, double probe_radius,
                             int resolution, double *sasa_out, double *iso_out, double *totals_out,
                             double *group_totals_out, int device, char *err_out, int err_len);

/* CHAIN GROUPS AMONG PERIODIC IMAGES: the two features above composed - the complex, its groups and the buried area of a
   system whose chains lie in different images of the box (a wrapped MD frame of a complex), with no clustering and no making
   whole by the caller.  The arguments are those of freesasa_gpu_groups_dev / freesasa_gpu_calc_groups with, behind n_groups,
   cells (HOST, [3 n_structs], or cells6 [6 n_structs] for the triclinic entries: the cell of every structure as
   freesasa_gpu_periodic_dev / freesasa_gpu_periodic_triclinic_dev take it) and, last of the outputs, images_out (host,
   [n_structs], may be NULL: the images of every complex).  Group ids, their validation and its message are those of
   freesasa_gpu_groups_dev.  For structure s with cell C_s:
     complex     d_sasa[i] is the periodic entry's area of atom i of s in C_s, d_totals[s] its total: bit for bit
                 freesasa_gpu_periodic_dev (_triclinic_dev) on the same batch and cells
     isolated    d_iso[i] is the periodic entry's area of atom i in the structure made of the atoms of i's group alone - in input
                 order, radii unchanged, in the SAME cell C_s, among that group's own images; the cutoff c = 2 (max radius +
                 probe) of an isolated group is that of ITS OWN atoms, exactly as the periodic entry takes it when handed the
                 group as a structure: bit for bit that entry on the group cut out.  A molecule split over a face is whole in
                 its isolated form too.  An atom with id -1: its complex area, as in freesasa_gpu_groups_dev.
     groups      d_group_totals [3 G]: per group the isolated total (the periodic entry's total of the group as a structure),
                 the complex areas of its atoms reduced by the totals kernels over the gathered array - layout, order and
                 kernels are freesasa_gpu_groups_dev's -, and their difference, the buried area
     cells       a group's max radius never exceeds its complex's, so a cell its complex passes is valid for every group: cells
                 are checked once per complex, and a refusal names the complex with the periodic entries' messages, unchanged
     limit       the atoms of the complexes, the atoms of their groups and the images of both, together at most 2^30 per call
                 (-1 with the three numbers in the message)
   ONE engine run holds complexes, groups and all their images (gpu_periodic.hip); the expansion is the periodic entries', the
   cut the group entry's.  A cell so large and so placed that no atom of s comes within c of a face gives every output of
   freesasa_gpu_groups_dev bit for bit; a right-angled triclinic cell gives the orthorhombic entry's.
   Not offered: exposure masks, volume or pairwise interfaces among periodic images (their entries take no cell).
   Trajectories: freesasa_gpu_trajectory_file_groups_periodic, and with the interfaces between the groups
   freesasa_gpu_trajectory_file_interfaces_periodic. */
int freesasa_gpu_groups_periodic_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                     const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                     const double *cells /* host, [3 n_structs] */, double probe_radius, int resolution,
                                     double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                     int64_t *images_out /* host, [n_structs], may be NULL */);
int freesasa_gpu_groups_periodic_triclinic_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                               const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                               const double *cells6 /* host, [6 n_structs] */, double probe_radius, int resolution,
                                               double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                               int64_t *images_out /* host, [n_structs], may be NULL */);
/* The same on host arrays, on a pooled per-thread context, with the host-batch path's sizing, upload and failure epilogue as
   freesasa_gpu_calc_groups; the cells are checked against the complexes' radii before a device is touched.  totals_out,
   group_totals_out and images_out may be NULL.  Returns 0 / -1 with err_out. */
int freesasa_gpu_calc_groups_periodic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                      const int32_t *group, const int32_t *n_groups, const double *cells, int alg,
                                      double probe_radius, int resolution, double *sasa_out, double *iso_out, double *totals_out,
                                      double *group_totals_out, int64_t *images_out, int device, char *err_out, int err_len);
int freesasa_gpu_calc_groups_periodic_triclinic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                const int32_t *group, const int32_t *n_groups, const double *cells6, int alg,
                                                double probe_radius, int resolution, double *sasa_out, double *iso_out,
                                                double *totals_out, double *group_totals_out, int64_t *images_out, int device,
                                                char *err_out, int err_len);

/* INTERFACES BETWEEN CHAIN GROUPS: which groups of a structure bury each other, and by how much - the interface areas of an
   oligomer, a capsid, an antibody-antigen pair - from ONE call: the chain-group pipeline above, a contact screen between the
   groups on the device, and one more batch that holds only the pairs that touch (csrc/iface_kernels.h, gpu_interfaces.hip;
   tests/interfaces_ref.py restates the definitions in numpy).  Input: that of freesasa_gpu_groups_dev.
   Contact.  Groups g < h of one structure are in contact iff some atom i of g and some atom j of h pass the reference's
     neighbour test (ref: src/nb.c:487-491; nb_test, csrc/sasa_kernels.h), in fp64, every operation rounded on its own:
         ri = radii[i] + probe,  rj = radii[j] + probe,  cut2 = (ri + rj) * (ri + rj),  dx = xj - xi ...
         dx * dx + dy * dy + dz * dz < cut2                                                     (strict)
     The engine admits exactly these pairs as neighbours: groups that are not in contact bury nothing of each other, by
     construction, and get no row.
   Pair table.  P rows, structure-major, then g ascending, then h ascending.  Row p: pair_struct[p] = s, pair_groups[2p], [2p + 1]
     = g, h (local ids), and six doubles pair_areas[6p ..] = iso_g, iso_h, in_pair_g, in_pair_h, buried_g, buried_h:
       iso_*      the group's isolated total: bit for bit column 0 of d_group_totals
       in_pair_*  the total of the group's atoms in the PAIR STRUCTURE of (g, h): the atoms of g in input order, then the atoms
                  of h in input order (two isolated groups of the combined batch, one behind the other), given to the engine
                  as a structure of its own; summed over the side's atoms in order (freesasa_gpu_segment_sums_dev)
       buried_*   = iso_* - in_pair_*
   Per atom (optional).  side_offsets [2P + 1] (int64): the boundaries of every pair's two sides among the M pair-structure
     atoms, side 2p that of g, side 2p + 1 that of h; pair_atom [M] (int32): the input atom of every pair-structure atom;
     pair_buried [M]: that atom's isolated area (d_iso) minus its area in the pair structure.  M is the sum over the rows of
     the atom counts of the row's two groups.
   d_sasa, d_iso, d_totals, d_group_totals: as freesasa_gpu_groups_dev delivers them, bit for bit.
   Capacities.  Every output array is given with its capacity, pair_capacity in rows (pair_struct: 1, pair_groups: 2, pair_areas:
     6 entries a row; side_offsets: 2 a row and one more) and atom_capacity in atoms; nothing is written beyond them.  A call
     whose P or M is larger fails with a message that names the number, after *n_pairs_out and *n_pair_atoms_out are set and
     before any of these arrays is written.  A NULL array is not delivered and its capacity not looked at.
   Refused, with a message that names the structure and the number: more than 4096 groups in one structure (8.4e6 pairs to
     test), more than 2^27 pairs to test in a call, n_atoms + the groups' atoms + M > 2^30; a bad group id or n_groups as by
     freesasa_gpu_groups_dev, with its message.
   Not offered: trajectory drivers, periodic images, pair batches cut into several engine runs, interfaces of more than two
     groups.  (Per-residue tables: freesasa_gpu_interface_residues_dev below; in the file sweep:
     freesasa_gpu_sweep_files_interfaces above.)

   freesasa_gpu_interface_pairs_dev: the screen alone - the chain-group pipeline, then boxes, candidates and contacts - one
     stream synchronization more than freesasa_gpu_groups_dev (the flags come back to the host).  d_sasa, d_iso, d_totals,
     d_group_totals may be NULL.  pair_struct_out [pair_capacity], pair_groups_out [2 pair_capacity]: HOST arrays, as offsets
     and n_groups are (NULL: only the two counts).  stats_out (may be NULL) [2]: the pairs tested and the candidates among them.
   freesasa_gpu_interfaces_dev: the whole pipeline; the arrays after the counts are DEVICE arrays; d_pair_areas is required,
     the others may be NULL.
   freesasa_gpu_calc_interfaces / _calc_interface_pairs: the same on host arrays, on a pooled context like
     freesasa_gpu_calc_groups; sasa_out, iso_out, totals_out, group_totals_out may be NULL.
   All: 0, or -1 with the context's error text / err_out; the context stays usable. */
int freesasa_gpu_interface_pairs_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                     const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                     double probe_radius, int resolution,
                                     double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                     long long pair_capacity, long long *n_pairs_out, long long *n_pair_atoms_out,
                                     int32_t *pair_struct_out, int32_t *pair_groups_out, long long *stats_out);
int freesasa_gpu_interfaces_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                double probe_radius, int resolution,
                                double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                long long pair_capacity, long long atom_capacity, long long *n_pairs_out, long long *n_pair_atoms_out,
                                int32_t *d_pair_struct, int32_t *d_pair_groups, double *d_pair_areas,
                                int64_t *d_side_offsets, int32_t *d_pair_atom, double *d_pair_buried);
int freesasa_gpu_calc_interface_pairs(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                      const int32_t *group, const int32_t *n_groups, int alg, double probe_radius, int resolution,
                                      long long pair_capacity, long long *n_pairs_out, long long *n_pair_atoms_out,
                                      int32_t *pair_struct_out, int32_t *pair_groups_out, long long *stats_out,
                                      int device, char *err_out, int err_len);
int freesasa_gpu_calc_interfaces(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                 const int32_t *group, const int32_t *n_groups, int alg, double probe_radius, int resolution,
                                 double *sasa_out, double *iso_out, double *totals_out, double *group_totals_out,
                                 long long pair_capacity, long long atom_capacity, long long *n_pairs_out, long long *n_pair_atoms_out,
                                 int32_t *pair_struct_out, int32_t *pair_groups_out, double *pair_areas_out,
                                 int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out,
                                 int device, char *err_out, int err_len);

/* PER-RESIDUE INTERFACE TABLES: which residues make up every interface above, and how much each loses - the interface-residue
   table of an assembly analysis - made on the device behind the interface pipeline and delivered compact: only the residues
   that lose area get a row, so the table's size is decided by areas and known to the device alone (csrc/iface_kernels.h,
   IfaceResArgs; tests/interface_residues_ref.py restates the definitions in numpy).
   Input: that of freesasa_gpu_interfaces_dev, and
     res_first [n_res + 1]  a HOST int64 array: the residue boundaries over the input batch, as freesasa_ingest_batch.res_first
                            has them; residue r owns the input atoms res_first[r] .. res_first[r + 1] - 1
     min_buried             a double, see Rows
   Everything of the interface definition stays: the pair table, the sides' order, side_offsets, pair_atom, pair_buried, and
   their bytes.
   Segments.  Within side q of the pair table (q = 2p: group g, q = 2p + 1: group h) the pair-structure atoms are in input
     order.  A SEGMENT is a maximal run of consecutive atoms of one side whose input atoms lie in the same residue.  The atoms of
     a residue are contiguous in the input, so a segment is all atoms of that residue that belong to the side's group.  Group
     ids are arbitrary: a residue split over several groups gives one segment in every side it occurs in.  Atoms in no group
     occur in no segment; empty residues (res_first[r] == res_first[r + 1]) occur in none.
   Sums per segment, each in strict atom order, one addition at a time from 0 (as freesasa_gpu_segment_sums_dev and
     freesasa_gpu_residue_areas_dev sum), fp64, every operation rounded on its own:
       iso_res      the sum of d_iso[pair_atom[m]] over the segment's atoms m
       in_pair_res  the sum of those atoms' areas in the pair structure (what in_pair_* sums over the whole side)
       buried_res   = iso_res - in_pair_res, the convention of the pair row's buried_* = iso_* - in_pair_*
   Rows.  A segment gets a row iff buried_res > min_buried (strict, fp64).  The R rows are in segment order: pair-major, side g
     before side h, residues ascending.  Row k: res_index[k] (int32) the batch-wide residue r, res_atoms[k] (int32) the atoms
     of the segment, res_areas[3k ..] = iso_res, in_pair_res, buried_res.  res_offsets [2P + 1] (int64): the row range of
     every side, in the order of side_offsets; a side with no rows has an empty range; res_offsets[2P] = R.
   min_buried.  With Shrake-Rupley a residue none of whose atoms loses a test point has buried_res == 0 exactly (its atoms'
     areas in the pair structure are those of the isolated group bit for bit), so min_buried = 0 gives exactly the residues that
     lose a test point.  With Lee-Richards nobody has measured whether an atom without a neighbour across the interface has the
     same area to the last bit in the pair structure as in its isolated group: min_buried is the caller's instrument against
     rows made of such last bits.  No tolerance is built in.
   Capacities.  As above, with res_capacity in rows (res_index, res_atoms: 1, res_areas: 3 entries a row; res_offsets goes by
     pair_capacity: 2 a row and one more).  *n_pairs_out, *n_pair_atoms_out and *n_res_rows_out are set first, then the three
     capacities are held against them in this order; a res_capacity below R fails with
     "res_capacity %lld is too small: the interfaces have %lld residue rows" before any of the caller's pair, atom or residue
     arrays is written.  R <= M: arrays of M rows always suffice.
   Refused with a message before a device is touched: everything the interface entries refuse, with their messages; res_first
     NULL or n_res <= 0; res_first[0] != 0, a decreasing entry, res_first[n_res] != offsets[n_structs]; a residue that spans
     a structure boundary (the message names residue and structures); min_buried negative, NaN or infinite; res_capacity < 0.
   One stream synchronization more than freesasa_gpu_interfaces_dev (R comes back to the host before delivery).
   Not offered: class splits (polar / apolar / main chain) of the buried area per residue, relative buried areas, per-residue
     tables in the trajectory drivers, interfaces among periodic images in the batch entries (over a trajectory:
     freesasa_gpu_trajectory_file_interfaces_periodic), a per-atom contact criterion by distance.  (In the file sweep,
     with the buried area of every side split by class: freesasa_gpu_sweep_files_interfaces above.)

   freesasa_gpu_interface_residues_dev: d_res_areas is required, d_res_offsets, d_res_index, d_res_atoms may be NULL; the rest
     as freesasa_gpu_interfaces_dev.
   freesasa_gpu_calc_interface_residues: the same on host arrays, as freesasa_gpu_calc_interfaces.
   Both: 0, or -1 with the context's error text / err_out; the context stays usable. */
int freesasa_gpu_interface_residues_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                        const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                        const int64_t *res_first, int n_res, double probe_radius, int resolution, double min_buried,
                                        double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                        long long pair_capacity, long long atom_capacity, long long res_capacity,
                                        long long *n_pairs_out, long long *n_pair_atoms_out, long long *n_res_rows_out,
                                        int32_t *d_pair_struct, int32_t *d_pair_groups, double *d_pair_areas,
                                        int64_t *d_side_offsets, int32_t *d_pair_atom, double *d_pair_buried,
                                        int64_t *d_res_offsets, int32_t *d_res_index, int32_t *d_res_atoms, double *d_res_areas);
int freesasa_gpu_calc_interface_residues(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                         const int32_t *group, const int32_t *n_groups, const int64_t *res_first, int n_res,
                                         int alg, double probe_radius, int resolution, double min_buried,
                                         double *sasa_out, double *iso_out, double *totals_out, double *group_totals_out,
                                         long long pair_capacity, long long atom_capacity, long long res_capacity,
                                         long long *n_pairs_out, long long *n_pair_atoms_out, long long *n_res_rows_out,
                                         int32_t *pair_struct_out, int32_t *pair_groups_out, double *pair_areas_out,
                                         int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out,
                                         int64_t *res_offsets_out, int32_t *res_index_out, int32_t *res_atoms_out,
                                         double *res_areas_out, int device, char *err_out, int err_len);

/* ATOM-ATOM CONTACT TABLES: what is in contact with what across every interface above - which atom of the partner buries which
   atom, and how much area each such pair accounts for: the contact map of an interface analysis.  Made on the device behind
   the interface pipeline from Shrake-Rupley exposure masks (csrc/contact_kernels.h; tests/interface_contacts_ref.py restates
   the definitions in numpy).  Shrake-Rupley only; fp64, every operation rounded on its own.
   Input: that of freesasa_gpu_interfaces_dev with alg = 1; N = resolution <= 128 test points u_k = freesasa_gpu_test_points(N);
     R_i = r_i + probe.  Everything of the interface definition stays: the pair table, side_offsets, pair_atom, pair_buried and
     their bytes.  Pair-structure atom i (0 <= i < M) lies on one side of one pair structure p = (g, h).
   Masks (as freesasa_gpu_sr_masks_dev makes them).  side_mask_i: atom i's exposure mask with its side taken as a structure of
     its own (the bits behind d_iso); pair_mask_i: its mask in the pair structure (the bits behind in_pair_*).
     buried_mask_i = side_mask_i & ~pair_mask_i over the N bits that exist: the test points the partner buries; bits at or above
     N are 0; its popcount is counts_side_i - counts_pair_i.
   Test point of set bit k: per component t = u_k * R_i; t += x_i (the engine's own, as the surface dots have it).
   Cover.  Atom j of the OTHER side of the same pair covers the point iff dx * dx + dy * dy + dz * dz <= R_j * R_j, dx = t_x - x_j
     and so on (the reference's operand order, src/sasa_sr.c:321-324).
   Partner.  The covering j with the smallest w = (dx * dx + dy * dy + dz * dz) - R_j * R_j: the deepest penetration; among equal
     w the smallest pair-structure index.  By the definition of the two masks a cover exists; if the device finds none the call
     fails with a message that names the pair-structure atom - it never invents a partner.
   Rows.  One row per (i, j) with at least one point, ordered by i ascending over all M atoms, then j ascending:
     contact_first [M + 1] (int64)  the exclusive prefix of the rows per atom; C = contact_first[M]
     contact_partner [C] (int32)    j, a pair-structure atom index: pair_atom[j] is the input atom
     contact_points [C] (int32)     n, the number of i's buried points whose partner is j
     contact_area [C] (fp64)        (4.0 * PI * R_i * R_i * n) / N, the reference's expression (src/sasa_sr.c:337)
     The table is directed: row (i -> j) lies in i's run, row (j -> i) in j's; they generally differ, nothing symmetrises them.
   Optional: buried_masks [M][4] (uint32, 16-byte aligned; freesasa_gpu_dots_from_masks draws the interface patch from it with
     the pair-structure atoms' coordinates) and dot_partner [D_b] (int32): the partner of every buried point in dot order (atom
     ascending, point ascending); D_b = the buried points of all atoms.
   Capacities.  As above: pair_capacity and atom_capacity (contact_first: atom_capacity + 1 entries; buried_masks: 4 words an
     atom), contact_capacity in rows, dot_capacity in dots.  The four counts are set first, then the capacities are held against
     P, M, C and D_b in this order; one that is too small fails with a message that names the number - "contact_capacity %lld is
     too small: the interfaces have %lld contact rows" - before any of the caller's arrays is written.  A NULL array is not
     delivered and its capacity not looked at.  C <= D_b <= M N.
   P == 0 or no buried point: C = 0 and contact_first, where delivered, is all zeros ([1] without a pair, [M + 1] otherwise).
   Refused with a message before a device is touched: everything the interface entries refuse; Lee-Richards; N > 128; a negative
     capacity; d_buried_masks not aligned to 16 bytes.  Refused with the mask request's messages (freesasa_gpu_sr_masks_dev):
     FREESASA_AMD_SR_CAPS=0, tiles beyond the cap-mask kernel's 128 records per atom.  More than 2^31 - 1 buried points.
   Two engine runs over the M pair-structure atoms and two stream synchronizations more than freesasa_gpu_interfaces_dev (D_b
     comes back before the arrays it sizes are made, then C and the flag of a dot without a cover).
   Not offered: Lee-Richards; the file sweep and the trajectory drivers; periodic images; class splits; a table with both
     directions added.  (The fold of the rows per residue pair: freesasa_gpu_interface_residue_contacts_dev below; over the
     frames of a run: freesasa_gpu_contact_occupancy_open.)

   freesasa_gpu_interface_contacts_dev: the arrays after the counts are DEVICE arrays; d_pair_areas is required, every other
     array and n_buried_dots_out may be NULL; the rest as freesasa_gpu_interfaces_dev.
   freesasa_gpu_calc_interface_contacts: the same on host arrays, on a pooled context, as freesasa_gpu_calc_interface_residues.
   Both: 0, or -1 with the context's error text / err_out; the context stays usable. */
int freesasa_gpu_interface_contacts_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                        const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                        double probe_radius, int resolution,
                                        double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                        long long pair_capacity, long long atom_capacity, long long contact_capacity, long long dot_capacity,
                                        long long *n_pairs_out, long long *n_pair_atoms_out, long long *n_contacts_out,
                                        long long *n_buried_dots_out,
                                        int32_t *d_pair_struct, int32_t *d_pair_groups, double *d_pair_areas,
                                        int64_t *d_side_offsets, int32_t *d_pair_atom, double *d_pair_buried,
                                        int64_t *d_contact_first, int32_t *d_contact_partner, int32_t *d_contact_points,
                                        double *d_contact_area, uint32_t *d_buried_masks, int32_t *d_dot_partner);
int freesasa_gpu_calc_interface_contacts(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                         const int32_t *group, const int32_t *n_groups, int alg, double probe_radius, int resolution,
                                         double *sasa_out, double *iso_out, double *totals_out, double *group_totals_out,
                                         long long pair_capacity, long long atom_capacity, long long contact_capacity, long long dot_capacity,
                                         long long *n_pairs_out, long long *n_pair_atoms_out, long long *n_contacts_out,
                                         long long *n_buried_dots_out,
                                         int32_t *pair_struct_out, int32_t *pair_groups_out, double *pair_areas_out,
                                         int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out,
                                         int64_t *contact_first_out, int32_t *contact_partner_out, int32_t *contact_points_out,
                                         double *contact_area_out, uint32_t *buried_masks_out, int32_t *dot_partner_out,
                                         int device, char *err_out, int err_len);

/* RESIDUE-RESIDUE CONTACT TABLES: which residue is in contact with which residue across every interface above, and over how
   much area - the contact rows above folded per pair of residues on the device, each folded row linked to the row that runs the
   other way (csrc/rescontact_kernels.h; tests/interface_residue_contacts_ref.py restates the definitions in numpy).  fp64, every
   operation rounded on its own.
   Input: that of freesasa_gpu_interface_contacts_dev, and res_first [n_res + 1], a HOST int64 array, exactly as
     freesasa_gpu_interface_residues_dev takes it (the same checks, the same messages).  Every output of the contact entry is
     delivered byte for byte.
   Segments.  Those of the per-residue tables: a maximal run of one side's pair-structure atoms whose input atoms lie in one
     residue; K of them, numbered pair-major, side g before side h.  Within one side a residue has at most one segment, so on the
     other side of a given pair "partner residue" and "partner segment" are the same thing.  A residue split over two groups has
     a segment on both sides of their pair and may be in contact with itself: a legal row whose two residues are equal and
     whose segments differ.
   Folded rows.  Segment a with atoms b .. e-1 has the contact rows contact_first[b] .. contact_first[e] - 1 (contiguous: i
     ascending, then j ascending).  They are folded by the residue of pair_atom[contact_partner[t]]: one folded row per distinct
     partner residue, the partner residues ascending, with
       n_rows (int32)    the contact rows folded
       n_points (int32)  the sum of their contact_points
       area (fp64)       the sum of their contact_area in row order, one addition at a time from 0
     The Q folded rows are in segment order: pair-major, side g before side h, source residue ascending, then partner residue
     ascending.
     rescontact_offsets [2P + 1] (int64)   the row range of every source side, in the order of side_offsets; [2P] = Q
     rescontact_residues [Q][2] (int32)    the batch-wide residue of the source and of the partner
     rescontact_counts [Q][2] (int32)      n_rows, n_points
     rescontact_area [Q] (fp64)
     rescontact_reverse [Q] (int32)        the folded row of the same pair that runs from the partner segment to the source
                                           segment, or -1: the partner buries points of the source and loses none to it (the
                                           small atom inside the large one does not bury the large one).  reverse[k] = r >= 0
                                           gives reverse[r] = k and the two rows' residues swapped.
     Nothing else symmetrises the table: the caller adds or averages the two directions as they see fit.
   Capacities.  As above, with rescontact_capacity in rows (rescontact_offsets goes by pair_capacity).  The five counts are set
     first, then the capacities are held against P, M, C, D_b and Q in this order - "rescontact_capacity %lld is too small: the
     interfaces have %lld residue contact rows" - before any of the caller's arrays is written.  Q <= C: arrays of C rows always
     suffice.
   P == 0 or no buried point: Q = 0 and rescontact_offsets, where delivered, is all zeros ([1] without a pair).
   Refused with a message before a device is touched: everything the contact entry refuses, everything the per-residue entry
     refuses about res_first and n_res, rescontact_capacity < 0.
   One stream synchronization more than freesasa_gpu_interface_contacts_dev (Q comes back to the host before delivery).
   Not offered: Lee-Richards; the file sweep and the trajectory drivers (the frames of a run reduced to one table of residue
     pairs: freesasa_gpu_contact_occupancy_open below); periodic images; class splits; a table with both directions added (the
     occupancy table's frames_either counts both).

   freesasa_gpu_interface_residue_contacts_dev: the contact entry's arguments, then res_first, n_res, rescontact_capacity,
     n_rescontacts_out and the five DEVICE arrays; d_rescontact_area is required, the other four may be NULL and are then not
     delivered.
   freesasa_gpu_calc_interface_residue_contacts: the same on host arrays, on a pooled context, as its siblings.
   Both: 0, or -1 with the context's error text / err_out; the context stays usable. */
int freesasa_gpu_interface_residue_contacts_dev(freesasa_gpu_ctx *ctx, int alg, const double *d_xyz, const double *d_radii,
                                                const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                                double probe_radius, int resolution,
                                                double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                                long long pair_capacity, long long atom_capacity, long long contact_capacity,
                                                long long dot_capacity,
                                                long long *n_pairs_out, long long *n_pair_atoms_out, long long *n_contacts_out,
                                                long long *n_buried_dots_out,
                                                int32_t *d_pair_struct, int32_t *d_pair_groups, double *d_pair_areas,
                                                int64_t *d_side_offsets, int32_t *d_pair_atom, double *d_pair_buried,
                                                int64_t *d_contact_first, int32_t *d_contact_partner, int32_t *d_contact_points,
                                                double *d_contact_area, uint32_t *d_buried_masks, int32_t *d_dot_partner,
                                                const int64_t *res_first, int n_res, long long rescontact_capacity,
                                                long long *n_rescontacts_out, int64_t *d_rescontact_offsets,
                                                int32_t *d_rescontact_residues, int32_t *d_rescontact_counts,
                                                double *d_rescontact_area, int32_t *d_rescontact_reverse);
int freesasa_gpu_calc_interface_residue_contacts(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                 const int32_t *group, const int32_t *n_groups, int alg, double probe_radius,
                                                 int resolution,
                                                 double *sasa_out, double *iso_out, double *totals_out, double *group_totals_out,
                                                 long long pair_capacity, long long atom_capacity, long long contact_capacity,
                                                 long long dot_capacity,
                                                 long long *n_pairs_out, long long *n_pair_atoms_out, long long *n_contacts_out,
                                                 long long *n_buried_dots_out,
                                                 int32_t *pair_struct_out, int32_t *pair_groups_out, double *pair_areas_out,
                                                 int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out,
                                                 int64_t *contact_first_out, int32_t *contact_partner_out, int32_t *contact_points_out,
                                                 double *contact_area_out, uint32_t *buried_masks_out, int32_t *dot_partner_out,
                                                 const int64_t *res_first, int n_res, long long rescontact_capacity,
                                                 long long *n_rescontacts_out, int64_t *rescontact_offsets_out,
                                                 int32_t *rescontact_residues_out, int32_t *rescontact_counts_out,
                                                 double *rescontact_area_out, int32_t *rescontact_reverse_out,
                                                 int device, char *err_out, int err_len);

/* RESIDUE CONTACT OCCUPANCY MAP: over the frames of a run, in how many frames residue a of one chain group touches residue b of
   another, and over how much area when it does - the folded rows above, made per frame and reduced on the device into ONE table
   by a streaming accumulator (csrc/occupancy_kernels.h; tests/contact_occupancy_ref.py restates the definitions in plain
   Python).  Frames go in, in any cut; the per-frame tables never leave the device; the table that comes out is byte for byte
   the same however the frames were cut.
   The system: n_atoms atoms with radii [n], group [n] (int32; -1: in no group, 0 <= id < n_groups) and res_first [n_res + 1], a
     HOST int64 array exactly as freesasa_gpu_interface_residues_dev takes it - all constant over the run.  Shrake-Rupley with
     resolution <= 128 points.
   A frame's rows: frame f as a batch of one structure - its coordinates, radii, group, n_groups, res_first - has the folded rows of
     freesasa_gpu_interface_residue_contacts_dev: P_f pairs, Q_f rows.  Nothing of that definition changes; the contact screen per
     frame stays.
   Key.  The key of a folded row is (g, h, side, res_a, res_b): (g, h) its pair, side 0 if the source segment is in g and 1 if in
     h, res_a / res_b the source and the partner residue, counted within the system.  A frame's keys ascend strictly as
     5-tuples.  The REVERSED key of (g, h, s, a, b) is (g, h, 1 - s, b, a).
   The run table after F frames: one row per distinct key seen so far, the U rows ascending by key, with
     keys [U][5] (int32)
     frames [U] (int64)          the frames in which the key has a folded row
     frames_either [U] (int64)   the frames in which the key OR its reversed key has one: the symmetric occupancy a map plots
     counts [U][2] (int64)       the sums over those frames of n_rows and of n_points
     area [U][3] (fp64)          sum, min, max over the frames in which the key is present; the sum in frame order, one addition
                                 at a time from 0.0, no fma
     span [U][2] (int64)         the first and the last frame (0-based in the run) in which the key is present
     reverse [U] (int32)         the row of the reversed key, or -1; reverse[k] = r >= 0 gives reverse[r] = k and
                                 frames_either[k] == frames_either[r]; with reverse[k] == -1, frames_either[k] == frames[k]
     Occupancy is frames / F, the mean area in contact area[0] / frames: the caller divides.
   Cut independence.  The table after F frames is a function of the F frames in order and of nothing else: not of how they were
     split over add calls, of frames_per_batch, of when snapshots were taken, of the launch shape.
   Failure.  What is refused before the device is touched leaves the handle usable.  An add that fails behind that poisons the
     handle: every later call but _close and _error returns -1 with the first failure's message - no partially merged table is
     ever delivered.  No call throws.
   Limits, refused with a message that names the number: U, or the folded rows of a chunk, beyond 2^31 - 1; everything the
     interface pipeline refuses, with its text behind the run's frame number(s).
   Not offered: Lee-Richards; periodic images; caller-named pairs (all pairs in contact are tabulated); atom-level occupancy;
     standard deviations and medians of the area; the file drivers, done-lists and multi-device runs (partial tables of two
     devices can be combined through _add_rows only per frame, not per table); a solvent gather (atom_index: pass the solute's
     coordinates); trajectory containers (the device decoders have no memory form: the caller's own reader feeds _add_frames).

   freesasa_gpu_contact_occupancy_open: the accumulator, or NULL with err.  radii == NULL and n_atoms == 0: an accumulator for
     rows only (_add_frames refuses it; group, res_first and the resolution are not looked at).  Refused before a device is touched:
     everything the residue-residue contact entry refuses about group, n_groups, res_first, n_res and the resolution, with its
     messages; a group id outside -1 .. n_groups - 1.  frames_per_batch: the frames of a chunk, one run of the interface pipeline;
     <= 0: the trajectory drivers' rule, 1250000 / atoms + 1, on THREE times the system's atoms - the frame, its isolated groups
     and a pair structure's worth.  Either is lowered to what the pipeline takes: 2^30 atoms (three to an atom) and 2^27 pairs of
     groups to a call, chunk-wide residue numbers below 2^31.  The handle keeps a pooled context until it is closed.
   freesasa_gpu_contact_occupancy_add_frames: xyz_frames [f][n][3] (host) are the run's next f frames; frame_counts_out [f][2]
     (int64, may be NULL) receives (P_f, Q_f).  Per chunk the coordinates go up and the pipeline runs with capacities that hold
     anything; nothing per row comes back - one stream synchronization more than the pipeline's own, for the number of new keys.
   freesasa_gpu_contact_occupancy_add_rows: the run's next f frames as rows the caller has already - from the batch entry, a file
     sweep, another run: frame_first [f + 1] (int64), keys [q][5], counts [q][2] (int32: n_rows, n_points), area [q], host arrays,
     through the same reduction.  Checked on the host before anything goes up, the frame and the row named in the message:
     frame_first begins at 0 and does not descend; 0 <= g < h; side 0 or 1; residues >= 0; a frame's keys strictly ascending; both
     counts >= 1; a finite area.
   freesasa_gpu_contact_occupancy_table: a snapshot of the run table in host arrays of the library's (of one element where the
     table has no row), to be given back with _table_free; the accumulator goes on.  n_frames: the frames added so far.
   freesasa_gpu_contact_occupancy_close: NULL is allowed.  _error: the text of the last failure of the handle.
   freesasa_gpu_calc_contact_occupancy: open, _add_frames over all frames, _table, close, on host arrays; the message in err_out.
   All: 0, or -1 with the message. */
typedef struct freesasa_gpu_contact_occupancy freesasa_gpu_contact_occupancy;
typedef struct {
    long long n_frames, n_rows;
    int32_t *keys;
    int64_t *frames, *frames_either, *counts;
    double *area;
    int64_t *span;
    int32_t *reverse;
} freesasa_gpu_contact_occupancy_table_t; /* (a type and a function cannot share a name in C) */
freesasa_gpu_contact_occupancy *freesasa_gpu_contact_occupancy_open(const double *radii, int n_atoms, const int32_t *group, int n_groups,
                                                                    const int64_t *res_first, int n_res, double probe_radius,
                                                                    int resolution, int frames_per_batch, int device, char *err_out,
                                                                    int err_len);
int freesasa_gpu_contact_occupancy_add_frames(freesasa_gpu_contact_occupancy *o, const double *xyz_frames, int n_frames,
                                              int64_t *frame_counts_out);
int freesasa_gpu_contact_occupancy_add_rows(freesasa_gpu_contact_occupancy *o, int n_frames, const int64_t *frame_first,
                                            const int32_t *keys, const int32_t *counts, const double *area);
int freesasa_gpu_contact_occupancy_table(freesasa_gpu_contact_occupancy *o, freesasa_gpu_contact_occupancy_table_t *out);
void freesasa_gpu_contact_occupancy_table_free(freesasa_gpu_contact_occupancy_table_t *t);
void freesasa_gpu_contact_occupancy_close(freesasa_gpu_contact_occupancy *o);
const char *freesasa_gpu_contact_occupancy_error(const freesasa_gpu_contact_occupancy *o);
int freesasa_gpu_calc_contact_occupancy(const double *xyz_frames, int n_frames, const double *radii, int n_atoms, const int32_t *group,
                                        int n_groups, const int64_t *res_first, int n_res, double probe_radius, int resolution,
                                        int frames_per_batch, int64_t *frame_counts_out, freesasa_gpu_contact_occupancy_table_t *out,
                                        int device, char *err_out, int err_len);

/* MOLECULAR VOLUME: the volume enclosed by the solvent-accessible surface of every structure, made of the Shrake-Rupley test
   points by the divergence theorem - what `gmx sasa -tv` prints per frame, in the same formulation:
       V = (1/3) sum_i a_i ( (x_i - o) . E_i + R_i n_i ),   E_i = sum over atom i's exposed points of u_k,  a_i = 4 pi R_i^2 / N
   The definition (csrc/vol_kernels.h; tests/volume_ref.py restates it in numpy).  fp64, every operation rounded on its own.
   Structure s, atoms b .. e-1, probe p, the N points u_k of freesasa_gpu_test_points(N):
     radius     R_i = r_i + p
     exposure   what the engine decides for the areas: t = u_k * R_i; t += x_i; covered iff for some other atom j
                dx^2 + dy^2 + dz^2 <= R_j * R_j.  n_i is the `counts` output.
     E_i        from (0, 0, 0); for k = 0 .. N-1 ascending, if point k is exposed, += u_k component by component: evec[3i .. 3i+2]
     origin     per axis o_s = (min_i x_i + max_i x_i) * 0.5 over the structure's atoms (one atom: o = x exactly)
     per atom   a = (4.0 * PI * R_i * R_i) / N;  d = x_i - o_s;  t = d_x * E_x + d_y * E_y + d_z * E_z, left to right;
                v_i = (a * (t + R_i * (double) n_i)) / 3.0
     volume     V_s = the engine's totals kernels over v (the sum that makes d_totals of the areas): deterministic, independent
                of launch shape, tile shape, device list, shard cut and restarts.  A structure without atoms: 0.
   A lone sphere gives 4/3 pi R^3 to the last bits at any N; two overlapping spheres of 3 A whose centres are 3 A apart along x:
   -0.9 % at 100 points, -0.2 % at 1000, +0.01 % at 5000 against the analytic union (tests/test_volume.py).
   The batch goes through the engine ONCE: d_sasa, d_counts and d_totals are bit for bit freesasa_gpu_sr_batch_dev's with the
   points of freesasa_gpu_test_points(n_points); E_i is one more output of the tile kernel's store phase (the mask of covered
   points never leaves the LDS), the rest two small kernels and the totals behind it.
   freesasa_gpu_sr_volume_dev: arrays on the device, offsets on the host; synchronous; batches in flight on the context are
   collected first.  d_counts [n], d_evec [3 n], d_vol [n] and d_totals [n_structs] may be NULL (the context keeps scratch of
   its own for the ones it needs); d_volumes [n_structs] is required.
   REFUSED, -1 with a message that names the reason, nothing returned: more than 128 test points; test points that are not
   unit vectors; FREESASA_AMD_SR_CAPS=0; a launch, or tiles of a batch, whose neighbour lists are beyond the cap-mask
   kernel's limits (more than 128 records per atom) and run the engine's second arrangement.  A volume made any other way
   is never returned.  The context stays usable.  Argument errors (NULL, n_points <= 0, bad offsets, an empty batch): -1
   with a message before a device is touched.
   Not offered: density (mass over V: the loader does no arithmetic and the batch holds no masses); Lee-Richards volume;
   more than 128 points; volume among periodic images; volume in the plain (radii, n_atoms) trajectory entries, the group
   entries and the file and cache sweeps; run statistics of the volume column (per-frame volumes are 8 bytes a frame, and
   freesasa_gpu_traj_stats_merge is exported for block averages); Connolly dot output (`gmx sasa -q`). */
int freesasa_gpu_sr_volume_dev(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                               int n_structs, double probe_radius, int n_points, double *d_sasa, int *d_counts, double *d_evec,
                               double *d_vol, double *d_totals, double *d_volumes);
/* The same on host arrays, on a pooled per-thread context like freesasa_gpu_calc_batch.  counts_out, evec_out, vol_out and
   totals_out may be NULL; sasa_out [n] and volumes_out [n_structs] are required.  Returns 0 / -1 with err_out. */
int freesasa_gpu_calc_volume(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, double probe_radius,
                             int n_points, double *sasa_out, int *counts_out, double *evec_out, double *vol_out,
                             double *totals_out, double *volumes_out, int device, char *err_out, int err_len);
/* ... and per frame of a trajectory: freesasa_gpu_trajectory_topology / freesasa_gpu_trajectory_file_topology with one more
   output behind sel_atoms_out
     volumes     1 per frame          (8 f)            V of the frame's topology atoms: bit for bit volumes_out of
                                                       freesasa_gpu_calc_volume on the frame taken as a structure of its own
   (memory form: volumes_out [n_frames]; file form: volumes_path, raw fp64, frame f at byte 8 f; required).  The solute index,
   residues, class sums and selections are what they are there, every other output byte for byte that entry's; all file formats,
   fp32 input, fp32 per-atom output and any device list work unchanged.  alg must be Shrake-Rupley (1).  The done-list's first
   line names the volume output (64 in outputs=): a list of a run without it and a list of a run with it refuse each other.
   -1 with a message before a device is touched or a file opened: volumes NULL, Lee-Richards, more than 128 points, bit 3 or 4
   of frames_f32 (among periodic images the surface is not closed within the cell). */
int freesasa_gpu_trajectory_volume(const double *xyz_frames, int n_frames, const struct freesasa_ingest_batch *batch, int structure,
                                   int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                   int alg, double probe_radius, int resolution, int frames_per_batch,
                                   double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                   double *sel_area_out, long long *sel_atoms_out, double *volumes_out,
                                   const int *devices, int n_devices, char *err, int err_len);
int freesasa_gpu_trajectory_file_volume(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                        const struct freesasa_ingest_batch *batch, int structure,
                                        int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                        int alg, double probe_radius, int resolution, int frames_per_batch,
                                        const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                        const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                        const char *volumes_path,
                                        const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                        long long *frames_total_out, char *err, int err_len);

/* EXPOSURE MASKS AND SURFACE DOTS: which Shrake-Rupley test points of every atom are exposed, and those points in space - the
   Connolly dots of `gmx sasa -q`.  The mask is the compact, lossless form of the dots (16 bytes per atom, where the dots of a
   protein atom take about 600): counts, dots and anything else made of the exposed points follow from it later without the engine.
   The definitions (csrc/dots_kernels.h; tests/dots_ref.py restates them in numpy).  Probe p, the N = n_points unit points u_k
   of freesasa_gpu_test_points(N), R_i = r_i + p:
     mask        uint32 [n_atoms][4], atoms in the caller's order: bit k & 31 of word k >> 5 of atom i is SET iff point k of atom
                 i is EXPOSED (by the engine's own test: what makes `counts`); bits k >= N are 0; popcount(mask_i) == counts[i]
     dot_first   int64 [n_atoms + 1]: the exclusive prefix sum of popcount(mask_i & the N bits that exist), taken from the masks
                 themselves.  D = dot_first[n_atoms]; the dots of structure s are dot_first[offsets[s]] .. dot_first[offsets[s + 1]]
     dots        for atom i ascending, within it for exposed k ascending, one dot at slot dot_first[i] + rank:
                 dot_xyz[3 slot ..] fp64, per component t = u_k * R_i; t += x_i - the engine's own test point, every operation
                 rounded on its own; optional dot_atom[slot] = i and dot_point[slot] = k (int32)
   The outward normal of a dot is u_k (freesasa_gpu_test_points(N)[dot_point]) and the area it stands for 4 pi R_i^2 / N: no array
   is delivered for either.
   freesasa_gpu_sr_masks_dev: freesasa_gpu_sr_batch_dev with the masks kept: arrays on the device, offsets on the host,
   synchronous.  d_sasa, d_counts and d_totals are that entry's bit for bit (d_counts, d_totals may be NULL); d_masks
   [n_atoms][4] is required, here and in the two entries below aligned to 16 bytes (-1 with a message otherwise).  The batch goes through the engine ONCE: the mask is one more output of the tile kernel's store
   phase, written in one 16-byte store per atom.
   REFUSED, -1 with a message that names the reason, nothing returned: more than 128 test points; test points that are not unit
   vectors; FREESASA_AMD_SR_CAPS=0; a launch, or tiles of a batch, whose neighbour lists are beyond the cap-mask kernel's limits
   (more than 128 records per atom) and run the engine's second arrangement.  A mask made any other way is never returned.  The
   context stays usable.  Argument errors (NULL, n_points <= 0, bad offsets, an empty batch): -1 before a device is touched.
   freesasa_gpu_dots_count_dev: dot_first of masks that are on the device (three plain launches; everything int64: 2^24 atoms
   with 128 exposed points have more than 2^31 dots) and D into *n_dots_out; synchronous.
   freesasa_gpu_dots_expand_dev: the dots of masks and their dot_first, into arrays that hold `capacity` dots: nothing is ever
   written at or beyond slot `capacity`, or outside an atom's own run of slots, whatever the masks and dot_first say; bits at or
   above n_points are ignored.  d_dot_atom and d_dot_point may be NULL.  D == 0 or capacity == 0: nothing is launched.
   Not offered: more than 128 points; Lee-Richards; masks among periodic images; masks in the plain (radii, n_atoms) trajectory
   entries, the group entries and the file and cache sweeps; fp32 dots; the volume's E_i made from stored masks instead of in
   the store phase (masks and the volume in one batch are refused: one store phase makes one of them). */
int freesasa_gpu_sr_masks_dev(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                              int n_structs, double probe_radius, int n_points, double *d_sasa, int *d_counts, double *d_totals,
                              uint32_t *d_masks);
int freesasa_gpu_dots_count_dev(freesasa_gpu_ctx *ctx, const uint32_t *d_masks, long long n_atoms, int n_points,
                                int64_t *d_dot_first, long long *n_dots_out);
int freesasa_gpu_dots_expand_dev(freesasa_gpu_ctx *ctx, const double *d_xyz, const double *d_radii, long long n_atoms,
                                 double probe_radius, int n_points, const uint32_t *d_masks, const int64_t *d_dot_first,
                                 long long capacity, double *d_dot_xyz, int *d_dot_atom, int *d_dot_point);
/* The same on host arrays, on a pooled per-thread context like freesasa_gpu_calc_batch.  counts_out and totals_out may be
   NULL; sasa_out [n] and masks_out [n][4] are required.  Returns 0 / -1 with err_out. */
int freesasa_gpu_calc_masks(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, double probe_radius,
                            int n_points, double *sasa_out, int *counts_out, double *totals_out, uint32_t *masks_out,
                            int device, char *err_out, int err_len);
/* The number of dots stored masks hold (host array, no device): the sum of their popcounts into *n_dots_out - what sizes the
   arrays of freesasa_gpu_dots_from_masks.  -1 with a message: NULL, n_atoms or n_points out of range, a bit at or above
   n_points set. */
int freesasa_gpu_masks_count(const uint32_t *masks, long long n_atoms, int n_points, long long *n_dots_out, char *err_out, int err_len);
/* The dots of stored masks, host arrays: upload, scan and expansion on the device.  n_dots is what the caller holds the masks
   to have (the sum of `counts`): -1 with a message before a device is touched if their popcount is another number or a bit at
   or above n_points is set.  dot_xyz_out [3 n_dots] is required; dot_first_out [n_atoms + 1], dot_atom_out [n_dots] and
   dot_point_out [n_dots] may be NULL. */
int freesasa_gpu_dots_from_masks(const double *xyz, const double *radii, long long n_atoms, double probe_radius, int n_points,
                                 const uint32_t *masks, long long n_dots, int64_t *dot_first_out, double *dot_xyz_out,
                                 int *dot_atom_out, int *dot_point_out, int device, char *err_out, int err_len);
/* ... and per frame of a trajectory: freesasa_gpu_trajectory_topology / freesasa_gpu_trajectory_file_topology with one more
   output behind sel_atoms_out
     masks       4 n uint32 per frame     (16 n f)       the masks of the frame's topology atoms: bit for bit masks_out of
                                                         freesasa_gpu_calc_masks on the frame taken as a structure of its own
   (memory form: masks_out [n_frames][n][4]; file form: masks_path, raw, frame f at byte 16 n f; required).  Every other output is
   byte for byte that entry's; all file formats, fp32 input, a gather index, fp32 per-atom output and any device list work
   unchanged.  alg must be Shrake-Rupley (1).  The done-list's first line names the mask output (128 in outputs=): a list of a
   run without it and a list of a run with it refuse each other.  The dots of any frame follow from its masks and coordinates
   with freesasa_gpu_dots_from_masks.
   -1 with a message before a device is touched or a file opened: masks NULL, Lee-Richards, more than 128 points, bit 3 or 4 of
   frames_f32 (periodic images).  Chain groups, a statistics word and the frames' volumes have entries of their own, which
   take no masks. */
int freesasa_gpu_trajectory_masks(const double *xyz_frames, int n_frames, const struct freesasa_ingest_batch *batch, int structure,
                                  int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                  int alg, double probe_radius, int resolution, int frames_per_batch,
                                  double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                  double *sel_area_out, long long *sel_atoms_out, uint32_t *masks_out,
                                  const int *devices, int n_devices, char *err, int err_len);
int freesasa_gpu_trajectory_file_masks(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                       const struct freesasa_ingest_batch *batch, int structure,
                                       int frame_atoms, const int32_t *atom_index, const struct freesasa_ingest_selection *sel,
                                       int alg, double probe_radius, int resolution, int frames_per_batch,
                                       const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                       const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                       const char *masks_path,
                                       const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                       long long *frames_total_out, char *err, int err_len);

#ifdef __cplusplus
}
#endif
#endif /* FREESASA_GPU_H */
