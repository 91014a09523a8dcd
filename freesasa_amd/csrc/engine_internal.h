/*
 * engine_internal.h — what the translation units of the engine share (never installed; the public surface is
 * include/freesasa_gpu.h):
 *
 *   gpu_kernels.hip    every __global__ wrapper around the phase functions of sasa_kernels.h / lr2_kernels.h and the
 *                      kl_* launchers below (the only file that holds device code)
 *   gpu_engine.hip     the per-device context (workspace, status words, events), the launch sequence of one batch,
 *                      asynchronous batches, the device-pointer entry points
 *   gpu_ops.hip        device-side aggregates (segments, classes, residues, selections) and the kernel test hooks
 *   gpu_hostbatch.hip  host-pointer batches: the context pool; the chunk path and its entries - one device, several devices,
 *                      the pipelined form, the cache sweep
 *   gpu_drivers.hip    trajectory drivers (one device or a list of devices); what the drivers share (device lists, the
 *                      host budget, DoneList)
 *   gpu_frames.hip     the trajectory drivers' frame source: raw, DCD, AMBER NetCDF, GROMACS XTC and TRR input - open and its
 *                      refusals, the layout of a shard, read + check on the host, the kernels that make compact fp64 frames;
 *                      the XTC decode's test hook
 *   gpu_sweep.hip      the file sweep (host or device parser, done-list, per-residue table, selections, chain groups, interfaces
 *                      between them) and the device parser's entries
 *   gpu_parse.hip      the device-side PDB / mmCIF parser: its kernels and their host driver (gpu_parse.h)
 *   gpu_groups.hip     chain groups: a batch and every group of it cut out as a structure of its own, in one batch; the
 *                      group ids made on the device
 *   gpu_volume.hip     molecular volume: the batch through the engine with the exposed-point vectors kept, the atoms' terms
 *                      and the structures' volumes behind it; its device-pointer and host-pointer entries
 *   gpu_dots.hip       exposure masks and surface dots: the batch through the engine with the store phase's masks kept; the scan
 *                      of their popcounts and the expansion into dots; their device-pointer and host-pointer entries
 *   gpu_interfaces.hip pairwise interface areas between chain groups: the contact screen behind the chain-group pipeline, the batch of
 *                      the pair structures through the engine, the pair table; their device-pointer and host-pointer entries
 *   gpu_periodic.hip   periodic images: a batch and its cells (orthorhombic or triclinic) expanded into a batch with the
 *                      images that matter, the areas of the real atoms collected; the stage the trajectory file drivers share;
 *                      chain groups among periodic images: the same stage over the chain-group entry's combined batch
 */
#ifndef FREESASA_AMD_ENGINE_INTERNAL_H
#define FREESASA_AMD_ENGINE_INTERNAL_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <functional>
#include <mutex>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/freesasa_gpu.h"
#include "../../include/freesasa_ingest.h"
#include "sasa_kernels.h"
#include "lr2_kernels.h"
#include "kat_kernels.h"
#include "group_kernels.h"
#include "select_kernels.h"
#include "traj_kernels.h"
#include "xtc_kernels.h"
#include "pbc_kernels.h"
#include "pbc_tri_kernels.h"
#include "vol_kernels.h"
#include "dots_kernels.h"
#include "iface_kernels.h"
#include "contact_kernels.h"
#include "rescontact_kernels.h"
#include "ifsweep_kernels.h"
#include "occupancy_kernels.h"
#include "gpu_parse.h"

/* ------------------------------------------------------------------ kernel launchers (gpu_kernels.hip) */

/* k_sort_struct: one workgroup sorts one structure in LDS */
#define SORT_B 1024
#define SORT_APT 16
#define SORT_ATOMS (SORT_B * SORT_APT - 256) /* atoms of a structure (the 256 short of 16 threads' worth: two workgroups' LDS per CU) */
#define SORT_CELLS (1 << 18) /* cells in LDS at a time (a bit each); a structure with more is done in that many passes */
#define SORT_WORDS (SORT_CELLS / 32)
#define SORT_CELL_BITS 26    /* cells of one structure this kernel can number (6 more bits hold the border flags) */

/* cell sort of a batch: per structure in one workgroup (batches of small structures), or the general pipeline
   (bounds, grid, cell numbering, histogram, scan, scatter: any structure size) */
hipError_t kl_prep_fused(const sasa::PipeArgs &pa, hipStream_t st);
hipError_t kl_prep_general(const sasa::PipeArgs &pa, long long cells_cap, hipStream_t st);
/* Lee-Richards, second generation: main launch (the build is picked by tile shape and pair-record rounds), second
   launch (larger LDS lists, more registers) */
hipError_t kl_lr2_main(int rmax, int grid, size_t lds, hipStream_t st, const sasa::Lr2Args &la);
hipError_t kl_lr2_mid(int grid, size_t lds, hipStream_t st, const sasa::Lr2Args &la);
/* first-generation tile kernels: tier 0 main launch, 1 second launch, 2 last launch (lists in a global slab) */
hipError_t kl_lr_tile(int tier, const sasa::TileCfg &c, const sasa::TileArgs &t, int grid, size_t lds, hipStream_t st, bool bucket);
/* (evec: the volume's exposed-point vectors [3 n_atoms], kept by the launches that run the third arrangement - sr_caps_shape;
   null: the builds without them; masks: the dots' exposure masks [n_atoms][SR_CAP_WORDS], kept the same way - one of the two at most) */
hipError_t kl_sr_tile(int tier, const sasa::TileCfg &c, const sasa::TileArgs &t, int grid, size_t lds, hipStream_t st, double *evec = nullptr, unsigned *masks = nullptr);
/* per-structure totals in two levels (chunk partials in `bpart`) */
hipError_t kl_totals(const sasa::PipeArgs &pa, int n_chunks, int n_structs, const double *d_sasa, double *bpart, double *d_totals, hipStream_t st);
hipError_t kl_segment_sums(const double *d_sasa, const int64_t *d_seg, int n_segs, bool short_segments, double *d_out, hipStream_t st);
hipError_t kl_class_sums(const double *d_sasa, const unsigned char *d_class, const int64_t *d_offsets, int n_structs, double *d_out, hipStream_t st);
hipError_t kl_residue_areas(const double *d_sasa, const unsigned char *d_class, const unsigned char *d_backbone, const int64_t *d_res_first,
                            const short *d_ref_row, const double *d_ref_table, double *d_abs, double *d_rel, int n_res, hipStream_t st);
hipError_t kl_arc_kat(const double *d_arcs, const int *d_first, int n_sets, double *d_out, hipStream_t st);
/* test hooks (kat_kernels.h): n operands in workgroups of 256; `rows` rows of 64 words through one wave */
hipError_t kl_kat_elementwise(int op, const double *d_a, const double *d_b, const double *d_c, double k, double *d_o0, double *d_o1, int n,
                              hipStream_t st);
hipError_t kl_kat_wave(int op, const unsigned long long *d_in, unsigned long long *d_out, int rows, hipStream_t st);
hipError_t kl_widen_f32(const float *d_in, double *d_out, long long n, hipStream_t st);
hipError_t kl_narrow_f64(const double *d_in, float *d_out, long long n, hipStream_t st);
void kl_dump_phase_clocks(void); /* (dev builds with -DSASA_PHASE_TIMING; else nothing) */
/* chain groups (group_kernels.h): count and validate (one thread per atom), the stable cut into the combined batch (one
   wave per structure), the finish (one thread per combined atom), totals (one thread per group / structure) */
hipError_t kl_grp_count(const sasa::GrpArgs &a, hipStream_t st);
hipError_t kl_grp_rank(const sasa::GrpArgs &a, hipStream_t st);
hipError_t kl_grp_finish(const sasa::GrpArgs &a, hipStream_t st);
hipError_t kl_grp_totals(const sasa::GrpArgs &a, hipStream_t st);
/* group ids made on the device (group_kernels.h): one wave per structure; the label of every group of separate chains */
hipError_t kl_gid_struct(const sasa::GidArgs &a, hipStream_t st);
hipError_t kl_gid_label(const sasa::GidLabelArgs &a, hipStream_t st);

/* selection areas (select_kernels.h): the mask word of every atom (one thread per atom), the masked sums (one workgroup per
   structure and SEL_G selections) */
hipError_t kl_sel_mask(const sasa::SelArgs &a, hipStream_t st);
hipError_t kl_sel_sums(const sasa::SelArgs &a, hipStream_t st);

/* the trajectory drivers' topology (traj_kernels.h): full frames (fp64, or fp32 widened on the way) -> the compact frames the
   engine reads; per-frame residue areas (one thread per frame and residue), class sums (one workgroup per frame) and
   selection areas (one workgroup per frame and SEL_G selections) */
hipError_t kl_traj_gather(const sasa::TrajArgs &a, const void *d_in, bool in_f32, double *d_out, hipStream_t st);
/* ... the same from the bytes of DCD frames (planar fp32 records, byte-swapped when big_endian): the gather and the widening in one */
hipError_t kl_traj_gather_dcd(const sasa::TrajDcdArgs &a, const void *d_in, bool big_endian, double *d_out, hipStream_t st);
/* ... and from the bytes of AMBER NetCDF records (big-endian fp32, atom by atom, at a record stride) */
hipError_t kl_traj_gather_nc(const sasa::TrajNcArgs &a, const void *d_in, double *d_out, hipStream_t st);
hipError_t kl_traj_gather_trr(const sasa::TrajTrrArgs &a, const void *d_in, bool is_double, double *d_out, hipStream_t st);
/* XTC input (xtc_kernels.h): one wavefront per frame walks the stream's groups; one thread per group unpacks them into raw fp32 frames */
hipError_t kl_xtc_scan(const sasa::XtcArgs &a, hipStream_t st);
hipError_t kl_xtc_unpack(const sasa::XtcArgs &a, hipStream_t st);
hipError_t kl_traj_residues(const sasa::TrajArgs &a, hipStream_t st);
hipError_t kl_traj_class(const sasa::TrajArgs &a, hipStream_t st);
hipError_t kl_traj_sel(const sasa::TrajArgs &a, hipStream_t st);
/* ... chain groups per frame: the combined batch's radii, the isolated structures' coordinates behind the compact frames (both
   one thread per element), the finish (one thread per combined atom), three columns per (frame, group) */
hipError_t kl_traj_group_radii(const sasa::TrajGroupArgs &a, hipStream_t st);
hipError_t kl_traj_group_gather(const sasa::TrajGroupArgs &a, hipStream_t st);
hipError_t kl_traj_group_finish(const sasa::TrajGroupArgs &a, hipStream_t st);
hipError_t kl_traj_group_totals(const sasa::TrajGroupArgs &a, hipStream_t st);
/* ... interfaces between chain groups per frame: the pair structures' radii and the sides' boundaries (once per shard length),
   their coordinates behind the isolated structures, six doubles per (frame, pair) behind kl_segment_sums over the sides */
hipError_t kl_traj_pair_radii(const sasa::TrajPairArgs &a, hipStream_t st);
hipError_t kl_traj_pair_gather(const sasa::TrajPairArgs &a, hipStream_t st);
hipError_t kl_traj_pair_rows(const sasa::TrajPairArgs &a, hipStream_t st);
/* ... and their per-residue table: four doubles per (frame, segment), one thread each, behind the engine */
hipError_t kl_traj_pair_res(const sasa::TrajPairResArgs &a, hipStream_t st);
/* ... run statistics: a shard's partial [4][W] of the outputs in the table of segments (one thread per column) */
hipError_t kl_traj_stats(const sasa::TrajStatsArgs &a, hipStream_t st);

/* periodic images (pbc_kernels.h): image counts and bases (one workgroup per structure); the expanded batch, the real atoms'
   areas out of its areas (both one thread per atom of the caller's batch) */
hipError_t kl_pbc_count(const sasa::PbcArgs &a, hipStream_t st);
hipError_t kl_pbc_emit(const sasa::PbcArgs &a, hipStream_t st);
hipError_t kl_pbc_collect(const sasa::PbcArgs &a, hipStream_t st);
/* ... in a triclinic cell (pbc_tri_kernels.h): the same two phases with the general geometry; the collect is kl_pbc_collect */
hipError_t kl_pbc_tri_count(const sasa::PbcTriArgs &a, hipStream_t st);
hipError_t kl_pbc_tri_emit(const sasa::PbcTriArgs &a, hipStream_t st);
/* ... chain groups among periodic images (pbc_kernels.h, GpbcArgs): the cell of every combined structure (one thread per
   structure); collect and the groups' finish in one (one thread per combined atom) */
hipError_t kl_gpbc_cells(const sasa::GpbcArgs &a, hipStream_t st);
hipError_t kl_gpbc_finish(const sasa::GpbcArgs &a, hipStream_t st);

/* molecular volume (vol_kernels.h): the origins (one workgroup per structure), the atoms' terms (one thread per atom) */
hipError_t kl_vol_origin(const sasa::VolArgs &a, hipStream_t st);
hipError_t kl_vol_atom(const sasa::VolArgs &a, hipStream_t st);

/* surface dots (dots_kernels.h): the scan in its three launches (dot_first and, at its end, D); the expansion */
hipError_t kl_dots_count(const sasa::DotsArgs &a, hipStream_t st);
hipError_t kl_dots_expand(const sasa::DotsArgs &a, hipStream_t st);

/* interfaces between chain groups (iface_kernels.h): the groups' boxes (one wave per group), the candidate pairs (one thread per
   test), the exact contact (one workgroup per candidate at a time), the pair batch (one thread per atom), the finish (per atom,
   then - behind kl_segment_sums over the sides - per row) */
hipError_t kl_iface_box(const sasa::IfaceArgs &a, hipStream_t st);
hipError_t kl_iface_candidates(const sasa::IfaceArgs &a, hipStream_t st);
hipError_t kl_iface_contact(const sasa::IfaceArgs &a, hipStream_t st);
hipError_t kl_iface_gather(const sasa::IfaceArgs &a, hipStream_t st);
hipError_t kl_iface_finish(const sasa::IfaceArgs &a, hipStream_t st);
/* ... their per-residue tables (IfaceResArgs): heads, the scan of the heads, the segments' first atoms and sums; the scan of the
   keep flags and the rows.  kl_iface_res_scan: the in-place exclusive block scan both use (scratch: ifr_scan_scratch(n) ints) */
hipError_t kl_iface_res_scan(int *a, int64_t n, int *scratch, hipStream_t st);
hipError_t kl_iface_res_segments(const sasa::IfaceResArgs &a, int *scratch, hipStream_t st);
hipError_t kl_iface_res_rows(const sasa::IfaceResArgs &a, int *scratch, hipStream_t st);
/* ... their atom-atom contact tables (contact_kernels.h): the buried masks; the partner of every buried dot; the rows (count, rank,
   the scan of the atoms' distinct partners - a.nd [M + 1], zeroed by the caller; scratch: ifr_scan_scratch(M) ints - and the write) */
hipError_t kl_contact_masks(const sasa::ContactArgs &a, hipStream_t st);
hipError_t kl_contact_attribute(const sasa::ContactArgs &a, hipStream_t st);
hipError_t kl_contact_rows(const sasa::ContactArgs &a, int *scratch, hipStream_t st);
/* ... their residue-residue contact tables (rescontact_kernels.h): the segments (the per-residue tables' heads, scan and first
   atoms, nothing else of them); the fold of the contact rows - count, the scan of a.fc [M + 1], write - and the reverse rows with
   the sides' offsets (scratch: ifr_scan_scratch(M) ints) */
hipError_t kl_rc_segments(const sasa::IfaceResArgs &s, int *scratch, hipStream_t st);
hipError_t kl_rc_fold(const sasa::ResContactArgs &a, int *scratch, hipStream_t st);
/* ... in the file sweep (ifsweep_kernels.h): the class of every pair-structure atom (one thread per atom; kl_class_sums over the
   sides follows it); the rows' place in their file and their labels (one thread per residue row).  Neither is launched without rows. */
hipError_t kl_ifs_side_class(const sasa::IfsClassArgs &a, hipStream_t st);
hipError_t kl_ifs_res_rows(const sasa::IfsRowArgs &a, hipStream_t st);
/* the residue contact occupancy map (occupancy_kernels.h): a chunk's keys and frame boundaries out of the folded table (one thread
   per folded row and per frame boundary); the first occurrences and their scan (a.fl [Q + 1]; scratch: ifr_scan_scratch(Q) ints);
   the merge by ranks and the accumulation (a.n_new = U + N known: one thread per old and per chunk row, then one per row of the
   next table); the reverse rows of a snapshot.  None is launched without rows. */
hipError_t kl_occ_keys(const sasa::OccKeyArgs &a, hipStream_t st);
hipError_t kl_occ_first(const sasa::OccArgs &a, int *scratch, hipStream_t st);
hipError_t kl_occ_merge(const sasa::OccArgs &a, hipStream_t st);
hipError_t kl_occ_reverse(const sasa::OccArgs &a, hipStream_t st);

/* ------------------------------------------------------------------ context (gpu_engine.hip) */

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct freesasa_gpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool timing = false;
    bool shared_radii = false; /* d_radii holds ONE structure's radii (trajectory frames) */
    char err[512] = {0};
    freesasa_gpu_stats stats = {};
    /* Two sets of what the HOST reads of a batch (page-locked status words, stage events, end-of-batch event): a batch
       submitted with freesasa_gpu_lr_batch_dev_async leaves its set behind until it is collected, while the next one
       is enqueued with the other set.  The device side needs no second copy: the copies into a set are enqueued at
       the end of their batch, in stream order before the next batch resets the device words. */
    int slot = 0;
    hipEvent_t evs[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
    hipEvent_t done[2] = {nullptr, nullptr};
    struct Pend {
        bool active = false;
        /* the call, for the rare batch that has to be redone (cell table sizing, see RC_RETRY) */
        const double *d_xyz = nullptr, *d_radii = nullptr;
        std::vector<int64_t> offsets;
        int n_structs = 0, resolution = 0;
        double probe = 0;
        double *d_sasa = nullptr, *d_totals = nullptr;
        /* what completing it needs */
        int n = 0, TA = 0, mw = 0, ds = 0, lds = 0;
        bool walk = false; /* the main launch was the walking build (far tiles stay in it: statistics) */
    } pend[2];
    /* workspace */
    DevBuf offsets, grid, ncells, sid, cell_of, rank, cell_start, blk_sums, cell_tbl, cell_first;
    DevBuf chunk_struct, chunk_begin, chunk_len, struct_chunk0, bpart;
    int n_chunks = 0;
    DevBuf sq, s_idx;
    DevBuf status, ovf_tiles, ovf_tiles2, ovf_atoms, unit_pts, slab, seg;
    DevBuf res_table;                  /* the reference areas of relative SASA, uploaded once (residue_areas_resident) */
    std::vector<double> res_table_host;
    std::vector<int64_t> offsets_host; /* last uploaded offsets */
    std::vector<double> unit_host;     /* last uploaded S&R unit points */
    /* S&R, third arrangement (sr_caps.h): the table of cap masks of unit_host, rebuilt when the points change */
    DevBuf captab;
    std::vector<sasa::SrCapEntry> captab_host;
    int captab_n = 0, captab_l = 0;    /* its resolution; 0: no table for these points (more than 128, not unit vectors, switched off) */
    /* host staging for freesasa_gpu_calc_batch (and freesasa_gpu_calc_groups: h_group, h_iso, h_gtot) */
    DevBuf h_xyz, h_radii, h_sasa, h_counts, h_totals, h_group, h_iso, h_gtot;
    /* chain groups (gpu_groups.hip): offsets and group bases, keys, counts, cursors, the combined batch, its results */
    DevBuf g_meta, g_key, g_count, g_cursor, g_xyz, g_radii, g_src, g_sasa, g_gath, g_tot, g_tot2;
    /* group ids made on the device: the spec's label table, the per-structure words (offsets, status in, n_groups and group
       status out), the groups' labels */
    DevBuf gi_tab, gi_words, gi_label;
    /* periodic images (gpu_periodic.hip): offsets | expanded offsets | cells | image counts | max radii; the atoms' image bases;
       the expanded batch and its areas; the chunk tables of the CALLER's batch (its totals are summed like any batch's) */
    DevBuf p_meta, p_ibase, p_xyz, p_radii, p_sasa, p_chunks, p_part;
    std::vector<int64_t> p_offsets_host; /* the offsets p_chunks was made for */
    int p_n_chunks = 0;
    /* chain groups among periodic images: the cell of every combined structure (the batch entries: the complexes' behind them) */
    DevBuf gp_cells;
    /* molecular volume (gpu_volume.hip): counts, exposed-point vectors, the atoms' terms, the structures' origins and volumes
       where the caller gives no array of its own; vol_evec: set for the length of ONE run_batch, which then keeps the vectors
       there - or refuses the batch (run_batch_once) */
    DevBuf v_counts, v_evec, v_vol, v_origin, v_volumes;
    double *vol_evec = nullptr;
    /* exposure masks and surface dots (gpu_dots.hip): sr_masks: set for the length of ONE run_batch, which then keeps the masks
       there - or refuses the batch (run_batch_once); the host-pointer entries' masks, prefix sums, block sums and dots */
    unsigned *sr_masks = nullptr;
    DevBuf dt_masks, dt_first, dt_bsum, dt_xyz, dt_atom, dt_point, dt_unit;
    /* interfaces between chain groups (gpu_interfaces.hip): group starts and test bases; boxes; the candidates' list, its length
       and the flags; the sides' tables; the pair batch, its areas and what is made of them */
    DevBuf if_meta, if_box, if_cand, if_flag, if_sides, if_xyz, if_radii, if_comb, if_sasa, if_inpair, if_areas, if_patom, if_pburied;
    /* ... their per-residue tables: the residue boundaries; the int32 work arrays; the segments' areas; the table itself */
    DevBuf if_rfirst, if_rwork, if_rsegs, if_rtable;
    /* ... their atom-atom contact tables: the side, pair and buried masks with the two runs' areas; the atoms' int32 work arrays
       and the flag; the buried dots (dot_first, points, atoms, point numbers, partners, counts, ranks); the table itself */
    DevBuf if_cmasks, if_cwork, if_cdots, if_ctable;
    /* ... their residue-residue contact tables: the segments' and the fold's int32 work arrays; the table itself */
    DevBuf if_rcwork, if_rctable;
    /* ... in the file sweep (gpu_sweep.hip): the structures' isolated areas are h_iso; the combined batch's offsets for the labels
       (run_batch over the pair structures has taken c->offsets); the sides' class sums, pair_struct, the rows' place and labels,
       the pair-structure atoms' classes */
    DevBuf ifs_comb, ifs_work;
    int dt_unit_n = 0; /* the point count whose unit points dt_unit holds (the expansion's; 0: none) */
    void *stage_in = nullptr, *stage_out = nullptr; /* page-locked host staging of freesasa_gpu_calc_batch_pipelined */
    size_t stage_in_cap = 0, stage_out_cap = 0;
    void *res_stage = nullptr; /* page-locked: a batch's per-residue areas and arrays on their way to the host (gpu_sweep.hip) */
    size_t res_stage_cap = 0;
    int *pinned = nullptr; /* page-locked host words for the small device->host readbacks: two sets of ST_WORDS + 4 */
    long long max_cells = 1LL << 30;
    long long cells_hint = 0; /* cells the last batch needed, with a margin: the table is never sized below it */
    int scan_epoch = 0;       /* batches that went through the general cell sort's chained scan (PipeArgs::scan_epoch) */
    /* adaptive neighbor-pool size, per algorithm: (resolution, TA) it was learnt for and the value */
    int hint_res[2] = {0, 0}, hint_ta[2] = {0, 0}, hint_pool[2] = {0, 0};
    double hint_probe = -1.0; /* the probe radius the hints were learnt with (another probe: other neighbor counts, so they start over) */
    bool hint_bucket = false; /* L&R: the last batch had long neighbor lists */
    bool sort_fused = true;   /* the per-structure cell sort (k_sort_struct) until a batch turns out not to fit it */
    double hint_nn = 0;       /* L&R (lr2): neighbor records per atom the main launch should hold */
    int hint_nn_max = 0;      /* ... and the longest neighbor list expected (mask words per item) */
    double hint_split2 = 0;   /* ... the share of its tiles above the 16-tiles-per-CU pool */
    bool hint_far = false;    /* ... a quarter or more of its tiles had an atom beyond LR2_WALK_Z: the next batch gets the walking build of the main launch */
    int hint_pool2 = 0, hint_ta2 = 0, hint_mw2 = 0; /* ... and the pool the last batch's demand histogram asks for, for tiles of that shape */
    /* the device-side parser's workspace and what its two phases hand each other (gpu_parse.hip) */
    DevBuf parse[PBUF_COUNT]; /* (enum ParseBuf, gpu_parse.h, says what each holds) */
    std::vector<long long> parse_off;
    std::vector<unsigned char> parse_table; /* host copy of a user classifier's table being uploaded (gpu_parse.hip) */
    long long parse_atoms = 0;
    int parse_lines = 0, parse_files = 0, parse_options = 0;
    unsigned parse_T = 0;
    int *dbg_nn = nullptr, *dbg_nb = nullptr; /* test hook: freesasa_gpu_lr_neighbors_dev */
    int dbg_cap = 0;
};

int ctx_fail(freesasa_gpu_ctx *c, const char *fmt, ...) __attribute__((format(printf, 2, 3))); /* sets the context's error text, returns -1 */

#define HIP_TRY(c, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ctx_fail((c), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

/* device / page-locked allocations (both honour the fault-injection hook freesasa_gpu_test_fail_after) */
hipError_t dev_malloc(void **p, size_t bytes);
hipError_t host_malloc(void **p, size_t bytes);
/* grow a workspace buffer to at least `bytes` (waits for the stream first when batches are in flight) */
int ensure(freesasa_gpu_ctx *c, DevBuf &b, size_t bytes);

/* One batch on device pointers, synchronous: redone when the cell table was too small; on failure nothing is still
   running on the stream when the caller gets control back.  lr: Lee-Richards (resolution = slices), else Shrake-Rupley
   (resolution = test points, unit_points on the host). */
int run_batch(freesasa_gpu_ctx *c, bool lr, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
              double probe, int resolution, const double *unit_points, double *d_sasa, int *d_counts, double *d_totals);

/* The cell sort of one batch, the first stage of run_batch_once and the whole of the test hook freesasa_gpu_cell_sort_dev
   (gpu_ops.hip): the workspace sized, offsets and chunk table uploaded when they changed, the status words cleared, `pa` filled,
   the cell table sized for cells_cap cells, and the launches enqueued on the context's stream - k_sort_struct (fused; with the
   compact table or the dense one) or the general pipeline (not fused: the dense table).  Nothing is waited for and nothing the
   context has learnt is touched, but for the launch-shape history: history 0 (Lee-Richards) / 1 (Shrake-Rupley) with the
   batch's resolution is run_batch_once's - another probe radius than the history's starts it over, and a batch with history
   takes no density samples (PipeArgs::occ_stride 0); history -1 (the hook) neither reads nor resets it and samples every
   (n / 256)-th atom.  prefill: all-ones bytes in grid, ncells, sq, s_idx and the table before the first launch (the hook).
   The caller has checked the arguments (n = offsets[n_structs] > 0). */
int cell_sort_enqueue(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs, int n,
                      double probe, int history, int resolution, bool fused, bool compact, long long cells_cap, bool prefill, sasa::PipeArgs &pa);
/* the cells a batch's table is sized for before its total is known: 10 per atom and 256 per structure, raised to what the
   context has seen (cells_hint), capped at max_cells */
long long batch_cells_cap(const freesasa_gpu_ctx *c, int n, int n_structs);

/* Per-residue areas (freesasa_gpu_residue_areas_dev's kernel) on arrays that are ALL on the device already - residue
   offsets [n_res + 1], reference rows [n_res] (NULL: no relative areas wanted, d_rel ignored), backbone flags, classes -
   enqueued on the context's stream, no synchronisation; the reference-area table goes up with the context's first call.
   (gpu_ops.hip) */
int residue_areas_resident(freesasa_gpu_ctx *c, const double *d_sasa, const unsigned char *d_class, const unsigned char *d_backbone,
                           const int64_t *d_res_first, const short *d_ref_row, int n_res, double *d_abs, double *d_rel);

/* Selection areas (freesasa_gpu_select_batch's kernels) for callers whose arrays are on the device already: the caller fills
   the atoms' keys, offsets, residue boundaries and labels, n_* and sasa of `sa`; this uploads the set's program, sizes the
   mask words and the results (c->parse[PBUF_SEL_*]; sa.bits / sa.area / sa.count say where) and enqueues sel_mask and
   sel_sums on the context's stream.  No synchronisation.  (gpu_ops.hip) */
int select_resident(freesasa_gpu_ctx *c, const struct freesasa_ingest_selection *sel, sasa::SelArgs &sa);

/* ------------------------------------------------------------------ chain groups for the file sweep (gpu_groups.hip) */

/* a chain-group request as the device takes it: freesasa_ingest_chain_groups_parse's labels sorted by their value as a word */
struct GroupSpec {
    bool separate = false;
    int n_groups = 0;                 /* the spec's (0: separate chains) */
    std::vector<uint32_t> lab;        /* ascending */
    std::vector<int32_t> lab_group;
    std::vector<uint32_t> first_label; /* [n_groups] the first label the spec names for the group */
};
int group_spec_parse(const char *spec, int flags, GroupSpec *out, char *err_out, int err_len); /* 0 / -1 with select.c's message */
/* The ids kernel on arrays that are on the device: the caller fills offsets, residues, labels, status and the outputs of
   `ga`; this uploads the spec's table (c->gi_tab; `gs` outlives the stream's work) and enqueues the kernel.  No synchronisation. */
int group_ids_resident(freesasa_gpu_ctx *c, const GroupSpec &gs, sasa::GidArgs &ga);
/* freesasa_gpu_groups_dev's pipeline on arrays that are on the context's stream already, nothing waited for at its end
   (inside, the counts come back and run_batch waits as ever).  d_sasa / d_iso / d_totals / d_group_totals may be null;
   unit_points: the S&R test points (null: made here); counts_out (may be null) receives the atoms of every group.  The
   combined batch's areas stay in c->g_sasa (the complex's first), its totals in c->g_tot, its offsets in c->offsets, the
   source atoms in c->g_src. */
int groups_resident(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                    const int32_t *d_group, const int32_t *n_groups, double probe, int resolution, const double *unit_points,
                    double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals, std::vector<int> *counts_out);
/* Its first two stages alone - count and validate, the stable cut - for the callers that put another stage between the cut and
   the finish (gpu_periodic.hip): the combined batch in c->g_xyz / c->g_radii, its offsets in `comb` [n_structs + G + 1], the
   atoms of every group in `cnt` (its first G entries; it must outlive the stream's work), and in `ga` the batch, the keys, the group
   bases and the source atoms; c->g_sasa, g_gath, g_tot and g_tot2 sized for it.  The refusals and their messages are
   groups_resident's. */
int groups_cut(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
               const int32_t *d_group, const int32_t *n_groups, sasa::GrpArgs &ga, std::vector<int64_t> &comb, std::vector<int> &cnt);
#define GRP_MAX_PER_STRUCT 65535 /* groups of a structure */
/* The grouped host batch - freesasa_gpu_calc_groups, its periodic forms (gpu_periodic.hip) and the interface entries' host form
   (gpu_interfaces.hip): host arrays with group ids as ONE chunk of the host-batch path (below), in place.  The caller fills the
   first two lines and runs its pipeline between the two calls, on the d_* pointers; -1: it owes chunk_failed.
   upload: G, the groups of all structures (a bad count is refused by the pipeline, with its message: staged for none here);
   the chunk's buffers and c->h_group, h_iso, h_gtot sized; xyz, radii and group enqueued; the d_* set (d_totals,
   d_group_totals: null where the caller's array is).  download: sasa, iso, totals and group_totals enqueued to the caller's
   arrays that are not null.  Nothing is waited for. */
struct BatchCall;
struct GroupBatch {
    const double *xyz = nullptr, *radii = nullptr; const int64_t *offsets = nullptr; int n_structs = 0; const int32_t *group = nullptr, *n_groups = nullptr;
    double *sasa_out = nullptr, *iso_out = nullptr, *totals_out = nullptr, *group_totals_out = nullptr;
    int64_t G = 0;
    const double *d_xyz = nullptr, *d_radii = nullptr; const int32_t *d_group = nullptr;
    double *d_sasa = nullptr, *d_iso = nullptr, *d_totals = nullptr, *d_group_totals = nullptr;
};
int group_batch_upload(const BatchCall &b, freesasa_gpu_ctx *c, GroupBatch &g);
int group_batch_download(freesasa_gpu_ctx *c, const GroupBatch &g);

/* ------------------------------------------------------------------ periodic images (gpu_periodic.hip) */

/* The cutoff of a structure, c = 2 (max radius + probe), and the check of one cell against it on the host: 0, or the 1-based
   axis of the first edge that is not finite (negative) or shorter than c (positive). */
double periodic_cutoff(const double *radii, int64_t n, double probe);
int periodic_cell_bad(const double *cell, double c);
/* freesasa_gpu_periodic_dev's pipeline on arrays that are on the context's stream already: count, the image counts back to
   the host (one synchronisation; run_batch takes host offsets), emit, run_batch on the expanded batch with per-atom radii,
   collect into d_sasa [offsets[n_structs]], totals over the real atoms into d_totals (may be null).  Nothing is waited for
   at its end.  n_fixed > 0: every structure holds n_fixed atoms and d_radii their n_fixed radii (the frames of a shard;
   offsets then is k n_fixed).  cells: host, [3 n_structs], checked by the caller to be finite; an edge shorter than a
   structure's c is refused here, after the count and before the engine runs; d_cells: the same on the device already
   (null: uploaded here).  unit_points: the S&R test points (null: made
   here).  images_out (host, may be null) receives the image count of every structure. */
int periodic_resident(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                      int n_fixed, const double *cells, const double *d_cells, double probe, int resolution, const double *unit_points,
                      double *d_sasa, double *d_totals, int64_t *images_out);
/* Triclinic cells (pbc_tri_kernels.h).  periodic_cell6_bad (cell.c): the shape check of six numbers ax, bx, by, cx, cy, cz on the host: 0,
   -(k + 1) when entry k is not finite, k + 1 when the diagonal entry k (0, 2, 5) is not positive.  periodic_widths_bad: 0, or
   the 1-based axis (a, b, c) of the first width below c.  periodic_resident_tri is periodic_resident for cells9 [9 n_structs] =
   per structure the six numbers and their three widths (freesasa_gpu_cell_widths), shape-checked by the caller; d_cells9: the
   same on the device already (null: uploaded here). */
extern "C" int periodic_cell6_bad(const double *cell6); /* (cell.c) */
int periodic_widths_bad(const double *widths, double c);
int periodic_resident_tri(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                          int n_fixed, const double *cells9, const double *d_cells9, double probe, int resolution, const double *unit_points,
                          double *d_sasa, double *d_totals, int64_t *images_out);

/* Chain groups among periodic images.  groups_periodic_stage: a COMBINED batch that is on the context's stream - n_cplx
   complexes, then their groups as structures (comb: its host offsets, n_comb structures; radii per atom) - through
   periodic_resident's pipeline, every group in the cell of its complex, in ONE engine run: the cells of the combined structures
   made on the device (c->gp_cells) from d_cells [W n_cplx], the stage's collect replaced by pbc_kernels.h's fused finish, then
   the totals kernels with the chunk table of `comb` over the compact combined areas (x.carea -> d_ctot [n_comb]) and, when
   d_ctot2 is not null, over the gathered complex areas (x.cgath -> d_ctot2 [n_comb]).  With x.k_fixed > 0 (a trajectory shard's
   interface pairs: behind the groups k_fixed pair structures per complex, x.pair_first their first atom) the pair structures are
   expanded and finished with the rest, d_ctot holds their totals too, and the reduction of x.cgath stops in front of them
   (d_ctot2 [n_cplx (1 + g_fixed)]): a pair atom has no gathered area.  The caller fills the layout and the
   outputs of `x` (n_cplx, n_comb, gbase / g_fixed, k_fixed, pair_first, n_atoms, n_all, src, n_fixed, n_iso_fixed, key, carea, cgath, sasa, iso);
   cells (host, [W n_cplx], W = 3 or PBC_TRI_CELL) are the complexes' rows only: a cell is checked once, against its complex, and
   the messages name the complex.  images_out (host, [n_cplx], may be null): the images of the complexes.  Nothing is waited for
   at its end.  groups_periodic_resident: freesasa_gpu_groups_periodic_dev's pipeline - groups_cut, that stage, k_grp_totals -
   on arrays that are on the context's stream; cells as above, uploaded here. */
int groups_periodic_stage(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_cxyz, const double *d_cradii, const int64_t *comb,
                          const double *cells, const double *d_cells, sasa::GpbcArgs &x, double probe, int resolution,
                          const double *unit_points, double *d_ctot, double *d_ctot2, int64_t *images_out);
int groups_periodic_resident(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                             int n_structs, const int32_t *d_group, const int32_t *n_groups, const double *cells, double probe,
                             int resolution, const double *unit_points, double *d_sasa, double *d_iso, double *d_totals,
                             double *d_group_totals, int64_t *images_out);

/* ------------------------------------------------------------------ molecular volume (gpu_volume.hip) */

/* freesasa_gpu_sr_volume_dev's pipeline on arrays that are on the context's stream already: run_batch (Shrake-Rupley, with
   c->shared_radii as the caller has set it) with the exposed-point vectors kept, then origins, the atoms' terms and the
   structures' volumes (kl_totals over the terms, with the chunk tables run_batch left on the device) enqueued on the stream;
   nothing is waited for at its end.  d_counts / d_evec / d_vol / d_totals may be null (the context's own scratch then);
   d_volumes [n_structs] is required.  0, or -1 with the context's message: a bad argument, or a batch whose volume the
   engine does not make (more than 128 points, no table of cap masks, a launch in the second arrangement). */
int volume_resident(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                    double probe, int n_points, const double *unit_points, double *d_sasa, int *d_counts, double *d_evec,
                    double *d_vol, double *d_totals, double *d_volumes);
/* the arguments both volume entries check before a device is touched: 0, or the message */
const char *volume_bad_args(const void *xyz, const void *radii, const int64_t *offsets, int n_structs, int n_points, const void *sasa, const void *volumes);

/* ------------------------------------------------------------------ exposure masks and surface dots (gpu_dots.hip) */

/* freesasa_gpu_sr_masks_dev's pipeline on arrays that are on the context's stream already: run_batch (Shrake-Rupley, with
   c->shared_radii as the caller has set it) with the exposure masks kept in d_masks [n_atoms][SR_CAP_WORDS]; nothing is
   waited for beyond what run_batch waits for.  d_counts / d_totals may be null.  0, or -1 with the context's message: a bad
   argument, or a batch whose masks the engine does not make (more than 128 points, no table of cap masks, a launch in the
   second arrangement, the volume's vectors asked for in the same batch). */
int masks_resident(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                   double probe, int n_points, const double *unit_points, double *d_sasa, int *d_counts, double *d_totals,
                   unsigned *d_masks);
/* the scan of the masks' popcounts on the context's stream: dot_first [n_atoms + 1]; nothing is waited for */
int dots_count_resident(freesasa_gpu_ctx *c, const unsigned *d_masks, int64_t n_atoms, int n_points, int64_t *d_dot_first);
/* the unit points of n_points on the context's device (c->dt_unit): the expansion's one host allocation - callers run it BEFORE
   they enqueue anything, so that a failure leaves nothing in flight */
int dots_unit_ready(freesasa_gpu_ctx *c, int n_points);
/* the expansion on the context's stream (dots_unit_ready first); nothing is waited for */
int dots_expand_resident(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, int64_t n_atoms, double probe, int n_points,
                         const unsigned *d_masks, const int64_t *d_dot_first, int64_t capacity, double *d_dot_xyz, int *d_dot_atom,
                         int *d_dot_point);
/* the arguments the mask entries check before a device is touched: 0, or the message */
const char *masks_bad_args(const void *xyz, const void *radii, const int64_t *offsets, int n_structs, int n_points, const void *sasa, const void *masks);

/* ------------------------------------------------------------------ interfaces between chain groups (gpu_interfaces.hip) */

/* What an entry was called with.  The batch and the four group outputs are where the pipeline reads and writes them: the caller's
   device arrays (iface_dev), or - behind the upload - the context's staging (iface_host, the file sweep).  A null output array is
   not delivered and asks for no capacity; a stage's own fields are looked at only where the stage is wanted. */
struct IfaceCall {
    const double *xyz = nullptr, *radii = nullptr;
    const int64_t *offsets = nullptr;
    int n_structs = 0;
    const int32_t *group = nullptr, *n_groups = nullptr;
    /* (the file sweep) the groups of every structure as the SCREEN counts them: n_groups[s], or 0 for a structure whose groups
       are cut and summed (step 1) but whose pairs are not looked for; null: n_groups */
    const int32_t *screen_groups = nullptr;
    int alg = 0, resolution = 0;
    double probe = 0;
    double *sasa = nullptr, *iso = nullptr, *totals = nullptr, *group_totals = nullptr;
    /* the stages behind the screen: steps 6 to 8, 9, 10, 11 (11 needs 10; 9 and 10 need 6 to 8) */
    bool whole = false, residues = false, contacts = false, rescontacts = false;
    const int64_t *res_first = nullptr;
    /* (the file sweep) res_first [n_res + 1] is on the device already - the loader's own, trusted as k_gid_struct trusts it: it is
       neither validated nor uploaded */
    const int64_t *res_first_dev = nullptr;
    int n_res = 0;
    double min_buried = 0;
    long long pair_capacity = 0, atom_capacity = 0, res_capacity = 0, contact_capacity = 0, dot_capacity = 0, rescontact_capacity = 0;
    long long *n_pairs = nullptr, *n_pair_atoms = nullptr, *n_res_rows = nullptr, *n_contacts = nullptr, *n_buried_dots = nullptr,
              *n_rescontacts = nullptr;
    long long *stats = nullptr; /* host: the tests and the candidates of the screen */
    /* the tables' arrays, all on the device (out_dev) or all on the host */
    bool out_dev = false;
    int32_t *pair_struct = nullptr, *pair_groups = nullptr, *pair_atom = nullptr;
    double *pair_areas = nullptr, *pair_buried = nullptr;
    int64_t *side_offsets = nullptr;
    int64_t *res_offsets = nullptr;
    int32_t *res_index = nullptr, *res_atoms = nullptr;
    double *res_areas = nullptr;
    int64_t *contact_first = nullptr;
    int32_t *contact_partner = nullptr, *contact_points = nullptr, *dot_partner = nullptr;
    double *contact_area = nullptr;
    uint32_t *buried_masks = nullptr;
    int64_t *rescontact_offsets = nullptr;
    int32_t *rescontact_residues = nullptr, *rescontact_counts = nullptr, *rescontact_reverse = nullptr;
    double *rescontact_area = nullptr;
};

struct IfacePlan {
    int64_t P = 0, M = 0, T = 0, n_cand = 0;
    int64_t n = 0, n_iso = 0;
    int G = 0;
    std::vector<int32_t> pair_struct, pair_groups; /* [P], [2 P] */
    std::vector<int64_t> side_off;                 /* [2 P + 1] */
    std::vector<int64_t> sides;                    /* the upload: side_off [2 P + 1] | side_start [2 P] | side_group [2 P] as int32 */
    std::vector<int64_t> pair_off;                 /* [P + 1] the pair batch's offsets */
    std::vector<int64_t> meta;                     /* the upload: gstart [G + 1] | tbase [n_structs + 1] */
    std::vector<double> tp;                        /* S&R test points */
};
/* the tables of steps 9 to 11 where the stages left them, on the device; a pointer is null where the stage made no such array
   (no pair; no buried point; no folded row), and iface_outputs' rows say what the caller gets then */
struct IfaceResTable { /* c->if_rtable: res_offsets [2 P + 1] | res_areas [3 M] | res_index [M] | res_atoms [M], R rows of them used */
    int64_t R = 0;
    const int64_t *off = nullptr;
    const double *areas = nullptr;
    const int32_t *index = nullptr, *atoms = nullptr;
};
struct IfaceContactTable { /* c->if_ctable: contact_first [M + 1] | contact_area [D_b] | contact_partner [D_b] | contact_points [D_b], C rows used */
    int64_t C = 0, D = 0;
    const int64_t *first = nullptr;
    const int32_t *partner = nullptr, *points = nullptr, *dot_partner = nullptr; /* (dot_partner: in c->if_cdots) */
    const double *area = nullptr;
    const unsigned *buried = nullptr; /* in c->if_cmasks */
};
struct IfaceResContactTable { /* c->if_rctable: rescontact_offsets [2 P + 1] | _area [C] | _residues [2 C] | _counts [2 C] | _reverse [C], Q rows used */
    int64_t Q = 0;
    const int64_t *off = nullptr;
    const double *area = nullptr;
    const int32_t *res = nullptr, *cnt = nullptr, *rev = nullptr;
};
/* What a call produced: the plan with P and M, the three tables with R, C and D_b, Q.  Its host arrays are the sources of copies
   enqueued on the stream - the plan's uploads and deliveries, res_first -, so it is ONE object that lives until the stream is
   idle: declared before the final synchronize in iface_dev and before the PoolLease in iface_host and in the sweep's worker. */
struct IfaceRun {
    IfacePlan pl;
    sasa::IfaceArgs ia;
    IfaceResTable rt;
    IfaceContactTable ct;
    IfaceResContactTable qt;
    std::vector<int64_t> res_first; /* the upload of res_first: what the device searches is what was copied here, whatever
                                       becomes of the caller's array while the stream runs */
};
/* The one run (gpu_interfaces.hip says what its stages are) on a call whose refusals the caller has made; every count output is
   set as soon as its count is known.  The file sweep calls it with capacities that hold anything and no output arrays, sizes its
   host arrays from r.pl.P, r.pl.M and r.rt.R, puts them into the call and delivers: */
int iface_run(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r);
/* The delivery, in two calls around the caller's stream synchronization.  idle = false: everything that goes over the stream is
   enqueued - to device arrays the context's buffers, the plan's arrays and the zeros; to host arrays the context's buffers (the
   zeros are written at once).  idle = true, once the synchronize has succeeded: the plan's arrays into host arrays, and stats. */
int iface_deliver(freesasa_gpu_ctx *c, const IfaceCall &k, const IfaceRun &r, bool idle);
/* The refusals of the residue-residue contact entries about a call's batch, groups, res_first and resolution, before a device is
   touched, with their messages (the capacities and the output arrays are not looked at): 0, or -1 with the message in msg.  For the
   callers that make a call of their own and run it through iface_run (gpu_occupancy.hip). */
int iface_bad_rescontact_call(const IfaceCall &k, char *msg, size_t len);

/* ------------------------------------------------------------------ host-side helpers (gpu_hostbatch.hip) */

/* A small pool of contexts so that concurrent host threads (the reference library is re-entrant,
   doc/doxy-main.md:741-756) each get their own stream and workspace. */
freesasa_gpu_ctx *pool_get(int device);
void pool_put(freesasa_gpu_ctx *c);
int set_err(char *out, int len, const char *msg); /* returns -1 */

/* ------------------------------------------------------------------ the C boundary and C++ exceptions
 * The engine is C++ behind a C ABI whose contract is the reference's: NULL / FREESASA_FAIL / -1 with a message, never
 * exit() (ref: src/util.c:89-113) - and therefore never an exception: a std::bad_alloc from a std::vector, or a
 * std::system_error from a thread that cannot start under a cgroup's pid limit, must not reach a C caller (it would end
 * in std::terminate).  Every extern "C" entry runs its body through guarded() / guarded_ctx(); every worker-thread
 * body catches for itself (an exception that leaves a std::thread's function terminates the process) and reports
 * through its FirstError / error slot; what a scope owns - threads, pooled contexts, loader batches, descriptors - is
 * held by the small RAII types below so that unwinding releases it.  tests/test_hostfault.py walks the n-th host
 * allocation / thread creation failing (hostfault.h) through the drivers. */
extern "C" int freesasa_hostfault_hit(void); /* hostfault.c: 1 = this thread creation has to fail (tests) */
/* text for the exception being handled (call inside a catch block) */
const char *exception_text(char *buf, size_t len) noexcept;

template <class F> int guarded(char *err_out, int err_len, F &&body) noexcept
{
    try { return body(); }
    catch (...) { char msg[200]; return set_err(err_out, err_len, exception_text(msg, sizeof msg)); }
}
/* ... for the entries that report through a context: nothing may still run on its stream when the caller is back */
template <class F> int guarded_ctx(freesasa_gpu_ctx *c, F &&body) noexcept
{
    try { return body(); }
    catch (...) {
        char msg[200];
        exception_text(msg, sizeof msg);
        if (!c) return -1;
        (void)hipStreamSynchronize(c->stream);
        return ctx_fail(c, "%s", msg);
    }
}

/* ------------------------------------------------------------------ a device's host side: its NUMA node
 * On an 8-GPU node every GPU hangs off one socket's PCIe root; a lane that reads files into page-locked staging and
 * feeds that GPU should run - and have its staging allocated - on that socket (the reference has no counterpart: its
 * threads share one structure in one address space, src/sasa_lr.c:219-253).  hwloc-free: the device's PCI address
 * (hipDeviceGetPCIBusId) -> <sysfs>/bus/pci/devices/<address>/numa_node -> <sysfs>/devices/system/node/node<k>/cpulist.
 * DeviceNodeScope binds the CALLING thread to those CPUs (intersected with the CPUs it is allowed now) for the length
 * of a scope and puts its old mask back; nothing happens when the node is unknown (-1: single-socket boxes, VMs), the
 * intersection is empty, or FREESASA_AMD_NO_AFFINITY is set.  node_cpus_for_pci is the mapping itself, testable on
 * a made-up sysfs tree without a GPU (freesasa_gpu_test_node_cpus, tests/test_multidevice.py). */
int node_cpus_for_pci(const char *sysfs_root, const char *pci_address, int *cpus_out, int cap); /* CPUs found (<= cap stored), 0: no node known, -1: unreadable */
struct DeviceNodeScope {
    bool bound = false;
    unsigned long old_mask[16] = {0}; /* cpu_set_t of 1024 CPUs */
    explicit DeviceNodeScope(int device);
    DeviceNodeScope(const DeviceNodeScope &) = delete;
    DeviceNodeScope &operator=(const DeviceNodeScope &) = delete;
    ~DeviceNodeScope();
};

/* threads of one scope: joined on every way out of it */
struct ThreadGroup {
    std::vector<std::thread> th;
    ThreadGroup() = default;
    ThreadGroup(const ThreadGroup &) = delete;
    ThreadGroup &operator=(const ThreadGroup &) = delete;
    ~ThreadGroup() { join(); }
    void join() noexcept
    {
        for (auto &t : th)
            if (t.joinable()) t.join();
        th.clear();
    }
    /* false: the thread did not start (no memory for its state, EAGAIN from the system, or the test hook) */
    template <class F, class... A> bool spawn(F &&f, A &&...a) noexcept
    {
        try {
            if (freesasa_hostfault_hit()) return false;
            th.emplace_back(std::forward<F>(f), std::forward<A>(a)...);
            return true;
        } catch (...) { return false; }
    }
};

/* a pooled context for the length of a scope; on the way out nothing is left running on its stream */
struct PoolLease {
    freesasa_gpu_ctx *c;
    explicit PoolLease(int device) : c(pool_get(device)) {}
    PoolLease(const PoolLease &) = delete;
    PoolLease &operator=(const PoolLease &) = delete;
    ~PoolLease()
    {
        if (!c) return;
        c->shared_radii = false;
        (void)hipStreamSynchronize(c->stream);
        pool_put(c);
    }
};
/* ------------------------------------------------------------------ what the drivers share (gpu_drivers.hip) */

bool pread_all(int fd, void *buf, size_t bytes, long long off);
bool pwrite_all(int fd, const void *buf, size_t bytes, long long off);
/* the device list of a call: every entry an existing device (entries may repeat); -1 with a message */
int check_devices(const int *devices, int n_devices, char *err_out, int err_len);
/* CPUs this process may count on (the cgroup's grant divided among the ranks of the node), and the host threads of one of
   n_workers loaders: the caller's total (or, <= 0, this process's CPUs) divided among them */
int process_cpus();
int threads_per_worker(int n_threads, int n_workers);

/* a descriptor of a driver's scope: closed on every way out of it */
struct Fd {
    int fd = -1;
    Fd() = default;
    Fd(const Fd &) = delete;
    Fd &operator=(const Fd &) = delete;
    ~Fd() { if (fd >= 0) close(fd); }
};

/* first failure of a set of workers wins; the others stop taking work */
struct FirstError {
    std::mutex mu;
    std::atomic<int> failed{0};
    char text[256] = {0};
    void set(const char *msg)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed.load()) snprintf(text, sizeof text, "%s", msg && msg[0] ? msg : "GPU driver failed");
        failed = 1;
    }
    void set_exception() noexcept /* inside a catch block */
    {
        char msg[200];
        try { set(exception_text(msg, sizeof msg)); } catch (...) { failed = 1; }
    }
};

/* The lanes (workers) of a driver: bodies 1 .. n-1 on threads of their own, started in that order, body 0 on the calling
   thread unless something has failed by then; all joined on the way out.  The bodies report through `fe` themselves. */
template <class F> void run_lanes(int n, FirstError &fe, F &&body)
{
    ThreadGroup tg;
    for (int k = 1; k < n; ++k)
        if (!tg.spawn(body, k)) { fe.set("could not start a worker thread"); break; }
    if (n > 0 && !fe.failed.load()) body(0);
}

/* The done-list of a resumable run: a first line that names the run (built by its driver), then "shard <unit> <a> <b>" per
   finished unit (a batch of files, a shard of frames), appended by one worker at a time once the unit's results are on disk.
   read: FRESH (no list, or an empty one), RESUMED (the list of this run: its complete lines that valid() accepts are done
   - a line cut short by a crash does not count) or REFUSED (another run's list; nothing is touched).  open: for appending -
   a fresh list is truncated and gets its first line; 0, -1 cannot open, -2 cannot write.  A driver opens its result files
   between the two, truncated unless resumed(). */
struct DoneList {
    enum { FRESH = 0, RESUMED = 1, REFUSED = 2 };
    int read(const char *path, const char *head, long long n_units, const std::function<bool(long long, long long, long long)> &valid);
    int open();
    bool active() const { return f.fd >= 0; }
    bool resumed() const { return resumed_; }
    bool done(long long k) const { return (size_t)k < done_.size() && done_[(size_t)k]; }
    int append(long long k, long long a, long long b); /* the line, flushed to disk; 0 / -1 */
private:
    Fd f;
    std::mutex mu;
    std::string path_, head_;
    bool resumed_ = false;
    std::vector<char> done_;
};

bool host_pinned(const void *p); /* page-locked already (hipHostMalloc / hipHostRegister, e.g. a pinned tensor)? */
int ensure_pinned(freesasa_gpu_ctx *c, void **p, size_t *cap, size_t bytes); /* grow a context's page-locked staging buffer */

/* The FRAME SOURCE of a trajectory run (gpu_frames.hip): where its frames come from, and everything that depends on it.  The
   driver opens it (a file: open, every refusal of the frames_f32 word and of the file's header; memory: open_memory), asks for
   the frames of the file and the two words of the done-list's first line, plans the run's shards, and per shard calls read and
   to_frames.  Nothing outside gpu_frames.hip looks at `kind` or at what lies below it. */
struct FrameContainer;
struct FrameSource {
    enum Kind { RAW_F64, RAW_F32, DCD, NETCDF, XTC, TRR };
    Kind kind = RAW_F64;
    const double *mem = nullptr; /* raw fp64 frames in host memory ... */
    Fd file;                     /* ... or the frame file: the driver opens it once open() has let the run through */
    bool pbc = false, tri = false; /* every frame among the images of its cell (gpu_periodic.hip); the cell decoded as a triclinic one */

    /* 0, or -1 with the message: before a device is touched or an output file opened */
    int open(const char *path, int frames_f32, long long header_bytes, long long frame_atoms, char *err_out, int err_len);
    void open_memory(const double *frames, size_t frame_atoms);
    long long frames_in_file(long long file_bytes) const;
    /* the done-list's first line: the bits of its f32= word that say what comes IN, and its header_bytes= word (the byte of frame 0) */
    int head_f32() const;
    long long head_bytes() const { return first; }

    /* once the run's shards are known (n_atoms: of a frame as the engine sees it; with_index: a topology's gather picks them
       from the fa atoms that come in) */
    void plan(size_t n_atoms, bool with_index, long long n_frames, int frames_per_batch, const double *radii, double probe);
    size_t shard_bytes(long long f0, long long nf) const; /* of the frames [f0, f0 + nf) as they come in */
    size_t up_bytes(size_t in_bytes, size_t nf) const;    /* what goes up in the shard's one copy */
    size_t xyz_bytes() const;                             /* what c->g_xyz holds of a full shard (0: nothing) ... */
    size_t widen_bytes() const { return (kind == RAW_F32 || kind == XTC) && !gather ? 12 * n * FB : 0; } /* ... and the head of c->h_counts: kl_widen_f32's input */
    size_t cell_doubles() const { return tri ? PBC_TRI_CELL : 3; } /* per frame of a periodic run: edges, or the cell's six numbers and three widths */
    const double *host_cells(const freesasa_gpu_ctx *c, size_t in_bytes) const; /* a periodic shard's cells [nf][cell_doubles] after read ... */
    const double *dev_cells(const freesasa_gpu_ctx *c, size_t in_bytes) const;  /* ... and after to_frames */

    /* host: the shard's bytes in page-locked memory at *src - the caller's own, or the lane's staging filled from memory or
       from the file -, a container's records checked against its header or index, a periodic run's cells decoded and checked */
    int read(freesasa_gpu_ctx *c, long long f0, int nf, size_t in_bytes, const void **src) const;
    /* device: the one copy up, then compact fp64 frames in c->h_xyz, on the context's stream (ta: the topology's gather).  An
       XTC shard waits for the status of its decode; nothing else is waited for. */
    int to_frames(freesasa_gpu_ctx *c, const sasa::TrajArgs &ta, long long f0, int nf, size_t in_bytes, const void *src) const;

    /* (gpu_frames.hip's own) */
    const FrameContainer *con = nullptr; /* the container's row of open's table; NULL: raw frames */
    size_t fa = 0, stride = 0;           /* atoms of a frame as it comes in; bytes from one frame to the next (raw, DCD, NetCDF) */
    long long first = 0;                 /* ... and the byte of frame 0 */
    freesasa_gpu_dcd_info dcd = {};      /* where a DCD frame's planes are (dcd.c) */
    freesasa_gpu_nc_info nc = {};        /* where a NetCDF record's coordinates and cell are (netcdf.c) */
    int real_bytes = 0;                  /* of a TRR file: 4 or 8 (trr.c) */
    std::vector<int64_t> off;            /* XTC, TRR: the byte of every frame [n_frames + 1], by which the shards are cut */
    bool indexed() const { return kind == XTC || kind == TRR; }
    size_t n = 0, FB = 0, max_bytes = 0; /* (plan) atoms the engine sees, frames of a full shard, the bytes of the largest shard */
    bool gather = false, mem_pinned = false;
    double cut = 0;                      /* every edge (width) of a periodic frame's cell must reach c = 2 (max radius + probe) */
    int read_header(const char *path, int *file_atoms, bool *has_cell, char *err_out, int err_len);
};

/* ------------------------------------------------------------------ host batches: the chunk path (gpu_hostbatch.hip)
 * freesasa_gpu_calc_batch, _calc_batch_devices, _calc_batch_pipelined and the cache sweep are ONE path: a BatchCall is what
 * the entry was called with, a Chunk a run of its structures in the hands of one pooled context, and a chunk goes through
 * chunk_size -> _fill -> _upload -> _compute -> _download -> _deliver (chunk_run), each 0 or -1 with the context's message.
 * Declared here: what freesasa_gpu_calc_groups (gpu_groups.hip) shares with them. */

/* the Shrake-Rupley test points of a call (none for Lee-Richards; a resolution <= 0 is run_batch's to refuse) */
std::vector<double> call_test_points(int alg, int resolution);

struct BatchCall {
    const double *xyz = nullptr, *radii = nullptr; /* the caller's arrays ... */
    freesasa_ingest_cache *cache = nullptr;        /* ... or a cache file that holds them */
    const int64_t *offsets = nullptr;              /* of all its structures */
    int alg = 0, resolution = 0;
    double probe = 0;
    std::vector<double> tp;                        /* call_test_points */
    /* the outputs that are wanted: per atom, S&R's counts per atom, per structure, three class sums per structure (cache) */
    double *sasa_out = nullptr;
    int *counts_out = nullptr;
    double *totals_out = nullptr, *class_sums_out = nullptr;
    /* inputs / outputs pass through the context's page-locked stage_in / stage_out (else: copied in place) */
    bool stage_in = false, stage_out = false;
    const char *fallback = "GPU batch failed"; /* the entry's error text when the context has none */
    bool want_counts() const { return counts_out && alg == 1; }
    size_t cols() const { return class_sums_out ? 4 : 1; } /* doubles per structure in c->h_totals: total | class sums */
};
struct Chunk {
    int s0 = 0, ns = 0;           /* structures [s0, s0 + ns) of the call, */
    int64_t a0 = 0;               /* their atoms [a0, a0 + n) */
    size_t n = 0;
    const int64_t *off = nullptr; /* their offsets [ns + 1], rebased to a0 */
    const double *xyz = nullptr, *radii = nullptr; /* (chunk_fill) its inputs where the device copies them from */
    const unsigned char *cls = nullptr;
    double *sasa = nullptr, *totals = nullptr;     /* (chunk_download) its outputs where the device copies them to */
    int *counts = nullptr;
};
/* the device buffers of a chunk - c->h_xyz, h_radii, h_sasa, h_totals; h_counts for what rides beside the atoms (S&R's counts
   out, the cache's classes in) - and the staging the call asks for; the inputs enqueued on the context's stream */
int chunk_size(const BatchCall &b, freesasa_gpu_ctx *c, const Chunk &h);
int chunk_upload(freesasa_gpu_ctx *c, const Chunk &h);
/* The one failure epilogue: nothing is left running on the stream (the caller's arrays are not touched after the entry
   returns); the text is the context's message or the entry's fallback. */
const char *chunk_failed(const BatchCall &b, freesasa_gpu_ctx *c);

#endif
