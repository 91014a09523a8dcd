/*
 * gpu_interfaces.hip — pairwise interface areas between chain groups (include/freesasa_gpu.h: freesasa_gpu_interface_pairs_dev,
 * freesasa_gpu_interfaces_dev, freesasa_gpu_calc_interface_pairs, freesasa_gpu_calc_interfaces) and their per-residue tables
 * (freesasa_gpu_interface_residues_dev, freesasa_gpu_calc_interface_residues) and atom-atom contact tables
 * (freesasa_gpu_interface_contacts_dev, freesasa_gpu_calc_interface_contacts).  Host code; the kernels are in gpu_kernels.hip
 * (phase functions: iface_kernels.h, contact_kernels.h).
 *
 *   1. groups_resident   the chain-group pipeline as it is: the combined batch stays in c->g_xyz / g_radii / g_src, its areas in
 *                        c->g_sasa, its totals in c->g_tot; the groups' atom counts are on the host
 *   2. boxes             k_iface_box: one wave per isolated group
 *   3. candidates        k_iface_candidates: one thread per pair (g < h) of a structure, the candidates appended to a list
 *   4. exact contact     k_iface_contact: a workgroup per candidate at a time, one flag per pair
 *   5. order and sizes   the flags come back (one stream synchronization, like the counts of step 1); the host walks them in
 *                        the table's order: rows, side_offsets, P, M
 *   6. pair batch        k_iface_gather: one thread per pair-structure atom
 *   7. one run_batch     over the P pair structures: same algorithm, probe, resolution and unit points
 *   8. finish            k_iface_finish_atom, kl_segment_sums over the 2 P sides, k_iface_finish_row
 *
 * iface_screen is steps 1 to 5, iface_pipeline all of them; the pipeline's results stay in the context's own buffers and the
 * entries deliver them - to device arrays or to host arrays - once the capacities have been held against P and M, so that a
 * call that fails for its capacities has written none of the caller's pair arrays.
 *
 * The residue entries run iface_pipeline as it is and one more stage behind it:
 *   9. residues          iface_residues: k_iface_res_head, the block scan, k_iface_res_first, k_iface_res_segment, the scan again,
 *                        k_iface_res_rows; R comes back (one more stream synchronization); the table stays in c->if_rtable
 * and hold the three capacities against P, M and R together, once R is known (iface_res_check_caps), before anything is delivered.
 *
 * The contact entries (freesasa_gpu_interface_contacts_dev, freesasa_gpu_calc_interface_contacts; Shrake-Rupley only; phase
 * functions: contact_kernels.h) likewise run iface_pipeline as it is and one more stage behind it:
 *  10. contacts          iface_contacts: two more engine runs over the M pair-structure atoms with the mask request (masks_resident:
 *                        as the P pair structures, as the 2 P sides), k_contact_masks, the dots' scan - D_b comes back (one stream
 *                        synchronization) and sizes what follows - the dots' expansion, k_contact_attribute, k_contact_rows_count /
 *                        _rank, the block scan, k_contact_rows_write; C and the flag come back (one more); the table stays in
 *                        c->if_ctable, the masks in c->if_cmasks, the dots in c->if_cdots
 * and hold the four capacities against P, M, C and D_b together (iface_contact_check_caps) before anything is delivered.
 *
 * The residue-residue contact entries (freesasa_gpu_interface_residue_contacts_dev, freesasa_gpu_calc_interface_residue_contacts;
 * phase functions: rescontact_kernels.h) run the contact entries' path as it is and one more stage behind it:
 *  11. residue contacts  iface_rescontacts: the per-residue tables' k_iface_res_head, block scan and k_iface_res_first (the segments),
 *                        k_rc_fold_count, the block scan, k_rc_fold_write, k_rc_reverse; Q comes back (one more stream
 *                        synchronization); the table stays in c->if_rctable
 * and hold the five capacities against P, M, C, D_b and Q together (iface_rescontact_check_caps) before anything is delivered.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "engine_internal.h"

using namespace sasa;

namespace {

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

/* what every entry checks before a device is touched: 0, or the message in msg */
int iface_bad_args(const void *xyz, const void *radii, const int64_t *offsets, int n_structs, const void *group, const int32_t *n_groups,
                   int alg, int resolution, char *msg, size_t len)
{
    const char *bad = nullptr;
    if (!xyz || !radii || !offsets || !group || !n_groups) bad = "null argument";
    else if (alg != 0 && alg != 1) { snprintf(msg, len, "unknown algorithm %d", alg); return -1; }
    else if (n_structs <= 0) bad = "n_structs must be > 0";
    else if (resolution <= 0) bad = "resolution must be > 0";
    else if (offsets[0] != 0) bad = "offsets[0] must be 0";
    if (bad) { snprintf(msg, len, "%s", bad); return -1; }
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] < offsets[s]) { snprintf(msg, len, "offsets must be non-decreasing"); return -1; }
    if (offsets[n_structs] <= 0) { snprintf(msg, len, "empty batch"); return -1; }
    int64_t T = 0;
    for (int s = 0; s < n_structs; ++s) {
        const int64_t ng = n_groups[s];
        if (ng > IF_MAX_GROUPS && ng <= 65535) { /* (a count the chain-group entry refuses is left to it, with its message) */
            snprintf(msg, len, "structure %d has %lld groups: interfaces are made for up to %d groups of a structure", s, (long long)ng, IF_MAX_GROUPS);
            return -1;
        }
        if (ng >= 2 && ng <= IF_MAX_GROUPS) T += ng * (ng - 1) / 2;
        if (T > IF_MAX_TESTS) {
            snprintf(msg, len, "structures 0 .. %d have %lld pairs of groups to test: a call takes up to %d", s, (long long)T, IF_MAX_TESTS);
            return -1;
        }
    }
    return 0;
}
int iface_bad_caps(long long pair_capacity, long long atom_capacity, char *msg, size_t len)
{
    if (pair_capacity < 0) { snprintf(msg, len, "pair_capacity must be >= 0 (it is %lld)", pair_capacity); return -1; }
    if (atom_capacity < 0) { snprintf(msg, len, "atom_capacity must be >= 0 (it is %lld)", atom_capacity); return -1; }
    return 0;
}

/* steps 1 to 5 on arrays that are on the context's stream; at its end the stream is idle (the flags are on the host) */
int iface_screen(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                 const int32_t *d_group, const int32_t *n_groups, double probe, int resolution, double *d_sasa, double *d_iso,
                 double *d_totals, double *d_group_totals, IfacePlan &pl, IfaceArgs &ia)
{
    if (alg == 1) pl.tp = call_test_points(alg, resolution);
    std::vector<int> cnt;
    if (groups_resident(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe, resolution, alg == 1 ? pl.tp.data() : nullptr,
                        d_sasa, d_iso, d_totals, d_group_totals, &cnt))
        return -1;
    const int G = (int)cnt.size();
    const int64_t n = offsets[n_structs];
    pl.G = G; pl.n = n;
    pl.meta.assign((size_t)G + 1 + (size_t)n_structs + 1, 0);
    int64_t *gstart = pl.meta.data(), *tbase = gstart + G + 1;
    gstart[0] = n;
    for (int k = 0; k < G; ++k) gstart[k + 1] = gstart[k] + cnt[(size_t)k];
    pl.n_iso = gstart[G] - n;
    int64_t T = 0;
    for (int s = 0; s < n_structs; ++s) {
        tbase[s] = T;
        const int64_t ng = n_groups[s];
        T += ng * (ng - 1) / 2;
    }
    tbase[n_structs] = T;
    pl.T = T;

    memset(&ia, 0, sizeof ia);
    ia.cxyz = (const double *)c->g_xyz.p; ia.cradii = (const double *)c->g_radii.p; ia.src = (const int *)c->g_src.p;
    ia.csasa = (const double *)c->g_sasa.p; ia.ctot = (const double *)c->g_tot.p;
    ia.n_atoms = (int)n; ia.n_structs = n_structs; ia.n_groups = G; ia.probe = probe;
    ia.gbase = (const int64_t *)c->g_meta.p + n_structs + 1;
    ia.n_tests = (int)T;
    pl.side_off.assign(1, 0);
    if (T == 0) return 0;

    hipStream_t st = c->stream;
    if (ensure(c, c->if_meta, 8 * pl.meta.size()) || ensure(c, c->if_box, 64 * (size_t)G) || ensure(c, c->if_cand, 4 * (size_t)T + 8) ||
        ensure(c, c->if_flag, (size_t)T))
        return -1;
    ia.gstart = (const int64_t *)c->if_meta.p; ia.tbase = ia.gstart + G + 1;
    ia.box = (double *)c->if_box.p;
    ia.n_cand = (int *)c->if_cand.p; ia.cand = ia.n_cand + 2;
    ia.flag = (unsigned char *)c->if_flag.p;
    HIP_TRY(c, hipMemcpyAsync(c->if_meta.p, pl.meta.data(), 8 * pl.meta.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->if_cand.p, 0, 8, st));
    HIP_TRY(c, hipMemsetAsync(c->if_flag.p, 0, (size_t)T, st));
    HIP_TRY(c, kl_iface_box(ia, st));
    HIP_TRY(c, kl_iface_candidates(ia, st));
    HIP_TRY(c, kl_iface_contact(ia, st));
    std::vector<unsigned char> flag((size_t)T);
    int nc = 0;
    HIP_TRY(c, hipMemcpyAsync(flag.data(), c->if_flag.p, (size_t)T, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&nc, c->if_cand.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    pl.n_cand = nc;

    /* 5. the table's order is the tests' order */
    int64_t P = 0;
    for (int64_t t = 0; t < T; ++t) P += flag[(size_t)t];
    pl.P = P;
    pl.pair_struct.reserve((size_t)P); pl.pair_groups.reserve(2 * (size_t)P); pl.side_off.reserve(2 * (size_t)P + 1);
    std::vector<int64_t> start; std::vector<int32_t> grp;
    start.reserve(2 * (size_t)P); grp.reserve(2 * (size_t)P);
    int64_t t = 0, k0 = 0, M = 0;
    for (int s = 0; s < n_structs; ++s) {
        const int ng = n_groups[s];
        for (int g = 0; g + 1 < ng; ++g)
            for (int h = g + 1; h < ng; ++h, ++t) {
                if (!flag[(size_t)t]) continue;
                pl.pair_struct.push_back(s);
                pl.pair_groups.push_back(g); pl.pair_groups.push_back(h);
                for (int side = 0; side < 2; ++side) {
                    const int64_t k = k0 + (side ? h : g);
                    start.push_back(gstart[k]); grp.push_back((int32_t)k);
                    M += cnt[(size_t)k];
                    pl.side_off.push_back(M);
                }
            }
        k0 += ng;
    }
    pl.M = M;
    pl.pair_off.resize((size_t)P + 1);
    for (int64_t p = 0; p <= P; ++p) pl.pair_off[(size_t)p] = pl.side_off[2 * (size_t)p];
    /* side_off | side_start | side_group (two int32 to a word) */
    pl.sides.assign(2 * (size_t)P + 1 + 2 * (size_t)P + (size_t)P, 0);
    if (P > 0) {
        memcpy(pl.sides.data(), pl.side_off.data(), 8 * (2 * (size_t)P + 1));
        memcpy(pl.sides.data() + 2 * P + 1, start.data(), 8 * 2 * (size_t)P);
        memcpy(pl.sides.data() + 4 * P + 1, grp.data(), 4 * 2 * (size_t)P);
    }
    return 0;
}

/* what an entry wants delivered: held against P and M before anything of steps 6 to 8 runs */
struct IfaceWant {
    long long pair_capacity = 0, atom_capacity = 0;
    bool rows = false;  /* one of pair_struct, pair_groups, pair_areas, side_offsets */
    bool atoms = false; /* one of pair_atom, pair_buried */
};
int iface_check_caps(freesasa_gpu_ctx *c, const IfacePlan &pl, const IfaceWant &w)
{
    if (w.rows && pl.P > w.pair_capacity)
        return ctx_fail(c, "pair_capacity %lld is too small: the batch has %lld pairs of groups in contact", w.pair_capacity, (long long)pl.P);
    if (w.atoms && pl.M > w.atom_capacity)
        return ctx_fail(c, "atom_capacity %lld is too small: the pair structures hold %lld atoms", w.atom_capacity, (long long)pl.M);
    return 0;
}

/* the whole pipeline: the rows in c->if_areas [6 P], the per-atom arrays in c->if_patom / c->if_pburied [M]; nothing is waited
   for at its end beyond what run_batch waits for */
int iface_pipeline(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                   const int32_t *d_group, const int32_t *n_groups, double probe, int resolution, double *d_sasa, double *d_iso,
                   double *d_totals, double *d_group_totals, const IfaceWant &w, IfacePlan &pl, long long *n_pairs_out,
                   long long *n_pair_atoms_out)
{
    IfaceArgs ia;
    if (iface_screen(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe, resolution, d_sasa, d_iso, d_totals,
                     d_group_totals, pl, ia))
        return -1;
    if (n_pairs_out) *n_pairs_out = pl.P;
    if (n_pair_atoms_out) *n_pair_atoms_out = pl.M;
    if (iface_check_caps(c, pl, w)) return -1;
    if (pl.n + pl.n_iso + pl.M > (int64_t)1 << 30)
        return ctx_fail(c, "the batch (%lld atoms), its groups (%lld) and the pair structures (%lld) hold more than 2^30 atoms together",
                        (long long)pl.n, (long long)pl.n_iso, (long long)pl.M);
    if (pl.P == 0) return 0;
    const size_t P = (size_t)pl.P, M = (size_t)pl.M;
    hipStream_t st = c->stream;
    if (ensure(c, c->if_sides, 8 * pl.sides.size()) || ensure(c, c->if_xyz, 24 * M) || ensure(c, c->if_radii, 8 * M) ||
        ensure(c, c->if_comb, 4 * M) || ensure(c, c->if_sasa, 8 * M) || ensure(c, c->if_inpair, 16 * P) || ensure(c, c->if_areas, 48 * P) ||
        ensure(c, c->if_patom, 4 * M) || ensure(c, c->if_pburied, 8 * M))
        return -1;
    ia.n_sides = 2 * pl.P; ia.n_pair_atoms = pl.M;
    ia.side_off = (const int64_t *)c->if_sides.p; ia.side_start = ia.side_off + 2 * P + 1; ia.side_group = (const int *)(ia.side_start + 2 * P);
    ia.pxyz = (double *)c->if_xyz.p; ia.pradii = (double *)c->if_radii.p; ia.pcomb = (int *)c->if_comb.p; ia.pair_atom = (int *)c->if_patom.p;
    ia.psasa = (const double *)c->if_sasa.p; ia.inpair = (const double *)c->if_inpair.p;
    ia.pair_buried = (double *)c->if_pburied.p; ia.pair_areas = (double *)c->if_areas.p;
    HIP_TRY(c, hipMemcpyAsync(c->if_sides.p, pl.sides.data(), 8 * pl.sides.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, kl_iface_gather(ia, st));
    if (run_batch(c, alg == 0, ia.pxyz, ia.pradii, pl.pair_off.data(), (int)P, probe, resolution, alg == 1 ? pl.tp.data() : nullptr,
                  (double *)c->if_sasa.p, nullptr, nullptr))
        return -1;
    HIP_TRY(c, kl_segment_sums(ia.psasa, ia.side_off, (int)(2 * P), pl.M < (int64_t)64 * 2 * (int64_t)P, (double *)c->if_inpair.p, st));
    HIP_TRY(c, kl_iface_finish(ia, st));
    return 0;
}

/* the per-residue tables: what an entry gives on top of the interface entries' arguments, and what it wants back */
struct IfaceResWant {
    const int64_t *res_first = nullptr;
    int n_res = 0;
    double min_buried = 0;
    long long res_capacity = 0;
    long long *n_res_rows_out = nullptr;
};
/* ... checked before a device is touched, behind iface_bad_args and iface_bad_caps: 0, or the message in msg */
int iface_res_bad_args(const IfaceResWant &rw, const int64_t *offsets, int n_structs, char *msg, size_t len)
{
    if (!rw.res_first || !rw.n_res_rows_out) { snprintf(msg, len, "null argument"); return -1; }
    if (rw.n_res <= 0) { snprintf(msg, len, "n_res must be > 0"); return -1; }
    if (!(rw.min_buried >= 0.0) || rw.min_buried > 1.7976931348623157e308) { snprintf(msg, len, "min_buried must be finite and >= 0"); return -1; }
    if (rw.res_capacity < 0) { snprintf(msg, len, "res_capacity must be >= 0 (it is %lld)", rw.res_capacity); return -1; }
    if (rw.res_first[0] != 0) { snprintf(msg, len, "res_first[0] must be 0"); return -1; }
    for (int r = 0; r < rw.n_res; ++r)
        if (rw.res_first[r + 1] < rw.res_first[r]) { snprintf(msg, len, "res_first must be non-decreasing"); return -1; }
    if (rw.res_first[rw.n_res] != offsets[n_structs]) {
        snprintf(msg, len, "res_first[n_res] is %lld: the batch has %lld atoms", (long long)rw.res_first[rw.n_res], (long long)offsets[n_structs]);
        return -1;
    }
    int s = 0;
    for (int r = 0; r < rw.n_res; ++r) {
        const int64_t b = rw.res_first[r], e = rw.res_first[r + 1];
        if (b == e) continue;
        while (offsets[s + 1] <= b) ++s; /* (b < offsets[n_structs]: the structure that holds the residue's first atom) */
        if (e > offsets[s + 1]) { snprintf(msg, len, "residue %d spans the boundary between structures %d and %d", r, s, s + 1); return -1; }
    }
    return 0;
}

/* the stage behind iface_pipeline (k_iface_finish is the last thing on the stream): the table in c->if_rtable - res_offsets
   [2 P + 1] | res_areas [3 M] | res_index [M] | res_atoms [M], R rows of them used; R comes back to the host (one stream
   synchronization), so at the stage's end the stream is idle */
struct IfaceResTable {
    int64_t R = 0;
    const int64_t *off = nullptr;
    const double *areas = nullptr;
    const int32_t *index = nullptr, *atoms = nullptr;
    std::vector<int64_t> first; /* the upload of res_first (like the plan, the table lives until the stream is idle) */
};
int iface_residues(freesasa_gpu_ctx *c, const IfacePlan &pl, const IfaceResWant &rw, const double *d_iso, IfaceResTable &t)
{
    t.R = 0;
    if (pl.P == 0) return 0;
    const size_t P = (size_t)pl.P, M = (size_t)pl.M;
    const size_t S = (size_t)ifr_scan_scratch(pl.M);
    hipStream_t st = c->stream;
    if (ensure(c, c->if_rfirst, 8 * ((size_t)rw.n_res + 1)) || ensure(c, c->if_rwork, 4 * (6 * M + 3 + S) + 8) ||
        ensure(c, c->if_rsegs, 24 * M) || ensure(c, c->if_rtable, 8 * (2 * P + 1) + 24 * M + 8 * M))
        return -1;
    IfaceResArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = pl.M; a.n_sides = 2 * pl.P; a.n_res = rw.n_res;
    a.side_off = (const int64_t *)c->if_sides.p; a.pair_atom = (const int *)c->if_patom.p;
    a.res_first = (const int64_t *)c->if_rfirst.p; a.iso = d_iso; a.psasa = (const double *)c->if_sasa.p;
    a.min_buried = rw.min_buried;
    int *w = (int *)c->if_rwork.p;
    a.atom_res = w; a.hs = w + M; a.seg_first = a.hs + M + 1; a.seg_res = a.seg_first + M + 1; a.seg_atoms = a.seg_res + M; a.ks = a.seg_atoms + M;
    int *scratch = a.ks + M + 1;
    a.seg_areas = (double *)c->if_rsegs.p;
    a.res_off = (int64_t *)c->if_rtable.p; a.res_areas = (double *)(a.res_off + 2 * P + 1);
    a.res_index = (int *)(a.res_areas + 3 * M); a.res_atoms = a.res_index + M;
    /* (the upload's source is the stage's own copy, as the plan's arrays are: what the device searches is what was copied here,
       whatever becomes of the caller's array while the stream runs) */
    t.first.assign(rw.res_first, rw.res_first + rw.n_res + 1);
    HIP_TRY(c, hipMemcpyAsync(c->if_rfirst.p, t.first.data(), 8 * t.first.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, kl_iface_res_segments(a, scratch, st));
    HIP_TRY(c, kl_iface_res_rows(a, scratch, st));
    int R = 0;
    HIP_TRY(c, hipMemcpyAsync(&R, a.ks + M, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    t.R = R; t.off = a.res_off; t.areas = a.res_areas; t.index = a.res_index; t.atoms = a.res_atoms;
    return 0;
}
/* the three capacities against P, M and R, in this order, with the interface entries' messages for the first two */
int iface_res_check_caps(freesasa_gpu_ctx *c, const IfacePlan &pl, const IfaceWant &w, const IfaceResWant &rw, int64_t R)
{
    if (iface_check_caps(c, pl, w)) return -1;
    if (R > rw.res_capacity)
        return ctx_fail(c, "res_capacity %lld is too small: the interfaces have %lld residue rows", rw.res_capacity, (long long)R);
    return 0;
}

/* the atom-atom contact tables: what an entry gives on top of the interface entries' arguments, and what it wants back */
struct IfaceContactWant {
    long long contact_capacity = 0, dot_capacity = 0;
    long long *n_contacts_out = nullptr, *n_buried_dots_out = nullptr;
    bool rows = false; /* one of contact_partner, contact_points, contact_area */
    bool dots = false; /* dot_partner */
};
/* ... checked before a device is touched, behind iface_bad_args and iface_bad_caps: 0, or the message in msg */
int iface_contact_bad_args(const IfaceContactWant &cw, int alg, int resolution, const void *masks, char *msg, size_t len)
{
    if (!cw.n_contacts_out) { snprintf(msg, len, "null argument"); return -1; }
    if (alg != 1) { snprintf(msg, len, "the contact tables are made of Shrake-Rupley test points: Lee-Richards has none"); return -1; }
    if (resolution > SR_CAP_POINTS_MAX) {
        snprintf(msg, len, "the contact tables are offered up to %d test points (%d asked for)", SR_CAP_POINTS_MAX, resolution);
        return -1;
    }
    if (cw.contact_capacity < 0) { snprintf(msg, len, "contact_capacity must be >= 0 (it is %lld)", cw.contact_capacity); return -1; }
    if (cw.dot_capacity < 0) { snprintf(msg, len, "dot_capacity must be >= 0 (it is %lld)", cw.dot_capacity); return -1; }
    if ((uintptr_t)masks % 16) { snprintf(msg, len, "the buried mask array must be aligned to 16 bytes (an atom's four words are one store)"); return -1; }
    return 0;
}

/* the stage behind iface_pipeline (Shrake-Rupley; k_iface_finish is the last thing on the stream): the table in c->if_ctable -
   contact_first [M + 1] | contact_area [D_b] | contact_partner [D_b] | contact_points [D_b], C rows of them used -, the buried masks
   in c->if_cmasks, the dots' partners in c->if_cdots.  D_b, then C and the flag come back to the host (two stream
   synchronizations), so at the stage's end the stream is idle. */
struct IfaceContactTable {
    int64_t C = 0, D = 0;
    const int64_t *first = nullptr;
    const int32_t *partner = nullptr, *points = nullptr, *dot_partner = nullptr;
    const double *area = nullptr;
    const unsigned *buried = nullptr;
};
int iface_contacts(freesasa_gpu_ctx *c, const IfacePlan &pl, double probe, int n_points, IfaceContactTable &t)
{
    t = IfaceContactTable();
    if (pl.P == 0) return 0;
    const size_t P = (size_t)pl.P, M = (size_t)pl.M;
    const size_t S = (size_t)ifr_scan_scratch(pl.M);
    hipStream_t st = c->stream;
    /* side masks | pair masks | buried masks (16 M bytes each) | the two runs' areas [M] (nobody reads them) */
    if (ensure(c, c->if_cmasks, 48 * M + 8 * M) || ensure(c, c->if_cwork, 8 * (M + 1) + 4 * (M + 1 + S + 1)) || dots_unit_ready(c, n_points))
        return -1;
    unsigned *side_masks = (unsigned *)c->if_cmasks.p, *pair_masks = side_masks + SR_CAP_WORDS * M, *buried = pair_masks + SR_CAP_WORDS * M;
    double *areas = (double *)(buried + SR_CAP_WORDS * M);
    int64_t *dot_first = (int64_t *)c->if_cwork.p;
    int *nd = (int *)(dot_first + M + 1), *scratch = nd + M + 1, *flag = scratch + S;
    const double *pxyz = (const double *)c->if_xyz.p, *pradii = (const double *)c->if_radii.p;
    /* the same atoms as P structures and as 2 P: what the pair run and the groups' run of the pipeline counted, as masks */
    if (masks_resident(c, pxyz, pradii, pl.pair_off.data(), (int)P, probe, n_points, pl.tp.data(), areas, nullptr, nullptr, pair_masks) ||
        masks_resident(c, pxyz, pradii, pl.side_off.data(), (int)(2 * P), probe, n_points, pl.tp.data(), areas, nullptr, nullptr, side_masks))
        return -1;
    ContactArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = pl.M; a.n_sides = 2 * pl.P; a.n_points = n_points; a.probe = probe;
    a.side_off = (const int64_t *)c->if_sides.p; a.pxyz = pxyz; a.pradii = pradii;
    a.side_masks = side_masks; a.pair_masks = pair_masks; a.buried = buried;
    a.dot_first = dot_first; a.nd = nd; a.flag = flag;
    HIP_TRY(c, kl_contact_masks(a, st));
    if (dots_count_resident(c, buried, pl.M, n_points, dot_first)) return -1;
    int64_t D = 0;
    HIP_TRY(c, hipMemcpyAsync(&D, dot_first + M, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    t.D = D; t.buried = buried;
    if (D > 0x7fffffffLL) return ctx_fail(c, "the interfaces bury %lld test points: a call takes up to 2^31 - 1", (long long)D);
    if (D == 0) return 0; /* (no buried point: no row) */
    const size_t Db = (size_t)D;
    if (ensure(c, c->if_cdots, 24 * Db + 4 * 5 * Db) || ensure(c, c->if_ctable, 8 * (M + 1) + 8 * Db + 4 * 2 * Db)) return -1;
    double *dot_xyz = (double *)c->if_cdots.p;
    int *dot_atom = (int *)(dot_xyz + 3 * Db), *dot_point = dot_atom + Db;
    a.n_dots = D; a.dot_xyz = dot_xyz; a.dot_atom = dot_atom; a.dot_partner = dot_point + Db; a.cnt = a.dot_partner + Db; a.rank = a.cnt + Db;
    a.contact_first = (int64_t *)c->if_ctable.p; a.contact_area = (double *)(a.contact_first + M + 1);
    a.contact_partner = (int *)(a.contact_area + Db); a.contact_points = a.contact_partner + Db;
    HIP_TRY(c, hipMemsetAsync(nd, 0, 4 * (M + 1 + S + 1), st)); /* (the atoms' counts, the scan's levels, the flag) */
    if (dots_expand_resident(c, pxyz, pradii, pl.M, probe, n_points, buried, dot_first, D, dot_xyz, dot_atom, dot_point)) return -1;
    HIP_TRY(c, kl_contact_attribute(a, st));
    HIP_TRY(c, kl_contact_rows(a, scratch, st));
    int back[2] = {0, 0}; /* C, the flag */
    HIP_TRY(c, hipMemcpyAsync(&back[0], nd + M, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&back[1], flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (back[1] != 0)
        return ctx_fail(c, "pair-structure atom %d has a buried test point that no atom of the other side covers: the exposure masks and the cover test disagree",
                        back[1] - 1);
    t.C = back[0]; t.first = a.contact_first; t.partner = a.contact_partner; t.points = a.contact_points; t.area = a.contact_area;
    t.dot_partner = a.dot_partner;
    return 0;
}
/* the four capacities against P, M, C and D_b, in this order, with the interface entries' messages for the first two */
int iface_contact_check_caps(freesasa_gpu_ctx *c, const IfacePlan &pl, const IfaceWant &w, const IfaceContactWant &cw, const IfaceContactTable &t)
{
    if (iface_check_caps(c, pl, w)) return -1;
    if (cw.rows && t.C > cw.contact_capacity)
        return ctx_fail(c, "contact_capacity %lld is too small: the interfaces have %lld contact rows", cw.contact_capacity, (long long)t.C);
    if (cw.dots && t.D > cw.dot_capacity)
        return ctx_fail(c, "dot_capacity %lld is too small: the interfaces bury %lld test points", cw.dot_capacity, (long long)t.D);
    return 0;
}

/* the residue-residue contact tables: what an entry gives on top of the contact entries' arguments, and what it wants back */
struct IfaceResContactWant {
    const int64_t *res_first = nullptr;
    int n_res = 0;
    long long rescontact_capacity = 0;
    long long *n_rescontacts_out = nullptr;
};
/* ... checked before a device is touched, behind the contact entries' checks: res_first by the residue entries' own check */
int iface_rescontact_bad_args(const IfaceResContactWant &qw, const int64_t *offsets, int n_structs, char *msg, size_t len)
{
    IfaceResWant rw;
    rw.res_first = qw.res_first; rw.n_res = qw.n_res; rw.n_res_rows_out = qw.n_rescontacts_out;
    if (iface_res_bad_args(rw, offsets, n_structs, msg, len)) return -1;
    if (qw.rescontact_capacity < 0) { snprintf(msg, len, "rescontact_capacity must be >= 0 (it is %lld)", qw.rescontact_capacity); return -1; }
    return 0;
}

/* the stage behind iface_contacts (the stream is idle, C is on the host): the segments of the per-residue tables by their own
   kernels, the fold of the contact rows per partner segment, the reverse rows; the table in c->if_rctable - rescontact_offsets
   [2 P + 1] | rescontact_area [C] | rescontact_residues [2 C] | rescontact_counts [2 C] | rescontact_reverse [C], Q rows of them
   used.  Q comes back to the host (one stream synchronization), so at the stage's end the stream is idle.  Without a contact row
   nothing is launched: Q = 0. */
struct IfaceResContactTable {
    int64_t Q = 0;
    const int64_t *off = nullptr;
    const double *area = nullptr;
    const int32_t *res = nullptr, *cnt = nullptr, *rev = nullptr;
    std::vector<int64_t> first; /* the upload of res_first (like the plan, the table lives until the stream is idle) */
};
int iface_rescontacts(freesasa_gpu_ctx *c, const IfacePlan &pl, const IfaceResContactWant &qw, const IfaceContactTable &ct, IfaceResContactTable &t)
{
    t.Q = 0;
    if (pl.P == 0 || ct.C == 0) return 0;
    const size_t P = (size_t)pl.P, M = (size_t)pl.M, Cn = (size_t)ct.C;
    const size_t S = (size_t)ifr_scan_scratch(pl.M);
    hipStream_t st = c->stream;
    if (ensure(c, c->if_rfirst, 8 * ((size_t)qw.n_res + 1)) || ensure(c, c->if_rcwork, 4 * (4 * M + 3 + S + Cn)) ||
        ensure(c, c->if_rctable, 8 * (2 * P + 1) + 8 * Cn + 4 * 5 * Cn))
        return -1;
    int *w = (int *)c->if_rcwork.p;
    IfaceResArgs s;
    memset(&s, 0, sizeof s);
    s.n_pair_atoms = pl.M; s.n_sides = 2 * pl.P; s.n_res = qw.n_res;
    s.side_off = (const int64_t *)c->if_sides.p; s.pair_atom = (const int *)c->if_patom.p; s.res_first = (const int64_t *)c->if_rfirst.p;
    s.atom_res = w; s.hs = w + M; s.seg_first = s.hs + M + 1;
    ResContactArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = pl.M; a.n_sides = 2 * pl.P; a.row_cap = ct.C;
    a.side_off = s.side_off; a.atom_res = s.atom_res; a.hs = s.hs; a.seg_first = s.seg_first;
    a.contact_first = ct.first; a.contact_partner = ct.partner; a.contact_points = ct.points; a.contact_area = ct.area;
    a.fc = s.seg_first + M + 1;
    int *scratch = a.fc + M + 1;
    a.pseg = scratch + S;
    a.rc_off = (int64_t *)c->if_rctable.p; a.rc_area = (double *)(a.rc_off + 2 * P + 1);
    a.rc_res = (int *)(a.rc_area + Cn); a.rc_cnt = a.rc_res + 2 * Cn; a.rc_rev = a.rc_cnt + 2 * Cn;
    t.first.assign(qw.res_first, qw.res_first + qw.n_res + 1); /* (the stage's own copy: iface_residues) */
    HIP_TRY(c, hipMemcpyAsync(c->if_rfirst.p, t.first.data(), 8 * t.first.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(a.fc, 0, 4 * (M + 1), st)); /* (the segments' counts: a slot at or beyond K has none) */
    HIP_TRY(c, kl_rc_segments(s, scratch, st));
    HIP_TRY(c, kl_rc_fold(a, scratch, st));
    int Q = 0;
    HIP_TRY(c, hipMemcpyAsync(&Q, a.fc + M, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    t.Q = Q; t.off = a.rc_off; t.area = a.rc_area; t.res = a.rc_res; t.cnt = a.rc_cnt; t.rev = a.rc_rev;
    return 0;
}
/* the five capacities against P, M, C, D_b and Q, in this order */
int iface_rescontact_check_caps(freesasa_gpu_ctx *c, const IfacePlan &pl, const IfaceWant &w, const IfaceContactWant &cw, const IfaceContactTable &ct,
                                const IfaceResContactWant &qw, int64_t Q)
{
    if (iface_contact_check_caps(c, pl, w, cw, ct)) return -1;
    if (Q > qw.rescontact_capacity)
        return ctx_fail(c, "rescontact_capacity %lld is too small: the interfaces have %lld residue contact rows", qw.rescontact_capacity, (long long)Q);
    return 0;
}

int iface_dev_checks(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                     const int32_t *d_group, const int32_t *n_groups, int alg, int resolution, long long pair_capacity, long long atom_capacity)
{
    char msg[200];
    c->err[0] = 0;
    if (iface_bad_args(d_xyz, d_radii, offsets, n_structs, d_group, n_groups, alg, resolution, msg, sizeof msg) ||
        iface_bad_caps(pair_capacity, atom_capacity, msg, sizeof msg))
        return ctx_fail(c, "%s", msg);
    if (offsets[n_structs] > (int64_t)1 << 30) return ctx_fail(c, "batch too large (max 2^30 atoms per call)");
    if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
    return 0;
}

/* the screen's rows into host arrays */
void iface_rows_to_host(const IfacePlan &pl, int32_t *pair_struct_out, int32_t *pair_groups_out, long long *stats_out)
{
    if (pair_struct_out && pl.P > 0) memcpy(pair_struct_out, pl.pair_struct.data(), 4 * (size_t)pl.P);
    if (pair_groups_out && pl.P > 0) memcpy(pair_groups_out, pl.pair_groups.data(), 8 * (size_t)pl.P);
    if (stats_out) { stats_out[0] = pl.T; stats_out[1] = pl.n_cand; }
}

} /* namespace */

extern "C" int freesasa_gpu_interface_pairs_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                                const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                                double probe_radius, int resolution, double *d_sasa, double *d_iso, double *d_totals,
                                                double *d_group_totals, long long pair_capacity, long long *n_pairs_out,
                                                long long *n_pair_atoms_out, int32_t *pair_struct_out, int32_t *pair_groups_out,
                                                long long *stats_out)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first) */
    return guarded_ctx(c, [&]() -> int {
        if (iface_dev_checks(c, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, alg, resolution, pair_capacity, 0)) return -1;
        if (!n_pairs_out || !n_pair_atoms_out) return ctx_fail(c, "null argument");
        IfacePlan pl;
        IfaceArgs ia;
        int rc = iface_screen(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe_radius, resolution, d_sasa, d_iso,
                              d_totals, d_group_totals, pl, ia);
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "stream synchronize failed");
        if (rc) return rc;
        *n_pairs_out = pl.P; *n_pair_atoms_out = pl.M;
        IfaceWant w;
        w.pair_capacity = pair_capacity; w.rows = pair_struct_out || pair_groups_out;
        if (iface_check_caps(c, pl, w)) return -1;
        iface_rows_to_host(pl, pair_struct_out, pair_groups_out, stats_out);
        return 0;
    });
}

extern "C" int freesasa_gpu_interfaces_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                           const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                           double probe_radius, int resolution, double *d_sasa, double *d_iso, double *d_totals,
                                           double *d_group_totals, long long pair_capacity, long long atom_capacity,
                                           long long *n_pairs_out, long long *n_pair_atoms_out, int32_t *d_pair_struct,
                                           int32_t *d_pair_groups, double *d_pair_areas, int64_t *d_side_offsets, int32_t *d_pair_atom,
                                           double *d_pair_buried)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1;
    return guarded_ctx(c, [&]() -> int {
        if (iface_dev_checks(c, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, alg, resolution, pair_capacity, atom_capacity)) return -1;
        if (!d_sasa || !d_iso || !n_pairs_out || !n_pair_atoms_out || !d_pair_areas) return ctx_fail(c, "null argument");
        IfacePlan pl; /* (its arrays are the sources of copies enqueued below: it lives until the stream is idle) */
        IfaceWant w;
        w.pair_capacity = pair_capacity; w.atom_capacity = atom_capacity; w.rows = true; w.atoms = d_pair_atom || d_pair_buried;
        int rc = [&]() -> int {
            if (iface_pipeline(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe_radius, resolution, d_sasa, d_iso,
                               d_totals, d_group_totals, w, pl, n_pairs_out, n_pair_atoms_out))
                return -1;
            const size_t P = (size_t)pl.P, M = (size_t)pl.M;
            hipStream_t st = c->stream;
            if (d_side_offsets) HIP_TRY(c, hipMemcpyAsync(d_side_offsets, pl.side_off.data(), 8 * (2 * P + 1), hipMemcpyHostToDevice, st));
            if (P == 0) return 0;
            if (d_pair_struct) HIP_TRY(c, hipMemcpyAsync(d_pair_struct, pl.pair_struct.data(), 4 * P, hipMemcpyHostToDevice, st));
            if (d_pair_groups) HIP_TRY(c, hipMemcpyAsync(d_pair_groups, pl.pair_groups.data(), 8 * P, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(d_pair_areas, c->if_areas.p, 48 * P, hipMemcpyDeviceToDevice, st));
            if (d_pair_atom) HIP_TRY(c, hipMemcpyAsync(d_pair_atom, c->if_patom.p, 4 * M, hipMemcpyDeviceToDevice, st));
            if (d_pair_buried) HIP_TRY(c, hipMemcpyAsync(d_pair_buried, c->if_pburied.p, 8 * M, hipMemcpyDeviceToDevice, st));
            return 0;
        }();
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "stream synchronize failed"); /* (the call is synchronous) */
        return rc;
    });
}

extern "C" int freesasa_gpu_interface_residues_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                                   const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                                   const int64_t *res_first, int n_res, double probe_radius, int resolution,
                                                   double min_buried, double *d_sasa, double *d_iso, double *d_totals,
                                                   double *d_group_totals, long long pair_capacity, long long atom_capacity,
                                                   long long res_capacity, long long *n_pairs_out, long long *n_pair_atoms_out,
                                                   long long *n_res_rows_out, int32_t *d_pair_struct, int32_t *d_pair_groups,
                                                   double *d_pair_areas, int64_t *d_side_offsets, int32_t *d_pair_atom,
                                                   double *d_pair_buried, int64_t *d_res_offsets, int32_t *d_res_index,
                                                   int32_t *d_res_atoms, double *d_res_areas)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1;
    return guarded_ctx(c, [&]() -> int {
        char msg[200];
        c->err[0] = 0;
        IfaceResWant rw;
        rw.res_first = res_first; rw.n_res = n_res; rw.min_buried = min_buried; rw.res_capacity = res_capacity; rw.n_res_rows_out = n_res_rows_out;
        if (iface_bad_args(d_xyz, d_radii, offsets, n_structs, d_group, n_groups, alg, resolution, msg, sizeof msg) ||
            iface_bad_caps(pair_capacity, atom_capacity, msg, sizeof msg) || iface_res_bad_args(rw, offsets, n_structs, msg, sizeof msg))
            return ctx_fail(c, "%s", msg);
        if (iface_dev_checks(c, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, alg, resolution, pair_capacity, atom_capacity)) return -1;
        if (!d_sasa || !d_iso || !n_pairs_out || !n_pair_atoms_out || !d_pair_areas || !d_res_areas) return ctx_fail(c, "null argument");
        IfacePlan pl; /* (plan and table hold the sources of copies enqueued below: they live until the stream is idle) */
        IfaceResTable t;
        IfaceWant w, none; /* (the pipeline holds no capacity against its counts here: the three are held together, once R is known) */
        w.pair_capacity = pair_capacity; w.atom_capacity = atom_capacity; w.rows = true; w.atoms = d_pair_atom || d_pair_buried;
        int rc = [&]() -> int {
            if (iface_pipeline(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe_radius, resolution, d_sasa, d_iso,
                               d_totals, d_group_totals, none, pl, n_pairs_out, n_pair_atoms_out) ||
                iface_residues(c, pl, rw, d_iso, t))
                return -1;
            *n_res_rows_out = t.R;
            if (iface_res_check_caps(c, pl, w, rw, t.R)) return -1;
            const size_t P = (size_t)pl.P, M = (size_t)pl.M, R = (size_t)t.R;
            hipStream_t st = c->stream;
            if (d_side_offsets) HIP_TRY(c, hipMemcpyAsync(d_side_offsets, pl.side_off.data(), 8 * (2 * P + 1), hipMemcpyHostToDevice, st));
            if (P == 0) {
                if (d_res_offsets) HIP_TRY(c, hipMemsetAsync(d_res_offsets, 0, 8, st));
                return 0;
            }
            if (d_pair_struct) HIP_TRY(c, hipMemcpyAsync(d_pair_struct, pl.pair_struct.data(), 4 * P, hipMemcpyHostToDevice, st));
            if (d_pair_groups) HIP_TRY(c, hipMemcpyAsync(d_pair_groups, pl.pair_groups.data(), 8 * P, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(d_pair_areas, c->if_areas.p, 48 * P, hipMemcpyDeviceToDevice, st));
            if (d_pair_atom) HIP_TRY(c, hipMemcpyAsync(d_pair_atom, c->if_patom.p, 4 * M, hipMemcpyDeviceToDevice, st));
            if (d_pair_buried) HIP_TRY(c, hipMemcpyAsync(d_pair_buried, c->if_pburied.p, 8 * M, hipMemcpyDeviceToDevice, st));
            if (d_res_offsets) HIP_TRY(c, hipMemcpyAsync(d_res_offsets, t.off, 8 * (2 * P + 1), hipMemcpyDeviceToDevice, st));
            if (R == 0) return 0;
            if (d_res_index) HIP_TRY(c, hipMemcpyAsync(d_res_index, t.index, 4 * R, hipMemcpyDeviceToDevice, st));
            if (d_res_atoms) HIP_TRY(c, hipMemcpyAsync(d_res_atoms, t.atoms, 4 * R, hipMemcpyDeviceToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(d_res_areas, t.areas, 24 * R, hipMemcpyDeviceToDevice, st));
            return 0;
        }();
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "stream synchronize failed"); /* (the call is synchronous) */
        return rc;
    });
}

/* the contact entry, and - with qw - the residue-residue contact entry: the same call with one more stage and five more arrays */
struct IfaceResContactOut { /* the residue-residue contact entries' arrays, on the device or on the host: area is required */
    int64_t *off = nullptr;
    int32_t *res = nullptr, *cnt = nullptr, *rev = nullptr;
    double *area = nullptr;
};
static int iface_contacts_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                              const int32_t *d_group, const int32_t *n_groups, double probe_radius, int resolution, double *d_sasa,
                              double *d_iso, double *d_totals, double *d_group_totals, long long pair_capacity, long long atom_capacity,
                              long long contact_capacity, long long dot_capacity, long long *n_pairs_out, long long *n_pair_atoms_out,
                              long long *n_contacts_out, long long *n_buried_dots_out, int32_t *d_pair_struct, int32_t *d_pair_groups,
                              double *d_pair_areas, int64_t *d_side_offsets, int32_t *d_pair_atom, double *d_pair_buried,
                              int64_t *d_contact_first, int32_t *d_contact_partner, int32_t *d_contact_points, double *d_contact_area,
                              uint32_t *d_buried_masks, int32_t *d_dot_partner, const IfaceResContactWant *qw, const IfaceResContactOut &qd)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1;
    return guarded_ctx(c, [&]() -> int {
        char msg[200];
        c->err[0] = 0;
        IfaceContactWant cw;
        cw.contact_capacity = contact_capacity; cw.dot_capacity = dot_capacity; cw.n_contacts_out = n_contacts_out; cw.n_buried_dots_out = n_buried_dots_out;
        cw.rows = d_contact_partner || d_contact_points || d_contact_area; cw.dots = d_dot_partner != nullptr;
        if (iface_bad_args(d_xyz, d_radii, offsets, n_structs, d_group, n_groups, alg, resolution, msg, sizeof msg) ||
            iface_bad_caps(pair_capacity, atom_capacity, msg, sizeof msg) || iface_contact_bad_args(cw, alg, resolution, d_buried_masks, msg, sizeof msg) ||
            (qw && iface_rescontact_bad_args(*qw, offsets, n_structs, msg, sizeof msg)))
            return ctx_fail(c, "%s", msg);
        if (iface_dev_checks(c, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, alg, resolution, pair_capacity, atom_capacity)) return -1;
        if (!d_sasa || !d_iso || !n_pairs_out || !n_pair_atoms_out || !d_pair_areas || (qw && !qd.area)) return ctx_fail(c, "null argument");
        IfacePlan pl; /* (the plan holds the sources of copies enqueued below: it lives until the stream is idle) */
        IfaceContactTable t;
        IfaceResContactTable qt;
        IfaceWant w, none; /* (the pipeline holds no capacity against its counts here: the four are held together, once C and D_b are known) */
        w.pair_capacity = pair_capacity; w.atom_capacity = atom_capacity; w.rows = true;
        w.atoms = d_pair_atom || d_pair_buried || d_contact_first || d_buried_masks;
        int rc = [&]() -> int {
            if (iface_pipeline(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe_radius, resolution, d_sasa, d_iso,
                               d_totals, d_group_totals, none, pl, n_pairs_out, n_pair_atoms_out) ||
                iface_contacts(c, pl, probe_radius, resolution, t))
                return -1;
            *n_contacts_out = t.C;
            if (n_buried_dots_out) *n_buried_dots_out = t.D;
            if (qw) {
                if (iface_rescontacts(c, pl, *qw, t, qt)) return -1;
                *qw->n_rescontacts_out = qt.Q;
            }
            if (qw ? iface_rescontact_check_caps(c, pl, w, cw, t, *qw, qt.Q) : iface_contact_check_caps(c, pl, w, cw, t)) return -1;
            const size_t P = (size_t)pl.P, M = (size_t)pl.M, Cn = (size_t)t.C, D = (size_t)t.D, Q = (size_t)qt.Q;
            hipStream_t st = c->stream;
            /* rescontact_offsets: zeros without a pair ([1]) or without a folded row ([2 P + 1]) */
            if (qd.off && Q == 0) HIP_TRY(c, hipMemsetAsync(qd.off, 0, 8 * (P == 0 ? 1 : 2 * P + 1), st));
            if (Q > 0) {
                if (qd.off) HIP_TRY(c, hipMemcpyAsync(qd.off, qt.off, 8 * (2 * P + 1), hipMemcpyDeviceToDevice, st));
                if (qd.res) HIP_TRY(c, hipMemcpyAsync(qd.res, qt.res, 8 * Q, hipMemcpyDeviceToDevice, st));
                if (qd.cnt) HIP_TRY(c, hipMemcpyAsync(qd.cnt, qt.cnt, 8 * Q, hipMemcpyDeviceToDevice, st));
                if (qd.rev) HIP_TRY(c, hipMemcpyAsync(qd.rev, qt.rev, 4 * Q, hipMemcpyDeviceToDevice, st));
                HIP_TRY(c, hipMemcpyAsync(qd.area, qt.area, 8 * Q, hipMemcpyDeviceToDevice, st));
            }
            if (d_side_offsets) HIP_TRY(c, hipMemcpyAsync(d_side_offsets, pl.side_off.data(), 8 * (2 * P + 1), hipMemcpyHostToDevice, st));
            if (P == 0) {
                if (d_contact_first) HIP_TRY(c, hipMemsetAsync(d_contact_first, 0, 8, st));
                return 0;
            }
            if (d_pair_struct) HIP_TRY(c, hipMemcpyAsync(d_pair_struct, pl.pair_struct.data(), 4 * P, hipMemcpyHostToDevice, st));
            if (d_pair_groups) HIP_TRY(c, hipMemcpyAsync(d_pair_groups, pl.pair_groups.data(), 8 * P, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(d_pair_areas, c->if_areas.p, 48 * P, hipMemcpyDeviceToDevice, st));
            if (d_pair_atom) HIP_TRY(c, hipMemcpyAsync(d_pair_atom, c->if_patom.p, 4 * M, hipMemcpyDeviceToDevice, st));
            if (d_pair_buried) HIP_TRY(c, hipMemcpyAsync(d_pair_buried, c->if_pburied.p, 8 * M, hipMemcpyDeviceToDevice, st));
            if (d_buried_masks) HIP_TRY(c, hipMemcpyAsync(d_buried_masks, t.buried, 4 * SR_CAP_WORDS * M, hipMemcpyDeviceToDevice, st));
            if (D == 0) {
                if (d_contact_first) HIP_TRY(c, hipMemsetAsync(d_contact_first, 0, 8 * (M + 1), st));
                return 0;
            }
            if (d_contact_first) HIP_TRY(c, hipMemcpyAsync(d_contact_first, t.first, 8 * (M + 1), hipMemcpyDeviceToDevice, st));
            if (d_contact_partner) HIP_TRY(c, hipMemcpyAsync(d_contact_partner, t.partner, 4 * Cn, hipMemcpyDeviceToDevice, st));
            if (d_contact_points) HIP_TRY(c, hipMemcpyAsync(d_contact_points, t.points, 4 * Cn, hipMemcpyDeviceToDevice, st));
            if (d_contact_area) HIP_TRY(c, hipMemcpyAsync(d_contact_area, t.area, 8 * Cn, hipMemcpyDeviceToDevice, st));
            if (d_dot_partner) HIP_TRY(c, hipMemcpyAsync(d_dot_partner, t.dot_partner, 4 * D, hipMemcpyDeviceToDevice, st));
            return 0;
        }();
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "stream synchronize failed"); /* (the call is synchronous) */
        return rc;
    });
}

extern "C" int freesasa_gpu_interface_contacts_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                                   const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                                   double probe_radius, int resolution, double *d_sasa, double *d_iso, double *d_totals,
                                                   double *d_group_totals, long long pair_capacity, long long atom_capacity,
                                                   long long contact_capacity, long long dot_capacity, long long *n_pairs_out,
                                                   long long *n_pair_atoms_out, long long *n_contacts_out, long long *n_buried_dots_out,
                                                   int32_t *d_pair_struct, int32_t *d_pair_groups, double *d_pair_areas,
                                                   int64_t *d_side_offsets, int32_t *d_pair_atom, double *d_pair_buried,
                                                   int64_t *d_contact_first, int32_t *d_contact_partner, int32_t *d_contact_points,
                                                   double *d_contact_area, uint32_t *d_buried_masks, int32_t *d_dot_partner)
{
    return iface_contacts_dev(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe_radius, resolution, d_sasa, d_iso, d_totals,
                              d_group_totals, pair_capacity, atom_capacity, contact_capacity, dot_capacity, n_pairs_out, n_pair_atoms_out,
                              n_contacts_out, n_buried_dots_out, d_pair_struct, d_pair_groups, d_pair_areas, d_side_offsets, d_pair_atom,
                              d_pair_buried, d_contact_first, d_contact_partner, d_contact_points, d_contact_area, d_buried_masks,
                              d_dot_partner, nullptr, IfaceResContactOut());
}

extern "C" int freesasa_gpu_interface_residue_contacts_dev(
    freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs, const int32_t *d_group,
    const int32_t *n_groups, double probe_radius, int resolution, double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
    long long pair_capacity, long long atom_capacity, long long contact_capacity, long long dot_capacity, long long *n_pairs_out,
    long long *n_pair_atoms_out, long long *n_contacts_out, long long *n_buried_dots_out, int32_t *d_pair_struct, int32_t *d_pair_groups,
    double *d_pair_areas, int64_t *d_side_offsets, int32_t *d_pair_atom, double *d_pair_buried, int64_t *d_contact_first,
    int32_t *d_contact_partner, int32_t *d_contact_points, double *d_contact_area, uint32_t *d_buried_masks, int32_t *d_dot_partner,
    const int64_t *res_first, int n_res, long long rescontact_capacity, long long *n_rescontacts_out, int64_t *d_rescontact_offsets,
    int32_t *d_rescontact_residues, int32_t *d_rescontact_counts, double *d_rescontact_area, int32_t *d_rescontact_reverse)
{
    IfaceResContactWant qw;
    qw.res_first = res_first; qw.n_res = n_res; qw.rescontact_capacity = rescontact_capacity; qw.n_rescontacts_out = n_rescontacts_out;
    IfaceResContactOut qd;
    qd.off = d_rescontact_offsets; qd.res = d_rescontact_residues; qd.cnt = d_rescontact_counts; qd.area = d_rescontact_area; qd.rev = d_rescontact_reverse;
    return iface_contacts_dev(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe_radius, resolution, d_sasa, d_iso, d_totals,
                              d_group_totals, pair_capacity, atom_capacity, contact_capacity, dot_capacity, n_pairs_out, n_pair_atoms_out,
                              n_contacts_out, n_buried_dots_out, d_pair_struct, d_pair_groups, d_pair_areas, d_side_offsets, d_pair_atom,
                              d_pair_buried, d_contact_first, d_contact_partner, d_contact_points, d_contact_area, d_buried_masks,
                              d_dot_partner, &qw, qd);
}

/* the host-pointer entries: the batch as one chunk of the host-batch path, in place, as freesasa_gpu_calc_groups has it */
struct IfaceContactHost { /* the contact entry's host arrays: any may be null */
    int64_t *first = nullptr;
    int32_t *partner = nullptr, *points = nullptr, *dot_partner = nullptr;
    double *area = nullptr;
    uint32_t *buried = nullptr;
};
static int iface_host(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, const int32_t *group,
                      const int32_t *n_groups, int alg, double probe, int resolution, double *sasa_out, double *iso_out, double *totals_out,
                      double *group_totals_out, bool whole, long long pair_capacity, long long atom_capacity, long long *n_pairs_out,
                      long long *n_pair_atoms_out, int32_t *pair_struct_out, int32_t *pair_groups_out, double *pair_areas_out,
                      int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out, long long *stats_out, int device,
                      char *err_out, int err_len, const IfaceResWant *rw = nullptr, int64_t *res_offsets_out = nullptr,
                      int32_t *res_index_out = nullptr, int32_t *res_atoms_out = nullptr, double *res_areas_out = nullptr,
                      const IfaceContactWant *cw = nullptr, const IfaceContactHost *co = nullptr, const IfaceResContactWant *qw = nullptr,
                      const IfaceResContactOut *qo = nullptr)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    char msg[200];
    if (iface_bad_args(xyz, radii, offsets, n_structs, group, n_groups, alg, resolution, msg, sizeof msg) ||
        iface_bad_caps(pair_capacity, atom_capacity, msg, sizeof msg) || (rw && iface_res_bad_args(*rw, offsets, n_structs, msg, sizeof msg)) ||
        (cw && iface_contact_bad_args(*cw, alg, resolution, nullptr, msg, sizeof msg)) ||
        (qw && iface_rescontact_bad_args(*qw, offsets, n_structs, msg, sizeof msg)))
        return set_err(err_out, err_len, msg);
    if (!n_pairs_out || !n_pair_atoms_out || (whole && !pair_areas_out) || (rw && !res_areas_out) || (qw && !(qo && qo->area)))
        return set_err(err_out, err_len, "null argument");
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    IfacePlan pl; /* (declared before the lease: freed after its stream is idle) */
    IfaceResTable t;
    IfaceContactTable ct;
    IfaceResContactTable qt;
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    const size_t n = (size_t)offsets[n_structs];
    int64_t G = 0; /* (bad counts are refused by the chain-group pipeline, with its message: staged for none here) */
    for (int s = 0; s < n_structs; ++s) G += n_groups[s] > 0 && n_groups[s] <= 65535 ? n_groups[s] : 0;
    BatchCall b;
    b.fallback = "GPU interface batch failed";
    Chunk h;
    h.ns = n_structs; h.n = n; h.off = offsets; h.xyz = xyz; h.radii = radii;
    const int rc = [&]() -> int {
        c->err[0] = 0;
        if (chunk_size(b, c, h) || ensure(c, c->h_group, 4 * n) || ensure(c, c->h_iso, 8 * n) || ensure(c, c->h_gtot, 24 * (size_t)G + 8)) return -1;
        if (chunk_upload(c, h)) return -1;
        hipStream_t st = c->stream;
        if (hipMemcpyAsync(c->h_group.p, group, 4 * n, hipMemcpyHostToDevice, st) != hipSuccess) return ctx_fail(c, "host-to-device copy failed");
        const double *d_xyz = (const double *)c->h_xyz.p, *d_radii = (const double *)c->h_radii.p;
        const int32_t *d_group = (const int32_t *)c->h_group.p;
        double *d_sasa = (double *)c->h_sasa.p, *d_iso = (double *)c->h_iso.p;
        double *d_tot = totals_out ? (double *)c->h_totals.p : nullptr, *d_gtot = group_totals_out ? (double *)c->h_gtot.p : nullptr;
        if (offsets[n_structs] > (int64_t)1 << 30) return ctx_fail(c, "batch too large (max 2^30 atoms per call)");
        IfaceWant w;
        w.pair_capacity = pair_capacity; w.atom_capacity = atom_capacity;
        if (whole) {
            w.rows = true; w.atoms = pair_atom_out || pair_buried_out || (co && (co->first || co->buried));
            /* (with residues or contacts the pipeline holds no capacity itself: all are held together, once R or C and D_b are known) */
            if (iface_pipeline(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe, resolution, d_sasa, d_iso, d_tot, d_gtot,
                               rw || cw ? IfaceWant() : w, pl, n_pairs_out, n_pair_atoms_out))
                return -1;
            if (cw) {
                if (iface_contacts(c, pl, probe, resolution, ct)) return -1;
                *cw->n_contacts_out = ct.C;
                if (cw->n_buried_dots_out) *cw->n_buried_dots_out = ct.D;
                if (qw) {
                    if (iface_rescontacts(c, pl, *qw, ct, qt)) return -1;
                    *qw->n_rescontacts_out = qt.Q;
                }
                if (qw ? iface_rescontact_check_caps(c, pl, w, *cw, ct, *qw, qt.Q) : iface_contact_check_caps(c, pl, w, *cw, ct)) return -1;
            }
            if (rw) {
                if (iface_residues(c, pl, *rw, d_iso, t)) return -1;
                *rw->n_res_rows_out = t.R;
                if (iface_res_check_caps(c, pl, w, *rw, t.R)) return -1;
            }
        } else {
            IfaceArgs ia;
            w.rows = pair_struct_out || pair_groups_out;
            if (iface_screen(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe, resolution, d_sasa, d_iso, d_tot, d_gtot, pl, ia))
                return -1;
            *n_pairs_out = pl.P; *n_pair_atoms_out = pl.M;
            if (iface_check_caps(c, pl, w)) return -1;
        }
        const size_t P = (size_t)pl.P, M = (size_t)pl.M, R = (size_t)t.R;
        if (rw && res_offsets_out && P == 0) res_offsets_out[0] = 0;
        if (rw && P > 0 &&
            ((res_offsets_out && hipMemcpyAsync(res_offsets_out, t.off, 8 * (2 * P + 1), hipMemcpyDeviceToHost, st) != hipSuccess) ||
             (R > 0 && res_index_out && hipMemcpyAsync(res_index_out, t.index, 4 * R, hipMemcpyDeviceToHost, st) != hipSuccess) ||
             (R > 0 && res_atoms_out && hipMemcpyAsync(res_atoms_out, t.atoms, 4 * R, hipMemcpyDeviceToHost, st) != hipSuccess) ||
             (R > 0 && hipMemcpyAsync(res_areas_out, t.areas, 24 * R, hipMemcpyDeviceToHost, st) != hipSuccess)))
            return ctx_fail(c, "device-to-host copy failed");
        if (cw && co) {
            const size_t Cn = (size_t)ct.C, D = (size_t)ct.D;
            if (co->first && (P == 0 || D == 0)) memset(co->first, 0, 8 * (P == 0 ? 1 : M + 1));
            if (P > 0 &&
                ((co->buried && hipMemcpyAsync(co->buried, ct.buried, 4 * SR_CAP_WORDS * M, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (D > 0 && co->first && hipMemcpyAsync(co->first, ct.first, 8 * (M + 1), hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (Cn > 0 && co->partner && hipMemcpyAsync(co->partner, ct.partner, 4 * Cn, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (Cn > 0 && co->points && hipMemcpyAsync(co->points, ct.points, 4 * Cn, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (Cn > 0 && co->area && hipMemcpyAsync(co->area, ct.area, 8 * Cn, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (D > 0 && co->dot_partner && hipMemcpyAsync(co->dot_partner, ct.dot_partner, 4 * D, hipMemcpyDeviceToHost, st) != hipSuccess)))
                return ctx_fail(c, "device-to-host copy failed");
        }
        if (qw) {
            const size_t Q = (size_t)qt.Q;
            if (qo->off && Q == 0) memset(qo->off, 0, 8 * (P == 0 ? 1 : 2 * P + 1));
            if (Q > 0 &&
                ((qo->off && hipMemcpyAsync(qo->off, qt.off, 8 * (2 * P + 1), hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (qo->res && hipMemcpyAsync(qo->res, qt.res, 8 * Q, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (qo->cnt && hipMemcpyAsync(qo->cnt, qt.cnt, 8 * Q, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 (qo->rev && hipMemcpyAsync(qo->rev, qt.rev, 4 * Q, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                 hipMemcpyAsync(qo->area, qt.area, 8 * Q, hipMemcpyDeviceToHost, st) != hipSuccess))
                return ctx_fail(c, "device-to-host copy failed");
        }
        if ((sasa_out && hipMemcpyAsync(sasa_out, d_sasa, 8 * n, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (iso_out && hipMemcpyAsync(iso_out, d_iso, 8 * n, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (totals_out && hipMemcpyAsync(totals_out, d_tot, 8 * (size_t)n_structs, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (group_totals_out && G > 0 && hipMemcpyAsync(group_totals_out, d_gtot, 24 * (size_t)G, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (whole && P > 0 && hipMemcpyAsync(pair_areas_out, c->if_areas.p, 48 * P, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (whole && P > 0 && pair_atom_out && hipMemcpyAsync(pair_atom_out, c->if_patom.p, 4 * M, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (whole && P > 0 && pair_buried_out && hipMemcpyAsync(pair_buried_out, c->if_pburied.p, 8 * M, hipMemcpyDeviceToHost, st) != hipSuccess))
            return ctx_fail(c, "device-to-host copy failed");
        if (hipStreamSynchronize(st) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        iface_rows_to_host(pl, pair_struct_out, pair_groups_out, stats_out);
        if (side_offsets_out) memcpy(side_offsets_out, pl.side_off.data(), 8 * (2 * P + 1));
        return 0;
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}

extern "C" int freesasa_gpu_calc_interface_pairs(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                 const int32_t *group, const int32_t *n_groups, int alg, double probe_radius,
                                                 int resolution, long long pair_capacity, long long *n_pairs_out,
                                                 long long *n_pair_atoms_out, int32_t *pair_struct_out, int32_t *pair_groups_out,
                                                 long long *stats_out, int device, char *err_out, int err_len)
{
    return iface_host(xyz, radii, offsets, n_structs, group, n_groups, alg, probe_radius, resolution, nullptr, nullptr, nullptr, nullptr,
                      false, pair_capacity, 0, n_pairs_out, n_pair_atoms_out, pair_struct_out, pair_groups_out, nullptr, nullptr, nullptr,
                      nullptr, stats_out, device, err_out, err_len);
}

extern "C" int freesasa_gpu_calc_interfaces(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                            const int32_t *group, const int32_t *n_groups, int alg, double probe_radius, int resolution,
                                            double *sasa_out, double *iso_out, double *totals_out, double *group_totals_out,
                                            long long pair_capacity, long long atom_capacity, long long *n_pairs_out,
                                            long long *n_pair_atoms_out, int32_t *pair_struct_out, int32_t *pair_groups_out,
                                            double *pair_areas_out, int64_t *side_offsets_out, int32_t *pair_atom_out,
                                            double *pair_buried_out, int device, char *err_out, int err_len)
{
    return iface_host(xyz, radii, offsets, n_structs, group, n_groups, alg, probe_radius, resolution, sasa_out, iso_out, totals_out,
                      group_totals_out, true, pair_capacity, atom_capacity, n_pairs_out, n_pair_atoms_out, pair_struct_out, pair_groups_out,
                      pair_areas_out, side_offsets_out, pair_atom_out, pair_buried_out, nullptr, device, err_out, err_len);
}

extern "C" int freesasa_gpu_calc_interface_residues(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                    const int32_t *group, const int32_t *n_groups, const int64_t *res_first, int n_res,
                                                    int alg, double probe_radius, int resolution, double min_buried, double *sasa_out,
                                                    double *iso_out, double *totals_out, double *group_totals_out,
                                                    long long pair_capacity, long long atom_capacity, long long res_capacity,
                                                    long long *n_pairs_out, long long *n_pair_atoms_out, long long *n_res_rows_out,
                                                    int32_t *pair_struct_out, int32_t *pair_groups_out, double *pair_areas_out,
                                                    int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out,
                                                    int64_t *res_offsets_out, int32_t *res_index_out, int32_t *res_atoms_out,
                                                    double *res_areas_out, int device, char *err_out, int err_len)
{
    IfaceResWant rw;
    rw.res_first = res_first; rw.n_res = n_res; rw.min_buried = min_buried; rw.res_capacity = res_capacity; rw.n_res_rows_out = n_res_rows_out;
    return iface_host(xyz, radii, offsets, n_structs, group, n_groups, alg, probe_radius, resolution, sasa_out, iso_out, totals_out,
                      group_totals_out, true, pair_capacity, atom_capacity, n_pairs_out, n_pair_atoms_out, pair_struct_out, pair_groups_out,
                      pair_areas_out, side_offsets_out, pair_atom_out, pair_buried_out, nullptr, device, err_out, err_len, &rw,
                      res_offsets_out, res_index_out, res_atoms_out, res_areas_out);
}

extern "C" int freesasa_gpu_calc_interface_contacts(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                    const int32_t *group, const int32_t *n_groups, int alg, double probe_radius,
                                                    int resolution, double *sasa_out, double *iso_out, double *totals_out,
                                                    double *group_totals_out, long long pair_capacity, long long atom_capacity,
                                                    long long contact_capacity, long long dot_capacity, long long *n_pairs_out,
                                                    long long *n_pair_atoms_out, long long *n_contacts_out, long long *n_buried_dots_out,
                                                    int32_t *pair_struct_out, int32_t *pair_groups_out, double *pair_areas_out,
                                                    int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out,
                                                    int64_t *contact_first_out, int32_t *contact_partner_out, int32_t *contact_points_out,
                                                    double *contact_area_out, uint32_t *buried_masks_out, int32_t *dot_partner_out,
                                                    int device, char *err_out, int err_len)
{
    IfaceContactWant cw;
    cw.contact_capacity = contact_capacity; cw.dot_capacity = dot_capacity; cw.n_contacts_out = n_contacts_out; cw.n_buried_dots_out = n_buried_dots_out;
    cw.rows = contact_partner_out || contact_points_out || contact_area_out; cw.dots = dot_partner_out != nullptr;
    IfaceContactHost co;
    co.first = contact_first_out; co.partner = contact_partner_out; co.points = contact_points_out; co.area = contact_area_out;
    co.buried = buried_masks_out; co.dot_partner = dot_partner_out;
    return iface_host(xyz, radii, offsets, n_structs, group, n_groups, alg, probe_radius, resolution, sasa_out, iso_out, totals_out,
                      group_totals_out, true, pair_capacity, atom_capacity, n_pairs_out, n_pair_atoms_out, pair_struct_out, pair_groups_out,
                      pair_areas_out, side_offsets_out, pair_atom_out, pair_buried_out, nullptr, device, err_out, err_len, nullptr, nullptr,
                      nullptr, nullptr, nullptr, &cw, &co);
}

extern "C" int freesasa_gpu_calc_interface_residue_contacts(
    const double *xyz, const double *radii, const int64_t *offsets, int n_structs, const int32_t *group, const int32_t *n_groups, int alg,
    double probe_radius, int resolution, double *sasa_out, double *iso_out, double *totals_out, double *group_totals_out,
    long long pair_capacity, long long atom_capacity, long long contact_capacity, long long dot_capacity, long long *n_pairs_out,
    long long *n_pair_atoms_out, long long *n_contacts_out, long long *n_buried_dots_out, int32_t *pair_struct_out, int32_t *pair_groups_out,
    double *pair_areas_out, int64_t *side_offsets_out, int32_t *pair_atom_out, double *pair_buried_out, int64_t *contact_first_out,
    int32_t *contact_partner_out, int32_t *contact_points_out, double *contact_area_out, uint32_t *buried_masks_out, int32_t *dot_partner_out,
    const int64_t *res_first, int n_res, long long rescontact_capacity, long long *n_rescontacts_out, int64_t *rescontact_offsets_out,
    int32_t *rescontact_residues_out, int32_t *rescontact_counts_out, double *rescontact_area_out, int32_t *rescontact_reverse_out, int device,
    char *err_out, int err_len)
{
    IfaceContactWant cw;
    cw.contact_capacity = contact_capacity; cw.dot_capacity = dot_capacity; cw.n_contacts_out = n_contacts_out; cw.n_buried_dots_out = n_buried_dots_out;
    cw.rows = contact_partner_out || contact_points_out || contact_area_out; cw.dots = dot_partner_out != nullptr;
    IfaceContactHost co;
    co.first = contact_first_out; co.partner = contact_partner_out; co.points = contact_points_out; co.area = contact_area_out;
    co.buried = buried_masks_out; co.dot_partner = dot_partner_out;
    IfaceResContactWant qw;
    qw.res_first = res_first; qw.n_res = n_res; qw.rescontact_capacity = rescontact_capacity; qw.n_rescontacts_out = n_rescontacts_out;
    IfaceResContactOut qo;
    qo.off = rescontact_offsets_out; qo.res = rescontact_residues_out; qo.cnt = rescontact_counts_out; qo.area = rescontact_area_out;
    qo.rev = rescontact_reverse_out;
    return iface_host(xyz, radii, offsets, n_structs, group, n_groups, alg, probe_radius, resolution, sasa_out, iso_out, totals_out,
                      group_totals_out, true, pair_capacity, atom_capacity, n_pairs_out, n_pair_atoms_out, pair_struct_out, pair_groups_out,
                      pair_areas_out, side_offsets_out, pair_atom_out, pair_buried_out, nullptr, device, err_out, err_len, nullptr, nullptr,
                      nullptr, nullptr, nullptr, &cw, &co, &qw, &qo);
}
