/*
 * gpu_interfaces.hip — pairwise interface areas between chain groups (include/freesasa_gpu.h: freesasa_gpu_interface_pairs_dev,
 * freesasa_gpu_interfaces_dev, freesasa_gpu_calc_interface_pairs, freesasa_gpu_calc_interfaces), their per-residue tables
 * (freesasa_gpu_interface_residues_dev, freesasa_gpu_calc_interface_residues), atom-atom contact tables
 * (freesasa_gpu_interface_contacts_dev, freesasa_gpu_calc_interface_contacts) and residue-residue contact tables
 * (freesasa_gpu_interface_residue_contacts_dev, freesasa_gpu_calc_interface_residue_contacts).  Host code; the kernels are in
 * gpu_kernels.hip (phase functions: iface_kernels.h, contact_kernels.h, rescontact_kernels.h).
 *
 * The ten entries are ONE path (and the file sweep's interfaces, gpu_sweep.hip, go through its iface_run and iface_deliver).  An IfaceCall is what an entry was called with, filled by field name; an IfaceRun what the call
 * produced and what has to outlive the stream's work.  iface_dev (arrays on the context's stream) and iface_host (host arrays: the
 * grouped host batch of gpu_groups.hip, in place) both go through
 *   iface_bad_call    every refusal before a device is touched, in one order
 *   iface_run         the stages below, each count output set as soon as the count is known, the capacities held once
 *   iface_deliver     the one table of outputs (iface_outputs), walked for device and for host destinations
 *
 * The stages of iface_run:
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
 *   9. residues          (the residue entries) k_iface_res_head, the block scan, k_iface_res_first, k_iface_res_segment, the scan
 *                        again, k_iface_res_rows; R comes back (one more stream synchronization); the table stays in c->if_rtable
 *  10. contacts          (the contact entries; Shrake-Rupley only) two more engine runs over the M pair-structure atoms with the
 *                        mask request (masks_resident: as the P pair structures, as the 2 P sides), k_contact_masks, the dots' scan -
 *                        D_b comes back (one stream synchronization) and sizes what follows - the dots' expansion,
 *                        k_contact_attribute, k_contact_rows_count / _rank, the block scan, k_contact_rows_write; C and the flag
 *                        come back (one more); the table stays in c->if_ctable, the masks in c->if_cmasks, the dots in c->if_cdots
 *  11. residue contacts  (the residue-residue contact entries, behind 10) the per-residue tables' k_iface_res_head, block scan and
 *                        k_iface_res_first (the segments), k_rc_fold_count, the block scan, k_rc_fold_write, k_rc_reverse; Q comes
 *                        back (one more stream synchronization); the table stays in c->if_rctable
 *
 * iface_screen is steps 1 to 5, iface_pairs steps 6 to 8; every stage leaves its results in the context's own buffers.  The
 * capacities are held against the counts in ONE place (iface_check_caps: P, M, R, C, D_b, Q in this order): behind the screen and
 * before steps 6 to 8 for the entries that end there or at step 8, behind the last stage - once all counts are known and set - for
 * the others; iface_deliver runs only behind it, so that a call that fails for a capacity has written none of the caller's pair,
 * atom, residue, contact or dot arrays.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <array>
#include <vector>

#include "engine_internal.h"

using namespace sasa;

namespace {

/* (IfaceCall - what an entry was called with - and IfaceRun - what the call produced - are in engine_internal.h: the file sweep
   goes through iface_run and iface_deliver too) */

/* ------------------------------------------------------------------ the refusals before a device is touched */

int iface_bad_batch(const IfaceCall &k, char *msg, size_t len)
{
    const char *bad = nullptr;
    if (!k.xyz || !k.radii || !k.offsets || !k.group || !k.n_groups) bad = "null argument";
    else if (k.alg != 0 && k.alg != 1) { snprintf(msg, len, "unknown algorithm %d", k.alg); return -1; }
    else if (k.n_structs <= 0) bad = "n_structs must be > 0";
    else if (k.resolution <= 0) bad = "resolution must be > 0";
    else if (k.offsets[0] != 0) bad = "offsets[0] must be 0";
    if (bad) { snprintf(msg, len, "%s", bad); return -1; }
    for (int s = 0; s < k.n_structs; ++s)
        if (k.offsets[s + 1] < k.offsets[s]) { snprintf(msg, len, "offsets must be non-decreasing"); return -1; }
    if (k.offsets[k.n_structs] <= 0) { snprintf(msg, len, "empty batch"); return -1; }
    int64_t T = 0;
    for (int s = 0; s < k.n_structs; ++s) {
        const int64_t ng = k.n_groups[s];
        if (ng > IF_MAX_GROUPS && ng <= GRP_MAX_PER_STRUCT) { /* (a count the chain-group entry refuses is left to it, with its message) */
            snprintf(msg, len, "structure %d has %lld groups: interfaces are made for up to %d groups of a structure", s, (long long)ng, IF_MAX_GROUPS);
            return -1;
        }
        if (ng >= 2 && ng <= IF_MAX_GROUPS) T += ng * (ng - 1) / 2;
        if (T > IF_MAX_TESTS) {
            snprintf(msg, len, "structures 0 .. %d have %lld pairs of groups to test: a call takes up to %d", s, (long long)T, IF_MAX_TESTS);
            return -1;
        }
    }
    if (k.pair_capacity < 0) { snprintf(msg, len, "pair_capacity must be >= 0 (it is %lld)", k.pair_capacity); return -1; }
    if (k.atom_capacity < 0) { snprintf(msg, len, "atom_capacity must be >= 0 (it is %lld)", k.atom_capacity); return -1; }
    return 0;
}
/* res_first, for the residue entries (with min_buried and their capacity) and for the residue-residue contact entries; n_rows_out:
   the entry's own count output */
int iface_bad_residues(const IfaceCall &k, const long long *n_rows_out, char *msg, size_t len)
{
    const int64_t *first = k.res_first, *offsets = k.offsets;
    if (!first || !n_rows_out) { snprintf(msg, len, "null argument"); return -1; }
    if (k.n_res <= 0) { snprintf(msg, len, "n_res must be > 0"); return -1; }
    if (k.residues) {
        if (!(k.min_buried >= 0.0) || k.min_buried > 1.7976931348623157e308) { snprintf(msg, len, "min_buried must be finite and >= 0"); return -1; }
        if (k.res_capacity < 0) { snprintf(msg, len, "res_capacity must be >= 0 (it is %lld)", k.res_capacity); return -1; }
    }
    if (first[0] != 0) { snprintf(msg, len, "res_first[0] must be 0"); return -1; }
    for (int r = 0; r < k.n_res; ++r)
        if (first[r + 1] < first[r]) { snprintf(msg, len, "res_first must be non-decreasing"); return -1; }
    if (first[k.n_res] != offsets[k.n_structs]) {
        snprintf(msg, len, "res_first[n_res] is %lld: the batch has %lld atoms", (long long)first[k.n_res], (long long)offsets[k.n_structs]);
        return -1;
    }
    int s = 0;
    for (int r = 0; r < k.n_res; ++r) {
        const int64_t b = first[r], e = first[r + 1];
        if (b == e) continue;
        while (offsets[s + 1] <= b) ++s; /* (b < offsets[n_structs]: the structure that holds the residue's first atom) */
        if (e > offsets[s + 1]) { snprintf(msg, len, "residue %d spans the boundary between structures %d and %d", r, s, s + 1); return -1; }
    }
    return 0;
}
int iface_bad_contacts(const IfaceCall &k, char *msg, size_t len)
{
    if (!k.n_contacts) { snprintf(msg, len, "null argument"); return -1; }
    if (k.alg != 1) { snprintf(msg, len, "the contact tables are made of Shrake-Rupley test points: Lee-Richards has none"); return -1; }
    if (k.resolution > SR_CAP_POINTS_MAX) {
        snprintf(msg, len, "the contact tables are offered up to %d test points (%d asked for)", SR_CAP_POINTS_MAX, k.resolution);
        return -1;
    }
    if (k.contact_capacity < 0) { snprintf(msg, len, "contact_capacity must be >= 0 (it is %lld)", k.contact_capacity); return -1; }
    if (k.dot_capacity < 0) { snprintf(msg, len, "dot_capacity must be >= 0 (it is %lld)", k.dot_capacity); return -1; }
    if (k.out_dev && (uintptr_t)k.buried_masks % 16) {
        snprintf(msg, len, "the buried mask array must be aligned to 16 bytes (an atom's four words are one store)");
        return -1;
    }
    return 0;
}
/* The one argument check of all entries - the batch and its two capacities, residues, contacts, residue contacts, in this order,
   each at most once - and the entry kind's own tail: ctx_device >= 0 is iface_dev's context (2^30 atoms, hipSetDevice, null
   outputs), < 0 iface_host (null outputs, the device count).  0, or -1 with the message in msg. */
int iface_bad_call(const IfaceCall &k, int ctx_device, char *msg, size_t len)
{
    if (iface_bad_batch(k, msg, len) || (k.residues && iface_bad_residues(k, k.n_res_rows, msg, len)) ||
        (k.contacts && iface_bad_contacts(k, msg, len)))
        return -1;
    if (k.rescontacts) {
        if (iface_bad_residues(k, k.n_rescontacts, msg, len)) return -1;
        if (k.rescontact_capacity < 0) { snprintf(msg, len, "rescontact_capacity must be >= 0 (it is %lld)", k.rescontact_capacity); return -1; }
    }
    const char *bad = nullptr;
    const bool null_out = !k.n_pairs || !k.n_pair_atoms || (k.whole && !k.pair_areas) || (k.residues && !k.res_areas) ||
                          (k.rescontacts && !k.rescontact_area) || (ctx_device >= 0 && k.whole && (!k.sasa || !k.iso));
    if (ctx_device >= 0) {
        if (k.offsets[k.n_structs] > (int64_t)1 << 30) bad = "batch too large (max 2^30 atoms per call)";
        else if (hipSetDevice(ctx_device) != hipSuccess) bad = "hipSetDevice failed";
        else if (null_out) bad = "null argument";
    } else {
        if (null_out) bad = "null argument";
        else if (freesasa_gpu_device_count() <= 0) bad = "no HIP device available: libfreesasa_amd has no CPU path";
    }
    if (bad) snprintf(msg, len, "%s", bad);
    return bad ? -1 : 0;
}

} /* namespace */

/* (engine_internal.h) the batch, the contact entries' algorithm and resolution, res_first - in the entries' order */
int iface_bad_rescontact_call(const IfaceCall &k, char *msg, size_t len)
{
    long long rows = 0, contacts = 0;
    IfaceCall d = k;
    d.n_contacts = &contacts; d.out_dev = false;
    d.pair_capacity = d.atom_capacity = d.contact_capacity = d.dot_capacity = 0;
    return iface_bad_batch(d, msg, len) || iface_bad_contacts(d, msg, len) || iface_bad_residues(d, &rows, msg, len) ? -1 : 0;
}

namespace {

/* ------------------------------------------------------------------ the stages */

/* steps 1 to 5; at its end the stream is idle (the flags are on the host) */
int iface_screen(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r)
{
    IfacePlan &pl = r.pl;
    IfaceArgs &ia = r.ia;
    const int n_structs = k.n_structs;
    if (k.alg == 1) pl.tp = call_test_points(k.alg, k.resolution);
    std::vector<int> cnt;
    if (groups_resident(c, k.alg, k.xyz, k.radii, k.offsets, n_structs, k.group, k.n_groups, k.probe, k.resolution,
                        k.alg == 1 ? pl.tp.data() : nullptr, k.sasa, k.iso, k.totals, k.group_totals, &cnt))
        return -1;
    const int G = (int)cnt.size();
    const int64_t n = k.offsets[n_structs];
    pl.G = G; pl.n = n;
    pl.meta.assign((size_t)G + 1 + (size_t)n_structs + 1, 0);
    int64_t *gstart = pl.meta.data(), *tbase = gstart + G + 1;
    gstart[0] = n;
    for (int g = 0; g < G; ++g) gstart[g + 1] = gstart[g] + cnt[(size_t)g];
    pl.n_iso = gstart[G] - n;
    const int32_t *sg = k.screen_groups ? k.screen_groups : k.n_groups; /* (a structure the screen passes over has no test) */
    int64_t T = 0;
    for (int s = 0; s < n_structs; ++s) {
        tbase[s] = T;
        const int64_t ng = sg[s];
        T += ng * (ng - 1) / 2;
    }
    tbase[n_structs] = T;
    pl.T = T;

    memset(&ia, 0, sizeof ia);
    ia.cxyz = (const double *)c->g_xyz.p; ia.cradii = (const double *)c->g_radii.p; ia.src = (const int *)c->g_src.p;
    ia.csasa = (const double *)c->g_sasa.p; ia.ctot = (const double *)c->g_tot.p;
    ia.n_atoms = (int)n; ia.n_structs = n_structs; ia.n_groups = G; ia.probe = k.probe;
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
        const int ng = sg[s];
        for (int g = 0; g + 1 < ng; ++g)
            for (int h = g + 1; h < ng; ++h, ++t) {
                if (!flag[(size_t)t]) continue;
                pl.pair_struct.push_back(s);
                pl.pair_groups.push_back(g); pl.pair_groups.push_back(h);
                for (int side = 0; side < 2; ++side) {
                    const int64_t q = k0 + (side ? h : g);
                    start.push_back(gstart[q]); grp.push_back((int32_t)q);
                    M += cnt[(size_t)q];
                    pl.side_off.push_back(M);
                }
            }
        k0 += k.n_groups[s];
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

/* steps 6 to 8 behind the screen: the rows in c->if_areas [6 P], the per-atom arrays in c->if_patom / c->if_pburied [M]; nothing
   is waited for at its end beyond what run_batch waits for */
int iface_pairs(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r)
{
    const IfacePlan &pl = r.pl;
    IfaceArgs &ia = r.ia;
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
    if (run_batch(c, k.alg == 0, ia.pxyz, ia.pradii, pl.pair_off.data(), (int)P, k.probe, k.resolution, k.alg == 1 ? pl.tp.data() : nullptr,
                  (double *)c->if_sasa.p, nullptr, nullptr))
        return -1;
    HIP_TRY(c, kl_segment_sums(ia.psasa, ia.side_off, (int)(2 * P), pl.M < (int64_t)64 * 2 * (int64_t)P, (double *)c->if_inpair.p, st));
    HIP_TRY(c, kl_iface_finish(ia, st));
    return 0;
}

/* res_first on the device (c->if_rfirst), from the run's own copy */
int iface_upload_res_first(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r)
{
    if (ensure(c, c->if_rfirst, 8 * ((size_t)k.n_res + 1))) return -1;
    r.res_first.assign(k.res_first, k.res_first + k.n_res + 1);
    HIP_TRY(c, hipMemcpyAsync(c->if_rfirst.p, r.res_first.data(), 8 * r.res_first.size(), hipMemcpyHostToDevice, c->stream));
    return 0;
}

/* step 9 behind iface_pairs (k_iface_finish is the last thing on the stream).  R comes back to the host (one stream
   synchronization), so at the stage's end the stream is idle. */
int iface_residues(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r)
{
    const IfacePlan &pl = r.pl;
    IfaceResTable &t = r.rt;
    if (pl.P == 0) return 0;
    const size_t P = (size_t)pl.P, M = (size_t)pl.M;
    const size_t S = (size_t)ifr_scan_scratch(pl.M);
    hipStream_t st = c->stream;
    if ((!k.res_first_dev && iface_upload_res_first(c, k, r)) || ensure(c, c->if_rwork, 4 * (6 * M + 3 + S) + 8) || ensure(c, c->if_rsegs, 24 * M) ||
        ensure(c, c->if_rtable, 8 * (2 * P + 1) + 24 * M + 8 * M))
        return -1;
    IfaceResArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = pl.M; a.n_sides = 2 * pl.P; a.n_res = k.n_res;
    a.side_off = (const int64_t *)c->if_sides.p; a.pair_atom = (const int *)c->if_patom.p;
    a.res_first = k.res_first_dev ? k.res_first_dev : (const int64_t *)c->if_rfirst.p; a.iso = k.iso; a.psasa = (const double *)c->if_sasa.p;
    a.min_buried = k.min_buried;
    int *w = (int *)c->if_rwork.p;
    a.atom_res = w; a.hs = w + M; a.seg_first = a.hs + M + 1; a.seg_res = a.seg_first + M + 1; a.seg_atoms = a.seg_res + M; a.ks = a.seg_atoms + M;
    int *scratch = a.ks + M + 1;
    a.seg_areas = (double *)c->if_rsegs.p;
    a.res_off = (int64_t *)c->if_rtable.p; a.res_areas = (double *)(a.res_off + 2 * P + 1);
    a.res_index = (int *)(a.res_areas + 3 * M); a.res_atoms = a.res_index + M;
    HIP_TRY(c, kl_iface_res_segments(a, scratch, st));
    HIP_TRY(c, kl_iface_res_rows(a, scratch, st));
    int R = 0;
    HIP_TRY(c, hipMemcpyAsync(&R, a.ks + M, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    t.R = R; t.off = a.res_off; t.areas = a.res_areas; t.index = a.res_index; t.atoms = a.res_atoms;
    return 0;
}

/* step 10 behind iface_pairs (Shrake-Rupley; k_iface_finish is the last thing on the stream).  D_b, then C and the flag come
   back to the host (two stream synchronizations), so at the stage's end the stream is idle.  Without a buried point there are
   the masks and nothing else. */
int iface_contacts(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r)
{
    const IfacePlan &pl = r.pl;
    IfaceContactTable &t = r.ct;
    const int n_points = k.resolution;
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
    if (masks_resident(c, pxyz, pradii, pl.pair_off.data(), (int)P, k.probe, n_points, pl.tp.data(), areas, nullptr, nullptr, pair_masks) ||
        masks_resident(c, pxyz, pradii, pl.side_off.data(), (int)(2 * P), k.probe, n_points, pl.tp.data(), areas, nullptr, nullptr, side_masks))
        return -1;
    ContactArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = pl.M; a.n_sides = 2 * pl.P; a.n_points = n_points; a.probe = k.probe;
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
    if (dots_expand_resident(c, pxyz, pradii, pl.M, k.probe, n_points, buried, dot_first, D, dot_xyz, dot_atom, dot_point)) return -1;
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

/* step 11 behind iface_contacts (the stream is idle, C is on the host): the segments of the per-residue tables by their own
   kernels, the fold of the contact rows per partner segment, the reverse rows.  Q comes back to the host (one stream
   synchronization), so at the stage's end the stream is idle.  Without a contact row nothing is launched: Q = 0; without a
   folded row there is no table. */
int iface_rescontacts(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r)
{
    const IfacePlan &pl = r.pl;
    const IfaceContactTable &ct = r.ct;
    IfaceResContactTable &t = r.qt;
    if (pl.P == 0 || ct.C == 0) return 0;
    const size_t P = (size_t)pl.P, M = (size_t)pl.M, Cn = (size_t)ct.C;
    const size_t S = (size_t)ifr_scan_scratch(pl.M);
    hipStream_t st = c->stream;
    if (iface_upload_res_first(c, k, r) || ensure(c, c->if_rcwork, 4 * (4 * M + 3 + S + Cn)) ||
        ensure(c, c->if_rctable, 8 * (2 * P + 1) + 8 * Cn + 4 * 5 * Cn))
        return -1;
    int *w = (int *)c->if_rcwork.p;
    IfaceResArgs s;
    memset(&s, 0, sizeof s);
    s.n_pair_atoms = pl.M; s.n_sides = 2 * pl.P; s.n_res = k.n_res;
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
    HIP_TRY(c, hipMemsetAsync(a.fc, 0, 4 * (M + 1), st)); /* (the segments' counts: a slot at or beyond K has none) */
    HIP_TRY(c, kl_rc_segments(s, scratch, st));
    HIP_TRY(c, kl_rc_fold(a, scratch, st));
    int Q = 0;
    HIP_TRY(c, hipMemcpyAsync(&Q, a.fc + M, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    t.Q = Q;
    if (Q == 0) return 0;
    t.off = a.rc_off; t.area = a.rc_area; t.res = a.rc_res; t.cnt = a.rc_cnt; t.rev = a.rc_rev;
    return 0;
}

/* The one capacity check: every capacity an array that is delivered asks for, against its count, in the order P, M, R, C, D_b, Q.
   (atom_capacity counts for contact_first and the masks too: they have M + 1 and M entries.) */
int iface_check_caps(freesasa_gpu_ctx *c, const IfaceCall &k, const IfaceRun &r)
{
    const struct { bool wanted; long long count, capacity; const char *message; } caps[] = {
        {k.whole || k.pair_struct || k.pair_groups, r.pl.P, k.pair_capacity,
         "pair_capacity %lld is too small: the batch has %lld pairs of groups in contact"},
        {k.pair_atom || k.pair_buried || k.contact_first || k.buried_masks, r.pl.M, k.atom_capacity,
         "atom_capacity %lld is too small: the pair structures hold %lld atoms"},
        {k.residues, r.rt.R, k.res_capacity, "res_capacity %lld is too small: the interfaces have %lld residue rows"},
        {k.contact_partner || k.contact_points || k.contact_area, r.ct.C, k.contact_capacity,
         "contact_capacity %lld is too small: the interfaces have %lld contact rows"},
        {k.dot_partner != nullptr, r.ct.D, k.dot_capacity, "dot_capacity %lld is too small: the interfaces bury %lld test points"},
        {k.rescontacts, r.qt.Q, k.rescontact_capacity, "rescontact_capacity %lld is too small: the interfaces have %lld residue contact rows"},
    };
    for (const auto &x : caps)
        if (x.wanted && x.count > x.capacity) return ctx_fail(c, x.message, x.capacity, x.count);
    return 0;
}

} /* namespace */

/* The one run: the screen or the whole pipeline, then the stages asked for.  Every count output is set as soon as its count is
   known; the capacities are held behind the screen where no stage follows step 8, else behind the last stage.  (engine_internal.h) */
int iface_run(freesasa_gpu_ctx *c, const IfaceCall &k, IfaceRun &r)
{
    const bool later = k.residues || k.contacts;
    if (iface_screen(c, k, r)) return -1;
    *k.n_pairs = r.pl.P; *k.n_pair_atoms = r.pl.M;
    if (!later && iface_check_caps(c, k, r)) return -1;
    if (k.whole && iface_pairs(c, k, r)) return -1;
    if (k.contacts) {
        if (iface_contacts(c, k, r)) return -1;
        *k.n_contacts = r.ct.C;
        if (k.n_buried_dots) *k.n_buried_dots = r.ct.D;
    }
    if (k.rescontacts) {
        if (iface_rescontacts(c, k, r)) return -1;
        *k.n_rescontacts = r.qt.Q;
    }
    if (k.residues) {
        if (iface_residues(c, k, r)) return -1;
        *k.n_res_rows = r.rt.R;
    }
    return later ? iface_check_caps(c, k, r) : 0;
}

/* ------------------------------------------------------------------ the one table of outputs and the one delivery */

namespace {

/* a deliverable array: `count` elements of `size` bytes from `src` - a device buffer of the context, or (plan) a host vector of
   the plan - to the caller's `dst` (null: not delivered); where the call made no such array (src null), `zeros` elements of 0 */
struct IfaceOut {
    void *dst;
    const void *src;
    bool plan;
    size_t size, count, zeros;
};
enum { IF_N_OUT = 21 };
std::array<IfaceOut, IF_N_OUT> iface_outputs(freesasa_gpu_ctx *c, const IfaceCall &k, const IfaceRun &r)
{
    const IfacePlan &pl = r.pl;
    const size_t P = (size_t)pl.P, M = (size_t)pl.M, R = (size_t)r.rt.R, C = (size_t)r.ct.C, D = (size_t)r.ct.D, Q = (size_t)r.qt.Q;
    const size_t sides = 2 * P + 1; /* (1 without a pair: the offsets of no side) */
    return {{
        {k.pair_struct, pl.pair_struct.data(), true, 4, P, 0},
        {k.pair_groups, pl.pair_groups.data(), true, 8, P, 0},
        {k.pair_areas, c->if_areas.p, false, 48, P, 0},
        {k.side_offsets, pl.side_off.data(), true, 8, sides, 0},
        {k.pair_atom, c->if_patom.p, false, 4, M, 0},
        {k.pair_buried, c->if_pburied.p, false, 8, M, 0},
        /* the per-residue table: without a pair res_offsets [1] = 0 */
        {k.res_offsets, r.rt.off, false, 8, sides, 1},
        {k.res_index, r.rt.index, false, 4, R, 0},
        {k.res_atoms, r.rt.atoms, false, 4, R, 0},
        {k.res_areas, r.rt.areas, false, 24, R, 0},
        /* the contact table: without a pair contact_first [1] = 0, without a buried point zeros [M + 1] behind the masks */
        {k.contact_first, r.ct.first, false, 8, M + 1, M + 1},
        {k.contact_partner, r.ct.partner, false, 4, C, 0},
        {k.contact_points, r.ct.points, false, 4, C, 0},
        {k.contact_area, r.ct.area, false, 8, C, 0},
        {k.buried_masks, r.ct.buried, false, 4 * SR_CAP_WORDS, M, 0},
        {k.dot_partner, r.ct.dot_partner, false, 4, D, 0},
        /* the folded table: without a folded row rescontact_offsets is zeros, [1] without a pair, else [2 P + 1] */
        {k.rescontact_offsets, r.qt.off, false, 8, sides, sides},
        {k.rescontact_residues, r.qt.res, false, 8, Q, 0},
        {k.rescontact_counts, r.qt.cnt, false, 8, Q, 0},
        {k.rescontact_area, r.qt.area, false, 8, Q, 0},
        {k.rescontact_reverse, r.qt.rev, false, 4, Q, 0},
    }};
}

} /* namespace */

/* The delivery, in two calls around the caller's stream synchronization.  idle = false: everything that goes over the stream is
   enqueued - to device arrays the context's buffers, the plan's arrays and the zeros; to host arrays the context's buffers (the
   zeros are written at once).  idle = true, once the synchronize has succeeded: the plan's arrays into host arrays, and stats.
   (engine_internal.h) */
int iface_deliver(freesasa_gpu_ctx *c, const IfaceCall &k, const IfaceRun &r, bool idle)
{
    hipStream_t st = c->stream;
    for (const IfaceOut &o : iface_outputs(c, k, r)) {
        const size_t bytes = o.size * (o.src ? o.count : o.zeros);
        if (!o.dst || !bytes || idle != (o.plan && !k.out_dev)) continue;
        hipError_t e = hipSuccess;
        if (idle) memcpy(o.dst, o.src, bytes);
        else if (!o.src && !k.out_dev) memset(o.dst, 0, bytes);
        else if (!o.src) e = hipMemsetAsync(o.dst, 0, bytes, st);
        else e = hipMemcpyAsync(o.dst, o.src, bytes, !k.out_dev ? hipMemcpyDeviceToHost : o.plan ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess)
            return k.out_dev ? ctx_fail(c, "delivery to the caller's device arrays failed: %s", hipGetErrorString(e)) : ctx_fail(c, "device-to-host copy failed");
    }
    if (idle && k.stats) { k.stats[0] = r.pl.T; k.stats[1] = r.pl.n_cand; }
    return 0;
}

/* ------------------------------------------------------------------ the two entry kinds */

namespace {

/* the batch on the context's stream; the call is synchronous, and a failed one drains the stream too */
int iface_dev(freesasa_gpu_ctx *c, const IfaceCall &k)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first) */
    return guarded_ctx(c, [&]() -> int {
        char msg[200];
        c->err[0] = 0;
        if (iface_bad_call(k, c->device, msg, sizeof msg)) return ctx_fail(c, "%s", msg);
        IfaceRun r;
        int rc = iface_run(c, k, r) || iface_deliver(c, k, r, false) ? -1 : 0;
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "stream synchronize failed");
        return rc ? rc : iface_deliver(c, k, r, true);
    });
}

/* the batch in host arrays: the grouped host batch (gpu_groups.hip) on a pooled context, the pipeline on its staging */
int iface_host(const IfaceCall &k, int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    char msg[200];
    if (iface_bad_call(k, -1, msg, sizeof msg)) return set_err(err_out, err_len, msg);
    return guarded(err_out, err_len, [&]() -> int {
    IfaceRun r;
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    BatchCall b;
    b.fallback = "GPU interface batch failed";
    GroupBatch g;
    g.xyz = k.xyz; g.radii = k.radii; g.offsets = k.offsets; g.n_structs = k.n_structs; g.group = k.group; g.n_groups = k.n_groups;
    g.sasa_out = k.sasa; g.iso_out = k.iso; g.totals_out = k.totals; g.group_totals_out = k.group_totals;
    const int rc = [&]() -> int {
        c->err[0] = 0;
        if (group_batch_upload(b, c, g)) return -1;
        if (k.offsets[k.n_structs] > (int64_t)1 << 30) return ctx_fail(c, "batch too large (max 2^30 atoms per call)");
        IfaceCall d = k; /* the same call on the staged batch */
        d.xyz = g.d_xyz; d.radii = g.d_radii; d.group = g.d_group;
        d.sasa = g.d_sasa; d.iso = g.d_iso; d.totals = g.d_totals; d.group_totals = g.d_group_totals;
        if (iface_run(c, d, r) || iface_deliver(c, d, r, false) || group_batch_download(c, g)) return -1;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        return iface_deliver(c, d, r, true);
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}

} /* namespace */

extern "C" int freesasa_gpu_interface_pairs_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                                const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                                double probe_radius, int resolution, double *d_sasa, double *d_iso, double *d_totals,
                                                double *d_group_totals, long long pair_capacity, long long *n_pairs_out,
                                                long long *n_pair_atoms_out, int32_t *pair_struct_out, int32_t *pair_groups_out,
                                                long long *stats_out)
{
    IfaceCall k;
    k.xyz = d_xyz; k.radii = d_radii; k.offsets = offsets; k.n_structs = n_structs; k.group = d_group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = d_sasa; k.iso = d_iso; k.totals = d_totals; k.group_totals = d_group_totals;
    k.pair_capacity = pair_capacity; k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out;
    k.pair_struct = pair_struct_out; k.pair_groups = pair_groups_out; k.stats = stats_out; /* (host arrays) */
    return iface_dev(c, k);
}

extern "C" int freesasa_gpu_interfaces_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                           const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                           double probe_radius, int resolution, double *d_sasa, double *d_iso, double *d_totals,
                                           double *d_group_totals, long long pair_capacity, long long atom_capacity,
                                           long long *n_pairs_out, long long *n_pair_atoms_out, int32_t *d_pair_struct,
                                           int32_t *d_pair_groups, double *d_pair_areas, int64_t *d_side_offsets, int32_t *d_pair_atom,
                                           double *d_pair_buried)
{
    IfaceCall k;
    k.xyz = d_xyz; k.radii = d_radii; k.offsets = offsets; k.n_structs = n_structs; k.group = d_group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = d_sasa; k.iso = d_iso; k.totals = d_totals; k.group_totals = d_group_totals;
    k.whole = true; k.out_dev = true;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out;
    k.pair_struct = d_pair_struct; k.pair_groups = d_pair_groups; k.pair_areas = d_pair_areas; k.side_offsets = d_side_offsets;
    k.pair_atom = d_pair_atom; k.pair_buried = d_pair_buried;
    return iface_dev(c, k);
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
    IfaceCall k;
    k.xyz = d_xyz; k.radii = d_radii; k.offsets = offsets; k.n_structs = n_structs; k.group = d_group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = d_sasa; k.iso = d_iso; k.totals = d_totals; k.group_totals = d_group_totals;
    k.whole = k.residues = true; k.out_dev = true;
    k.res_first = res_first; k.n_res = n_res; k.min_buried = min_buried;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.res_capacity = res_capacity;
    k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out; k.n_res_rows = n_res_rows_out;
    k.pair_struct = d_pair_struct; k.pair_groups = d_pair_groups; k.pair_areas = d_pair_areas; k.side_offsets = d_side_offsets;
    k.pair_atom = d_pair_atom; k.pair_buried = d_pair_buried;
    k.res_offsets = d_res_offsets; k.res_index = d_res_index; k.res_atoms = d_res_atoms; k.res_areas = d_res_areas;
    return iface_dev(c, k);
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
    IfaceCall k;
    k.xyz = d_xyz; k.radii = d_radii; k.offsets = offsets; k.n_structs = n_structs; k.group = d_group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = d_sasa; k.iso = d_iso; k.totals = d_totals; k.group_totals = d_group_totals;
    k.whole = k.contacts = true; k.out_dev = true;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.contact_capacity = contact_capacity; k.dot_capacity = dot_capacity;
    k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out; k.n_contacts = n_contacts_out; k.n_buried_dots = n_buried_dots_out;
    k.pair_struct = d_pair_struct; k.pair_groups = d_pair_groups; k.pair_areas = d_pair_areas; k.side_offsets = d_side_offsets;
    k.pair_atom = d_pair_atom; k.pair_buried = d_pair_buried;
    k.contact_first = d_contact_first; k.contact_partner = d_contact_partner; k.contact_points = d_contact_points;
    k.contact_area = d_contact_area; k.buried_masks = d_buried_masks; k.dot_partner = d_dot_partner;
    return iface_dev(c, k);
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
    IfaceCall k;
    k.xyz = d_xyz; k.radii = d_radii; k.offsets = offsets; k.n_structs = n_structs; k.group = d_group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = d_sasa; k.iso = d_iso; k.totals = d_totals; k.group_totals = d_group_totals;
    k.whole = k.contacts = k.rescontacts = true; k.out_dev = true;
    k.res_first = res_first; k.n_res = n_res;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.contact_capacity = contact_capacity; k.dot_capacity = dot_capacity;
    k.rescontact_capacity = rescontact_capacity;
    k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out; k.n_contacts = n_contacts_out; k.n_buried_dots = n_buried_dots_out;
    k.n_rescontacts = n_rescontacts_out;
    k.pair_struct = d_pair_struct; k.pair_groups = d_pair_groups; k.pair_areas = d_pair_areas; k.side_offsets = d_side_offsets;
    k.pair_atom = d_pair_atom; k.pair_buried = d_pair_buried;
    k.contact_first = d_contact_first; k.contact_partner = d_contact_partner; k.contact_points = d_contact_points;
    k.contact_area = d_contact_area; k.buried_masks = d_buried_masks; k.dot_partner = d_dot_partner;
    k.rescontact_offsets = d_rescontact_offsets; k.rescontact_residues = d_rescontact_residues; k.rescontact_counts = d_rescontact_counts;
    k.rescontact_area = d_rescontact_area; k.rescontact_reverse = d_rescontact_reverse;
    return iface_dev(c, k);
}

extern "C" int freesasa_gpu_calc_interface_pairs(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                 const int32_t *group, const int32_t *n_groups, int alg, double probe_radius,
                                                 int resolution, long long pair_capacity, long long *n_pairs_out,
                                                 long long *n_pair_atoms_out, int32_t *pair_struct_out, int32_t *pair_groups_out,
                                                 long long *stats_out, int device, char *err_out, int err_len)
{
    IfaceCall k;
    k.xyz = xyz; k.radii = radii; k.offsets = offsets; k.n_structs = n_structs; k.group = group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.pair_capacity = pair_capacity; k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out;
    k.pair_struct = pair_struct_out; k.pair_groups = pair_groups_out; k.stats = stats_out;
    return iface_host(k, device, err_out, err_len);
}

extern "C" int freesasa_gpu_calc_interfaces(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                            const int32_t *group, const int32_t *n_groups, int alg, double probe_radius, int resolution,
                                            double *sasa_out, double *iso_out, double *totals_out, double *group_totals_out,
                                            long long pair_capacity, long long atom_capacity, long long *n_pairs_out,
                                            long long *n_pair_atoms_out, int32_t *pair_struct_out, int32_t *pair_groups_out,
                                            double *pair_areas_out, int64_t *side_offsets_out, int32_t *pair_atom_out,
                                            double *pair_buried_out, int device, char *err_out, int err_len)
{
    IfaceCall k;
    k.xyz = xyz; k.radii = radii; k.offsets = offsets; k.n_structs = n_structs; k.group = group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = sasa_out; k.iso = iso_out; k.totals = totals_out; k.group_totals = group_totals_out;
    k.whole = true;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out;
    k.pair_struct = pair_struct_out; k.pair_groups = pair_groups_out; k.pair_areas = pair_areas_out; k.side_offsets = side_offsets_out;
    k.pair_atom = pair_atom_out; k.pair_buried = pair_buried_out;
    return iface_host(k, device, err_out, err_len);
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
    IfaceCall k;
    k.xyz = xyz; k.radii = radii; k.offsets = offsets; k.n_structs = n_structs; k.group = group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = sasa_out; k.iso = iso_out; k.totals = totals_out; k.group_totals = group_totals_out;
    k.whole = k.residues = true;
    k.res_first = res_first; k.n_res = n_res; k.min_buried = min_buried;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.res_capacity = res_capacity;
    k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out; k.n_res_rows = n_res_rows_out;
    k.pair_struct = pair_struct_out; k.pair_groups = pair_groups_out; k.pair_areas = pair_areas_out; k.side_offsets = side_offsets_out;
    k.pair_atom = pair_atom_out; k.pair_buried = pair_buried_out;
    k.res_offsets = res_offsets_out; k.res_index = res_index_out; k.res_atoms = res_atoms_out; k.res_areas = res_areas_out;
    return iface_host(k, device, err_out, err_len);
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
    IfaceCall k;
    k.xyz = xyz; k.radii = radii; k.offsets = offsets; k.n_structs = n_structs; k.group = group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = sasa_out; k.iso = iso_out; k.totals = totals_out; k.group_totals = group_totals_out;
    k.whole = k.contacts = true;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.contact_capacity = contact_capacity; k.dot_capacity = dot_capacity;
    k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out; k.n_contacts = n_contacts_out; k.n_buried_dots = n_buried_dots_out;
    k.pair_struct = pair_struct_out; k.pair_groups = pair_groups_out; k.pair_areas = pair_areas_out; k.side_offsets = side_offsets_out;
    k.pair_atom = pair_atom_out; k.pair_buried = pair_buried_out;
    k.contact_first = contact_first_out; k.contact_partner = contact_partner_out; k.contact_points = contact_points_out;
    k.contact_area = contact_area_out; k.buried_masks = buried_masks_out; k.dot_partner = dot_partner_out;
    return iface_host(k, device, err_out, err_len);
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
    IfaceCall k;
    k.xyz = xyz; k.radii = radii; k.offsets = offsets; k.n_structs = n_structs; k.group = group; k.n_groups = n_groups;
    k.alg = alg; k.probe = probe_radius; k.resolution = resolution;
    k.sasa = sasa_out; k.iso = iso_out; k.totals = totals_out; k.group_totals = group_totals_out;
    k.whole = k.contacts = k.rescontacts = true;
    k.res_first = res_first; k.n_res = n_res;
    k.pair_capacity = pair_capacity; k.atom_capacity = atom_capacity; k.contact_capacity = contact_capacity; k.dot_capacity = dot_capacity;
    k.rescontact_capacity = rescontact_capacity;
    k.n_pairs = n_pairs_out; k.n_pair_atoms = n_pair_atoms_out; k.n_contacts = n_contacts_out; k.n_buried_dots = n_buried_dots_out;
    k.n_rescontacts = n_rescontacts_out;
    k.pair_struct = pair_struct_out; k.pair_groups = pair_groups_out; k.pair_areas = pair_areas_out; k.side_offsets = side_offsets_out;
    k.pair_atom = pair_atom_out; k.pair_buried = pair_buried_out;
    k.contact_first = contact_first_out; k.contact_partner = contact_partner_out; k.contact_points = contact_points_out;
    k.contact_area = contact_area_out; k.buried_masks = buried_masks_out; k.dot_partner = dot_partner_out;
    k.rescontact_offsets = rescontact_offsets_out; k.rescontact_residues = rescontact_residues_out; k.rescontact_counts = rescontact_counts_out;
    k.rescontact_area = rescontact_area_out; k.rescontact_reverse = rescontact_reverse_out;
    return iface_host(k, device, err_out, err_len);
}
