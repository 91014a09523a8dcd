/*
 * occupancy_kernels.h — phase functions of the RESIDUE CONTACT OCCUPANCY MAP over a trajectory's interfaces
 * (freesasa_gpu_contact_occupancy_*; include/freesasa_gpu.h has the definitions, tests/contact_occupancy_ref.py restates them in
 * plain Python): the folded rows of the residue-residue contact tables (rescontact_kernels.h) of a CHUNK of frames reduced into
 * the RUN TABLE, one row per distinct key (g, h, side, res_a, res_b), ascending, that lives on the device between calls.
 *
 * A chunk is F frames whose rows are frame after frame, ff [F + 1] their first rows, every frame's keys strictly ascending.  The
 * run table of U rows and a chunk give the next table of U + N rows in a second set of arrays (two sets, swapped):
 *
 *   occ_keys        (frames that went through the interface pipeline) one thread per folded row of the chunk and per frame boundary:
 *                   the row's side from rescontact_offsets, its pair, the pair's structure = the frame; the key from pair_groups, the
 *                   side and rescontact_residues less frame * n_res; ff[f] = rescontact_offsets[2 * (the frame's first pair)]
 *   occ_first       one thread per chunk row: fl = 1 for a FIRST OCCURRENCE - neither the run table nor an earlier frame of the
 *                   chunk holds the key (binary searches: every list ascends)
 *   scan            kl_iface_res_scan over fl [Q + 1] in place: the first occurrences before every row, fl[Q] = N
 *   occ_rank        one thread per old row and per chunk row: an old row's place is its index plus the first occurrences below its
 *                   key, a first occurrence's the old rows below its key plus the first occurrences below it - per frame
 *                   fl[lower bound of the key] - fl[ff[f]].  The keys are distinct, so the places are: a merge by ranks, no sort,
 *                   no atomics.  Old rows carry their accumulators; a new row starts empty, its frames_either at that of its
 *                   reversed key's old row (the two are one number: the frames that hold the key OR its reverse)
 *   occ_accumulate  one thread per row of the next table: the chunk's frames in order, a search for the key and one for the reversed
 *                   key in each; the area one addition at a time in frame order
 *   occ_reverse     (at a snapshot) one thread per row: the row of the reversed key, or -1
 *
 * The three phases that walk the chunk's frames are chains of dependent loads - a binary search a frame - on few threads; they step
 * the searches of OCC_SIDE frames side by side (occ_lower_frames) so that a thread has that many loads in flight.  What is added
 * is added in frame order all the same.
 *
 * A thread works alone: no barrier, no workgroup waits for another, no floating-point atomics, no sum combined across lanes; what
 * a row holds does not depend on the launch shape.  A key is compared component by component (five int32, exact over their whole
 * range).  Sizes: Q, U + N < 2^31; no phase writes at or beyond the capacity it is given.
 *
 * Written like rescontact_kernels.h: plain phase functions, so that a -DSASA_EMU build can drive them on the CPU
 * (tests/emu/emu_occupancy.cpp); the __global__ wrappers and kl_occ_* launchers are in gpu_kernels.hip, the host side in
 * gpu_occupancy.hip.
 */
#ifndef FREESASA_AMD_OCCUPANCY_KERNELS_H
#define FREESASA_AMD_OCCUPANCY_KERNELS_H

#include "iface_kernels.h"

namespace sasa {

#define OCC_KEY 5  /* int32 to a key: g, h, side, res_a, res_b */
#define OCC_SIDE 8 /* frames of a chunk whose binary searches one thread steps side by side (occ_lower_frames) */

/* one set of the run table's arrays; `cap` rows each */
struct OccTable {
    int *keys;        /* [cap][5] */
    int64_t *frames;  /* [cap] */
    int64_t *either;  /* [cap] */
    int64_t *counts;  /* [cap][2] n_rows, n_points */
    double *area;     /* [cap][3] sum, min, max */
    int64_t *span;    /* [cap][2] first, last frame */
    int64_t cap;
};

struct OccKeyArgs {
    int64_t n_rows, n_sides; /* Q, 2 P of the chunk */
    int n_frames, n_res;     /* F; the residues of ONE frame */
    const int64_t *rc_off;   /* [2 P + 1] rescontact_offsets */
    const int *rc_res;       /* [Q][2] rescontact_residues (chunk-wide numbers) */
    const int *pair_struct;  /* [P] */
    const int *pair_groups;  /* [P][2] */
    const int *pair_first;   /* [F + 1] the first pair of every frame; pair_first[F] = P */
    int *ck;                 /* [Q][5] */
    int64_t *ff;             /* [F + 1] */
};

struct OccArgs {
    int64_t n_rows;       /* Q of the chunk */
    int n_frames;         /* F of the chunk */
    int64_t frame0;       /* the run's number of the chunk's first frame */
    int64_t n_old, n_new; /* U; U + N (occ_first and occ_rank do not read n_new) */
    const int64_t *ff;    /* [F + 1] */
    const int *ck;        /* [Q][5] */
    const int *cc;        /* [Q][2] n_rows, n_points */
    const double *ca;     /* [Q] */
    int *fl;              /* [Q + 1] first-occurrence flags, then their exclusive scan; fl[Q] = N */
    OccTable old, next;
    int *reverse;         /* (occ_reverse) [n_new] over `next` */
};

/* -1, 0, 1: key a below, equal to, above key b */
SASA_D int occ_cmp(const int *a, const int *b)
{
    for (int k = 0; k < OCC_KEY; ++k) {
        if (a[k] < b[k]) return -1;
        if (a[k] > b[k]) return 1;
    }
    return 0;
}
/* the first of rows lo .. hi - 1 of an ascending key list whose key is not below k (hi if there is none) */
SASA_D int64_t occ_lower(const int *keys, int64_t lo, int64_t hi, const int *k)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (occ_cmp(keys + OCC_KEY * mid, k) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
/* the row of rows lo .. hi - 1 that holds key k, or -1 */
SASA_D int64_t occ_find(const int *keys, int64_t lo, int64_t hi, const int *k)
{
    const int64_t at = occ_lower(keys, lo, hi, k);
    return at < hi && occ_cmp(keys + OCC_KEY * at, k) == 0 ? at : -1;
}
SASA_D void occ_reversed(const int *k, int *r)
{
    r[0] = k[0]; r[1] = k[1]; r[2] = 1 - k[2]; r[3] = k[4]; r[4] = k[3];
}
/* the last of n + 1 ascending boundaries (b[0] = 0) at or before t, among 0 .. n - 1 */
SASA_D int64_t occ_segment(const int64_t *b, int64_t n, int64_t t)
{
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (b[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* -1, 0, 1 for the key of row r of a list below, equal to, above k: all five components loaded before any is looked at, no branch */
SASA_D int occ_cmp_row(const int *keys, int64_t r, const int *k)
{
    const int *a = keys + OCC_KEY * r;
    const int a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4];
    int c = (a4 > k[4]) - (a4 < k[4]);
    c = a3 != k[3] ? (a3 > k[3]) - (a3 < k[3]) : c;
    c = a2 != k[2] ? (a2 > k[2]) - (a2 < k[2]) : c;
    c = a1 != k[1] ? (a1 > k[1]) - (a1 < k[1]) : c;
    c = a0 != k[0] ? (a0 > k[0]) - (a0 < k[0]) : c;
    return c;
}
/* The lower bounds of k in the chunk's frames e0 .. e0 + n - 1 (1 <= n <= OCC_SIDE), occ_lower's results: the n binary searches
   step side by side, so that a thread has n loads in flight where one search after the other waits for each of its own.  A
   search that has ended goes on comparing a row it has no use for (n_rows >= 1: row min(mid, n_rows - 1) exists). */
SASA_D void occ_lower_frames(const int *ck, const int64_t *ff, int64_t n_rows, int e0, int n, const int *k, int64_t *at)
{
    int64_t lo[OCC_SIDE], hi[OCC_SIDE];
#pragma unroll
    for (int j = 0; j < OCC_SIDE; ++j) {
        const int e = e0 + (j < n ? j : 0);
        lo[j] = ff[e];
        hi[j] = j < n ? ff[e + 1] : lo[j];
    }
    for (bool any = true; any;) {
        int c[OCC_SIDE];
        any = false;
#pragma unroll
        for (int j = 0; j < OCC_SIDE; ++j) {
            const int64_t mid = (lo[j] + hi[j]) >> 1;
            c[j] = occ_cmp_row(ck, mid < n_rows ? mid : n_rows - 1, k);
        }
#pragma unroll
        for (int j = 0; j < OCC_SIDE; ++j) {
            if (lo[j] >= hi[j]) continue;
            const int64_t mid = (lo[j] + hi[j]) >> 1;
            if (c[j] < 0) lo[j] = mid + 1;
            else hi[j] = mid;
            any = true;
        }
    }
#pragma unroll
    for (int j = 0; j < OCC_SIDE; ++j) at[j] = lo[j];
}

/* one thread per folded row of the chunk and per frame boundary */
SASA_D void occ_keys(const OccKeyArgs &a, int64_t t)
{
    if (t <= a.n_frames) a.ff[t] = a.rc_off[2 * (int64_t)a.pair_first[t]];
    if (t >= a.n_rows) return;
    const int64_t q = occ_segment(a.rc_off, a.n_sides, t); /* (the last side that begins at or before t: the one that holds it) */
    const int64_t p = q >> 1;
    const int base = a.pair_struct[p] * a.n_res;
    int *k = a.ck + OCC_KEY * t;
    k[0] = a.pair_groups[2 * p]; k[1] = a.pair_groups[2 * p + 1]; k[2] = (int)(q & 1);
    k[3] = a.rc_res[2 * t] - base; k[4] = a.rc_res[2 * t + 1] - base;
}

/* one thread per chunk row */
SASA_D void occ_first(const OccArgs &a, int64_t t)
{
    if (t >= a.n_rows) return;
    const int *k = a.ck + OCC_KEY * t;
    const int64_t f = occ_segment(a.ff, a.n_frames, t);
    bool seen = occ_find(a.old.keys, 0, a.n_old, k) >= 0;
    for (int e0 = 0; e0 < f && !seen; e0 += OCC_SIDE) {
        const int n = f - e0 < OCC_SIDE ? (int)(f - e0) : OCC_SIDE;
        int64_t at[OCC_SIDE];
        occ_lower_frames(a.ck, a.ff, a.n_rows, e0, n, k, at);
#pragma unroll
        for (int j = 0; j < OCC_SIDE; ++j)
            if (j < n && at[j] < a.ff[e0 + j + 1] && occ_cmp_row(a.ck, at[j], k) == 0) seen = true;
    }
    a.fl[t] = seen ? 0 : 1;
}

/* the chunk's first occurrences whose key is below k (behind the scan of fl) */
SASA_D int64_t occ_new_below(const OccArgs &a, const int *k)
{
    int64_t n = 0;
    for (int e0 = 0; e0 < a.n_frames; e0 += OCC_SIDE) {
        const int m = a.n_frames - e0 < OCC_SIDE ? a.n_frames - e0 : OCC_SIDE;
        int64_t at[OCC_SIDE];
        occ_lower_frames(a.ck, a.ff, a.n_rows, e0, m, k, at);
#pragma unroll
        for (int j = 0; j < OCC_SIDE; ++j)
            if (j < m) n += a.fl[at[j]] - a.fl[a.ff[e0 + j]];
    }
    return n;
}

/* one thread per old row (t < U) and per chunk row (U <= t < U + Q), behind the scan of fl */
SASA_D void occ_rank(const OccArgs &a, int64_t t)
{
    const OccTable &o = a.old, &w = a.next;
    if (t < a.n_old) {
        const int *k = o.keys + OCC_KEY * t;
        const int64_t at = t + occ_new_below(a, k);
        if (at >= w.cap) return;
        for (int j = 0; j < OCC_KEY; ++j) w.keys[OCC_KEY * at + j] = k[j];
        w.frames[at] = o.frames[t]; w.either[at] = o.either[t];
        w.counts[2 * at] = o.counts[2 * t]; w.counts[2 * at + 1] = o.counts[2 * t + 1];
        w.area[3 * at] = o.area[3 * t]; w.area[3 * at + 1] = o.area[3 * t + 1]; w.area[3 * at + 2] = o.area[3 * t + 2];
        w.span[2 * at] = o.span[2 * t]; w.span[2 * at + 1] = o.span[2 * t + 1];
        return;
    }
    const int64_t r = t - a.n_old;
    if (r >= a.n_rows || a.fl[r + 1] == a.fl[r]) return;
    const int *k = a.ck + OCC_KEY * r;
    const int64_t at = occ_lower(o.keys, 0, a.n_old, k) + occ_new_below(a, k);
    if (at >= w.cap) return;
    int rk[OCC_KEY];
    occ_reversed(k, rk);
    const int64_t rev = occ_find(o.keys, 0, a.n_old, rk);
    for (int j = 0; j < OCC_KEY; ++j) w.keys[OCC_KEY * at + j] = k[j];
    w.frames[at] = 0; w.either[at] = rev >= 0 ? o.either[rev] : 0;
    w.counts[2 * at] = 0; w.counts[2 * at + 1] = 0;
    w.area[3 * at] = 0.0; w.area[3 * at + 1] = 0.0; w.area[3 * at + 2] = 0.0;
    w.span[2 * at] = -1; w.span[2 * at + 1] = -1;
}

/* one thread per row of the next table, behind occ_rank */
SASA_D void occ_accumulate(const OccArgs &a, int64_t t)
{
    const OccTable &w = a.next;
    if (t >= a.n_new || t >= w.cap) return;
    int k[OCC_KEY], rk[OCC_KEY];
    for (int j = 0; j < OCC_KEY; ++j) k[j] = w.keys[OCC_KEY * t + j];
    occ_reversed(k, rk);
    int64_t frames = w.frames[t], either = w.either[t], n_rows = w.counts[2 * t], n_points = w.counts[2 * t + 1];
    int64_t first = w.span[2 * t], last = w.span[2 * t + 1];
    double sum = w.area[3 * t], lo = w.area[3 * t + 1], hi = w.area[3 * t + 2];
    for (int e0 = 0; e0 < a.n_frames; e0 += OCC_SIDE) {
        /* the searches of OCC_SIDE frames side by side, for the key and for the reversed key; then the frames in order */
        const int m = a.n_frames - e0 < OCC_SIDE ? a.n_frames - e0 : OCC_SIDE;
        int64_t at[OCC_SIDE], rat[OCC_SIDE];
        occ_lower_frames(a.ck, a.ff, a.n_rows, e0, m, k, at);
        occ_lower_frames(a.ck, a.ff, a.n_rows, e0, m, rk, rat);
        bool here[OCC_SIDE], there[OCC_SIDE];
        double xs[OCC_SIDE];
        int nr[OCC_SIDE], np[OCC_SIDE];
#pragma unroll
        for (int j = 0; j < OCC_SIDE; ++j) {
            const int64_t end = j < m ? a.ff[e0 + j + 1] : 0;
            here[j] = j < m && at[j] < end && occ_cmp_row(a.ck, at[j], k) == 0;
            there[j] = j < m && rat[j] < end && occ_cmp_row(a.ck, rat[j], rk) == 0;
            xs[j] = here[j] ? a.ca[at[j]] : 0.0;
            nr[j] = here[j] ? a.cc[2 * at[j]] : 0;
            np[j] = here[j] ? a.cc[2 * at[j] + 1] : 0;
        }
#pragma unroll
        for (int j = 0; j < OCC_SIDE; ++j) {
            if (here[j]) {
                const double x = xs[j];
                if (frames == 0) { lo = x; hi = x; first = a.frame0 + e0 + j; }
                else { if (x < lo) lo = x; if (x > hi) hi = x; }
                ++frames;
                n_rows += nr[j]; n_points += np[j];
                sum = sum + x;
                last = a.frame0 + e0 + j;
            }
            if (here[j] || there[j]) ++either;
        }
    }
    w.frames[t] = frames; w.either[t] = either; w.counts[2 * t] = n_rows; w.counts[2 * t + 1] = n_points;
    w.area[3 * t] = sum; w.area[3 * t + 1] = lo; w.area[3 * t + 2] = hi;
    w.span[2 * t] = first; w.span[2 * t + 1] = last;
}

/* one thread per row of `next` */
SASA_D void occ_reverse(const OccArgs &a, int64_t t)
{
    if (t >= a.n_new) return;
    int rk[OCC_KEY];
    occ_reversed(a.next.keys + OCC_KEY * t, rk);
    a.reverse[t] = (int)occ_find(a.next.keys, 0, a.n_new, rk);
}

} /* namespace sasa */

#endif
