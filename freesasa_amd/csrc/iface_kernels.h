/*
 * iface_kernels.h — phase functions of the pairwise interface areas between chain groups (freesasa_gpu_interfaces_dev,
 * include/freesasa_gpu.h has the definitions): which groups of a structure touch, the batch of their pair structures, and
 * what is made of its areas.  The SASA of the pair batch is the ordinary pipeline, unchanged.
 *
 * Written like group_kernels.h: every function is one thread's (iface_box: one wave's, iface_contact: one thread of a
 * workgroup's) share of a phase, so that a -DSASA_EMU build can drive them on the CPU (tests/emu/emu_iface.cpp); the
 * __global__ wrappers and kl_iface_* launchers are in gpu_kernels.hip, the host side in gpu_interfaces.hip.
 *
 * The input is the combined batch the chain-group entry leaves on the device (group_kernels.h): the n input atoms, then the
 * G groups as structures of their own, group k = gbase[s] + g at combined atoms gstart[k] .. gstart[k + 1] - 1 in input order.
 * The groups of one structure are screened pair by pair - test t = tbase[s] + u, u counting the pairs (g < h) of the structure
 * row by row - in three steps: a box per group, the pairs whose boxes come close (candidates), the reference's neighbour test
 * between the atoms of a candidate's two sides.  Flags are indexed by t and the table is made of them in ascending t: the
 * order the candidates' list was appended in (an integer atomic) shows in no result.  No float atomics anywhere.
 *
 * Why the two conservative steps cannot drop a contact.  Atoms i of g and j of h are in contact iff, every operation rounded,
 *     dx * dx + dy * dy + dz * dz < (Ri + Rj) * (Ri + Rj),    dx = xj - xi ...,  Ri = radii[i] + probe
 * Rounding is monotone: a <= b gives fl(a op c) <= fl(b op c) for a sum, a difference, and a product of non-negative
 * numbers.  The left side is at least fl(dx * dx) (non-negative terms are added), so fl(dx * dx) < fl(s * s) with s = fl(Ri + Rj), and
 * since x -> fl(x * x) does not decrease on x >= 0, |dx| < s.  The steps below test differences formed the same way against
 * sums formed the same way, with one operand replaced by a bound of it: xj <= max_h gives fl(xi - max_h) <= fl(xi - xj) <= |dx|,
 * and Rj <= rmax_h gives s <= fl(Ri + rmax_h); so fl(xi - max_h) < fl(Ri + rmax_h), which is the clip; with xi >= min_g and
 * Ri <= rmax_g on top, fl(min_g - max_h) < fl(rmax_g + rmax_h), which is the candidate test.  Nowhere is a bound computed in
 * one way compared with a quantity computed in another.
 */
#ifndef FREESASA_AMD_IFACE_KERNELS_H
#define FREESASA_AMD_IFACE_KERNELS_H

#include "sasa_kernels.h"
#include "lr2_kernels.h" /* (the wave primitive LR2_SHFL and its SASA_EMU form) */

namespace sasa {

#define IF_B 256               /* threads per workgroup of every phase */
#define IF_MAX_GROUPS 4096     /* groups of one structure: 8.4e6 tests */
#define IF_MAX_TESTS (1 << 27) /* tests of one call */
/* Survivors of one side kept in LDS: 32 bytes each, 32 KiB - four workgroups of 256 threads on a CU's 160 KiB, the most the
   CU runs of such workgroups anyway; every lane reads the same entry at the same time (a broadcast: no bank conflicts).  A
   2 000-atom globule keeps a few hundred atoms near a partner; a side with more survivors than this is read from memory. */
#define IF_LDS_ATOMS 1024
#define IF_TRIP 4            /* partners a thread tests between two looks at whether it has hit */
#define IF_CONTACT_GRID 1024 /* workgroups of the contact kernel: four to a CU */
#ifdef SASA_EMU
#define IF_BARRIER() sasa_emu::wave_sync()
#define IF_INF HUGE_VAL
#else
#define IF_BARRIER() __syncthreads()
#define IF_INF __builtin_huge_val()
#endif

struct IfaceLds {
    double at[4 * IF_LDS_ATOMS]; /* x, y, z, r + probe */
    int cnt, hit;
};

struct IfaceArgs {
    /* the combined batch (GrpArgs: cxyz, cradii, src) and its results */
    const double *cxyz, *cradii;
    const int *src;           /* [n_iso] input atom of combined atom n + . */
    const double *csasa;      /* [n + n_iso] */
    const double *ctot;       /* [n_structs + G] */
    int n_atoms, n_structs, n_groups;
    double probe;
    const int64_t *gstart;    /* [G + 1] first combined atom of every group */
    const int64_t *gbase;     /* [n_structs + 1] first group of every structure */
    const int64_t *tbase;     /* [n_structs + 1] first test of every structure (prefix of ng (ng - 1) / 2) */
    int n_tests;
    /* the screen */
    double *box;              /* [8 G] min x y z, max x y z, the largest r + probe, unused; an empty group: +inf, -inf, 0 */
    int *n_cand;              /* [1] */
    int *cand;                /* [n_tests] the candidates' tests, in the order they were appended */
    unsigned char *flag;      /* [n_tests] zeroed by the host; 1: the pair is in contact */
    /* the pair batch */
    int64_t n_sides, n_pair_atoms; /* 2 P, M */
    const int64_t *side_off;   /* [2 P + 1] */
    const int64_t *side_start; /* [2 P] first combined atom of the side's group */
    const int *side_group;     /* [2 P] its k */
    double *pxyz, *pradii;     /* [3 M], [M] */
    int *pcomb;                /* [M] combined atom of every pair-structure atom */
    int *pair_atom;            /* [M] its input atom */
    /* finish */
    const double *psasa;       /* [M] */
    const double *inpair;      /* [2 P] */
    double *pair_buried;       /* [M] or null */
    double *pair_areas;        /* [6 P] */
};

/* a double from lane src, as two words through the tree's shuffle */
SASA_D double if_shfl_d(double v, int src)
{
    unsigned long long b;
    __builtin_memcpy(&b, &v, 8);
    const unsigned lo = (unsigned)LR2_SHFL((int)(unsigned)b, src), hi = (unsigned)LR2_SHFL((int)(unsigned)(b >> 32), src);
    b = ((unsigned long long)hi << 32) | lo;
    __builtin_memcpy(&v, &b, 8);
    return v;
}

/* Step 2, ONE WAVE PER GROUP k (every lane calls this with the same k): the group's box and its largest r + probe.  Minimum
   and maximum do not depend on the order they are taken in. */
SASA_D void iface_box(const IfaceArgs &a, int k, int lane)
{
    const int64_t b = a.gstart[k], e = a.gstart[k + 1];
    double v[7] = {IF_INF, IF_INF, IF_INF, -IF_INF, -IF_INF, -IF_INF, 0.0};
    for (int64_t j = b + lane; j < e; j += 64) {
        const double R = a.cradii[j] + a.probe;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = a.cxyz[3 * j + c];
            if (x < v[c]) v[c] = x;
            if (x > v[3 + c]) v[3 + c] = x;
        }
        if (R > v[6]) v[6] = R;
    }
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const double o = if_shfl_d(v[c], lane ^ d);
            if (c < 3 ? o < v[c] : o > v[c]) v[c] = o;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 7; ++c) a.box[8 * (int64_t)k + c] = v[c];
        a.box[8 * (int64_t)k + 7] = 0.0;
    }
}

/* test t -> its structure and its two groups (k = gbase[s] + g): row g of a structure with ng groups begins at
   u = g (2 ng - g - 1) / 2; the square root gives the row within one, the two loops settle it (every number below 2^26) */
SASA_D int64_t if_row_first(int64_t g, int64_t ng) { return g * (2 * ng - g - 1) / 2; }
SASA_D void if_decode(const IfaceArgs &a, int t, int &s, int &g, int &h)
{
    int lo = 0, hi = a.n_structs - 1;
    while (lo < hi) { /* the last s with tbase[s] <= t: the structure that holds the test */
        const int mid = (lo + hi + 1) >> 1;
        if (a.tbase[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    s = lo;
    const int64_t ng = a.gbase[s + 1] - a.gbase[s], u = t - a.tbase[s];
    const double w = (double)(2 * ng - 1);
    const double disc = w * w - 8.0 * (double)u;
    int64_t r = (int64_t)((w - sqrt(disc > 0.0 ? disc : 0.0)) * 0.5);
    if (r < 0) r = 0;
    if (r > ng - 2) r = ng - 2;
    while (r + 1 <= ng - 2 && if_row_first(r + 1, ng) <= u) ++r;
    while (r > 0 && if_row_first(r, ng) > u) --r;
    g = (int)r;
    h = (int)(r + 1 + (u - if_row_first(r, ng)));
}

/* boxes closer than the sum of the largest radii on every axis (the file's head: it cannot drop a contact; an empty box is
   at +inf from everything) */
SASA_D bool if_boxes_near(const double *bg, const double *bh)
{
    const double c = bg[6] + bh[6];
    return bh[0] - bg[3] < c && bg[0] - bh[3] < c && bh[1] - bg[4] < c && bg[1] - bh[4] < c && bh[2] - bg[5] < c && bg[2] - bh[5] < c;
}
/* an atom within the other side's box inflated by its r + probe plus that side's largest (the clip) */
SASA_D bool if_atom_near(double x, double y, double z, double R, const double *bo)
{
    const double c = R + bo[6];
    return x - bo[3] < c && bo[0] - x < c && y - bo[4] < c && bo[1] - y < c && z - bo[5] < c && bo[2] - z < c;
}
/* the reference's neighbour test, operand for operand (ref: src/nb.c:487-491; nb_test, sasa_kernels.h) */
SASA_D bool if_contact(double xi, double yi, double zi, double ri, double xq, double yq, double zq, double rq)
{
    const double cut2 = (ri + rq) * (ri + rq);
    const double dx = xq - xi, dy = yq - yi, dz = zq - zi;
    return dx * dx + dy * dy + dz * dz < cut2;
}

/* Step 3, one thread per test t */
SASA_D void iface_candidates(const IfaceArgs &a, int t)
{
    if (t >= a.n_tests) return;
    int s, g, h;
    if_decode(a, t, s, g, h);
    const int64_t kg = a.gbase[s] + g, kh = a.gbase[s] + h;
    if (if_boxes_near(a.box + 8 * kg, a.box + 8 * kh)) a.cand[SASA_ATOMIC_ADD_GLB(a.n_cand, 1)] = t;
}

/* Step 4, ONE WORKGROUP OF IF_B THREADS PER CANDIDATE c (every thread calls this with the same c; the barriers are in uniform
   control flow): side h clipped to g's box into LDS, then every thread takes atoms of g that survive the clip to h's box
   through the survivors of h - from LDS where they all fit, from memory (all of h: the test decides) where they do not.
   A thread that hits raises the flag in LDS; the others see it at their next atom of g and stop. */
SASA_D void iface_contact(const IfaceArgs &a, IfaceLds &m, int c, int tid)
{
    const int t = a.cand[c];
    int s, g, h;
    if_decode(a, t, s, g, h);
    const int64_t kg = a.gbase[s] + g, kh = a.gbase[s] + h;
    const double *bg = a.box + 8 * kg, *bh = a.box + 8 * kh;
    const int64_t g0 = a.gstart[kg], g1 = a.gstart[kg + 1], h0 = a.gstart[kh], h1 = a.gstart[kh + 1];
    if (tid == 0) { m.cnt = 0; m.hit = 0; }
    IF_BARRIER();
    for (int64_t j = h0 + tid; j < h1; j += IF_B) {
        const double x = a.cxyz[3 * j], y = a.cxyz[3 * j + 1], z = a.cxyz[3 * j + 2], R = a.cradii[j] + a.probe;
        if (if_atom_near(x, y, z, R, bg)) {
            const int slot = SASA_ATOMIC_ADD_LDS(&m.cnt, 1);
            if (slot < IF_LDS_ATOMS) { m.at[4 * slot] = x; m.at[4 * slot + 1] = y; m.at[4 * slot + 2] = z; m.at[4 * slot + 3] = R; }
        }
    }
    IF_BARRIER();
    const int nh = m.cnt;
    volatile int *hit = &m.hit;
    for (int64_t i0 = g0; i0 < g1; i0 += IF_B) {
        if (*hit) break;
        const int64_t i = i0 + tid;
        if (i >= g1) continue;
        const double x = a.cxyz[3 * i], y = a.cxyz[3 * i + 1], z = a.cxyz[3 * i + 2], R = a.cradii[i] + a.probe;
        if (!if_atom_near(x, y, z, R, bh)) continue;
        /* (four partners to a trip: their loads are in flight together, the exit is looked at once per trip) */
        bool found = false;
        if (nh <= IF_LDS_ATOMS) {
            int q = 0;
            for (; q + IF_TRIP <= nh && !found; q += IF_TRIP) {
#pragma unroll
                for (int u = 0; u < IF_TRIP; ++u)
                    found |= if_contact(x, y, z, R, m.at[4 * (q + u)], m.at[4 * (q + u) + 1], m.at[4 * (q + u) + 2], m.at[4 * (q + u) + 3]);
            }
            for (; q < nh && !found; ++q) found = if_contact(x, y, z, R, m.at[4 * q], m.at[4 * q + 1], m.at[4 * q + 2], m.at[4 * q + 3]);
        } else {
            int64_t j = h0;
            for (; j + IF_TRIP <= h1 && !found; j += IF_TRIP) {
#pragma unroll
                for (int u = 0; u < IF_TRIP; ++u)
                    found |= if_contact(x, y, z, R, a.cxyz[3 * (j + u)], a.cxyz[3 * (j + u) + 1], a.cxyz[3 * (j + u) + 2], a.cradii[j + u] + a.probe);
            }
            for (; j < h1 && !found; ++j)
                found = if_contact(x, y, z, R, a.cxyz[3 * j], a.cxyz[3 * j + 1], a.cxyz[3 * j + 2], a.cradii[j] + a.probe);
        }
        if (found) *hit = 1;
    }
    IF_BARRIER();
    if (tid == 0) a.flag[t] = m.hit ? 1 : 0;
    IF_BARRIER(); /* (the next candidate of this workgroup clears the flag) */
}

/* Step 6, one thread per pair-structure atom m: its side by binary search, its atom out of the combined batch */
SASA_D void iface_gather(const IfaceArgs &a, int64_t m)
{
    if (m >= a.n_pair_atoms) return;
    int64_t lo = 0, hi = a.n_sides - 1;
    while (lo < hi) { /* the last side that begins at or before m (no side of a pair is empty) */
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.side_off[mid] <= m) lo = mid;
        else hi = mid - 1;
    }
    const int64_t j = a.side_start[lo] + (m - a.side_off[lo]);
    a.pxyz[3 * m] = a.cxyz[3 * j];
    a.pxyz[3 * m + 1] = a.cxyz[3 * j + 1];
    a.pxyz[3 * m + 2] = a.cxyz[3 * j + 2];
    a.pradii[m] = a.cradii[j];
    a.pcomb[m] = (int)j;
    a.pair_atom[m] = a.src[j - a.n_atoms];
}

/* Step 8, one thread per pair-structure atom: its isolated area minus its area in the pair structure */
SASA_D void iface_finish_atom(const IfaceArgs &a, int64_t m)
{
    if (m >= a.n_pair_atoms || !a.pair_buried) return;
    a.pair_buried[m] = a.csasa[a.pcomb[m]] - a.psasa[m];
}
/* ... one thread per row: the six doubles, the isolated totals those of the groups */
SASA_D void iface_finish_row(const IfaceArgs &a, int64_t p)
{
    if (2 * p >= a.n_sides) return;
    const double ig = a.ctot[a.n_structs + a.side_group[2 * p]], ih = a.ctot[a.n_structs + a.side_group[2 * p + 1]];
    const double pg = a.inpair[2 * p], ph = a.inpair[2 * p + 1];
    double *o = a.pair_areas + 6 * p;
    o[0] = ig; o[1] = ih; o[2] = pg; o[3] = ph; o[4] = ig - pg; o[5] = ih - ph;
}

/*
 * PER-RESIDUE TABLES (freesasa_gpu_interface_residues_dev; include/freesasa_gpu.h has the definitions, tests/interface_residues_ref.py
 * restates them in numpy): behind step 8, the residues of every side that lose area, as a compact table whose size only the
 * device knows.  A SEGMENT is a maximal run of consecutive pair-structure atoms of one side whose input atoms lie in one
 * residue; a segment whose buried area exceeds min_buried gets a ROW.
 *
 *   iface_res_head       one thread per pair-structure atom m: its residue (the last r with res_first[r] <= pair_atom[m]: empty
 *                        residues are never found) and its head flag - m starts a side, or the atom before it lies in another
 *                        residue - into hs[m]
 *   scan                 hs[0 .. M] becomes the exclusive prefix sum of the flags in place, hs[M] = K segments (below)
 *   iface_res_first      one thread per m: a head writes seg_first[hs[m]] = m; the last atom also seg_first[K] = M
 *   iface_res_segment    one thread per k < M: segment k < K sums iso (d_iso[pair_atom[m]]) and in_pair (the pair batch's area)
 *                        over its atoms in strict atom order, one addition at a time, as segsum_small does; buried = iso - in_pair;
 *                        ks[k] = buried > min_buried (strict, fp64); k >= K: ks[k] = 0
 *   scan                 ks[0 .. M] likewise, ks[M] = R rows
 *   iface_res_rows       one thread per t <= M: a kept segment t writes its row at ks[t]; side t <= 2 P writes
 *                        res_off[t] = ks[hs[side_off[t]]], the rows before the side's first segment
 *
 * The scan is a plain multi-level block scan of int32 counts in place, IF_B elements to a workgroup (ifr_scan_sums: a block's
 * sum; ifr_scan_apply: a block's exclusive scan plus what precedes the block): the blocks' sums are scanned by the same two
 * phases a level up until one workgroup holds a level, then the levels are applied top down.  Every launch is ordered behind
 * the one before by the stream; no workgroup waits for another inside a launch.  M <= 2^30: four levels at most.  Integer sums:
 * no result depends on launch shape or scheduling.
 */
#define IFR_MAX_LEVELS 5

struct IfaceResArgs {
    int64_t n_pair_atoms, n_sides; /* M, 2 P */
    int n_res;
    const int64_t *side_off;       /* [2 P + 1] */
    const int *pair_atom;          /* [M] */
    const int64_t *res_first;      /* [n_res + 1] */
    const double *iso;             /* [n] the isolated areas of the input atoms (d_iso) */
    const double *psasa;           /* [M] the pair batch's areas */
    double min_buried;
    int *atom_res;                 /* [M] */
    int *hs;                       /* [M + 1] head flags, then their exclusive scan; hs[M] = K */
    int *seg_first;                /* [M + 1] first pair-structure atom of every segment; seg_first[K] = M */
    int *seg_res, *seg_atoms;      /* [M] */
    double *seg_areas;             /* [3 M] iso, in_pair, buried */
    int *ks;                       /* [M + 1] keep flags, then their exclusive scan; ks[M] = R */
    int64_t *res_off;              /* [2 P + 1] */
    int *res_index, *res_atoms;    /* [M] (R used) */
    double *res_areas;             /* [3 M] (3 R used) */
};

/* the sizes of the scan's levels over n elements: cnt[0] = n, cnt[l + 1] = the blocks of level l; returns the top level, the
   first that one workgroup holds (host and device agree on it: the launcher and the emulation both ask here) */
inline int ifr_scan_levels(int64_t n, int64_t *cnt)
{
    int top = 0;
    cnt[0] = n;
    while (cnt[top] > IF_B) { cnt[top + 1] = (cnt[top] + IF_B - 1) / IF_B; ++top; }
    return top;
}
/* the ints the levels above the first need: a level begins where the one below it ends */
inline int64_t ifr_scan_scratch(int64_t n)
{
    int64_t cnt[IFR_MAX_LEVELS], s = 0;
    const int top = ifr_scan_levels(n, cnt);
    for (int l = 1; l <= top; ++l) s += cnt[l];
    return s;
}

/* thread tid of block `block` over the n ints of `in`: the block's sum -> sums[block] (part: [IF_B] ints of LDS; a barrier
   between the two phases) */
SASA_D void ifr_scan_sums_phase0(const int *in, int64_t n, int *part, int64_t block, int tid)
{
    const int64_t i = block * IF_B + tid;
    part[tid] = i < n ? in[i] : 0;
}
SASA_D void ifr_scan_sums_phase1(const int *part, int *sums, int64_t block, int tid)
{
    if (tid != 0) return;
    int s = 0;
    for (int t = 0; t < IF_B; ++t) s += part[t];
    sums[block] = s;
}
/* ... the block's exclusive scan in place, plus base[block] (null: 0 - the top level, whose sum goes to *total); three phases */
SASA_D void ifr_scan_apply_phase0(const int *a, int64_t n, int *part, int64_t block, int tid) { ifr_scan_sums_phase0(a, n, part, block, tid); }
SASA_D void ifr_scan_apply_phase1(int *part, int *total, int tid)
{
    if (tid != 0) return;
    int s = 0;
    for (int t = 0; t < IF_B; ++t) { const int v = part[t]; part[t] = s; s += v; }
    if (total) *total = s;
}
SASA_D void ifr_scan_apply_phase2(int *a, int64_t n, const int *part, const int *base, int64_t block, int tid)
{
    const int64_t i = block * IF_B + tid;
    if (i < n) a[i] = (base ? base[block] : 0) + part[tid];
}

/* the residue of input atom i: the last r with res_first[r] <= i (res_first[0] = 0 <= i < res_first[n_res]) */
SASA_D int ifr_residue(const IfaceResArgs &a, int64_t i)
{
    int lo = 0, hi = a.n_res - 1;
    while (lo < hi) {
        const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
        if (a.res_first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
SASA_D void iface_res_head(const IfaceResArgs &a, int64_t m)
{
    if (m >= a.n_pair_atoms) return;
    const int r = ifr_residue(a, a.pair_atom[m]);
    a.atom_res[m] = r;
    int64_t lo = 0, hi = a.n_sides - 1;
    while (lo < hi) { /* the last side that begins at or before m (iface_gather) */
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.side_off[mid] <= m) lo = mid;
        else hi = mid - 1;
    }
    a.hs[m] = a.side_off[lo] == m || ifr_residue(a, a.pair_atom[m - 1]) != r ? 1 : 0;
}
SASA_D void iface_res_first(const IfaceResArgs &a, int64_t m)
{
    if (m >= a.n_pair_atoms) return;
    const int k = a.hs[m], next = a.hs[m + 1];
    if (next != k) a.seg_first[k] = (int)m;
    if (m == a.n_pair_atoms - 1) a.seg_first[next] = (int)a.n_pair_atoms;
}
SASA_D void iface_res_segment(const IfaceResArgs &a, int64_t k)
{
    if (k >= a.n_pair_atoms) return;
    if (k >= a.hs[a.n_pair_atoms]) { a.ks[k] = 0; return; }
    const int b = a.seg_first[k], e = a.seg_first[k + 1];
    double iso = 0, inp = 0;
    for (int m = b; m < e; ++m) { iso += a.iso[a.pair_atom[m]]; inp += a.psasa[m]; }
    const double buried = iso - inp;
    a.seg_res[k] = a.atom_res[b];
    a.seg_atoms[k] = e - b;
    a.seg_areas[3 * k] = iso; a.seg_areas[3 * k + 1] = inp; a.seg_areas[3 * k + 2] = buried;
    a.ks[k] = buried > a.min_buried ? 1 : 0;
}
SASA_D void iface_res_rows(const IfaceResArgs &a, int64_t t)
{
    if (t > a.n_pair_atoms) return;
    if (t <= a.n_sides) a.res_off[t] = a.ks[a.hs[a.side_off[t]]];
    if (t >= a.hs[a.n_pair_atoms]) return;
    const int j = a.ks[t];
    if (a.ks[t + 1] == j) return;
    a.res_index[j] = a.seg_res[t];
    a.res_atoms[j] = a.seg_atoms[t];
    a.res_areas[3 * (int64_t)j] = a.seg_areas[3 * t]; a.res_areas[3 * (int64_t)j + 1] = a.seg_areas[3 * t + 1];
    a.res_areas[3 * (int64_t)j + 2] = a.seg_areas[3 * t + 2];
}

} /* namespace sasa */

#endif
