/*
 * dots_kernels.h — phase functions of the SURFACE DOTS (freesasa_gpu_dots_count_dev / freesasa_gpu_dots_expand_dev and the
 * entries built on them, include/freesasa_gpu.h): the exposed Shrake-Rupley test points of every atom as points in space -
 * what `gmx sasa -q` writes - made from the EXPOSURE MASKS the tile kernel's store phase keeps (sr_caps_store<SR_STORE_MASK>,
 * sr_caps.h).  The mask is the compact, lossless form: 16 bytes per atom; counts, dots, and anything else made of the
 * exposed points follow from it without the engine.
 *
 * The definitions (the tests pin them; tests/dots_ref.py restates them in numpy).  Probe p, the N = n_points unit test
 * points u_k of freesasa_gpu_test_points(N), R_i = r_i + p:
 *   mask        uint32 [n_atoms][SR_CAP_WORDS = 4], atoms in the caller's order: bit k & 31 of word k >> 5 of atom i is SET
 *               iff point k of atom i is EXPOSED; bits k >= N are 0; popcount(mask_i) == counts[i].
 *   dot_first   int64 [n_atoms + 1]: the exclusive prefix sum of popcount(mask_i & full), full = the N bits that exist -
 *               taken from the masks themselves, so that scan and expansion agree by construction.  D = dot_first[n_atoms];
 *               the dots of structure s are dot_first[offsets[s]] .. dot_first[offsets[s + 1]].
 *   dots        for atom i ascending and within it for exposed k ascending, one dot at slot dot_first[i] + rank:
 *               dot_xyz[3 slot ..] fp64, per component t = u_k * R_i; t += x_i - the engine's own test point (the one its
 *               exposure test is made with: sr_caps_test), each operation rounded on its own (the build has -ffp-contract=off);
 *               optional dot_atom[slot] = i and dot_point[slot] = k (int32).
 *               The outward normal of a dot is u_k, the area it stands for 4 pi R_i^2 / N: no array is needed for either.
 *
 *   dots_count_phase0 / 1      (k_dots_block_sums) one workgroup of DOTS_SCAN_T threads per DOTS_SCAN_B atoms: every thread
 *                              the popcount of its DOTS_SCAN_PER consecutive atoms, thread 0 their sum -> bsum[block]
 *   dots_scan_phase0 / 1 / 2   (k_dots_scan_blocks) ONE workgroup of DOTS_SCAN_T threads: every thread the sum of its run of
 *                              consecutive block sums, thread 0 the exclusive scan of the DOTS_SCAN_T run sums and D, every
 *                              thread the exclusive scan of its run in place
 *   dots_first_phase0 / 1 / 2  (k_dots_first) the first kernel's shape again: the popcounts, thread 0 their exclusive scan,
 *                              every thread dot_first of its atoms = bsum[block] + its place in the block + what precedes
 * Three plain launches, each ordered behind the one before by the stream; no workgroup waits for another inside a launch
 * (no look-back, no flags, no epochs).  Everything that can exceed 2^31 is int64: 2^24 atoms with 128 exposed points have.
 *
 *   dots_expand                (k_dots_expand) one lane per (atom, point) pair of the flattened n_atoms x N index space,
 *                              DOTS_EXPAND_U pairs a thread, a workgroup's width apart: a
 *                              lane whose bit is set takes rank = popcount of the atom's mask bits below k and writes its dot
 *                              at dot_first[i] + rank.  Consecutive exposed lanes of a wave write consecutive slots, across
 *                              atom boundaries too: a wave's stores form one contiguous run of 24-byte dots (and of 4-byte
 *                              indices).  A lane writes only if its slot is < dot_first[i + 1] and < capacity, and stray
 *                              bits >= N are masked off: bad input gives wrong dots, never a write outside the arrays.
 *
 * Written like vol_kernels.h: every function is one thread's share of a phase, so that a -DSASA_EMU build can drive them on
 * the CPU (tests/emu/emu_dots.cpp); the __global__ wrappers and kl_dots_* launchers are in gpu_kernels.hip, the host side in
 * gpu_dots.hip.
 */
#ifndef FREESASA_AMD_DOTS_KERNELS_H
#define FREESASA_AMD_DOTS_KERNELS_H

#include "sasa_kernels.h"

namespace sasa {

#define DOTS_SCAN_T 256                            /* threads of a workgroup of the scan's kernels */
#define DOTS_SCAN_PER 4                            /* consecutive atoms per thread: 64 bytes of masks */
#define DOTS_SCAN_B (DOTS_SCAN_T * DOTS_SCAN_PER)  /* atoms per block */
#define DOTS_EXPAND_B 256                          /* threads per workgroup of dots_expand */
#define DOTS_EXPAND_U 4                            /* pairs per lane, DOTS_EXPAND_B apart: their loads are in flight together */

struct DotsArgs {
    const unsigned *masks;  /* [n_atoms][SR_CAP_WORDS] */
    int64_t n_atoms;
    int n_points;
    int64_t n_blocks;       /* (n_atoms + DOTS_SCAN_B - 1) / DOTS_SCAN_B */
    int64_t *bsum;          /* [n_blocks]: the blocks' sums, then (dots_scan_phase2) what precedes every block */
    int64_t *dot_first;     /* [n_atoms + 1] */
    /* the expansion */
    const double *xyz;      /* [3 n_atoms] */
    const double *radii;    /* [n_atoms] */
    const double *unit_pts; /* [3 n_points] */
    double probe;
    double inv_points;      /* 1.0 / n_points (dots_args_expand): the lane's atom is its pair index times this, put right by one step */
    int64_t capacity;       /* dots the output arrays hold */
    double *dot_xyz;        /* [3 capacity] */
    int *dot_atom;          /* [capacity] or null */
    int *dot_point;         /* [capacity] or null */
};

/* exposed points of atom i: the bits that exist */
SASA_D int dots_popcount(const DotsArgs &a, int64_t i)
{
    const unsigned *m = a.masks + SR_CAP_WORDS * i;
    int c = 0;
    for (int w = 0; w < SR_CAP_WORDS; ++w) c += __builtin_popcount(m[w] & sr_cap_full_word(a.n_points, w));
    return c;
}
/* thread tid of block `block`: the sum over its atoms (part: [DOTS_SCAN_T] ints of LDS) */
SASA_D void dots_count_phase0(const DotsArgs &a, int *part, int64_t block, int tid)
{
    const int64_t b = block * DOTS_SCAN_B + (int64_t)tid * DOTS_SCAN_PER;
    int c = 0;
    for (int j = 0; j < DOTS_SCAN_PER; ++j)
        if (b + j < a.n_atoms) c += dots_popcount(a, b + j);
    part[tid] = c;
}
SASA_D void dots_count_phase1(const DotsArgs &a, const int *part, int64_t block, int tid)
{
    if (tid != 0) return;
    int64_t s = 0;
    for (int t = 0; t < DOTS_SCAN_T; ++t) s += part[t];
    a.bsum[block] = s;
}

/* ONE workgroup: thread tid owns the block sums [tid * per, (tid + 1) * per) (part: [DOTS_SCAN_T] int64 of LDS) */
SASA_D int64_t dots_scan_run(const DotsArgs &a) { return (a.n_blocks + DOTS_SCAN_T - 1) / DOTS_SCAN_T; }
SASA_D void dots_scan_phase0(const DotsArgs &a, int64_t *part, int tid)
{
    const int64_t per = dots_scan_run(a), b = tid * per, e = b + per < a.n_blocks ? b + per : a.n_blocks;
    int64_t s = 0;
    for (int64_t k = b; k < e; ++k) s += a.bsum[k];
    part[tid] = s;
}
SASA_D void dots_scan_phase1(const DotsArgs &a, int64_t *part, int tid)
{
    if (tid != 0) return;
    int64_t s = 0;
    for (int t = 0; t < DOTS_SCAN_T; ++t) { const int64_t v = part[t]; part[t] = s; s += v; }
    a.dot_first[a.n_atoms] = s; /* D */
}
SASA_D void dots_scan_phase2(const DotsArgs &a, const int64_t *part, int tid)
{
    const int64_t per = dots_scan_run(a), b = tid * per, e = b + per < a.n_blocks ? b + per : a.n_blocks;
    int64_t s = part[tid];
    for (int64_t k = b; k < e; ++k) { const int64_t v = a.bsum[k]; a.bsum[k] = s; s += v; }
}

/* the first kernel's shape again: part[tid] the thread's sum, then what precedes the thread in its block */
SASA_D void dots_first_phase0(const DotsArgs &a, int *part, int64_t block, int tid) { dots_count_phase0(a, part, block, tid); }
SASA_D void dots_first_phase1(const DotsArgs &a, int *part, int64_t block, int tid)
{
    (void)a; (void)block;
    if (tid != 0) return;
    int s = 0;
    for (int t = 0; t < DOTS_SCAN_T; ++t) { const int v = part[t]; part[t] = s; s += v; }
}
SASA_D void dots_first_phase2(const DotsArgs &a, const int *part, int64_t block, int tid)
{
    const int64_t b = block * DOTS_SCAN_B + (int64_t)tid * DOTS_SCAN_PER;
    int64_t s = a.bsum[block] + part[tid];
    for (int j = 0; j < DOTS_SCAN_PER; ++j)
        if (b + j < a.n_atoms) { a.dot_first[b + j] = s; s += dots_popcount(a, b + j); }
}

/* atom and point of pair g = i * n_points + k, 0 <= g < 2^30 n_points, without the 64-bit division - which was most of the
   expansion's time: a billion lanes of ~200 instructions on the coil batch, 6.26 ms where the bytes written need 0.6.  g < 2^37
   and i < 2^30 are exact in fp64, the product with 1 / n_points is off by less than one, and one step either way puts quotient
   and remainder right (tests/emu/dots_check walks the boundaries of every n_points). */
SASA_D void dots_pair(int64_t g, int n_points, double inv_points, int64_t &i, int &k)
{
    i = (int64_t)(int)((double)g * inv_points);
    k = (int)(g - i * n_points);
    if (k < 0) { --i; k += n_points; }
    else if (k >= n_points) { ++i; k -= n_points; }
}

/* One lane per (atom, point) pair g of the batch, in two steps: dots_expand_load reads everything the pair needs - none of its
   loads depends on another, and a lane without an exposed point reads what an exposed one reads, at places that exist - and
   makes the dot in registers; dots_expand_store writes it if there is one.  A lane of k_dots_expand runs the loads of
   DOTS_EXPAND_U pairs, 256 apart, before the first store: the kernel is bound by the latency of its loads (86 % of the coil
   batch's pairs are covered points, whose lanes have nothing to write), and with a pair per lane and the loads behind the test of
   the bit it took 6.2 ms on the coil batch where the bytes written need 0.6 (profiles/dots_bench.md). */
struct DotsLane {
    int64_t slot; /* < 0: nothing to write */
    double t[3];
    int i, k;
};
SASA_D void dots_expand_load(const DotsArgs &a, int64_t g, DotsLane &L)
{
    const int64_t pairs = a.n_atoms * a.n_points;
    const bool in = g < pairs;
    int64_t i;
    int k;
    dots_pair(in ? g : pairs - 1, a.n_points, a.inv_points, i, k);
    const SrMaskWords m = *(const SrMaskWords *)(a.masks + SR_CAP_WORDS * i);
    const int64_t first = a.dot_first[i], next = a.dot_first[i + 1];
    const double R = a.radii[i] + a.probe;
    const double *u = a.unit_pts + 3 * k, *x = a.xyz + 3 * i;
    for (int c = 0; c < 3; ++c) {
        double t = u[c] * R; /* (the point in two rounded steps, as the exposure test makes it) */
        t += x[c];
        L.t[c] = t;
    }
    const int kw = k >> 5;
    unsigned word = 0;
    int rank = 0;
    for (int w = 0; w < SR_CAP_WORDS; ++w) {
        word = w == kw ? m.w[w] & sr_cap_full_word(a.n_points, w) : word;
        rank += w < kw ? __builtin_popcount(m.w[w]) : 0; /* (whole words below k: all their bits exist) */
    }
    rank += __builtin_popcount(word & ((1u << (k & 31)) - 1u));
    const int64_t slot = first + rank;
    bool write = (int)in & (int)((word >> (k & 31)) & 1u) & (int)(slot >= 0) & (int)(slot < next) & (int)(slot < a.capacity); /* (no short cuts: see below) */
    /* (always true, capacity being >= 0 - but not to the compiler, which otherwise moves the loads of the point and the centre
       behind the test of the bit, into a branch of their own with a wait of its own for every pair: a second trip to memory, and
       the DOTS_EXPAND_U pairs of a lane one after the other) */
    write &= (L.t[0] == L.t[0]) | (L.t[1] == L.t[1]) | (L.t[2] == L.t[2]) | (a.capacity >= 0);
    L.slot = write ? slot : -1;
    L.i = (int)i; L.k = k;
}
SASA_D void dots_expand_store(const DotsArgs &a, const DotsLane &L)
{
    if (L.slot < 0) return;
    double *d = a.dot_xyz + 3 * L.slot;
    d[0] = L.t[0]; d[1] = L.t[1]; d[2] = L.t[2];
    if (a.dot_atom) a.dot_atom[L.slot] = L.i;
    if (a.dot_point) a.dot_point[L.slot] = L.k;
}
/* thread tid of workgroup `block`: pairs (block DOTS_EXPAND_U + u) DOTS_EXPAND_B + tid, u = 0 .. DOTS_EXPAND_U - 1 */
SASA_D void dots_expand(const DotsArgs &a, int64_t block, int tid)
{
    DotsLane L[DOTS_EXPAND_U];
#pragma unroll
    for (int u = 0; u < DOTS_EXPAND_U; ++u) dots_expand_load(a, (block * DOTS_EXPAND_U + u) * DOTS_EXPAND_B + tid, L[u]);
#pragma unroll
    for (int u = 0; u < DOTS_EXPAND_U; ++u) dots_expand_store(a, L[u]);
}

} /* namespace sasa */

#endif
