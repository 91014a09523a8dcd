/* TESTS ONLY: the phase functions of the surface dots (freesasa_amd/csrc/dots_kernels.h) driven on the CPU as gpu_kernels.hip
 * launches them: the scan in its three launches - dots_count_phase0 / 1 one workgroup of DOTS_SCAN_T threads per DOTS_SCAN_B
 * atoms, dots_scan_phase0 / 1 / 2 ONE workgroup, dots_first_phase0 / 1 / 2 the first launch's grid again (a barrier between two
 * phases is the end of the loop over the threads; the end of a launch the end of the loop over the workgroups) - and
 * dots_expand thread by thread of k_dots_expand's grid (DOTS_EXPAND_U pairs each), idle threads included.
 * And the Shrake-Rupley tile kernel's phases with the store phase of k_sr_tile_mask: emu.cpp, as it is, compiled into this
 * library once more with its call of sr_caps_store sent through a hook that runs sr_caps_store<SR_STORE_MASK> while a place
 * for the masks is set (emu_set_sr_masks) - launch_sr picks the kernel by that pointer in the same way.
 * With -DDOTS_CHECK_MAIN: a stand-alone program (tests/emu/dots_check, built with AddressSanitizer + UBSan) that drives scan
 * and expansion over the shapes of tests/test_dots.py against a plain loop, the outputs in heap blocks of their exact size:
 * one line per case.
 * Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../freesasa_amd/csrc/dots_kernels.h"

#ifndef DOTS_CHECK_MAIN
static unsigned *emu_sr_masks = nullptr; /* [n][4]: where the next emu_run_batch calls of THIS library keep the masks */
extern "C" void emu_set_sr_masks(unsigned *masks) { emu_sr_masks = masks; }
static inline void emu_store_hook(const sasa::TileArgs &a, sasa::TileMem &m, int tile, int tid)
{
    if (emu_sr_masks) sasa::sr_caps_store<sasa::SR_STORE_MASK>(a, m, tile, tid, nullptr, emu_sr_masks);
    else sasa::sr_caps_store<sasa::SR_STORE_NONE>(a, m, tile, tid);
}
#define sr_caps_store(a, m, tile, tid) emu_store_hook(a, m, tile, tid) /* (emu.cpp's one call; the templates above are spelled with <>) */
#include "emu.cpp"
#undef sr_caps_store
#else
namespace sasa { long long sr_caps_count_emu[4]; }
#endif

using namespace sasa;

extern "C" void emu_dots_shape(int *atoms_per_block, int *threads) { *atoms_per_block = DOTS_SCAN_B; *threads = DOTS_SCAN_T; }

/* masks [n_atoms][4] -> dot_first [n_atoms + 1] (the last: D).  0, -1 on a bad argument. */
extern "C" int emu_dots_count(const unsigned *masks, long long n_atoms, int n_points, int64_t *dot_first)
{
    if (!masks || n_atoms <= 0 || n_points <= 0 || n_points > SR_CAP_POINTS_MAX || !dot_first) return -1;
    DotsArgs a;
    memset(&a, 0, sizeof a);
    a.masks = masks; a.n_atoms = n_atoms; a.n_points = n_points; a.n_blocks = (n_atoms + DOTS_SCAN_B - 1) / DOTS_SCAN_B;
    std::vector<int64_t> bsum((size_t)a.n_blocks), part64(DOTS_SCAN_T);
    std::vector<int> part(DOTS_SCAN_T);
    a.bsum = bsum.data(); a.dot_first = dot_first;
    for (int64_t b = 0; b < a.n_blocks; ++b) { /* k_dots_block_sums */
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_count_phase0(a, part.data(), b, tid);
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_count_phase1(a, part.data(), b, tid);
    }
    for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_scan_phase0(a, part64.data(), tid); /* k_dots_scan_blocks */
    for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_scan_phase1(a, part64.data(), tid);
    for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_scan_phase2(a, part64.data(), tid);
    for (int64_t b = 0; b < a.n_blocks; ++b) { /* k_dots_first */
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_first_phase0(a, part.data(), b, tid);
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_first_phase1(a, part.data(), b, tid);
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_first_phase2(a, part.data(), b, tid);
    }
    return 0;
}

/* the dots of the masks into arrays that hold `capacity` of them (dot_atom, dot_point may be null).  0, -1 on a bad argument. */
extern "C" int emu_dots_expand(const double *xyz, const double *radii, long long n_atoms, double probe, int n_points, const double *unit,
                               const unsigned *masks, const int64_t *dot_first, long long capacity, double *dot_xyz, int *dot_atom, int *dot_point)
{
    if (!xyz || !radii || n_atoms <= 0 || n_points <= 0 || n_points > SR_CAP_POINTS_MAX || !unit || !masks || !dot_first || capacity < 0 || !dot_xyz) return -1;
    DotsArgs a;
    memset(&a, 0, sizeof a);
    a.masks = masks; a.n_atoms = n_atoms; a.n_points = n_points; a.dot_first = const_cast<int64_t *>(dot_first);
    a.xyz = xyz; a.radii = radii; a.unit_pts = unit; a.probe = probe; a.inv_points = 1.0 / n_points; a.capacity = capacity;
    a.dot_xyz = dot_xyz; a.dot_atom = dot_atom; a.dot_point = dot_point;
    const int64_t pairs = n_atoms * n_points, per_wg = (int64_t)DOTS_EXPAND_B * DOTS_EXPAND_U, grid = (pairs + per_wg - 1) / per_wg;
    for (int64_t b = 0; b < grid; ++b)
        for (int tid = 0; tid < DOTS_EXPAND_B; ++tid) dots_expand(a, b, tid);
    return 0;
}

/* dots_pair against the integer division at the atoms' boundaries: pairs i n_points - 1, i n_points, i n_points + 1 and the last
   point of atom i, for i = 0 .. 2^30 in steps (all of them below 10^5), every n_points 1 .. 128.  Returns the number of misses. */
extern "C" long long emu_dots_pair_misses(void)
{
    long long bad = 0;
    for (int N = 1; N <= SR_CAP_POINTS_MAX; ++N) {
        const double inv = 1.0 / N;
        const int64_t end = ((int64_t)1 << 30) * N;
        auto miss = [&](int64_t g) {
            if (g < 0 || g >= end) return 0;
            int64_t i; int k;
            dots_pair(g, N, inv, i, k);
            return i != g / N || k != (int)(g % N) ? 1 : 0;
        };
        for (int64_t i = 0; i <= (int64_t)1 << 30; i += i < 100000 ? 1 : 9973)
            for (int d = -1; d <= 1; ++d) bad += miss(i * N + d) + miss(i * N + N - 1 + d);
        for (int64_t g = end - 3 * N; g < end; ++g) bad += miss(g);
    }
    return bad;
}

#ifdef DOTS_CHECK_MAIN
/* a small generator of its own: the cases are the program's, whatever the C library */
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static unsigned full_word(int np, int w) { const int left = np - 32 * w; return left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (1u << left) - 1u; }

/* kind 0: random bits, all-zero and all-set atoms among them; 1: all zero; 2: the same as 0 with stray bits at and above n_points */
static void make_masks(std::vector<unsigned> &m, long long n, int np, int kind)
{
    m.assign((size_t)(4 * n), 0u);
    for (long long i = 0; i < n && kind != 1; ++i) {
        const uint32_t how = rnd() % 6;
        for (int w = 0; w < 4; ++w) {
            const unsigned bits = how == 0 ? 0u : how == 1 ? 0xffffffffu : (rnd() & rnd()) | (rnd() << 16);
            m[(size_t)(4 * i + w)] = kind == 2 ? bits | (rnd() & ~full_word(np, w)) : bits & full_word(np, w);
        }
    }
}

static int check_scan(const char *name, long long n, int np, int kind)
{
    std::vector<unsigned> m;
    make_masks(m, n, np, kind);
    int64_t *first = new int64_t[(size_t)n + 1]; /* (its exact size: a write behind it is the sanitizer's to find) */
    int bad = emu_dots_count(m.data(), n, np, first);
    int64_t s = 0;
    for (long long i = 0; i < n && !bad; ++i) {
        if (first[i] != s) bad = 1;
        for (int w = 0; w < 4; ++w) s += __builtin_popcount(m[(size_t)(4 * i + w)] & full_word(np, w));
    }
    if (!bad && first[n] != s) bad = 1;
    delete[] first;
    printf("%s %s\n", name, bad ? "FAILED" : "ok");
    return bad;
}

static int check_expand(const char *name, long long n, int np, int kind, long long short_by)
{
    std::vector<unsigned> m;
    make_masks(m, n, np, kind);
    std::vector<double> xyz((size_t)(3 * n)), radii((size_t)n), unit((size_t)(3 * np));
    for (double &v : xyz) v = (double)(rnd() % 200000) / 1000.0 - 100.0;
    for (double &v : radii) v = 1.0 + (double)(rnd() % 1000) / 1000.0;
    for (double &v : unit) v = (double)(rnd() % 2001) / 1000.0 - 1.0; /* (any numbers: the arithmetic is the same) */
    std::vector<int64_t> first((size_t)n + 1);
    if (emu_dots_count(m.data(), n, np, first.data())) { printf("%s FAILED\n", name); return 1; }
    const long long D = first[(size_t)n], cap = D > short_by ? D - short_by : 0;
    double *dx = new double[(size_t)(3 * cap) + 1]; /* (+1: new[0] is not to be dereferenced; the last element is never written) */
    int *da = new int[(size_t)cap + 1], *dp = new int[(size_t)cap + 1];
    dx[3 * cap] = -7.0; da[cap] = dp[cap] = -7;
    int bad = emu_dots_expand(xyz.data(), radii.data(), n, 1.4, np, unit.data(), m.data(), first.data(), cap, dx, da, dp);
    long long slot = 0;
    for (long long i = 0; i < n && !bad; ++i)
        for (int k = 0; k < np && !bad; ++k) {
            if (!((m[(size_t)(4 * i + (k >> 5))] >> (k & 31)) & 1u)) continue;
            if (slot < cap) {
                const double R = radii[(size_t)i] + 1.4;
                for (int c = 0; c < 3; ++c) {
                    double t = unit[(size_t)(3 * k + c)] * R;
                    t += xyz[(size_t)(3 * i + c)];
                    if (dx[3 * slot + c] != t) bad = 1;
                }
                if (da[slot] != (int)i || dp[slot] != k) bad = 1;
            }
            ++slot;
        }
    if (!bad && (slot != D || dx[3 * cap] != -7.0 || da[cap] != -7 || dp[cap] != -7)) bad = 1;
    delete[] dx; delete[] da; delete[] dp;
    printf("%s %s\n", name, bad ? "FAILED" : "ok");
    return bad;
}

int main()
{
    const long long B = DOTS_SCAN_B, T = DOTS_SCAN_T;
    const long long sizes[6] = {1, B - 1, B, B + 1, 2 * B + 3, B * T + 1};
    int bad = 0;
    char name[64];
    { const long long m = emu_dots_pair_misses(); printf("pair-index %s\n", m ? "FAILED" : "ok"); bad |= m != 0; }
    for (int k = 0; k < 6; ++k) {
        snprintf(name, sizeof name, "scan-%lld", sizes[k]);
        bad |= check_scan(name, sizes[k], 100, 0);
    }
    bad |= check_scan("scan-all-zero", 2 * B + 3, 100, 1);
    bad |= check_scan("scan-stray-bits", B + 1, 33, 2);
    const int points[4] = {1, 33, 100, 128};
    for (int k = 0; k < 4; ++k) {
        snprintf(name, sizeof name, "expand-%d", points[k]);
        bad |= check_expand(name, 700, points[k], 0, 0);
    }
    bad |= check_expand("expand-all-zero", 300, 100, 1, 0);
    bad |= check_expand("expand-stray-bits", 700, 33, 2, 0);
    bad |= check_expand("expand-capacity-short-by-3", 700, 100, 0, 3);
    return bad;
}
#endif
