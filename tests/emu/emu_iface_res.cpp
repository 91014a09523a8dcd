/* TESTS ONLY: the phase functions of the per-residue interface tables (freesasa_amd/csrc/iface_kernels.h, IfaceResArgs) driven on
 * the CPU as gpu_kernels.hip launches them: every kernel a loop over its grid's workgroups of IF_B threads, idle threads
 * included, and inside a workgroup the phases one after the other where the kernel has a barrier between them (no phase
 * function holds a barrier of its own, so no fibers are needed).  The scan goes through ifr_scan_levels like kl_iface_res_scan.
 * With -DIFACE_RES_CHECK_MAIN: a stand-alone program (tests/emu/iface_res_check, built with AddressSanitizer + UBSan) that drives
 * the same phases over generated pair tables against a plain loop, every array a heap block of its exact size: one line per
 * case.
 * Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../freesasa_amd/csrc/iface_kernels.h"

using namespace sasa;

static void run_scan_sums(const int *in, int64_t n, int *sums, int64_t blocks)
{
    int part[IF_B];
    for (int64_t b = 0; b < blocks; ++b) {
        for (int t = 0; t < IF_B; ++t) ifr_scan_sums_phase0(in, n, part, b, t);
        for (int t = 0; t < IF_B; ++t) ifr_scan_sums_phase1(part, sums, b, t);
    }
}
static void run_scan_apply(int *a, int64_t n, const int *base, int *total, int64_t blocks)
{
    int part[IF_B];
    for (int64_t b = 0; b < blocks; ++b) {
        for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase0(a, n, part, b, t);
        for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase1(part, total, t);
        for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase2(a, n, part, base, b, t);
    }
}
/* kl_iface_res_scan: a [n + 1] in place; scratch of its exact size.  Returns the top level. */
static int scan_in_place(int *a, int64_t n)
{
    int64_t cnt[IFR_MAX_LEVELS];
    int *lvl[IFR_MAX_LEVELS];
    const int top = ifr_scan_levels(n, cnt);
    int *scratch = new int[(size_t)ifr_scan_scratch(n) + 1];
    lvl[0] = a;
    for (int l = 1; l <= top; ++l) lvl[l] = l == 1 ? scratch : lvl[l - 1] + cnt[l - 1];
    for (int l = 0; l < top; ++l) run_scan_sums(lvl[l], cnt[l], lvl[l + 1], cnt[l + 1]);
    run_scan_apply(lvl[top], cnt[top], nullptr, a + n, 1);
    for (int l = top - 1; l >= 0; --l) run_scan_apply(lvl[l], cnt[l], lvl[l + 1], nullptr, cnt[l + 1]);
    delete[] scratch;
    return top;
}

extern "C" void emu_iface_res_shape(int *threads, int *max_levels) { *threads = IF_B; *max_levels = IFR_MAX_LEVELS; }

/* a [n + 1]: the counts in a[0 .. n - 1] become their exclusive prefix sums, a[n] the total.  Returns the levels above the first. */
extern "C" int emu_iface_res_scan(int *a, long long n)
{
    if (!a || n < 0) return -1;
    return scan_in_place(a, n);
}

/* The stage behind the interface pipeline, from the pair table (side_off [n_sides + 1], pair_atom [M]), res_first [n_res + 1],
 * the isolated areas iso [n] and the pair batch's areas psasa [M]: heads [M] and seg_first [M + 1] (K + 1 used) as the first scan
 * leaves them, then - when res_cap holds the R rows - res_off [n_sides + 1], res_index / res_atoms [res_cap], res_areas
 * [3 res_cap].  *n_segs_out: K, *n_rows_out: R.  Returns R; -1 on a bad argument, -2 when res_cap is too small (none of the four
 * row arrays written). */
extern "C" long long emu_iface_res_table(const int64_t *side_off, long long n_sides, const int32_t *pair_atom, long long M,
                                         const int64_t *res_first, int n_res, const double *iso, const double *psasa, double min_buried,
                                         long long res_cap, unsigned char *heads, int64_t *seg_first, long long *n_segs_out,
                                         long long *n_rows_out, int64_t *res_off, int32_t *res_index, int32_t *res_atoms, double *res_areas)
{
    if (!side_off || n_sides <= 0 || !pair_atom || M <= 0 || !res_first || n_res <= 0 || !iso || !psasa || !heads || !seg_first ||
        !n_segs_out || !n_rows_out || !res_off || !res_index || !res_atoms || !res_areas || side_off[n_sides] != M)
        return -1;
    const size_t m = (size_t)M;
    int *atom_res = new int[m], *hs = new int[m + 1], *sf = new int[m + 1], *seg_res = new int[m], *seg_atoms = new int[m], *ks = new int[m + 1];
    double *seg_areas = new double[3 * m], *t_areas = new double[3 * m];
    int64_t *t_off = new int64_t[(size_t)n_sides + 1];
    int *t_index = new int[m], *t_atoms = new int[m];
    IfaceResArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = M; a.n_sides = n_sides; a.n_res = n_res;
    a.side_off = side_off; a.pair_atom = pair_atom; a.res_first = res_first; a.iso = iso; a.psasa = psasa; a.min_buried = min_buried;
    a.atom_res = atom_res; a.hs = hs; a.seg_first = sf; a.seg_res = seg_res; a.seg_atoms = seg_atoms; a.seg_areas = seg_areas; a.ks = ks;
    a.res_off = t_off; a.res_index = t_index; a.res_atoms = t_atoms; a.res_areas = t_areas;
    const int64_t grid = (M + IF_B - 1) / IF_B * IF_B, grid1 = (M + 1 + IF_B - 1) / IF_B * IF_B;
    for (int64_t i = 0; i < grid; ++i) iface_res_head(a, i);
    for (int64_t i = 0; i < M; ++i) heads[i] = (unsigned char)hs[i];
    scan_in_place(hs, M);
    const int64_t K = hs[M];
    for (int64_t i = 0; i < grid; ++i) iface_res_first(a, i);
    for (int64_t i = 0; i <= K; ++i) seg_first[i] = sf[i];
    for (int64_t i = 0; i < grid; ++i) iface_res_segment(a, i);
    scan_in_place(ks, M);
    const int64_t R = ks[M];
    for (int64_t i = 0; i < grid1; ++i) iface_res_rows(a, i);
    *n_segs_out = K; *n_rows_out = R;
    if (R <= res_cap) {
        memcpy(res_off, t_off, 8 * ((size_t)n_sides + 1));
        if (R > 0) {
            memcpy(res_index, t_index, 4 * (size_t)R); memcpy(res_atoms, t_atoms, 4 * (size_t)R); memcpy(res_areas, t_areas, 24 * (size_t)R);
        }
    }
    delete[] atom_res; delete[] hs; delete[] sf; delete[] seg_res; delete[] seg_atoms; delete[] ks; delete[] seg_areas; delete[] t_areas;
    delete[] t_off; delete[] t_index; delete[] t_atoms;
    return R <= res_cap ? R : -2;
}

#ifdef IFACE_RES_CHECK_MAIN
/* a small generator of its own: the cases are the program's, whatever the C library */
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() % 1000001) / 1000000.0; }

static int check_scan(long long n)
{
    int *a = new int[(size_t)n + 1]; /* (its exact size: a write behind it is the sanitizer's to find) */
    std::vector<int> in((size_t)n);
    for (long long i = 0; i < n; ++i) a[i] = in[(size_t)i] = (int)(rnd() % 3);
    a[n] = -7;
    const int top = emu_iface_res_scan(a, n);
    long long s = 0;
    int bad = 0;
    for (long long i = 0; i < n && !bad; ++i) { bad = a[i] != s; s += in[(size_t)i]; }
    bad |= a[n] != s;
    delete[] a;
    printf("scan-%lld %s (levels above the first %d, total %lld)\n", n, bad ? "FAILED" : "ok", top, s);
    return bad;
}

/* a pair table of n_sides sides over an input of n atoms in residues of 1 .. max_res atoms (some empty); every side takes every
   step-th atom of a window of the input, so that residues are split and segments have every length; areas are random, and a part
   of the atoms has its pair area equal to its isolated area */
static int check_table(const char *name, int n, int n_sides, int max_res, int step, double min_buried, long long short_by)
{
    std::vector<int64_t> res_first(1, 0);
    while (res_first.back() < n) {
        const int len = rnd() % 7 == 0 ? 0 : 1 + (int)(rnd() % (unsigned)max_res);
        res_first.push_back(res_first.back() + len < n ? res_first.back() + len : n);
    }
    res_first.push_back(n); /* an empty residue at the end */
    const int n_res = (int)res_first.size() - 1;
    std::vector<int64_t> side_off(1, 0);
    std::vector<int32_t> pair_atom;
    for (int q = 0; q < n_sides; ++q) {
        const int lo = (int)(rnd() % (unsigned)(n / 2)), hi = lo + 1 + (int)(rnd() % (unsigned)(n - lo));
        for (int i = lo + (q % step); i < hi; i += 1 + (int)(rnd() % (unsigned)step)) pair_atom.push_back(i);
        if ((int64_t)pair_atom.size() == side_off.back()) pair_atom.push_back(lo); /* (no side is empty) */
        side_off.push_back((int64_t)pair_atom.size());
    }
    const int64_t M = (int64_t)pair_atom.size();
    double *iso = new double[(size_t)n], *psasa = new double[(size_t)M];
    for (int i = 0; i < n; ++i) iso[i] = uni(0, 40);
    for (int64_t m = 0; m < M; ++m) psasa[m] = rnd() % 3 ? iso[pair_atom[(size_t)m]] : uni(0, 1) * iso[pair_atom[(size_t)m]];
    /* the plain loop */
    std::vector<int> w_index, w_atoms;
    std::vector<double> w_areas;
    std::vector<int64_t> w_off(1, 0), w_first;
    std::vector<unsigned char> w_head((size_t)M, 0);
    for (int q = 0; q < n_sides; ++q) {
        int64_t m = side_off[(size_t)q];
        int r = 0; /* (a side's atoms ascend: so do its residues) */
        while (m < side_off[(size_t)q + 1]) {
            while (!(res_first[(size_t)r] <= pair_atom[(size_t)m] && pair_atom[(size_t)m] < res_first[(size_t)r + 1])) ++r;
            int64_t e = m;
            double a = 0, b = 0;
            while (e < side_off[(size_t)q + 1] && pair_atom[(size_t)e] >= res_first[(size_t)r] && pair_atom[(size_t)e] < res_first[(size_t)r + 1]) {
                a += iso[pair_atom[(size_t)e]]; b += psasa[e]; ++e;
            }
            w_head[(size_t)m] = 1; w_first.push_back(m);
            if (a - b > min_buried) { w_index.push_back(r); w_atoms.push_back((int)(e - m)); w_areas.push_back(a); w_areas.push_back(b); w_areas.push_back(a - b); }
            m = e;
        }
        w_off.push_back((int64_t)w_index.size());
    }
    w_first.push_back(M);
    const int64_t K = (int64_t)w_first.size() - 1, R = (int64_t)w_index.size();
    const int64_t cap = R > short_by ? R - short_by : 0;
    unsigned char *heads = new unsigned char[(size_t)M];
    int64_t *seg_first = new int64_t[(size_t)M + 1], *res_off = new int64_t[(size_t)n_sides + 1];
    int32_t *res_index = new int32_t[(size_t)cap + 1], *res_atoms = new int32_t[(size_t)cap + 1];
    double *res_areas = new double[3 * (size_t)cap + 1];
    for (int q = 0; q <= n_sides; ++q) res_off[q] = -7;
    long long k_got = -1, r_got = -1;
    const long long got = emu_iface_res_table(side_off.data(), n_sides, pair_atom.data(), M, res_first.data(), n_res, iso, psasa, min_buried, cap,
                                              heads, seg_first, &k_got, &r_got, res_off, res_index, res_atoms, res_areas);
    int bad = k_got != K || r_got != R || memcmp(heads, w_head.data(), (size_t)M) != 0;
    for (int64_t k = 0; k <= K && !bad; ++k) bad = seg_first[k] != w_first[(size_t)k];
    if (!bad && short_by && R > 0) {
        bad = got != -2;
        for (int q = 0; q <= n_sides && !bad; ++q) bad = res_off[q] != -7;
    } else if (!bad) {
        bad = got != R;
        for (int q = 0; q <= n_sides && !bad; ++q) bad = res_off[q] != w_off[(size_t)q];
        for (int64_t j = 0; j < R && !bad; ++j)
            bad = res_index[j] != w_index[(size_t)j] || res_atoms[j] != w_atoms[(size_t)j] ||
                  memcmp(res_areas + 3 * j, w_areas.data() + 3 * j, 24) != 0;
    }
    delete[] iso; delete[] psasa; delete[] heads; delete[] seg_first; delete[] res_off; delete[] res_index; delete[] res_atoms; delete[] res_areas;
    printf("%s %s (atoms %lld, segments %lld, rows %lld)\n", name, bad ? "FAILED" : "ok", (long long)M, (long long)K, (long long)R);
    return bad;
}

int main()
{
    int bad = 0;
    const long long sizes[] = {0, 1, IF_B - 1, IF_B, IF_B + 1, (long long)IF_B * IF_B, (long long)IF_B * IF_B + 1};
    for (long long n : sizes) bad |= check_scan(n);
    bad |= check_table("one-side", 300, 1, 5, 1, 0.0, 0);
    bad |= check_table("split-residues", 2000, 12, 9, 3, 0.0, 0);
    bad |= check_table("long-segments", 3000, 6, 700, 1, 0.0, 0);
    bad |= check_table("min-buried", 2000, 12, 9, 2, 15.0, 0);
    bad |= check_table("no-rows", 2000, 12, 9, 2, 1e300, 0);
    bad |= check_table("rows-short-by-1", 2000, 12, 9, 2, 0.0, 1);
    bad |= check_table("many-segments", 40000, 8, 2, 1, 0.0, 0);
    return bad;
}
#endif
