/* TESTS ONLY: the phase functions of the residue-residue contact tables of the interfaces between chain groups
 * (freesasa_amd/csrc/rescontact_kernels.h) driven on the CPU as gpu_interfaces.hip drives the kernels: the segments by the
 * per-residue tables' phases (iface_res_head, the block scan through ifr_scan_levels like kl_iface_res_scan, iface_res_first),
 * rc_fold_count one wave per segment over fc zeroed beforehand, the scan again, rc_fold_write one wave per segment - one wave's LDS
 * for all segments, one behind the other, as a wave of the kernels strides over them -, rc_reverse one thread per folded row and
 * per side boundary, idle threads included.  The 64 lanes of a
 * wave of the two fold kernels are fibers in lock step (as in emu_contacts.cpp): a shuffle or a wave synchronization deposits the
 * lane's operand and yields; the scheduler resumes the lanes once all have arrived.
 * With -DRESCONTACTS_CHECK_MAIN: a stand-alone program (tests/emu/rescontacts_check, built with AddressSanitizer + UBSan) that
 * drives the same phases over generated contact tables against plain loops, every array a heap block of its exact size: one line
 * per case.
 * Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>

#include <ucontext.h>

#include "../../freesasa_amd/csrc/rescontact_kernels.h"

using namespace sasa;

namespace sasa_emu {
static const int W = RC_WAVE;
static ucontext_t g_main, g_fiber[W];
static bool g_done[W];
static int g_lane = -1;
static long long g_dep[W], g_snap[W];
static unsigned long long g_ballot;
static void (*g_body)(int lane, void *ctx);
static void *g_ctx;
static char *g_stacks = nullptr;

static void yield_to_scheduler() { swapcontext(&g_fiber[g_lane], &g_main); }
unsigned long long wave_ballot(bool p) { g_dep[g_lane] = p ? 1 : 0; yield_to_scheduler(); return g_ballot; }
void wave_sync() { g_dep[g_lane] = 0; yield_to_scheduler(); }
long long wave_exchange(long long v, int src) { g_dep[g_lane] = v; yield_to_scheduler(); return g_snap[src & 63]; }
static void trampoline()
{
    g_body(g_lane, g_ctx);
    g_done[g_lane] = true;
    swapcontext(&g_fiber[g_lane], &g_main);
}
static void run_wave(void (*body)(int, void *), void *ctx)
{
    const size_t STK = 64 * 1024;
    if (!g_stacks) g_stacks = new char[STK * W]; /* (kept for the life of the process) */
    g_body = body; g_ctx = ctx;
    for (int l = 0; l < W; ++l) {
        getcontext(&g_fiber[l]);
        g_fiber[l].uc_stack.ss_sp = g_stacks + STK * l;
        g_fiber[l].uc_stack.ss_size = STK;
        g_fiber[l].uc_link = &g_main;
        makecontext(&g_fiber[l], trampoline, 0);
        g_done[l] = false;
    }
    for (;;) {
        bool any = false;
        for (int l = 0; l < W; ++l) {
            if (g_done[l]) continue;
            any = true;
            g_lane = l;
            swapcontext(&g_main, &g_fiber[l]);
        }
        if (!any) break;
        g_ballot = 0;
        for (int l = 0; l < W; ++l) {
            if (!g_done[l] && g_dep[l]) g_ballot |= 1ull << l;
            g_snap[l] = g_dep[l];
        }
    }
    g_lane = -1;
}
} /* namespace sasa_emu */

struct FoldRun { const ResContactArgs *a; ResContactLds *m; int64_t s; bool write; };
static void fold_body(int lane, void *ctx)
{
    const FoldRun *r = (const FoldRun *)ctx;
    if (r->write) rc_fold_write(*r->a, *r->m, r->s, lane);
    else rc_fold_count(*r->a, *r->m, r->s, lane);
}

/* kl_iface_res_scan: a [n + 1] in place */
static void scan_in_place(int *a, int64_t n)
{
    int64_t cnt[IFR_MAX_LEVELS];
    int *lvl[IFR_MAX_LEVELS];
    int part[IF_B];
    const int top = ifr_scan_levels(n, cnt);
    int *scratch = new int[(size_t)ifr_scan_scratch(n) + 1];
    lvl[0] = a;
    for (int l = 1; l <= top; ++l) lvl[l] = l == 1 ? scratch : lvl[l - 1] + cnt[l - 1];
    auto apply = [&](int *x, int64_t m, const int *base, int *total, int64_t blocks) {
        for (int64_t b = 0; b < blocks; ++b) {
            for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase0(x, m, part, b, t);
            for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase1(part, total, t);
            for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase2(x, m, part, base, b, t);
        }
    };
    for (int l = 0; l < top; ++l)
        for (int64_t b = 0; b < cnt[l + 1]; ++b) {
            for (int t = 0; t < IF_B; ++t) ifr_scan_sums_phase0(lvl[l], cnt[l], part, b, t);
            for (int t = 0; t < IF_B; ++t) ifr_scan_sums_phase1(part, lvl[l + 1], b, t);
        }
    apply(lvl[top], cnt[top], nullptr, a + n, 1);
    for (int l = top - 1; l >= 0; --l) apply(lvl[l], cnt[l], lvl[l + 1], nullptr, cnt[l + 1]);
    delete[] scratch;
}

extern "C" void emu_rescontacts_shape(int *wave, int *stage) { *wave = RC_WAVE; *stage = RC_STAGE; }

/* The stage behind the contact stage, from the pair table (side_off [n_sides + 1], pair_atom [M]), res_first [n_res + 1] and the
 * contact table (contact_first [M + 1], contact_partner / contact_points / contact_area [C], C > 0): when row_cap holds the Q folded
 * rows, rc_off [n_sides + 1], rc_res / rc_cnt [2 row_cap], rc_area / rc_rev [row_cap].  *n_segs_out: K, *n_rows_out: Q.  Returns Q;
 * -1 on a bad argument, -2 when row_cap is too small (none of the five arrays written). */
extern "C" long long emu_rescontacts_table(const int64_t *side_off, long long n_sides, const int32_t *pair_atom, long long M, const int64_t *res_first,
                                           int n_res, const int64_t *contact_first, const int32_t *contact_partner, const int32_t *contact_points,
                                           const double *contact_area, long long C, long long row_cap, long long *n_segs_out, long long *n_rows_out,
                                           int64_t *rc_off, int32_t *rc_res, int32_t *rc_cnt, double *rc_area, int32_t *rc_rev)
{
    if (!side_off || n_sides <= 0 || (n_sides & 1) || !pair_atom || M <= 0 || !res_first || n_res <= 0 || !contact_first || !contact_partner ||
        !contact_points || !contact_area || C <= 0 || contact_first[M] != C || row_cap < 0 || !n_segs_out || !n_rows_out || !rc_off || !rc_res ||
        !rc_cnt || !rc_area || !rc_rev || side_off[n_sides] != M)
        return -1;
    const size_t m = (size_t)M, c = (size_t)C;
    /* the arrays as iface_rescontacts makes them: M (+ 1) and exactly C entries each */
    int *atom_res = new int[m], *hs = new int[m + 1], *sf = new int[m + 1], *fc = new int[m + 1], *pseg = new int[c];
    int64_t *t_off = new int64_t[(size_t)n_sides + 1];
    int *t_res = new int[2 * c], *t_cnt = new int[2 * c], *t_rev = new int[c];
    double *t_area = new double[c];
    IfaceResArgs s;
    memset(&s, 0, sizeof s);
    s.n_pair_atoms = M; s.n_sides = n_sides; s.n_res = n_res; s.side_off = side_off; s.pair_atom = pair_atom; s.res_first = res_first;
    s.atom_res = atom_res; s.hs = hs; s.seg_first = sf;
    const int64_t grid = (M + IF_B - 1) / IF_B * IF_B;
    for (int64_t i = 0; i < grid; ++i) iface_res_head(s, i);
    scan_in_place(hs, M);
    for (int64_t i = 0; i < grid; ++i) iface_res_first(s, i);
    ResContactArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = M; a.n_sides = n_sides; a.row_cap = C; a.side_off = side_off; a.atom_res = atom_res; a.hs = hs; a.seg_first = sf;
    a.contact_first = contact_first; a.contact_partner = contact_partner; a.contact_points = contact_points; a.contact_area = contact_area;
    a.fc = fc; a.pseg = pseg; a.rc_off = t_off; a.rc_res = t_res; a.rc_cnt = t_cnt; a.rc_area = t_area; a.rc_rev = t_rev;
    ResContactLds *lds = new ResContactLds;
    memset(fc, 0, 4 * (m + 1));
    const int64_t K = hs[M];
    for (int64_t k = 0; k < K; ++k) {
        FoldRun r = {&a, lds, k, false};
        sasa_emu::run_wave(fold_body, &r);
    }
    scan_in_place(fc, M);
    for (int64_t k = 0; k < K; ++k) {
        FoldRun r = {&a, lds, k, true};
        sasa_emu::run_wave(fold_body, &r);
    }
    delete lds;
    const int64_t Q = fc[M], n_rev = C > n_sides + 1 ? C : n_sides + 1;
    for (int64_t t = 0; t < (n_rev + IF_B - 1) / IF_B * IF_B; ++t) rc_reverse(a, t);
    *n_segs_out = hs[M]; *n_rows_out = Q;
    const bool fits = Q <= row_cap;
    if (fits) {
        memcpy(rc_off, t_off, 8 * ((size_t)n_sides + 1));
        memcpy(rc_res, t_res, 8 * (size_t)Q); memcpy(rc_cnt, t_cnt, 8 * (size_t)Q);
        memcpy(rc_area, t_area, 8 * (size_t)Q); memcpy(rc_rev, t_rev, 4 * (size_t)Q);
    }
    delete[] atom_res; delete[] hs; delete[] sf; delete[] fc; delete[] pseg; delete[] t_off; delete[] t_res; delete[] t_cnt; delete[] t_rev; delete[] t_area;
    return fits ? Q : -2;
}

#ifdef RESCONTACTS_CHECK_MAIN
/* a small generator of its own: the cases are the program's, whatever the C library */
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() % 1000001) / 1000000.0; }

/* n_pairs pairs whose sides take consecutive input atoms (more than half of max_side of them) of an input cut into residues of 1 .. max_res
   atoms; every atom gets 0 .. max_rows contact rows to distinct atoms of the other side, ascending; short_by: the capacity is that
   much below Q; mix: 31 residues of 32 have one atom, so that a long residue meets many partner residues */
static int check_case(const char *name, int n_pairs, int max_side, int max_res, int max_rows, long long short_by, bool mix = false)
{
    std::vector<int64_t> side_off(1, 0), res_first(1, 0);
    std::vector<int32_t> pair_atom;
    int n = 0;
    for (int q = 0; q < 2 * n_pairs; ++q) {
        const int cnt = max_side <= 2 ? max_side : max_side / 2 + 1 + (int)(rnd() % (unsigned)(max_side / 2));
        for (int k = 0; k < cnt; ++k) pair_atom.push_back(n++);
        side_off.push_back((int64_t)pair_atom.size());
    }
    while (res_first.back() < n) { /* (residues run across the sides' boundaries: such a residue has a segment on both sides) */
        const int len = rnd() % 9 == 0 ? 0 : mix && rnd() % 32 ? 1 : 1 + (int)(rnd() % (unsigned)max_res);
        res_first.push_back(res_first.back() + len < n ? res_first.back() + len : n);
    }
    const int n_res = (int)res_first.size() - 1;
    const int64_t M = n;
    std::vector<int64_t> cf(1, 0);
    std::vector<int32_t> cp, cn;
    std::vector<double> ca;
    for (int q = 0; q < 2 * n_pairs; ++q)
        for (int64_t i = side_off[(size_t)q]; i < side_off[(size_t)q + 1]; ++i) {
            const int64_t o0 = side_off[(size_t)(q ^ 1)], o1 = side_off[(size_t)(q ^ 1) + 1];
            const int want = max_rows ? (int)(rnd() % (unsigned)(max_rows + 1)) : 0;
            std::vector<int32_t> js;
            for (int k = 0; k < want; ++k) js.push_back((int32_t)(o0 + rnd() % (unsigned)(o1 - o0)));
            std::sort(js.begin(), js.end());
            js.erase(std::unique(js.begin(), js.end()), js.end());
            for (int32_t j : js) { cp.push_back(j); cn.push_back(1 + (int)(rnd() % 100)); ca.push_back(uni(0.01, 30.0)); }
            cf.push_back((int64_t)cp.size());
        }
    const int64_t C = (int64_t)cp.size();
    if (C == 0) { cp.push_back(0); cn.push_back(0); ca.push_back(0); } /* (never read: data() of an empty vector may be null) */
    /* the plain loops: the residue of every atom, the segments, the fold in a map per segment, the reverse rows by a map */
    std::vector<int> res_of((size_t)n), seg_of((size_t)M);
    for (int r = 0; r < n_res; ++r)
        for (int64_t i = res_first[(size_t)r]; i < res_first[(size_t)r + 1]; ++i) res_of[(size_t)i] = r;
    std::vector<int64_t> seg_first;
    std::vector<int> seg_side;
    for (int q = 0; q < 2 * n_pairs; ++q)
        for (int64_t i = side_off[(size_t)q]; i < side_off[(size_t)q + 1]; ++i) {
            if (i == side_off[(size_t)q] || res_of[(size_t)i] != res_of[(size_t)i - 1]) { seg_first.push_back(i); seg_side.push_back(q); }
            seg_of[(size_t)i] = (int)seg_first.size() - 1;
        }
    const int64_t K = (int64_t)seg_first.size();
    seg_first.push_back(M);
    struct Row { int n_rows, n_points; double area; };
    std::vector<int> w_res, w_cnt, w_src, w_dst;
    std::vector<double> w_area;
    std::vector<int64_t> w_off((size_t)(2 * n_pairs) + 1, 0);
    std::map<std::pair<int, int>, int> where;
    long long most_rows = 0, most_partners = 0;
    for (int64_t a = 0; a < K; ++a) {
        std::map<int, Row> rows;
        for (int64_t t = cf[(size_t)seg_first[(size_t)a]]; t < cf[(size_t)seg_first[(size_t)a + 1]]; ++t) {
            Row &r = rows.insert(std::make_pair(seg_of[(size_t)cp[(size_t)t]], Row{0, 0, 0.0})).first->second;
            ++r.n_rows; r.n_points += cn[(size_t)t]; r.area += ca[(size_t)t];
        }
        const long long seg_rows = cf[(size_t)seg_first[(size_t)a + 1]] - cf[(size_t)seg_first[(size_t)a]];
        most_rows = seg_rows > most_rows ? seg_rows : most_rows;
        most_partners = (long long)rows.size() > most_partners ? (long long)rows.size() : most_partners;
        for (const auto &kv : rows) {
            where[std::make_pair((int)a, kv.first)] = (int)w_area.size();
            w_src.push_back((int)a); w_dst.push_back(kv.first);
            w_res.push_back(res_of[(size_t)pair_atom[(size_t)seg_first[(size_t)a]]]);
            w_res.push_back(res_of[(size_t)pair_atom[(size_t)seg_first[(size_t)kv.first]]]);
            w_cnt.push_back(kv.second.n_rows); w_cnt.push_back(kv.second.n_points); w_area.push_back(kv.second.area);
            ++w_off[(size_t)seg_side[(size_t)a] + 1];
        }
    }
    for (int q = 0; q < 2 * n_pairs; ++q) w_off[(size_t)q + 1] += w_off[(size_t)q];
    const int64_t Q = (int64_t)w_area.size();
    const int64_t cap = Q > short_by ? Q - short_by : 0;
    int64_t *off = new int64_t[(size_t)(2 * n_pairs) + 1];
    int32_t *res = new int32_t[2 * (size_t)cap + 1], *cnt = new int32_t[2 * (size_t)cap + 1], *rev = new int32_t[(size_t)cap + 1];
    double *area = new double[(size_t)cap + 1];
    for (int q = 0; q <= 2 * n_pairs; ++q) off[q] = -7;
    long long k_got = -1, q_got = -1, got = 0;
    int bad = 0;
    if (C > 0) {
        got = emu_rescontacts_table(side_off.data(), 2 * n_pairs, pair_atom.data(), M, res_first.data(), n_res, cf.data(), cp.data(), cn.data(), ca.data(), C,
                                    cap, &k_got, &q_got, off, res, cnt, area, rev);
        bad = k_got != K || q_got != Q;
    }
    if (!bad && C > 0 && short_by && Q > 0) {
        bad = got != -2;
        for (int q = 0; q <= 2 * n_pairs && !bad; ++q) bad = off[q] != -7;
    } else if (!bad && C > 0) {
        bad = got != Q;
        for (int q = 0; q <= 2 * n_pairs && !bad; ++q) bad = off[q] != w_off[(size_t)q];
        for (int64_t k = 0; k < Q && !bad; ++k) {
            const auto it = where.find(std::make_pair(w_dst[(size_t)k], w_src[(size_t)k]));
            bad = res[2 * k] != w_res[2 * (size_t)k] || res[2 * k + 1] != w_res[2 * (size_t)k + 1] || cnt[2 * k] != w_cnt[2 * (size_t)k] ||
                  cnt[2 * k + 1] != w_cnt[2 * (size_t)k + 1] || memcmp(area + k, w_area.data() + k, 8) != 0 ||
                  rev[k] != (it == where.end() ? -1 : it->second);
        }
    }
    delete[] off; delete[] res; delete[] cnt; delete[] rev; delete[] area;
    printf("%s %s (atoms %lld, segments %lld, contact rows %lld, folded rows %lld; a segment's most rows %lld, most partners %lld)\n", name,
           bad ? "FAILED" : "ok", (long long)M, (long long)K, (long long)C, (long long)Q, most_rows, most_partners);
    return bad;
}

int main()
{
    int bad = 0;
    bad |= check_case("one-atom-sides", 9, 1, 1, 1, 0);
    bad |= check_case("two-atom-sides", 9, 2, 3, 2, 0);
    bad |= check_case("small-sides", 6, 40, 6, 5, 0);
    bad |= check_case("whole-chain-residues", 1, 300, 2000, 12, 0);  /* more than a thousand rows to a segment, beyond the staged keys */
    bad |= check_case("many-partners", 1, 160, 1, 110, 0);           /* more distinct partners than a wave has lanes */
    bad |= check_case("long-residues-many-partners", 1, 400, 150, 12, 0, true); /* both at once */
    bad |= check_case("short-by-1", 3, 50, 5, 4, 1);
    return bad;
}
#endif
