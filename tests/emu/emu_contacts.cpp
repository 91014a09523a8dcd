/* TESTS ONLY: the phase functions of the atom-atom contact tables of the interfaces between chain groups
 * (freesasa_amd/csrc/contact_kernels.h) driven on the CPU as gpu_interfaces.hip drives the kernels: contact_masks one thread per
 * pair-structure atom, the dots' scan and expansion (dots_kernels.h) as emu_dots.cpp drives them, contact_attribute one workgroup
 * of CT_B threads per CT_B dots, contact_rows_count / _rank one thread per dot, the block scan through ifr_scan_levels like
 * kl_iface_res_scan, contact_rows_write one thread per dot and per atom - every kernel a loop over its grid's workgroups, idle
 * threads included.  The CT_B threads of a workgroup of contact_attribute are fibers in lock step (as in emu_iface.cpp): a
 * ballot, a shuffle or a barrier deposits the thread's operand and yields; the scheduler resumes the threads once all have
 * arrived; a ballot or a shuffle reads within the thread's own wave of 64.
 * With -DCONTACTS_CHECK_MAIN: a stand-alone program (tests/emu/contacts_check, built with AddressSanitizer + UBSan) that drives
 * the same phases over generated pair structures against plain loops, every array a heap block of its exact size: one line per
 * case.
 * Never linked into the product. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include <ucontext.h>

#include "../../freesasa_amd/csrc/contact_kernels.h"

using namespace sasa;

namespace sasa_emu {
static const int W = CT_B;
static ucontext_t g_main, g_fiber[W];
static bool g_done[W];
static int g_lane = -1;
static long long g_dep[W], g_snap[W];
static unsigned long long g_ballot[W / 64];
static void (*g_body)(int tid, void *ctx);
static void *g_ctx;
static char *g_stacks = nullptr;

static void yield_to_scheduler() { swapcontext(&g_fiber[g_lane], &g_main); }
unsigned long long wave_ballot(bool p) { g_dep[g_lane] = p ? 1 : 0; yield_to_scheduler(); return g_ballot[g_lane >> 6]; }
void wave_sync() { g_dep[g_lane] = 0; yield_to_scheduler(); }
long long wave_exchange(long long v, int src) { g_dep[g_lane] = v; yield_to_scheduler(); return g_snap[(g_lane & ~63) + (src & 63)]; }
static void trampoline()
{
    g_body(g_lane, g_ctx);
    g_done[g_lane] = true;
    swapcontext(&g_fiber[g_lane], &g_main);
}
static void run_group(void (*body)(int, void *), void *ctx)
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
        for (int w = 0; w < W / 64; ++w) g_ballot[w] = 0;
        for (int l = 0; l < W; ++l) {
            if (!g_done[l] && g_dep[l]) g_ballot[l >> 6] |= 1ull << (l & 63);
            g_snap[l] = g_dep[l];
        }
    }
    g_lane = -1;
}
} /* namespace sasa_emu */

struct AttributeRun { const ContactArgs *a; ContactLds *m; int64_t block; };
static void attribute_body(int tid, void *ctx)
{
    const AttributeRun *r = (const AttributeRun *)ctx;
    contact_attribute(*r->a, *r->m, r->block, tid);
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

extern "C" void emu_contacts_shape(int *threads) { *threads = CT_B; }

/* The stage behind the interface pipeline from the pair batch (side_off [n_sides + 1], pxyz [3 M], pradii [M]), the unit points
 * [3 n_points] and the two sets of masks [M][4]: buried [M][4] and dot_first [M + 1] always; then - when dot_cap holds the D_b dots
 * and row_cap the C rows - dot_partner [dot_cap], contact_first [M + 1], contact_partner / contact_points / contact_area [row_cap].
 * *n_dots_out: D_b, *n_rows_out: C, *flag_out: 0, or 1 + the largest atom with a dot that no atom covers.  Returns C; -1 on a bad
 * argument, -2 when a capacity is too small (none of the five arrays behind it written). */
extern "C" long long emu_contacts_table(const int64_t *side_off, long long n_sides, const double *pxyz, const double *pradii, long long M,
                                        double probe, int n_points, const double *unit, const unsigned *side_masks, const unsigned *pair_masks,
                                        long long dot_cap, long long row_cap, unsigned *buried, int64_t *dot_first, int32_t *dot_partner,
                                        int64_t *contact_first, int32_t *contact_partner, int32_t *contact_points, double *contact_area,
                                        long long *n_dots_out, long long *n_rows_out, int *flag_out)
{
    if (!side_off || n_sides <= 0 || (n_sides & 1) || !pxyz || !pradii || M <= 0 || n_points <= 0 || n_points > SR_CAP_POINTS_MAX || !unit ||
        !side_masks || !pair_masks || !buried || !dot_first || !n_dots_out || !n_rows_out || !flag_out || side_off[n_sides] != M || dot_cap < 0 || row_cap < 0)
        return -1;
    ContactArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = M; a.n_sides = n_sides; a.n_points = n_points; a.probe = probe;
    a.side_off = side_off; a.pxyz = pxyz; a.pradii = pradii; a.side_masks = side_masks; a.pair_masks = pair_masks; a.buried = buried;
    for (int64_t i = 0; i < (M + CT_B - 1) / CT_B * CT_B; ++i) contact_masks(a, i);
    /* kl_dots_count */
    DotsArgs d;
    memset(&d, 0, sizeof d);
    d.masks = buried; d.n_atoms = M; d.n_points = n_points; d.n_blocks = (M + DOTS_SCAN_B - 1) / DOTS_SCAN_B;
    int64_t *bsum = new int64_t[(size_t)d.n_blocks], part64[DOTS_SCAN_T];
    int part[DOTS_SCAN_T];
    d.bsum = bsum; d.dot_first = dot_first;
    for (int64_t b = 0; b < d.n_blocks; ++b) {
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_count_phase0(d, part, b, tid);
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_count_phase1(d, part, b, tid);
    }
    for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_scan_phase0(d, part64, tid);
    for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_scan_phase1(d, part64, tid);
    for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_scan_phase2(d, part64, tid);
    for (int64_t b = 0; b < d.n_blocks; ++b) {
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_first_phase0(d, part, b, tid);
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_first_phase1(d, part, b, tid);
        for (int tid = 0; tid < DOTS_SCAN_T; ++tid) dots_first_phase2(d, part, b, tid);
    }
    delete[] bsum;
    const int64_t D = dot_first[M];
    *n_dots_out = D; *n_rows_out = 0; *flag_out = 0;
    if (D == 0) {
        if (contact_first) memset(contact_first, 0, 8 * ((size_t)M + 1));
        return 0;
    }
    /* the arrays D_b sizes, as iface_contacts makes them: exactly D_b entries each */
    const size_t Db = (size_t)D;
    double *dot_xyz = new double[3 * Db], *t_area = new double[Db];
    int *dot_atom = new int[Db], *dot_point = new int[Db], *t_dpart = new int[Db], *cnt = new int[Db], *rank = new int[Db], *nd = new int[(size_t)M + 1];
    int *t_partner = new int[Db], *t_points = new int[Db];
    int64_t *t_first = new int64_t[(size_t)M + 1];
    int flag = 0;
    d.xyz = pxyz; d.radii = pradii; d.unit_pts = unit; d.probe = probe; d.inv_points = 1.0 / n_points; d.capacity = D;
    d.dot_xyz = dot_xyz; d.dot_atom = dot_atom; d.dot_point = dot_point;
    const int64_t pairs = M * n_points, per_wg = (int64_t)DOTS_EXPAND_B * DOTS_EXPAND_U;
    for (int64_t b = 0; b < (pairs + per_wg - 1) / per_wg; ++b)
        for (int tid = 0; tid < DOTS_EXPAND_B; ++tid) dots_expand(d, b, tid);
    a.n_dots = D; a.dot_first = dot_first; a.dot_xyz = dot_xyz; a.dot_atom = dot_atom; a.dot_partner = t_dpart; a.flag = &flag;
    a.cnt = cnt; a.rank = rank; a.nd = nd; a.contact_first = t_first; a.contact_partner = t_partner; a.contact_points = t_points; a.contact_area = t_area;
    memset(nd, 0, 4 * ((size_t)M + 1));
    ContactLds *m = new ContactLds;
    const int64_t blocks = (D + CT_B - 1) / CT_B;
    for (int64_t b = 0; b < blocks; ++b) {
        AttributeRun r = {&a, m, b};
        sasa_emu::run_group(attribute_body, &r);
    }
    delete m;
    for (int64_t t = 0; t < blocks * CT_B; ++t) contact_rows_count(a, t);
    for (int64_t t = 0; t < blocks * CT_B; ++t) contact_rows_rank(a, t);
    scan_in_place(nd, M);
    const int64_t C = nd[M], n_write = D > M + 1 ? D : M + 1;
    for (int64_t t = 0; t < (n_write + CT_B - 1) / CT_B * CT_B; ++t) contact_rows_write(a, t);
    *n_rows_out = C; *flag_out = flag;
    const bool fits = D <= dot_cap && C <= row_cap;
    if (fits) {
        if (dot_partner) memcpy(dot_partner, t_dpart, 4 * Db);
        if (contact_first) memcpy(contact_first, t_first, 8 * ((size_t)M + 1));
        if (contact_partner) memcpy(contact_partner, t_partner, 4 * (size_t)C);
        if (contact_points) memcpy(contact_points, t_points, 4 * (size_t)C);
        if (contact_area) memcpy(contact_area, t_area, 8 * (size_t)C);
    }
    delete[] dot_xyz; delete[] t_area; delete[] dot_atom; delete[] dot_point; delete[] t_dpart; delete[] cnt; delete[] rank; delete[] nd;
    delete[] t_partner; delete[] t_points; delete[] t_first;
    return fits ? C : -2;
}

#ifdef CONTACTS_CHECK_MAIN
/* a small generator of its own: the cases are the program's, whatever the C library */
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() % 1000001) / 1000000.0; }

/* the points of a spiral on the unit sphere: any unit vectors do, the definitions take them as given */
static void spiral(int N, std::vector<double> &u)
{
    u.resize(3 * (size_t)N);
    for (int k = 0; k < N; ++k) {
        const double z = 1.0 - (2.0 * k + 1.0) / N, r = sqrt(1.0 - z * z), phi = 2.399963229728653 * k;
        u[3 * (size_t)k] = r * cos(phi); u[3 * (size_t)k + 1] = r * sin(phi); u[3 * (size_t)k + 2] = z;
    }
}
/* does atom j cover point k of atom i (the definition, operand for operand); w: the penetration */
static bool covers(const std::vector<double> &x, const std::vector<double> &R, const std::vector<double> &u, int i, int k, int j, double &w)
{
    double t[3];
    for (int c = 0; c < 3; ++c) { t[c] = u[3 * (size_t)k + c] * R[(size_t)i]; t[c] += x[3 * (size_t)i + c]; }
    const double dx = t[0] - x[3 * (size_t)j], dy = t[1] - x[3 * (size_t)j + 1], dz = t[2] - x[3 * (size_t)j + 2], r2 = R[(size_t)j] * R[(size_t)j];
    const double s = dx * dx + dy * dy + dz * dz;
    w = s - r2;
    return s <= r2;
}

/* n_pairs pair structures whose sides have 1 .. max_side atoms in a cube sized for about `density` neighbours, N points; twins:
   every fourth atom is a copy of the atom before it (equal penetrations: the lower index has to win); short_by: the capacities
   are that much below D_b and C */
static int check_case(const char *name, int n_pairs, int max_side, int N, bool twins, long long short_by)
{
    const double probe = 1.4;
    std::vector<double> u;
    spiral(N, u);
    std::vector<int64_t> side_off(1, 0);
    std::vector<double> x, r, R;
    for (int q = 0; q < 2 * n_pairs; ++q) {
        const int cnt = max_side <= 2 ? max_side : 1 + (int)(rnd() % (unsigned)max_side);
        /* (side h lies half an edge above side g of its pair: the two interpenetrate) */
        const double edge = cbrt(12.0 * (cnt + 1)), ox = 40.0 * (q / 2);
        for (int k = 0; k < cnt; ++k) {
            const bool twin = twins && k > 0 && (k & 3) == 3;
            const size_t prev = r.size() - 1;
            for (int c = 0; c < 3; ++c) x.push_back(twin ? x[3 * prev + c] : (c == 0 ? ox : 0.0) + uni(0, edge) + ((q & 1) && c == 2 ? 0.5 * edge : 0.0));
            r.push_back(twin ? r[prev] : uni(1.0, 2.0));
        }
        side_off.push_back((int64_t)r.size());
    }
    const int64_t M = (int64_t)r.size();
    for (int64_t i = 0; i < M; ++i) R.push_back(r[(size_t)i] + probe);
    /* the masks and the table by plain loops */
    unsigned *side_masks = new unsigned[4 * (size_t)M], *pair_masks = new unsigned[4 * (size_t)M];
    memset(side_masks, 0, 16 * (size_t)M); memset(pair_masks, 0, 16 * (size_t)M);
    std::vector<int64_t> w_first(1, 0);
    std::vector<int> w_partner, w_points, w_dpart;
    std::vector<double> w_area;
    std::vector<unsigned> w_buried(4 * (size_t)M, 0u);
    for (int q = 0; q < 2 * n_pairs; ++q)
        for (int64_t i = side_off[(size_t)q]; i < side_off[(size_t)q + 1]; ++i) {
            std::vector<int> npts((size_t)M, 0);
            for (int k = 0; k < N; ++k) {
                double w, best_w = 0;
                bool own = false;
                int best = -1;
                for (int64_t j = side_off[(size_t)q]; j < side_off[(size_t)q + 1] && !own; ++j) own = j != i && covers(x, R, u, (int)i, k, (int)j, w);
                for (int64_t j = side_off[(size_t)(q ^ 1)]; j < side_off[(size_t)(q ^ 1) + 1]; ++j)
                    if (covers(x, R, u, (int)i, k, (int)j, w) && (best < 0 || w < best_w)) { best = (int)j; best_w = w; }
                if (!own) side_masks[4 * i + (k >> 5)] |= 1u << (k & 31);
                if (!own && best < 0) pair_masks[4 * i + (k >> 5)] |= 1u << (k & 31);
                if (!own && best >= 0) { w_buried[4 * (size_t)i + (size_t)(k >> 5)] |= 1u << (k & 31); w_dpart.push_back(best); ++npts[(size_t)best]; }
            }
            for (int64_t j = 0; j < M; ++j)
                if (npts[(size_t)j]) {
                    w_partner.push_back((int)j); w_points.push_back(npts[(size_t)j]);
                    w_area.push_back((4.0 * SASA_PI * R[(size_t)i] * R[(size_t)i] * npts[(size_t)j]) / N);
                }
            w_first.push_back((int64_t)w_partner.size());
        }
    const int64_t D = (int64_t)w_dpart.size(), C = (int64_t)w_partner.size();
    const int64_t dcap = D > short_by ? D - short_by : 0, rcap = C > short_by ? C - short_by : 0;
    unsigned *buried = new unsigned[4 * (size_t)M];
    int64_t *dot_first = new int64_t[(size_t)M + 1], *first = new int64_t[(size_t)M + 1];
    int32_t *dpart = new int32_t[(size_t)dcap + 1], *partner = new int32_t[(size_t)rcap + 1], *points = new int32_t[(size_t)rcap + 1];
    double *area = new double[(size_t)rcap + 1];
    for (int64_t i = 0; i <= M; ++i) first[i] = -7;
    long long d_got = -1, c_got = -1;
    int flag = -1;
    const long long got = emu_contacts_table(side_off.data(), 2 * n_pairs, x.data(), r.data(), M, probe, N, u.data(), side_masks, pair_masks, dcap, rcap,
                                             buried, dot_first, dpart, first, partner, points, area, &d_got, &c_got, &flag);
    int bad = d_got != D || c_got != C || flag != 0 || memcmp(buried, w_buried.data(), 16 * (size_t)M) != 0 || dot_first[M] != D;
    if (!bad && short_by && D > 0) {
        bad = got != -2;
        for (int64_t i = 0; i <= M && !bad; ++i) bad = first[i] != -7;
    } else if (!bad) {
        bad = got != C;
        for (int64_t i = 0; i <= M && !bad; ++i) bad = first[i] != w_first[(size_t)i];
        for (int64_t e = 0; e < D && !bad; ++e) bad = dpart[e] != w_dpart[(size_t)e];
        for (int64_t k = 0; k < C && !bad; ++k)
            bad = partner[k] != w_partner[(size_t)k] || points[k] != w_points[(size_t)k] || memcmp(area + k, w_area.data() + k, 8) != 0;
    }
    delete[] side_masks; delete[] pair_masks; delete[] buried; delete[] dot_first; delete[] first; delete[] dpart; delete[] partner; delete[] points; delete[] area;
    printf("%s %s (atoms %lld, buried dots %lld, rows %lld)\n", name, bad ? "FAILED" : "ok", (long long)M, (long long)D, (long long)C);
    return bad;
}

int main()
{
    int bad = 0;
    bad |= check_case("one-atom-sides", 9, 1, 100, false, 0);
    bad |= check_case("two-atom-sides-N1", 9, 2, 1, false, 0);
    bad |= check_case("small-sides", 6, 40, 33, false, 0);
    bad |= check_case("twins", 4, 60, 100, true, 0);
    bad |= check_case("large-sides", 2, 700, 128, false, 0);
    bad |= check_case("short-by-1", 3, 50, 31, false, 1);
    return bad;
}
#endif
