/* TESTS ONLY: the phase functions of the interfaces between chain groups (freesasa_amd/csrc/iface_kernels.h) driven on the CPU as
 * gpu_interfaces.hip drives the kernels: iface_box one wave per group (four to a workgroup), iface_candidates one thread per
 * test, iface_contact one workgroup of IF_B threads per candidate, then the table made of the flags in the tests' order as the
 * host makes it, iface_gather one thread per pair-structure atom, iface_finish_atom / _row.  The IF_B threads of a workgroup are
 * fibers in lock step (as in emu_pbc.cpp): a shuffle or a barrier deposits the thread's operand and yields; the scheduler
 * resumes the threads once all have arrived; a shuffle reads within the thread's own wave of 64.  The combined batch of the
 * chain-group entry is cut here by a plain loop (its kernels have their own emulation, emu_traj_groups.cpp).
 * With -DIFACE_CHECK_MAIN: a stand-alone program (tests/emu/iface_check, built with AddressSanitizer + UBSan) that drives the
 * same phases over generated structures against a plain double loop, the outputs in heap blocks of their exact size: one
 * line per case.
 * Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include <ucontext.h>

#include "../../freesasa_amd/csrc/iface_kernels.h"

using namespace sasa;

namespace sasa_emu {
static const int W = IF_B;
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

/* the combined batch and the tables of a call, as groups_resident and iface_screen make them */
struct Combined {
    std::vector<double> cxyz, cradii;
    std::vector<int> src, cnt;
    std::vector<int64_t> gstart, gbase, tbase;
    int64_t n = 0, T = 0;
    int G = 0;
};
static int combine(const double *xyz, const double *radii, const int64_t *offsets, int ns, const int32_t *group, const int32_t *n_groups, Combined &cb)
{
    cb.n = offsets[ns];
    cb.gbase.assign((size_t)ns + 1, 0); cb.tbase.assign((size_t)ns + 1, 0);
    for (int s = 0; s < ns; ++s) {
        if (n_groups[s] < 0 || n_groups[s] > IF_MAX_GROUPS) return -1;
        cb.gbase[(size_t)s + 1] = cb.gbase[(size_t)s] + n_groups[s];
        cb.tbase[(size_t)s + 1] = cb.tbase[(size_t)s] + (int64_t)n_groups[s] * (n_groups[s] - 1) / 2;
    }
    cb.G = (int)cb.gbase[(size_t)ns]; cb.T = cb.tbase[(size_t)ns];
    if (cb.T > IF_MAX_TESTS) return -1;
    cb.cnt.assign((size_t)cb.G, 0);
    for (int s = 0; s < ns; ++s)
        for (int64_t i = offsets[s]; i < offsets[s + 1]; ++i) {
            if (group[i] < -1 || group[i] >= n_groups[s]) return -1;
            if (group[i] >= 0) ++cb.cnt[(size_t)(cb.gbase[(size_t)s] + group[i])];
        }
    cb.gstart.assign((size_t)cb.G + 1, cb.n);
    for (int k = 0; k < cb.G; ++k) cb.gstart[(size_t)k + 1] = cb.gstart[(size_t)k] + cb.cnt[(size_t)k];
    const int64_t N = cb.gstart[(size_t)cb.G];
    cb.cxyz.assign(3 * (size_t)N, 0.0); cb.cradii.assign((size_t)N, 0.0); cb.src.assign((size_t)(N - cb.n), 0);
    memcpy(cb.cxyz.data(), xyz, 24 * (size_t)cb.n);
    memcpy(cb.cradii.data(), radii, 8 * (size_t)cb.n);
    std::vector<int64_t> cur(cb.gstart.begin(), cb.gstart.end());
    for (int s = 0; s < ns; ++s)
        for (int64_t i = offsets[s]; i < offsets[s + 1]; ++i) {
            if (group[i] < 0) continue;
            const int64_t j = cur[(size_t)(cb.gbase[(size_t)s] + group[i])]++;
            for (int c = 0; c < 3; ++c) cb.cxyz[3 * (size_t)j + c] = xyz[3 * i + c];
            cb.cradii[(size_t)j] = radii[i];
            cb.src[(size_t)(j - cb.n)] = (int)i;
        }
    return 0;
}
static void base_args(const Combined &cb, int ns, double probe, IfaceArgs &a)
{
    memset(&a, 0, sizeof a);
    a.cxyz = cb.cxyz.data(); a.cradii = cb.cradii.data(); a.src = cb.src.data();
    a.n_atoms = (int)cb.n; a.n_structs = ns; a.n_groups = cb.G; a.probe = probe;
    a.gstart = cb.gstart.data(); a.gbase = cb.gbase.data(); a.tbase = cb.tbase.data(); a.n_tests = (int)cb.T;
}

struct BoxRun { const IfaceArgs *a; int k0; };
static void box_body(int tid, void *ctx)
{
    const BoxRun *r = (const BoxRun *)ctx;
    const int k = r->k0 + (tid >> 6);
    if (k < r->a->n_groups) iface_box(*r->a, k, tid & 63);
}
struct ContactRun { const IfaceArgs *a; IfaceLds *m; int c; };
static void contact_body(int tid, void *ctx)
{
    const ContactRun *r = (const ContactRun *)ctx;
    iface_contact(*r->a, *r->m, r->c, tid);
}

extern "C" void emu_iface_shape(int *threads, int *lds_atoms) { *threads = IF_B; *lds_atoms = IF_LDS_ATOMS; }

/* steps 2 to 4: box [8 G], is_cand [T], flag [T] (t_cap entries each).  Returns T, -1 on a bad argument. */
extern "C" long long emu_iface_screen(const double *xyz, const double *radii, const int64_t *offsets, int ns, const int32_t *group,
                                      const int32_t *n_groups, double probe, double *box, unsigned char *is_cand, unsigned char *flag,
                                      long long t_cap)
{
    if (!xyz || !radii || !offsets || ns <= 0 || !group || !n_groups || !box || !is_cand || !flag) return -1;
    Combined cb;
    if (combine(xyz, radii, offsets, ns, group, n_groups, cb) || cb.T > t_cap) return -1;
    IfaceArgs a;
    base_args(cb, ns, probe, a);
    std::vector<int> cand((size_t)cb.T + 1);
    int n_cand = 0;
    a.box = box; a.n_cand = &n_cand; a.cand = cand.data(); a.flag = flag;
    for (int64_t t = 0; t < cb.T; ++t) is_cand[t] = flag[t] = 0;
    for (int k0 = 0; k0 < cb.G; k0 += IF_B / 64) { /* (k_iface_box: four waves to a workgroup) */
        BoxRun r = {&a, k0};
        sasa_emu::run_group(box_body, &r);
    }
    for (int64_t t = 0; t < (cb.T + IF_B - 1) / IF_B * IF_B; ++t) iface_candidates(a, (int)t); /* (the grid, idle threads included) */
    IfaceLds *m = new IfaceLds;
    for (int c = 0; c < n_cand; ++c) {
        is_cand[cand[(size_t)c]] = 1;
        ContactRun r = {&a, m, c};
        sasa_emu::run_group(contact_body, &r);
    }
    delete m;
    return cb.T;
}

/* steps 5, 6 and 8 from the flags: the table in the tests' order (pair_struct [p_cap], pair_groups [2 p_cap], side_off
 * [2 p_cap + 1]), the gathered pair batch (pxyz [3 m_cap], pradii, pair_atom [m_cap]) and - when csasa [n + n_iso], ctot
 * [ns + G] and psasa [M] are given - pair_buried [m_cap] and pair_areas [6 p_cap], the sides summed in order.  n_pairs_out: P.
 * Returns M; -1 on a bad argument, -2 when a capacity is too small (nothing written but *n_pairs_out). */
extern "C" long long emu_iface_table(const double *xyz, const double *radii, const int64_t *offsets, int ns, const int32_t *group,
                                     const int32_t *n_groups, const unsigned char *flag, const double *csasa, const double *ctot,
                                     const double *psasa, long long p_cap, long long m_cap, long long *n_pairs_out, int32_t *pair_struct,
                                     int32_t *pair_groups, int64_t *side_off, double *pxyz, double *pradii, int32_t *pair_atom,
                                     double *pair_buried, double *pair_areas)
{
    if (!xyz || !radii || !offsets || ns <= 0 || !group || !n_groups || !flag || !n_pairs_out) return -1;
    Combined cb;
    if (combine(xyz, radii, offsets, ns, group, n_groups, cb)) return -1;
    std::vector<int32_t> ps, pg, sg;
    std::vector<int64_t> so(1, 0), ss;
    int64_t t = 0, M = 0;
    for (int s = 0; s < ns; ++s)
        for (int g = 0; g + 1 < n_groups[s]; ++g)
            for (int h = g + 1; h < n_groups[s]; ++h, ++t) {
                if (!flag[t]) continue;
                ps.push_back(s); pg.push_back(g); pg.push_back(h);
                for (int side = 0; side < 2; ++side) {
                    const int64_t k = cb.gbase[(size_t)s] + (side ? h : g);
                    ss.push_back(cb.gstart[(size_t)k]); sg.push_back((int32_t)k);
                    M += cb.cnt[(size_t)k];
                    so.push_back(M);
                }
            }
    const int64_t P = (int64_t)ps.size();
    *n_pairs_out = P;
    if (P > p_cap || M > m_cap) return -2;
    if (!pair_struct || !pair_groups || !side_off || !pxyz || !pradii || !pair_atom) return -1;
    memcpy(side_off, so.data(), 8 * so.size());
    if (P == 0) return 0;
    memcpy(pair_struct, ps.data(), 4 * (size_t)P);
    memcpy(pair_groups, pg.data(), 8 * (size_t)P);
    IfaceArgs a;
    base_args(cb, ns, 0.0, a);
    std::vector<int> pcomb((size_t)M);
    std::vector<double> inpair(2 * (size_t)P, 0.0);
    a.n_sides = 2 * P; a.n_pair_atoms = M;
    a.side_off = so.data(); a.side_start = ss.data(); a.side_group = sg.data();
    a.pxyz = pxyz; a.pradii = pradii; a.pcomb = pcomb.data(); a.pair_atom = pair_atom;
    for (int64_t m = 0; m < (M + IF_B - 1) / IF_B * IF_B; ++m) iface_gather(a, m);
    if (csasa && ctot && psasa && pair_areas) {
        for (int64_t q = 0; q < 2 * P; ++q)
            for (int64_t m = so[(size_t)q]; m < so[(size_t)q + 1]; ++m) inpair[(size_t)q] += psasa[m];
        a.csasa = csasa; a.ctot = ctot; a.psasa = psasa; a.inpair = inpair.data(); a.pair_buried = pair_buried; a.pair_areas = pair_areas;
        for (int64_t m = 0; m < (M + IF_B - 1) / IF_B * IF_B; ++m) iface_finish_atom(a, m);
        for (int64_t p = 0; p < (P + IF_B - 1) / IF_B * IF_B; ++p) iface_finish_row(a, p);
    }
    return M;
}

#ifdef IFACE_CHECK_MAIN
/* a small generator of its own: the cases are the program's, whatever the C library */
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() % 1000001) / 1000000.0; }

struct Case {
    std::vector<double> xyz, radii;
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> group, n_groups;
    /* a cloud of `count` atoms of group g in a cube of edge `edge` at (cx, cy, cz), into the structure being built */
    void cloud(int g, int count, double cx, double cy, double cz, double edge)
    {
        for (int i = 0; i < count; ++i) {
            xyz.push_back(cx + uni(0, edge)); xyz.push_back(cy + uni(0, edge)); xyz.push_back(cz + uni(0, edge));
            radii.push_back(uni(1.0, 2.0)); group.push_back(g);
        }
    }
    void end_struct(int ng) { offsets.push_back((int64_t)radii.size()); n_groups.push_back(ng); }
};

static int check(const char *name, Case &cs, long long short_p, long long short_m)
{
    const double probe = 1.4;
    const int ns = (int)cs.n_groups.size();
    const int64_t n = cs.offsets.back();
    int64_t T = 0, G = 0;
    for (int s = 0; s < ns; ++s) { T += (int64_t)cs.n_groups[(size_t)s] * (cs.n_groups[(size_t)s] - 1) / 2; G += cs.n_groups[(size_t)s]; }
    double *box = new double[(size_t)(8 * G) + 1]; /* (their exact sizes: a write behind one is the sanitizer's to find) */
    unsigned char *is_cand = new unsigned char[(size_t)T + 1], *flag = new unsigned char[(size_t)T + 1];
    int bad = emu_iface_screen(cs.xyz.data(), cs.radii.data(), cs.offsets.data(), ns, cs.group.data(), cs.n_groups.data(), probe, box, is_cand, flag, T) != T;
    /* the plain double loop */
    std::vector<unsigned char> want((size_t)T, 0);
    std::vector<int64_t> sizes;
    int64_t t = 0, P = 0, M = 0;
    for (int s = 0; s < ns && !bad; ++s)
        for (int g = 0; g + 1 < cs.n_groups[(size_t)s]; ++g)
            for (int h = g + 1; h < cs.n_groups[(size_t)s]; ++h, ++t) {
                int64_t ng_ = 0, nh_ = 0;
                for (int64_t i = cs.offsets[(size_t)s]; i < cs.offsets[(size_t)s + 1]; ++i) {
                    ng_ += cs.group[(size_t)i] == g; nh_ += cs.group[(size_t)i] == h;
                    if (cs.group[(size_t)i] != g || want[(size_t)t]) continue;
                    for (int64_t j = cs.offsets[(size_t)s]; j < cs.offsets[(size_t)s + 1] && !want[(size_t)t]; ++j) {
                        if (cs.group[(size_t)j] != h) continue;
                        const double ri = cs.radii[(size_t)i] + probe, rj = cs.radii[(size_t)j] + probe, cut2 = (ri + rj) * (ri + rj);
                        const double dx = cs.xyz[3 * (size_t)j] - cs.xyz[3 * (size_t)i], dy = cs.xyz[3 * (size_t)j + 1] - cs.xyz[3 * (size_t)i + 1],
                                     dz = cs.xyz[3 * (size_t)j + 2] - cs.xyz[3 * (size_t)i + 2];
                        if (dx * dx + dy * dy + dz * dz < cut2) want[(size_t)t] = 1;
                    }
                }
                if (want[(size_t)t]) { ++P; M += ng_ + nh_; sizes.push_back(ng_); sizes.push_back(nh_); }
                if (flag[t] != want[(size_t)t] || (want[(size_t)t] && !is_cand[t])) bad = 1;
            }
    /* the table and the gather, at the capacities asked for */
    const int64_t pc = P > short_p ? P - short_p : 0, mc = M > short_m ? M - short_m : 0;
    int32_t *ps = new int32_t[(size_t)pc + 1], *pg = new int32_t[2 * (size_t)pc + 1], *pa = new int32_t[(size_t)mc + 1];
    int64_t *so = new int64_t[2 * (size_t)pc + 1];
    double *px = new double[3 * (size_t)mc + 1], *pr = new double[(size_t)mc + 1], *pb = new double[(size_t)mc + 1], *ar = new double[6 * (size_t)pc + 1];
    std::vector<double> csasa((size_t)(2 * n) + 1), ctot((size_t)(ns + G) + 1), psasa((size_t)M + 1);
    for (double &v : csasa) v = uni(0, 50);
    for (double &v : ctot) v = uni(0, 5000);
    for (double &v : psasa) v = uni(0, 50);
    long long np = -1;
    const long long got = emu_iface_table(cs.xyz.data(), cs.radii.data(), cs.offsets.data(), ns, cs.group.data(), cs.n_groups.data(), flag,
                                          csasa.data(), ctot.data(), psasa.data(), pc, mc, &np, ps, pg, so, px, pr, pa, pb, ar);
    if (!bad) {
        if (short_p || short_m) bad = P > 0 ? got != -2 || np != P : got != M;
        else {
            bad = got != M || np != P || so[2 * P] != M;
            for (int64_t q = 0; q < 2 * P && !bad; ++q) bad = so[q + 1] - so[q] != sizes[(size_t)q];
            for (int64_t m = 0; m < M && !bad; ++m) {
                const int32_t i = pa[m];
                bad = i < 0 || i >= n || px[3 * m] != cs.xyz[3 * (size_t)i] || px[3 * m + 1] != cs.xyz[3 * (size_t)i + 1] ||
                      px[3 * m + 2] != cs.xyz[3 * (size_t)i + 2] || pr[m] != cs.radii[(size_t)i];
            }
            for (int64_t p = 0; p < P && !bad; ++p) bad = ar[6 * p + 4] != ar[6 * p] - ar[6 * p + 2] || ar[6 * p + 5] != ar[6 * p + 1] - ar[6 * p + 3];
        }
    }
    delete[] box; delete[] is_cand; delete[] flag; delete[] ps; delete[] pg; delete[] pa; delete[] so; delete[] px; delete[] pr; delete[] pb; delete[] ar;
    printf("%s %s (pairs %lld, atoms %lld)\n", name, bad ? "FAILED" : "ok", (long long)P, (long long)M);
    return bad;
}

int main()
{
    int bad = 0;
    { /* group sizes around the wave and the workgroup, an empty group, atoms in no group, touching and apart */
        Case cs;
        const int sizes[7] = {0, 1, 63, 64, 65, 256, 257};
        for (int g = 0; g < 7; ++g) cs.cloud(g, sizes[g], 14.0 * (g % 4), 14.0 * (g / 4), 0.0, 12.0);
        cs.cloud(-1, 40, 0, 0, 0, 30.0);
        cs.end_struct(7);
        cs.cloud(0, 300, 0, 0, 0, 15.0); /* one group */
        cs.end_struct(1);
        cs.cloud(-1, 10, 0, 0, 0, 15.0); /* no group */
        cs.end_struct(0);
        cs.cloud(0, 70, 0, 0, 0, 10.0); cs.cloud(1, 70, 11.0, 0, 0, 10.0); cs.cloud(2, 5, 200.0, 0, 0, 3.0);
        cs.end_struct(3);
        bad |= check("sizes", cs, 0, 0);
        bad |= check("sizes-rows-short-by-1", cs, 1, 0);
        bad |= check("sizes-atoms-short-by-1", cs, 0, 1);
    }
    { /* interleaved atom by atom, and globules placed diagonally: boxes close, atoms apart */
        Case cs;
        for (int i = 0; i < 600; ++i) cs.cloud(i % 3, 1, 0, 0, 0, 20.0);
        cs.end_struct(3);
        cs.cloud(0, 200, 0, 0, 0, 12.0); cs.cloud(1, 200, 16.5, 16.5, 16.5, 12.0); cs.cloud(0, 1, 40.0, 0, 0, 0.1); cs.cloud(1, 1, 0, 40.0, 0, 0.1);
        cs.end_struct(2);
        bad |= check("interleaved-and-diagonal", cs, 0, 0);
    }
    { /* more survivors than LDS holds: a hit (two interleaved clouds) and no hit (a sparse grid around atoms that touch none of it) */
        Case cs;
        for (int i = 0; i < 2 * (IF_LDS_ATOMS + 80); ++i) cs.cloud(i & 1, 1, 0, 0, 0, 40.0);
        cs.end_struct(2);
        for (int i = 0; i < 11; ++i)
            for (int j = 0; j < 11; ++j)
                for (int k = 0; k < 10; ++k) { cs.xyz.push_back(10.0 * i); cs.xyz.push_back(10.0 * j); cs.xyz.push_back(10.0 * k); cs.radii.push_back(1.5); cs.group.push_back(1); }
        for (int i = 0; i < 1000; ++i) { cs.xyz.push_back(5.0 + 10.0 * (i % 10)); cs.xyz.push_back(5.0 + 10.0 * ((i / 10) % 10)); cs.xyz.push_back(5.0 + 10.0 * (i / 100)); cs.radii.push_back(1.5); cs.group.push_back(0); }
        cs.end_struct(2);
        bad |= check("lds-overflow", cs, 0, 0);
    }
    { /* many groups: the decode of a test into its row */
        Case cs;
        for (int g = 0; g < 90; ++g) cs.cloud(g, 1 + g % 5, 9.0 * (g % 10), 9.0 * (g / 10), 0, 6.0);
        cs.end_struct(90);
        bad |= check("ninety-groups", cs, 0, 0);
    }
    return bad;
}
#endif
