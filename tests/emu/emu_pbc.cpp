/* TESTS ONLY: the phase functions of periodic images (freesasa_amd/csrc/pbc_kernels.h) driven on the CPU as gpu_periodic.hip
 * drives the kernels: pbc_count_struct one workgroup of PBC_B threads per structure, then the expanded offsets made of its
 * image counts, pbc_emit_atom one thread per atom, and (emu_pbc_collect) pbc_collect_atom one thread per atom.  The PBC_B
 * threads of a workgroup are fibers in lock step (as the 64 lanes of a wave are in emu_groups.cpp): a shuffle or a barrier
 * deposits the thread's operand and yields; the scheduler resumes the threads once all have arrived.  A shuffle reads within
 * the thread's own wave of 64.  Never linked into the product. */
#include <stdint.h>
#include <string.h>
#include <vector>

#include <ucontext.h>

#include "../../freesasa_amd/csrc/pbc_kernels.h"

using namespace sasa;

namespace sasa_emu {
static const int W = PBC_B;
static ucontext_t g_main, g_fiber[W];
static bool g_done[W];
static int g_lane = -1;
static long long g_dep[W], g_snap[W];
static unsigned long long g_ballot[W / 64];
static void (*g_body)(int tid, void *ctx);
static void *g_ctx;
static std::vector<char> g_stacks;

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
    if (g_stacks.empty()) g_stacks.resize(STK * W);
    g_body = body; g_ctx = ctx;
    for (int l = 0; l < W; ++l) {
        getcontext(&g_fiber[l]);
        g_fiber[l].uc_stack.ss_sp = g_stacks.data() + STK * l;
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

struct Run { const PbcArgs *a; double *lds_d; int *lds_w; int s; };
static void count_body(int tid, void *ctx)
{
    const Run *r = (const Run *)ctx;
    pbc_count_struct(*r->a, r->lds_d, r->lds_w, r->s, tid);
}

/* xyz [3 n], radii [n] (shared_radii: [n_fixed]), offsets [n_structs + 1] (NULL: n_fixed atoms per structure), cells
 * [3 n_structs].  Out: n_img [n_structs], rmax [n_structs], ibase [n], eoff [n_structs + 1]; exyz / eradii, when not NULL,
 * hold cap atoms: filled when the expanded batch fits.  Returns the expanded batch's atoms, -1 on a bad argument. */
extern "C" long long emu_pbc_expand(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, int n_fixed, int shared_radii,
                                    const double *cells, double probe, int64_t *n_img, double *rmax, int *ibase, int64_t *eoff,
                                    double *exyz, double *eradii, long long cap)
{
    if (!xyz || !radii || !cells || n_structs <= 0 || !n_img || !rmax || !ibase || !eoff || (!offsets && n_fixed <= 0)) return -1;
    PbcArgs a;
    memset(&a, 0, sizeof a);
    a.xyz = xyz; a.radii = radii; a.offsets = offsets; a.cells = cells;
    a.n_structs = n_structs; a.n_fixed = offsets ? 0 : n_fixed; a.shared_radii = shared_radii;
    a.n_atoms = offsets ? offsets[n_structs] : (int64_t)n_structs * n_fixed;
    a.probe = probe;
    a.ibase = ibase; a.n_img = n_img; a.rmax = rmax;
    double lds_d[PBC_B];
    int lds_w[PBC_WAVES];
    for (int s = 0; s < n_structs; ++s) { /* (k_pbc_count: one workgroup per structure) */
        Run r = {&a, lds_d, lds_w, s};
        sasa_emu::run_group(count_body, &r);
    }
    eoff[0] = 0;
    for (int s = 0; s < n_structs; ++s) eoff[s + 1] = eoff[s] + (pbc_begin(a, s + 1) - pbc_begin(a, s)) + n_img[s];
    if (exyz && eradii && eoff[n_structs] <= cap) {
        a.eoff = eoff; a.exyz = exyz; a.eradii = eradii;
        for (int64_t t = 0; t < (a.n_atoms + PBC_B - 1) / PBC_B * PBC_B; ++t) pbc_emit_atom(a, t); /* (k_pbc_emit's grid, idle threads included) */
    }
    return eoff[n_structs];
}

/* sasa [n] <- esasa [eoff[n_structs]] */
extern "C" int emu_pbc_collect(const int64_t *offsets, int n_structs, int n_fixed, const int64_t *eoff, const double *esasa, double *sasa)
{
    if (n_structs <= 0 || !eoff || !esasa || !sasa || (!offsets && n_fixed <= 0)) return -1;
    PbcArgs a;
    memset(&a, 0, sizeof a);
    a.offsets = offsets; a.n_structs = n_structs; a.n_fixed = offsets ? 0 : n_fixed;
    a.n_atoms = offsets ? offsets[n_structs] : (int64_t)n_structs * n_fixed;
    a.eoff = eoff; a.esasa = esasa; a.sasa = sasa;
    for (int64_t t = 0; t < (a.n_atoms + PBC_B - 1) / PBC_B * PBC_B; ++t) pbc_collect_atom(a, t);
    return 0;
}
