/* TESTS ONLY: chain groups per frame (freesasa_amd/csrc/traj_kernels.h, traj_group_*) driven thread by thread on the CPU in
 * the launch order of gpu_drivers.hip - the host cut once, then per shard the radii, the gather, the finish, the totals
 * kernels over cgath with the combined batch's chunk tables (built as gpu_engine.hip builds them) and the three columns - and,
 * as the yardstick, the phase functions of freesasa_gpu_groups_dev (group_kernels.h: count, rank, finish, totals) on ONE frame
 * given as a batch of one structure.  The areas of the combined batch are the caller's (seeded): the tile kernels are not what
 * is under test here.  The 64 lanes of grp_count_atom / grp_rank_struct are fibers in lock step, as in emu_groups.cpp.
 * Never linked into the product. */
#include <stdint.h>
#include <string.h>
#include <vector>

#include <ucontext.h>

#include "../../freesasa_amd/csrc/group_kernels.h"
#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

namespace sasa_emu {
static const int W = 64;
static ucontext_t g_main, g_fiber[W];
static bool g_done[W];
static int g_lane = -1;
static long long g_dep[W], g_snap[W];
static unsigned long long g_ballot;
static void (*g_body)(int lane, void *ctx);
static void *g_ctx;
static std::vector<char> g_stacks;

static void yield_to_scheduler() { swapcontext(&g_fiber[g_lane], &g_main); }
unsigned long long wave_ballot(bool p) { g_dep[g_lane] = p ? 1 : 0; yield_to_scheduler(); return g_ballot; }
void wave_sync() { g_dep[g_lane] = 0; yield_to_scheduler(); }
long long wave_exchange(long long v, int src) { g_dep[g_lane] = v; yield_to_scheduler(); return g_snap[src]; }
static void trampoline()
{
    g_body(g_lane, g_ctx);
    g_done[g_lane] = true;
    swapcontext(&g_fiber[g_lane], &g_main);
}
static void run_wave(void (*body)(int, void *), void *ctx)
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
        unsigned long long b = 0;
        for (int l = 0; l < W; ++l) {
            if (!g_done[l] && g_dep[l]) b |= 1ull << l;
            g_snap[l] = g_dep[l];
        }
        g_ballot = b;
    }
    g_lane = -1;
}
} /* namespace sasa_emu */

/* kl_totals over `sasa` with the chunk tables run_batch_once derives from `offs` */
static void totals_by_chunks(const std::vector<int64_t> &offs, const double *sasa, double *totals)
{
    const int ns = (int)offs.size() - 1;
    std::vector<int> cs, cl, sc0((size_t)ns + 1);
    std::vector<int64_t> cb;
    for (int s = 0; s < ns; ++s) {
        sc0[s] = (int)cs.size();
        for (int64_t b = offs[s]; b < offs[s + 1]; b += SASA_BOUNDS_CHUNK) {
            const int64_t e = b + SASA_BOUNDS_CHUNK < offs[s + 1] ? b + SASA_BOUNDS_CHUNK : offs[s + 1];
            cs.push_back(s); cb.push_back(b); cl.push_back((int)(e - b));
        }
    }
    sc0[ns] = (int)cs.size();
    PipeArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.n_structs = ns; pa.n_atoms = (int)offs[ns]; pa.offsets = offs.data();
    pa.n_chunks = (int)cs.size(); pa.chunk_struct = cs.data(); pa.chunk_begin = cb.data(); pa.chunk_len = cl.data(); pa.struct_chunk0 = sc0.data();
    std::vector<double> part(SASA_TOT_B), chunk_tot(cs.size() + 1);
    for (int k = 0; k < pa.n_chunks; ++k) {
        for (int t = 0; t < SASA_TOT_B; ++t) totals_chunk_phase0(pa, sasa, part.data(), k, t);
        for (int t = 0; t < SASA_TOT_B; ++t) totals_chunk_phase1(part.data(), chunk_tot.data(), k, t);
    }
    for (int blk = 0; blk < (ns + 255) / 256; ++blk)
        for (int t = 0; t < 256; ++t) totals_struct(pa, chunk_tot.data(), totals, blk * 256 + t);
}

/* the host cut: gfirst [n_groups + 1], src [n]; returns n_iso, or -1 with the first atom that has a bad id in *bad */
extern "C" long long emu_tg_cut(const int32_t *group, int n, int n_groups, int64_t *gfirst, int32_t *src, long long *bad)
{
    int64_t b = -1;
    const int64_t r = traj_group_cut(group, n, n_groups, gfirst, src, &b);
    *bad = b;
    return r;
}

/* One shard of nf frames.  xyz [3 nf (n + n_iso)]: the compact frames in front (in), the isolated part behind (out);
 * cradii [nf (n + n_iso)] out; csasa [nf (n + n_iso)] the combined batch's areas (in); iso [nf n] (out, may be null);
 * totals [nf] and out [nf G 3] (out).  Returns 0, -1 on a bad argument. */
extern "C" int emu_tg_shard(const int32_t *group, int n, int n_groups, const double *radii, int nf, double *xyz, double *cradii,
                            const double *csasa, double *iso, double *totals, double *out)
{
    if (!group || n < 1 || n_groups < 1 || nf < 1 || !xyz || !cradii || !csasa || !totals || !out) return -1;
    std::vector<int64_t> gfirst((size_t)n_groups + 1);
    std::vector<int32_t> src((size_t)n);
    int64_t bad = 0;
    const int64_t n_iso = traj_group_cut(group, n, n_groups, gfirst.data(), src.data(), &bad);
    if (n_iso < 0) return -1;
    const int64_t N = (int64_t)nf * (n + n_iso), NS = (int64_t)nf * (1 + n_groups);
    std::vector<int64_t> offs((size_t)NS + 1); /* (TrajRun::batch_offsets) */
    for (int k = 0; k <= nf; ++k) offs[k] = (int64_t)k * n;
    for (int f = 0; f < nf; ++f)
        for (int g = 1; g <= n_groups; ++g) offs[(size_t)nf + (size_t)f * n_groups + g] = (int64_t)nf * n + f * n_iso + gfirst[g];
    std::vector<double> cgath((size_t)N), ctot((size_t)NS), ctot2((size_t)NS);
    TrajGroupArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.n_iso = (int)n_iso; a.n_groups = n_groups; a.n_frames = nf;
    a.group = group; a.src = src.data(); a.radii = radii;
    a.xyz = xyz; a.cradii = cradii; a.csasa = csasa; a.cgath = cgath.data(); a.iso = iso;
    a.ctot = ctot.data(); a.ctot2 = ctot2.data(); a.out = out;
    auto launch = [&](int64_t threads, void (*fn)(const TrajGroupArgs &, int64_t)) {
        for (int64_t blk = 0; blk < (threads + TRAJ_B - 1) / TRAJ_B; ++blk)
            for (int t = 0; t < TRAJ_B; ++t) fn(a, blk * TRAJ_B + t);
    };
    launch(N, [](const TrajGroupArgs &x, int64_t t) { traj_group_radii(x, t); });
    launch(3 * (int64_t)nf * n_iso, [](const TrajGroupArgs &x, int64_t t) { traj_group_gather(x, t); });
    totals_by_chunks(offs, csasa, ctot.data()); /* (the engine's d_totals) */
    launch(N, [](const TrajGroupArgs &x, int64_t t) { traj_group_finish(x, t); });
    totals_by_chunks(offs, cgath.data(), ctot2.data());
    launch((int64_t)nf * n_groups, [](const TrajGroupArgs &x, int64_t t) { traj_group_totals(x, t); });
    for (int f = 0; f < nf; ++f) totals[f] = ctot[f];
    return 0;
}

/* ------------------------------------------------------------------ the yardstick: group_kernels.h on a batch of ONE structure */

struct CountRun { const GrpArgs *a; int blk; int wave; };
static void count_body(int lane, void *ctx)
{
    const CountRun *r = (const CountRun *)ctx;
    grp_count_atom(*r->a, r->blk * GRP_B + r->wave * 64 + lane, lane);
}
struct RankRun { const GrpArgs *a; };
static void rank_body(int lane, void *ctx) { grp_rank_struct(*((const RankRun *)ctx)->a, 0, lane); }

/* xyz [3 n], radii [n], group [n], n_groups; csasa [n + n_iso]: the combined batch's areas (in), in the order the rank kernel
 * makes (the caller knows it: src_out of a first call with csasa NULL).  Out: src_out [n], cxyz [3 (n + n_iso)], cradii
 * [n + n_iso], sasa / iso [n], total [1], gtot [3 G].  Returns n_iso, -1 on a bad argument or id. */
extern "C" long long emu_grp_one(const double *xyz, const double *radii, const int32_t *group, int n, int n_groups, const double *csasa,
                                 int32_t *src_out, double *cxyz, double *cradii, double *sasa, double *iso, double *total, double *gtot)
{
    if (!xyz || !radii || !group || n < 1 || n_groups < 1 || !src_out) return -1;
    const int G = n_groups;
    const int64_t offsets[2] = {0, n}, gbase[2] = {0, G};
    std::vector<int> key((size_t)n), count((size_t)G + 2, 0), cursor((size_t)G + 1);
    GrpArgs a;
    memset(&a, 0, sizeof a);
    a.xyz = xyz; a.radii = radii; a.group = group; a.offsets = offsets; a.gbase = gbase;
    a.n_structs = 1; a.n_atoms = n; a.n_groups = G; a.key = key.data(); a.count = count.data();
    for (int blk = 0; blk < (n + GRP_B - 1) / GRP_B; ++blk)
        for (int w = 0; w < GRP_B / 64; ++w) {
            CountRun r = {&a, blk, w};
            sasa_emu::run_wave(count_body, &r);
        }
    if (count[(size_t)G]) return -1;
    std::vector<int64_t> comb((size_t)G + 2); /* (groups_resident's combined offsets) */
    comb[0] = 0; comb[1] = n;
    int64_t pos = n;
    for (int k = 0; k < G; ++k) { cursor[(size_t)k] = (int)pos; pos += count[(size_t)k]; comb[(size_t)k + 2] = pos; }
    const int64_t n_iso = pos - n;
    std::vector<double> xyz_c(3 * (size_t)pos), rad_c((size_t)pos);
    std::vector<int> src((size_t)n_iso + 1);
    memcpy(xyz_c.data(), xyz, 24 * (size_t)n);
    memcpy(rad_c.data(), radii, 8 * (size_t)n);
    a.cursor = cursor.data(); a.cxyz = xyz_c.data(); a.cradii = rad_c.data(); a.src = src.data(); a.n_iso = (int)n_iso;
    RankRun rr = {&a};
    sasa_emu::run_wave(rank_body, &rr);
    for (int64_t j = 0; j < n_iso; ++j) src_out[j] = src[(size_t)j];
    if (cxyz) memcpy(cxyz, xyz_c.data(), 24 * (size_t)pos);
    if (cradii) memcpy(cradii, rad_c.data(), 8 * (size_t)pos);
    if (!csasa) return n_iso;
    if (!sasa || !iso || !total || !gtot) return -1;
    std::vector<double> cgath((size_t)pos), ctot((size_t)G + 1), ctot2((size_t)G + 1);
    totals_by_chunks(comb, csasa, ctot.data());
    a.csasa = csasa; a.ctot = ctot.data(); a.ctot2 = ctot2.data(); a.cgath = cgath.data();
    a.sasa = sasa; a.iso = iso; a.totals = total; a.gtot = gtot;
    for (int64_t blk = 0; blk < (pos + GRP_B - 1) / GRP_B; ++blk)
        for (int t = 0; t < GRP_B; ++t) grp_finish_atom(a, blk * GRP_B + t);
    totals_by_chunks(comb, cgath.data(), ctot2.data());
    const int m = G > 1 ? G : 1;
    for (int blk = 0; blk < (m + GRP_B - 1) / GRP_B; ++blk)
        for (int t = 0; t < GRP_B; ++t) grp_totals_item(a, blk * GRP_B + t);
    return n_iso;
}
