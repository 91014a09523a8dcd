/* TESTS ONLY: the phase function of the group-ids kernel (freesasa_amd/csrc/group_kernels.h, gid_struct) driven on the CPU
 * over a loaded batch, one wave per structure as k_gid_struct launches it.  The 64 lanes of a wave are fibers in lock step
 * (as in emu.cpp): a cross-lane operation deposits the lane's operand and yields; the scheduler resumes the lanes once all
 * have arrived.  The spec comes parsed from the product library (freesasa_ingest_chain_groups_parse); this file sorts the
 * labels as gpu_groups.hip does and runs the kernel.  Never linked into the product. */
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

#include <ucontext.h>

#include "freesasa_ingest.h"
#include "../../freesasa_amd/csrc/group_kernels.h"

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

struct Run { const GidArgs *a; unsigned *present; int s; };
static void lane_body(int lane, void *ctx)
{
    const Run *r = (const Run *)ctx;
    gid_struct(*r->a, r->present, r->s, lane);
}

/* labels [4 * n_lab] / label_group [n_lab] in the spec's order (n_lab 0: separate chains), n_spec_groups; the batch's arrays.
 * group_out [n_atoms], n_groups_out / status_out [n_structs].  Returns 0, -1 on a bad argument. */
extern "C" int emu_group_ids(const char *labels, const int32_t *label_group, int n_lab, int n_spec_groups, const freesasa_ingest_batch *b,
                             int32_t *group_out, int32_t *n_groups_out, int32_t *status_out)
{
    if (!b || !group_out || !n_groups_out || !status_out || n_lab < 0 || n_lab > GID_MAX_LABELS) return -1;
    const int ns = b->n_structs;
    const int64_t R = b->n_residues;
    if (ns <= 0) return 0;
    std::vector<std::pair<uint32_t, int32_t>> tab((size_t)n_lab);
    for (int i = 0; i < n_lab; ++i) { uint32_t w; memcpy(&w, labels + 4 * i, 4); tab[(size_t)i] = {w, label_group[i]}; }
    std::sort(tab.begin(), tab.end());
    std::vector<uint32_t> lab((size_t)n_lab), chain((size_t)R);
    std::vector<int32_t> grp((size_t)n_lab), st((size_t)ns, 0);
    for (int i = 0; i < n_lab; ++i) { lab[(size_t)i] = tab[(size_t)i].first; grp[(size_t)i] = tab[(size_t)i].second; }
    if (R > 0) memcpy(chain.data(), b->res_chain, 4 * (size_t)R);
    if (b->status) memcpy(st.data(), b->status, 4 * (size_t)ns);
    const int64_t zero = 0;
    GidArgs a;
    memset(&a, 0, sizeof a);
    a.offsets = b->offsets; a.n_structs = ns;
    a.res_first = R > 0 ? b->res_first : &zero; a.n_res = R; a.n_res_dev = 0;
    a.chain_h = chain.data();
    a.status = st.data();
    a.lab = lab.data(); a.lab_group = grp.data(); a.n_lab = n_lab; a.n_spec_groups = n_spec_groups;
    a.group = group_out; a.n_groups = n_groups_out; a.group_status = status_out;
    unsigned present[GID_MAX_LABELS / 32];
    for (int s = 0; s < ns; ++s) {
        Run r = {&a, present, s};
        sasa_emu::run_wave(lane_body, &r);
    }
    return 0;
}
