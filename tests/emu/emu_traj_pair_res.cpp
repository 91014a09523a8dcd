/* TESTS ONLY: the per-residue interface tables per frame (freesasa_amd/csrc/traj_kernels.h, traj_pair_res_cut and traj_pair_res)
 * driven on the CPU: the groups' cut, the pairs' cut and the segments once, then traj_pair_res thread by thread in the grid of
 * gpu_kernels.hip (workgroups of 64, the last one padded) over the areas of a combined batch that are the caller's (seeded): the
 * tile kernels are not what is under test here.  With -DPAIR_RES_CHECK_MAIN a stand-alone program for the sanitizers: the cut
 * and the kernel on a small topology in blocks of exactly their size.  Never linked into the product. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

#define EMU_PRES_B 64 /* TRAJ_PRES_B (gpu_kernels.hip) */

struct Cut {
    std::vector<int64_t> gfirst, pfirst, pside, seg_first, seg_iso;
    std::vector<int32_t> src, psrc, seg_res, seg_side;
    int64_t n_iso = 0, n_pair = 0, S = 0;
};

/* 0, -1 on a bad group id or pair */
static int make_cut(const int32_t *group, int n, int G, const int32_t *pairs, int K, const int64_t *res_first, int n_res, Cut &c)
{
    c.gfirst.resize((size_t)G + 1); c.src.resize((size_t)n); c.pfirst.resize((size_t)K + 1); c.pside.resize(2 * (size_t)K + 1);
    int64_t bad = 0;
    c.n_iso = traj_group_cut(group, n, G, c.gfirst.data(), c.src.data(), &bad);
    if (c.n_iso < 0) return -1;
    for (int k = 0; k < K; ++k)
        if (pairs[2 * k] < 0 || pairs[2 * k] >= pairs[2 * k + 1] || pairs[2 * k + 1] >= G) return -1;
    c.n_pair = traj_pair_cut(pairs, K, c.gfirst.data(), c.src.data(), c.pfirst.data(), c.pside.data(), nullptr);
    c.psrc.resize((size_t)c.n_pair);
    traj_pair_cut(pairs, K, c.gfirst.data(), c.src.data(), c.pfirst.data(), c.pside.data(), c.psrc.data());
    c.S = traj_pair_res_cut(pairs, K, c.gfirst.data(), c.pside.data(), c.psrc.data(), res_first, n_res, nullptr, nullptr, nullptr, nullptr);
    c.seg_first.resize((size_t)c.S + 1); c.seg_iso.resize((size_t)c.S); c.seg_res.resize((size_t)c.S); c.seg_side.resize((size_t)c.S);
    traj_pair_res_cut(pairs, K, c.gfirst.data(), c.pside.data(), c.psrc.data(), res_first, n_res, c.seg_first.data(), c.seg_res.data(),
                      c.seg_side.data(), c.seg_iso.data());
    return 0;
}

/* the segments: returns S (-1: bad argument); with cap >= S seg_first [S + 1], seg_res, seg_side, seg_iso [S] */
extern "C" long long emu_tpr_cut(const int32_t *group, int n, int n_groups, const int32_t *pairs, int n_pairs, const int64_t *res_first, int n_res,
                                 long long cap, int64_t *seg_first, int32_t *seg_res, int32_t *seg_side, int64_t *seg_iso)
{
    Cut c;
    if (make_cut(group, n, n_groups, pairs, n_pairs, res_first, n_res, c)) return -1;
    if (cap < c.S) return c.S;
    memcpy(seg_first, c.seg_first.data(), 8 * ((size_t)c.S + 1));
    if (c.S) {
        memcpy(seg_res, c.seg_res.data(), 4 * (size_t)c.S); memcpy(seg_side, c.seg_side.data(), 4 * (size_t)c.S);
        memcpy(seg_iso, c.seg_iso.data(), 8 * (size_t)c.S);
    }
    return c.S;
}

/* One shard of nf frames: csasa [nf (n + n_iso + n_pair)] the combined batch's areas (in), out [nf S 4].  0, -1: bad argument */
extern "C" int emu_tpr_shard(const int32_t *group, int n, int n_groups, const int32_t *pairs, int n_pairs, const int64_t *res_first, int n_res,
                             int nf, const double *csasa, double min_buried, double *out)
{
    Cut c;
    if (nf < 1 || make_cut(group, n, n_groups, pairs, n_pairs, res_first, n_res, c)) return -1;
    TrajPairResArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.n_iso = (int)c.n_iso; a.n_pair = (int)c.n_pair; a.n_seg = (int)c.S; a.n_frames = nf;
    a.seg_first = c.seg_first.data(); a.seg_iso = c.seg_iso.data(); a.csasa = csasa; a.min_buried = min_buried; a.out = out;
    const int64_t threads = (int64_t)nf * c.S;
    for (int64_t blk = 0; blk < (threads + EMU_PRES_B - 1) / EMU_PRES_B; ++blk)
        for (int t = 0; t < EMU_PRES_B; ++t) traj_pair_res(a, blk * EMU_PRES_B + t);
    return 0;
}

#ifdef PAIR_RES_CHECK_MAIN
/* 40 atoms, residues of 0, 3, 0, 5, 1, 17, 14, 0 atoms, three groups and atoms in no group, one group empty, group 0 in two pairs;
   every array handed over is a heap block of exactly its size */
int main(void)
{
    const int n = 40, G = 4, K = 3, R = 8, nf = 3;
    std::vector<int64_t> res_first = {0, 0, 3, 3, 8, 9, 26, 40, 40};
    std::vector<int32_t> group((size_t)n), pairs = {0, 1, 0, 2, 1, 3};
    for (int i = 0; i < n; ++i) group[(size_t)i] = i % 7 == 6 ? -1 : i < 5 ? 0 : i < 20 ? 1 : i < 24 ? 0 : 2;
    Cut c;
    if (make_cut(group.data(), n, G, pairs.data(), K, res_first.data(), R, c)) { printf("cut failed\n"); return 1; }
    int64_t atoms = 0;
    for (int64_t s = 0; s < c.S; ++s) {
        const int64_t len = c.seg_first[(size_t)s + 1] - c.seg_first[(size_t)s];
        if (len < 1 || c.seg_res[(size_t)s] < 0 || c.seg_res[(size_t)s] >= R || c.seg_iso[(size_t)s] + len > c.n_iso) { printf("segment %lld is off\n", (long long)s); return 1; }
        atoms += len;
    }
    if (atoms != c.n_pair) { printf("the segments do not cover the pair part\n"); return 1; }
    printf("cut ok\n");
    const int64_t nc = n + c.n_iso + c.n_pair;
    std::vector<double> csasa((size_t)(nf * nc)), out((size_t)(nf * c.S * 4), NAN);
    for (size_t i = 0; i < csasa.size(); ++i) csasa[i] = (double)((i * 2654435761u) % 1000) / 16.0;
    if (emu_tpr_shard(group.data(), n, G, pairs.data(), K, res_first.data(), R, nf, csasa.data(), 1.0, out.data())) { printf("shard failed\n"); return 1; }
    for (size_t i = 0; i < out.size(); ++i)
        if (isnan(out[i])) { printf("value %zu was not written\n", i); return 1; }
    for (int64_t t = 0; t < nf * c.S; ++t)
        if (out[(size_t)(4 * t + 2)] != out[(size_t)(4 * t)] - out[(size_t)(4 * t + 1)] || out[(size_t)(4 * t + 3)] != (out[(size_t)(4 * t + 2)] > 1.0 ? 1.0 : 0.0)) { printf("row %lld is off\n", (long long)t); return 1; }
    printf("shard ok\n");
    return 0;
}
#endif
