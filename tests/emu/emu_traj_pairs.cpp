/* TESTS ONLY: interfaces between chain groups per frame (freesasa_amd/csrc/traj_kernels.h, traj_pair_*) driven thread by thread
 * on the CPU in the launch order of gpu_drivers.hip - the groups' cut and the pairs' cut once, then per shard the groups' radii
 * and gather, the pairs' radii, side boundaries and gather, the engine's totals over the WHOLE combined batch, the groups' finish,
 * the totals kernels over cgath with the pair structures' chunks kept out, the groups' three columns, k_totals over the sides
 * (totals_phase0 / totals_phase1) and the six columns per (frame, pair).  The areas of the combined batch are the caller's
 * (seeded): the tile kernels are not what is under test here.  cgath's pair part is left NaN: a sum that touched it would show.
 * Never linked into the product. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

/* kl_totals over `sasa` with the chunk tables cell_sort_enqueue derives from `offs`, for the first n_first structures only:
   the chunks of the others - they lie behind in the tables - are not run */
static void totals_by_chunks(const std::vector<int64_t> &offs, int n_first, const double *sasa, double *totals)
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
    pa.n_structs = n_first; pa.n_atoms = (int)offs[n_first]; pa.offsets = offs.data();
    pa.n_chunks = sc0[n_first]; pa.chunk_struct = cs.data(); pa.chunk_begin = cb.data(); pa.chunk_len = cl.data(); pa.struct_chunk0 = sc0.data();
    std::vector<double> part(SASA_TOT_B), chunk_tot(cs.size() + 1);
    for (int k = 0; k < pa.n_chunks; ++k) {
        for (int t = 0; t < SASA_TOT_B; ++t) totals_chunk_phase0(pa, sasa, part.data(), k, t);
        for (int t = 0; t < SASA_TOT_B; ++t) totals_chunk_phase1(part.data(), chunk_tot.data(), k, t);
    }
    for (int blk = 0; blk < (n_first + 255) / 256; ++blk)
        for (int t = 0; t < 256; ++t) totals_struct(pa, chunk_tot.data(), totals, blk * 256 + t);
}

/* kl_segment_sums(..., short_segments = false): one workgroup of SASA_TOT_B threads per segment */
static void segment_sums(const double *sasa, const int64_t *seg, int n_segs, double *out)
{
    std::vector<double> part(SASA_TOT_B);
    for (int s = 0; s < n_segs; ++s) {
        for (int t = 0; t < SASA_TOT_B; ++t) totals_phase0(sasa, seg, part.data(), s, t);
        for (int t = 0; t < SASA_TOT_B; ++t) totals_phase1(part.data(), out, s, t);
    }
}

extern "C" int emu_tp_tot_b(void) { return SASA_TOT_B; }

/* k_totals over ONE segment v[0 .. len) */
extern "C" double emu_tp_ktotals(const double *v, long long len)
{
    const int64_t seg[2] = {0, len};
    double out = NAN;
    segment_sums(v, seg, 1, &out);
    return out;
}

/* the two host cuts: gfirst [G + 1], src [n], pfirst [K + 1], pside [2 K + 1], psrc [cap]; returns n_pair, -1 on a bad group
   id, -2 when psrc is too short (cap: its entries) */
extern "C" long long emu_tp_cut(const int32_t *group, int n, int n_groups, const int32_t *pairs, int n_pairs, int64_t *gfirst, int32_t *src,
                                int64_t *pfirst, int64_t *pside, int32_t *psrc, long long cap)
{
    int64_t bad = 0;
    if (traj_group_cut(group, n, n_groups, gfirst, src, &bad) < 0) return -1;
    if (traj_pair_cut(pairs, n_pairs, gfirst, src, pfirst, pside, nullptr) > cap) return -2;
    return traj_pair_cut(pairs, n_pairs, gfirst, src, pfirst, pside, psrc);
}

/* One shard of nf frames.  xyz [3 nf nc], nc = n + n_iso + n_pair: the compact frames in front (in), the isolated and the pair
 * part behind (out); cradii [nf nc] out; csasa [nf nc] the combined batch's areas (in); iso [nf n] (out, may be null); totals
 * [nf], gout [nf G 3], pout [nf K 6] and side_off [2 K nf + 1] (out).  Returns 0, -1 on a bad argument. */
extern "C" int emu_tp_shard(const int32_t *group, int n, int n_groups, const int32_t *pairs, int n_pairs, const double *radii, int nf,
                            double *xyz, double *cradii, const double *csasa, double *iso, double *totals, double *gout, double *pout,
                            int64_t *side_off)
{
    if (!group || n < 1 || n_groups < 1 || !pairs || n_pairs < 1 || nf < 1 || !xyz || !cradii || !csasa || !totals || !gout || !pout || !side_off) return -1;
    const int G = n_groups, K = n_pairs;
    std::vector<int64_t> gfirst((size_t)G + 1), pfirst((size_t)K + 1), pside(2 * (size_t)K + 1);
    std::vector<int32_t> src((size_t)n);
    int64_t bad = 0;
    const int64_t n_iso = traj_group_cut(group, n, G, gfirst.data(), src.data(), &bad);
    if (n_iso < 0) return -1;
    for (int k = 0; k < K; ++k)
        if (pairs[2 * k] < 0 || pairs[2 * k] >= pairs[2 * k + 1] || pairs[2 * k + 1] >= G) return -1;
    const int64_t n_pair = traj_pair_cut(pairs, K, gfirst.data(), src.data(), pfirst.data(), pside.data(), nullptr);
    std::vector<int32_t> psrc((size_t)n_pair + 1);
    traj_pair_cut(pairs, K, gfirst.data(), src.data(), pfirst.data(), pside.data(), psrc.data());
    const int64_t NG = (int64_t)nf * (n + n_iso), N = NG + (int64_t)nf * n_pair, NSG = (int64_t)nf * (1 + G), NS = NSG + (int64_t)nf * K;
    std::vector<int64_t> offs((size_t)NS + 1); /* (TrajRun::batch_offsets) */
    for (int k = 0; k <= nf; ++k) offs[k] = (int64_t)k * n;
    for (int f = 0; f < nf; ++f)
        for (int g = 1; g <= G; ++g) offs[(size_t)nf + (size_t)f * G + g] = (int64_t)nf * n + f * n_iso + gfirst[g];
    for (int f = 0; f < nf; ++f)
        for (int k = 1; k <= K; ++k) offs[(size_t)NSG + (size_t)f * K + k] = NG + f * n_pair + pfirst[k];
    std::vector<double> cgath((size_t)N, NAN), ctot((size_t)NS), ctot2((size_t)NSG), inpair(2 * (size_t)K * nf);
    TrajGroupArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.n_iso = (int)n_iso; a.n_groups = G; a.n_frames = nf;
    a.group = group; a.src = src.data(); a.radii = radii;
    a.xyz = xyz; a.cradii = cradii; a.csasa = csasa; a.cgath = cgath.data(); a.iso = iso;
    a.ctot = ctot.data(); a.ctot2 = ctot2.data(); a.out = gout;
    TrajPairArgs x;
    memset(&x, 0, sizeof x);
    x.n = n; x.n_iso = (int)n_iso; x.n_pair = (int)n_pair; x.n_groups = G; x.n_pairs = K; x.n_frames = nf;
    x.pairs = pairs; x.pside = pside.data(); x.psrc = psrc.data(); x.radii = radii;
    x.xyz = xyz; x.cradii = cradii; x.side_off = side_off; x.ctot = ctot.data(); x.inpair = inpair.data(); x.out = pout;
    auto launch_g = [&](int64_t threads, void (*fn)(const TrajGroupArgs &, int64_t)) {
        for (int64_t blk = 0; blk < (threads + TRAJ_B - 1) / TRAJ_B; ++blk)
            for (int t = 0; t < TRAJ_B; ++t) fn(a, blk * TRAJ_B + t);
    };
    auto launch_p = [&](int64_t threads, void (*fn)(const TrajPairArgs &, int64_t)) {
        for (int64_t blk = 0; blk < (threads + TRAJ_B - 1) / TRAJ_B; ++blk)
            for (int t = 0; t < TRAJ_B; ++t) fn(x, blk * TRAJ_B + t);
    };
    /* shard_upload */
    launch_g(NG, [](const TrajGroupArgs &q, int64_t t) { traj_group_radii(q, t); });
    launch_g(3 * (int64_t)nf * n_iso, [](const TrajGroupArgs &q, int64_t t) { traj_group_gather(q, t); });
    if (n_pair) launch_p((int64_t)nf * n_pair, [](const TrajPairArgs &q, int64_t t) { traj_pair_radii(q, t); });
    launch_p(2 * (int64_t)nf * K + 1, [](const TrajPairArgs &q, int64_t t) { traj_pair_sides(q, t); });
    if (n_pair) launch_p(3 * (int64_t)nf * n_pair, [](const TrajPairArgs &q, int64_t t) { traj_pair_gather(q, t); });
    /* shard_compute */
    totals_by_chunks(offs, (int)NS, csasa, ctot.data()); /* (the engine's d_totals) */
    launch_g(NG, [](const TrajGroupArgs &q, int64_t t) { traj_group_finish(q, t); });
    totals_by_chunks(offs, (int)NSG, cgath.data(), ctot2.data());
    launch_g((int64_t)nf * G, [](const TrajGroupArgs &q, int64_t t) { traj_group_totals(q, t); });
    segment_sums(csasa, side_off, 2 * K * nf, inpair.data());
    launch_p((int64_t)nf * K, [](const TrajPairArgs &q, int64_t t) { traj_pair_rows(q, t); });
    for (int f = 0; f < nf; ++f) totals[f] = ctot[f];
    return 0;
}
