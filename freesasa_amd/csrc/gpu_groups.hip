/*
 * gpu_groups.hip — chain groups (include/freesasa_gpu.h, freesasa_gpu_groups_dev / freesasa_gpu_calc_groups): the area
 * of every atom in its complex and in its group cut out as a structure of its own (ref: freesasa_structure_get_chains_lcl,
 * src/structure.c:1026-1080, without the re-classification), in ONE batch.  Host code; the kernels are in
 * gpu_kernels.hip (phase functions: group_kernels.h).
 *
 *   1. count and validate   k_grp_count: atoms per group, bad ids into the status words; the counts come back to the
 *                           host (the batch's offsets are a host array)
 *   2. stable cut           k_grp_rank: every group's atoms, in input order, behind the complex structures: one
 *                           combined batch (32 bytes per atom: xyz and radius) and the source index of each atom
 *   3. one run_batch        the complex and all its groups share one cell sort and one sequence of tile launches
 *   4. finish               k_grp_finish (areas back to input order), the totals kernels over the groups' complex
 *                           areas, k_grp_totals
 *
 * groups_cut is stages 1 and 2 alone, for chain groups among periodic images (gpu_periodic.hip puts the periodic stage between
 * the cut and the finish).  groups_resident is that pipeline for callers whose arrays are on the context's stream (the file sweep, gpu_sweep.hip);
 * freesasa_gpu_calc_groups brings host arrays to it as the grouped host batch (group_batch_upload / _download: the host-batch
 * path's sizing, upload and failure epilogue - chunk_size, chunk_upload, chunk_failed: gpu_hostbatch.hip - and the groups'
 * extras), which its periodic forms (gpu_periodic.hip) and the interface entries (gpu_interfaces.hip) share; below it, the
 * group ids themselves made on the device from residues and chain labels (k_gid_struct).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

#include "engine_internal.h"

using namespace sasa;

static_assert(GID_EGROUP == FREESASA_INGEST_EGROUP && GID_MAX_PER_STRUCT == GRP_MAX_PER_STRUCT && GID_MAX_LABELS == FREESASA_INGEST_MAX_GROUP_LABELS, "group_kernels.h");

/* (engine_internal.h) */
int groups_cut(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
               const int32_t *d_group, const int32_t *n_groups, GrpArgs &ga, std::vector<int64_t> &comb, std::vector<int> &cnt)
{
    const int64_t n64 = offsets[n_structs];
    if (n64 <= 0) return ctx_fail(c, "empty batch");
    if (n64 > (int64_t)1 << 30) return ctx_fail(c, "batch too large (max 2^30 atoms per call)");
    const int n = (int)n64;
    /* offsets and the group bases, one upload */
    std::vector<int64_t> meta(2 * ((size_t)n_structs + 1));
    int64_t G64 = 0;
    for (int s = 0; s < n_structs; ++s) {
        if (n_groups[s] < 0 || n_groups[s] > GRP_MAX_PER_STRUCT)
            return ctx_fail(c, "n_groups[%d] = %d is outside 0 .. %d", s, n_groups[s], GRP_MAX_PER_STRUCT);
        meta[s] = offsets[s];
        meta[(size_t)n_structs + 1 + s] = G64;
        G64 += n_groups[s];
    }
    meta[n_structs] = offsets[n_structs];
    meta[2 * (size_t)n_structs + 1] = G64;
    if (G64 + n_structs > (int64_t)1 << 30) return ctx_fail(c, "too many groups (max 2^30 structures and groups per call)");
    const int G = (int)G64;

    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (ensure(c, c->g_meta, meta.size() * sizeof(int64_t)) || ensure(c, c->g_key, 4 * (size_t)n) ||
        ensure(c, c->g_count, 4 * ((size_t)G + 2)))
        return -1;
    memset(&ga, 0, sizeof ga);
    ga.xyz = d_xyz; ga.radii = d_radii; ga.group = d_group;
    ga.offsets = (const int64_t *)c->g_meta.p; ga.gbase = ga.offsets + n_structs + 1;
    ga.n_structs = n_structs; ga.n_atoms = n; ga.n_groups = G;
    ga.key = (int *)c->g_key.p; ga.count = (int *)c->g_count.p;

    /* 1. count and validate; the counts and the two status words back (stream sync 1 of 2 beyond run_batch's) */
    HIP_TRY(c, hipMemcpyAsync(c->g_meta.p, meta.data(), meta.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->g_count.p, 0, 4 * ((size_t)G + 2), st));
    HIP_TRY(c, kl_grp_count(ga, st));
    cnt.assign((size_t)G + 2, 0);
    HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->g_count.p, 4 * ((size_t)G + 2), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (cnt[G]) {
        const int64_t i = (int64_t)cnt[(size_t)G + 1] - 1;
        int32_t g = 0;
        HIP_TRY(c, hipMemcpy(&g, d_group + i, sizeof g, hipMemcpyDeviceToHost));
        int s = 0;
        while (s + 1 < n_structs && offsets[s + 1] <= i) ++s;
        return ctx_fail(c, "atom %lld (structure %d) has group id %d: ids are -1 .. n_groups[s] - 1 = %d", (long long)i, s, g,
                        n_groups[s] - 1);
    }

    /* the combined batch: the complex structures, then every group as a structure */
    comb.assign((size_t)n_structs + G + 1, 0);
    cnt.resize(2 * (size_t)G + 3); /* (the cursors behind the counts: the caller's vector outlives the stream's read of them) */
    int *const cursor = cnt.data() + G + 2;
    for (int s = 0; s <= n_structs; ++s) comb[s] = offsets[s];
    int64_t pos = n;
    for (int k = 0; k < G; ++k) {
        cursor[k] = (int)pos;
        pos += cnt[k];
        comb[(size_t)n_structs + 1 + k] = pos;
    }
    const int64_t n_iso = pos - n;
    if (pos > (int64_t)1 << 30) return ctx_fail(c, "batch and groups too large (max 2^30 atoms per call together)");
    const size_t N = (size_t)pos, NS = (size_t)n_structs + G;
    if (ensure(c, c->g_cursor, 4 * ((size_t)G + 1)) || ensure(c, c->g_xyz, 24 * N) || ensure(c, c->g_radii, 8 * N) ||
        ensure(c, c->g_src, 4 * ((size_t)n_iso + 1)) || ensure(c, c->g_sasa, 8 * N) || ensure(c, c->g_gath, 8 * N) ||
        ensure(c, c->g_tot, 8 * NS) || ensure(c, c->g_tot2, 8 * NS))
        return -1;
    ga.cursor = (int *)c->g_cursor.p; ga.cxyz = (double *)c->g_xyz.p; ga.cradii = (double *)c->g_radii.p;
    ga.src = (int *)c->g_src.p; ga.n_iso = (int)n_iso;

    /* 2. the stable cut */
    HIP_TRY(c, hipMemcpyAsync(c->g_xyz.p, d_xyz, 24 * (size_t)n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->g_radii.p, d_radii, 8 * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (G > 0) {
        HIP_TRY(c, hipMemcpyAsync(c->g_cursor.p, cursor, 4 * (size_t)G, hipMemcpyHostToDevice, st));
        HIP_TRY(c, kl_grp_rank(ga, st));
    }
    return 0;
}

/* (engine_internal.h) */
int groups_resident(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                    const int32_t *d_group, const int32_t *n_groups, double probe, int resolution, const double *unit_points,
                    double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals, std::vector<int> *counts_out)
{
    GrpArgs ga;
    std::vector<int64_t> comb;
    std::vector<int> cnt;
    if (groups_cut(c, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, ga, comb, cnt)) return -1;
    const int G = ga.n_groups;
    const size_t N = (size_t)comb.back(), NS = (size_t)n_structs + G;
    hipStream_t st = c->stream;

    /* 3. one batch over the complex and its groups */
    std::vector<double> tp;
    if (alg == 1 && !unit_points) { tp = call_test_points(alg, resolution); unit_points = tp.data(); }
    if (run_batch(c, alg == 0, (const double *)c->g_xyz.p, (const double *)c->g_radii.p, comb.data(), (int)NS, probe, resolution,
                  alg == 1 ? unit_points : nullptr, (double *)c->g_sasa.p, nullptr, (double *)c->g_tot.p))
        return -1;

    /* 4. finish: areas to the caller, each group's complex area reduced like its isolated total (the chunk tables of
          the combined batch, which run_batch left on the device) */
    ga.csasa = (const double *)c->g_sasa.p; ga.ctot = (const double *)c->g_tot.p; ga.ctot2 = (const double *)c->g_tot2.p;
    ga.cgath = (double *)c->g_gath.p; ga.sasa = d_sasa; ga.iso = d_iso; ga.totals = d_totals; ga.gtot = d_group_totals;
    HIP_TRY(c, kl_grp_finish(ga, st));
    if (G > 0 && d_group_totals) {
        PipeArgs pa;
        memset(&pa, 0, sizeof pa);
        pa.n_structs = (int)NS; pa.n_atoms = (int)N; pa.offsets = (const int64_t *)c->offsets.p;
        pa.n_chunks = c->n_chunks; pa.chunk_struct = (const int *)c->chunk_struct.p; pa.chunk_begin = (const int64_t *)c->chunk_begin.p;
        pa.chunk_len = (const int *)c->chunk_len.p; pa.struct_chunk0 = (const int *)c->struct_chunk0.p;
        HIP_TRY(c, kl_totals(pa, c->n_chunks, (int)NS, (const double *)c->g_gath.p, (double *)c->bpart.p, (double *)c->g_tot2.p, st));
    }
    if (d_totals || (G > 0 && d_group_totals)) HIP_TRY(c, kl_grp_totals(ga, st));
    if (counts_out) { cnt.resize((size_t)G); counts_out->swap(cnt); }
    return 0;
}

static int groups_impl(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                       int n_structs, const int32_t *d_group, const int32_t *n_groups, double probe, int resolution,
                       double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals)
{
    c->err[0] = 0;
    if (!d_xyz || !d_radii || !offsets || !d_group || !n_groups || !d_sasa || !d_iso) return ctx_fail(c, "null argument");
    if (alg != 0 && alg != 1) return ctx_fail(c, "unknown algorithm %d", alg);
    if (n_structs <= 0) return ctx_fail(c, "n_structs must be > 0");
    if (resolution <= 0) return ctx_fail(c, "resolution must be > 0");
    if (offsets[0] != 0) return ctx_fail(c, "offsets[0] must be 0");
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] < offsets[s]) return ctx_fail(c, "offsets must be non-decreasing");
    if (groups_resident(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe, resolution, nullptr, d_sasa, d_iso,
                        d_totals, d_group_totals, nullptr))
        return -1;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); /* (stream sync 2 of 2 beyond run_batch's: the call is synchronous) */
    return 0;
}

extern "C" int freesasa_gpu_groups_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                       const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                       double probe_radius, int resolution, double *d_sasa, double *d_iso, double *d_totals,
                                       double *d_group_totals)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first) */
    return guarded_ctx(c, [&]() -> int {
        const int rc = groups_impl(c, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, probe_radius, resolution,
                                   d_sasa, d_iso, d_totals, d_group_totals);
        if (rc) (void)hipStreamSynchronize(c->stream);
        return rc;
    });
}

/* (engine_internal.h) */
int group_batch_upload(const BatchCall &b, freesasa_gpu_ctx *c, GroupBatch &g)
{
    const size_t n = (size_t)g.offsets[g.n_structs];
    g.G = 0;
    for (int s = 0; s < g.n_structs; ++s) g.G += g.n_groups[s] > 0 && g.n_groups[s] <= GRP_MAX_PER_STRUCT ? g.n_groups[s] : 0;
    Chunk h;
    h.ns = g.n_structs; h.n = n; h.off = g.offsets; h.xyz = g.xyz; h.radii = g.radii;
    if (chunk_size(b, c, h) || ensure(c, c->h_group, 4 * n) || ensure(c, c->h_iso, 8 * n) || ensure(c, c->h_gtot, 24 * (size_t)g.G + 8)) return -1;
    if (chunk_upload(c, h)) return -1;
    if (hipMemcpyAsync(c->h_group.p, g.group, 4 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ctx_fail(c, "host-to-device copy failed");
    g.d_xyz = (const double *)c->h_xyz.p; g.d_radii = (const double *)c->h_radii.p; g.d_group = (const int32_t *)c->h_group.p;
    g.d_sasa = (double *)c->h_sasa.p; g.d_iso = (double *)c->h_iso.p;
    g.d_totals = g.totals_out ? (double *)c->h_totals.p : nullptr; g.d_group_totals = g.group_totals_out ? (double *)c->h_gtot.p : nullptr;
    return 0;
}

/* (engine_internal.h) */
int group_batch_download(freesasa_gpu_ctx *c, const GroupBatch &g)
{
    const size_t n = (size_t)g.offsets[g.n_structs];
    hipStream_t st = c->stream;
    if ((g.sasa_out && hipMemcpyAsync(g.sasa_out, g.d_sasa, 8 * n, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (g.iso_out && hipMemcpyAsync(g.iso_out, g.d_iso, 8 * n, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (g.totals_out && hipMemcpyAsync(g.totals_out, g.d_totals, 8 * (size_t)g.n_structs, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (g.group_totals_out && g.G > 0 && hipMemcpyAsync(g.group_totals_out, g.d_group_totals, 24 * (size_t)g.G, hipMemcpyDeviceToHost, st) != hipSuccess))
        return ctx_fail(c, "device-to-host copy failed");
    return 0;
}

extern "C" int freesasa_gpu_calc_groups(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                        const int32_t *group, const int32_t *n_groups, int alg, double probe_radius,
                                        int resolution, double *sasa_out, double *iso_out, double *totals_out,
                                        double *group_totals_out, int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz || !radii || !offsets || !group || !n_groups || !sasa_out || !iso_out) return set_err(err_out, err_len, "null argument");
    if (n_structs <= 0 || offsets[n_structs] <= 0) return set_err(err_out, err_len, "empty batch");
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    const BatchCall b; /* (nothing staged, no counts, the fallback text of the batches) */
    GroupBatch g;
    g.xyz = xyz; g.radii = radii; g.offsets = offsets; g.n_structs = n_structs; g.group = group; g.n_groups = n_groups;
    g.sasa_out = sasa_out; g.iso_out = iso_out; g.totals_out = totals_out; g.group_totals_out = group_totals_out;
    const int rc = [&]() -> int {
        if (group_batch_upload(b, c, g)) return -1;
        if (freesasa_gpu_groups_dev(c, alg, g.d_xyz, g.d_radii, offsets, n_structs, g.d_group, n_groups, probe_radius, resolution, g.d_sasa,
                                    g.d_iso, g.d_totals, g.d_group_totals))
            return -1;
        if (group_batch_download(c, g)) return -1;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        return 0;
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}

/* ------------------------------------------------------------------ group ids made on the device (group_kernels.h) */

/* (engine_internal.h) */
int group_spec_parse(const char *spec, int flags, GroupSpec *out, char *err_out, int err_len)
{
    std::vector<char> labels(4 * (size_t)FREESASA_INGEST_MAX_GROUP_LABELS);
    std::vector<int32_t> groups((size_t)FREESASA_INGEST_MAX_GROUP_LABELS);
    int n_lab = 0;
    const int G = freesasa_ingest_chain_groups_parse(spec, flags, labels.data(), groups.data(), &n_lab, err_out, err_len);
    if (G < 0) return -1;
    out->separate = (flags & FREESASA_INGEST_SEPARATE_CHAINS) != 0;
    out->n_groups = G;
    out->first_label.assign((size_t)G, 0);
    std::vector<char> named((size_t)G, 0);
    std::vector<std::pair<uint32_t, int32_t>> tab((size_t)n_lab);
    for (int i = 0; i < n_lab; ++i) {
        uint32_t w;
        memcpy(&w, labels.data() + 4 * (size_t)i, 4);
        tab[(size_t)i] = {w, groups[(size_t)i]};
        if (!named[(size_t)groups[(size_t)i]]) { named[(size_t)groups[(size_t)i]] = 1; out->first_label[(size_t)groups[(size_t)i]] = w; }
    }
    std::sort(tab.begin(), tab.end());
    out->lab.resize((size_t)n_lab); out->lab_group.resize((size_t)n_lab);
    for (int i = 0; i < n_lab; ++i) { out->lab[(size_t)i] = tab[(size_t)i].first; out->lab_group[(size_t)i] = tab[(size_t)i].second; }
    return 0;
}

/* (engine_internal.h) */
int group_ids_resident(freesasa_gpu_ctx *c, const GroupSpec &gs, GidArgs &ga)
{
    const size_t n_lab = gs.lab.size();
    if (ga.n_structs <= 0 || (!gs.separate && n_lab == 0)) return ctx_fail(c, "bad argument");
    ga.n_lab = (int)n_lab; ga.n_spec_groups = gs.n_groups;
    if (n_lab > 0) {
        if (ensure(c, c->gi_tab, 8 * n_lab)) return -1;
        ga.lab = (const uint32_t *)c->gi_tab.p; ga.lab_group = (const int32_t *)(ga.lab + n_lab);
        HIP_TRY(c, hipMemcpyAsync(c->gi_tab.p, gs.lab.data(), 4 * n_lab, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync((char *)c->gi_tab.p + 4 * n_lab, gs.lab_group.data(), 4 * n_lab, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, kl_gid_struct(ga, c->stream));
    return 0;
}

extern "C" int freesasa_gpu_chain_group_ids(const freesasa_ingest_batch *b, const char *spec, int flags, int32_t *group_out,
                                            int32_t *n_groups_out, int32_t *status_out, int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!b || !group_out || !n_groups_out || !status_out) return set_err(err_out, err_len, "null argument");
    return guarded(err_out, err_len, [&]() -> int {
        GroupSpec gs; /* (declared before the lease: freed after its stream is idle) */
        if (group_spec_parse(spec, flags, &gs, err_out, err_len)) return -1;
        const int ns = b->n_structs;
        const int64_t n = b->n_atoms, R = b->n_residues;
        if (ns < 0 || n < 0 || R < 0 || n > (int64_t)1 << 30 || (n > 0 && (R == 0 || ns == 0))) return set_err(err_out, err_len, "inconsistent batch");
        for (int k = 0; k < ns; ++k)
            if (b->offsets[k + 1] < b->offsets[k]) return set_err(err_out, err_len, "structure offsets must be non-decreasing");
        for (int64_t r = 0; r < R; ++r)
            if (b->res_first[r + 1] < b->res_first[r]) return set_err(err_out, err_len, "residue offsets must be non-decreasing");
        if (ns > 0 && (b->offsets[0] != 0 || b->offsets[ns] != n || (R > 0 && (b->res_first[0] != 0 || b->res_first[R] != n))))
            return set_err(err_out, err_len, "inconsistent batch");
        if (ns == 0) return 0;
        if (freesasa_gpu_device_count() <= 0) return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
        std::vector<int32_t> st_in((size_t)ns, 0);
        if (b->status) memcpy(st_in.data(), b->status, 4 * (size_t)ns);
        const int64_t zero = 0;
        PoolLease lease(device);
        freesasa_gpu_ctx *c = lease.c;
        if (!c) return set_err(err_out, err_len, "could not create a GPU context");
        c->err[0] = 0;
        const int rc = [&]() -> int {
            HIP_TRY(c, hipSetDevice(c->device));
            DevBuf *B = c->parse;
            const size_t b_off = 8 * ((size_t)ns + 1), b_first = 8 * ((size_t)R + 1);
            if (ensure(c, c->seg, b_off + b_first) || ensure(c, B[PBUF_SEL_LABELS], 4 * (size_t)R + 4) || ensure(c, c->h_group, 4 * (size_t)n + 4) ||
                ensure(c, c->gi_words, 12 * (size_t)ns))
                return -1;
            char *seg = (char *)c->seg.p;
            int32_t *words = (int32_t *)c->gi_words.p;
            hipStream_t st = c->stream;
            HIP_TRY(c, hipMemcpyAsync(seg, b->offsets, b_off, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(seg + b_off, R > 0 ? b->res_first : &zero, b_first, hipMemcpyHostToDevice, st));
            if (R > 0) HIP_TRY(c, hipMemcpyAsync(B[PBUF_SEL_LABELS].p, b->res_chain, 4 * (size_t)R, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(words, st_in.data(), 4 * (size_t)ns, hipMemcpyHostToDevice, st));
            GidArgs ga;
            memset(&ga, 0, sizeof ga);
            ga.offsets = (const int64_t *)seg; ga.n_structs = ns;
            ga.res_first = (const int64_t *)(seg + b_off); ga.n_res = R; ga.n_res_dev = 0;
            ga.chain_h = (const uint32_t *)B[PBUF_SEL_LABELS].p;
            ga.status = words; ga.n_groups = words + ns; ga.group_status = words + 2 * (size_t)ns;
            ga.group = (int32_t *)c->h_group.p;
            if (group_ids_resident(c, gs, ga)) return -1;
            if (n > 0) HIP_TRY(c, hipMemcpyAsync(group_out, ga.group, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(n_groups_out, ga.n_groups, 4 * (size_t)ns, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(status_out, ga.group_status, 4 * (size_t)ns, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            return 0;
        }();
        if (rc) { (void)hipStreamSynchronize(c->stream); return set_err(err_out, err_len, c->err[0] ? c->err : "group ids failed"); }
        return 0;
    });
}
