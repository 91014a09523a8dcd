/*
 * gpu_volume.hip — molecular volume (include/freesasa_gpu.h, freesasa_gpu_sr_volume_dev / freesasa_gpu_calc_volume): the
 * volume enclosed by the solvent-accessible surface of every structure of a batch, made of the Shrake-Rupley test points
 * (vol_kernels.h has the definition).  The batch goes through the engine once, as any Shrake-Rupley batch does - areas,
 * counts and totals are freesasa_gpu_sr_batch_dev's bit for bit - with one more output of the tile kernel's store phase: the
 * sum of every atom's exposed unit points.  Behind it on the stream: the structures' origins, the atoms' terms, and the
 * engine's totals kernels over the terms.  The trajectory topology entries (gpu_drivers.hip) call volume_resident per shard.
 *
 * What the engine cannot make this way it refuses (run_batch_once, gpu_engine.hip): more than 128 test points, points that
 * are not unit vectors, FREESASA_AMD_SR_CAPS=0, a launch or a tile that runs the second arrangement.  A volume made any
 * other way is never returned.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>
#include <vector>

#include "engine_internal.h"

using namespace sasa;

const char *volume_bad_args(const void *xyz, const void *radii, const int64_t *offsets, int n_structs, int n_points, const void *sasa, const void *volumes)
{
    if (!xyz || !radii || !offsets || !sasa || !volumes) return "null argument";
    if (n_structs <= 0) return "n_structs must be > 0";
    if (n_points <= 0) return "n_points must be > 0";
    if (offsets[0] != 0) return "offsets[0] must be 0";
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] < offsets[s]) return "offsets must be non-decreasing";
    if (offsets[n_structs] <= 0) return "empty batch";
    if (offsets[n_structs] > (int64_t)1 << 30) return "batch too large (max 2^30 atoms per call)";
    return nullptr;
}

int volume_resident(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                    double probe, int n_points, const double *unit_points, double *d_sasa, int *d_counts, double *d_evec,
                    double *d_vol, double *d_totals, double *d_volumes)
{
    c->err[0] = 0;
    if (const char *bad = volume_bad_args(d_xyz, d_radii, offsets, n_structs, n_points, d_sasa, d_volumes)) return ctx_fail(c, "%s", bad);
    const size_t n = (size_t)offsets[n_structs];
    if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
    if ((!d_counts && ensure(c, c->v_counts, 4 * n)) || (!d_evec && ensure(c, c->v_evec, 24 * n)) || (!d_vol && ensure(c, c->v_vol, 8 * n)) ||
        ensure(c, c->v_origin, 24 * (size_t)n_structs))
        return -1;
    if (!d_counts) d_counts = (int *)c->v_counts.p;
    if (!d_evec) d_evec = (double *)c->v_evec.p;
    if (!d_vol) d_vol = (double *)c->v_vol.p;
    std::vector<double> own;
    if (!unit_points) {
        own.resize(3 * (size_t)n_points);
        freesasa_gpu_test_points(n_points, own.data());
        unit_points = own.data();
    }
    /* (the request lives for this one batch: whatever way run_batch comes back, the next batch of the context is an ordinary one) */
    struct Request {
        freesasa_gpu_ctx *c;
        Request(freesasa_gpu_ctx *c_, double *e) : c(c_) { c->vol_evec = e; }
        ~Request() { c->vol_evec = nullptr; }
    };
    const bool shared = c->shared_radii;
    {
        const Request rq(c, d_evec);
        if (run_batch(c, false, d_xyz, d_radii, offsets, n_structs, probe, n_points, unit_points, d_sasa, d_counts, d_totals)) return -1;
    }
    VolArgs va;
    memset(&va, 0, sizeof va);
    va.xyz = d_xyz; va.radii = d_radii; va.offsets = (const int64_t *)c->offsets.p; /* (run_batch's copy of them) */
    va.n_structs = n_structs; va.shared_radii = shared ? 1 : 0; va.n_points = n_points; va.n_atoms = (int64_t)n; va.probe = probe;
    va.counts = d_counts; va.evec = d_evec; va.origin = (double *)c->v_origin.p; va.vol = d_vol;
    PipeArgs pa; /* (the chunk tables of these offsets: run_batch left them on the device, as gpu_groups.hip relies on) */
    memset(&pa, 0, sizeof pa);
    pa.n_structs = n_structs; pa.n_atoms = (int)n; pa.offsets = va.offsets;
    pa.n_chunks = c->n_chunks; pa.chunk_struct = (const int *)c->chunk_struct.p; pa.chunk_begin = (const int64_t *)c->chunk_begin.p;
    pa.chunk_len = (const int *)c->chunk_len.p; pa.struct_chunk0 = (const int *)c->struct_chunk0.p;
    HIP_TRY(c, kl_vol_origin(va, c->stream));
    HIP_TRY(c, kl_vol_atom(va, c->stream));
    HIP_TRY(c, kl_totals(pa, c->n_chunks, n_structs, d_vol, (double *)c->bpart.p, d_volumes, c->stream));
    return 0;
}

extern "C" int freesasa_gpu_sr_volume_dev(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                                          int n_structs, double probe, int n_points, double *d_sasa, int *d_counts, double *d_evec,
                                          double *d_vol, double *d_totals, double *d_volumes)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first) */
    return guarded_ctx(c, [&]() -> int {
        int rc = volume_resident(c, d_xyz, d_radii, offsets, n_structs, probe, n_points, nullptr, d_sasa, d_counts, d_evec, d_vol, d_totals, d_volumes);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = ctx_fail(c, "stream synchronize failed"); /* (the call is synchronous) */
        if (rc) (void)hipStreamSynchronize(c->stream);
        return rc;
    });
}

extern "C" int freesasa_gpu_calc_volume(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, double probe,
                                        int n_points, double *sasa_out, int *counts_out, double *evec_out, double *vol_out,
                                        double *totals_out, double *volumes_out, int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (const char *bad = volume_bad_args(xyz, radii, offsets, n_structs, n_points, sasa_out, volumes_out)) return set_err(err_out, err_len, bad);
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    const size_t n = (size_t)offsets[n_structs], ns = (size_t)n_structs;
    /* the batch as one chunk of the host-batch path, in place: its sizing, upload and failure epilogue; the volume's extras here */
    BatchCall b;
    b.alg = 1; b.counts_out = counts_out; b.totals_out = totals_out;
    b.fallback = "GPU volume batch failed";
    Chunk h;
    h.ns = n_structs; h.n = n; h.off = offsets; h.xyz = xyz; h.radii = radii;
    const int rc = [&]() -> int {
        if (chunk_size(b, c, h) || ensure(c, c->v_volumes, 8 * ns)) return -1;
        if (chunk_upload(c, h)) return -1;
        if (volume_resident(c, (const double *)c->h_xyz.p, (const double *)c->h_radii.p, offsets, n_structs, probe, n_points, nullptr,
                            (double *)c->h_sasa.p, counts_out ? (int *)c->h_counts.p : nullptr, nullptr, nullptr,
                            totals_out ? (double *)c->h_totals.p : nullptr, (double *)c->v_volumes.p))
            return -1;
        if (hipMemcpyAsync(sasa_out, c->h_sasa.p, 8 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(volumes_out, c->v_volumes.p, 8 * ns, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (counts_out && hipMemcpyAsync(counts_out, c->h_counts.p, 4 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (evec_out && hipMemcpyAsync(evec_out, c->v_evec.p, 24 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (vol_out && hipMemcpyAsync(vol_out, c->v_vol.p, 8 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (totals_out && hipMemcpyAsync(totals_out, c->h_totals.p, 8 * ns, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
            return ctx_fail(c, "device-to-host copy failed");
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        return 0;
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}
