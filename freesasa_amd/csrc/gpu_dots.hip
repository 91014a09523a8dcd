/*
 * gpu_dots.hip — exposure masks and surface dots (include/freesasa_gpu.h: freesasa_gpu_sr_masks_dev / freesasa_gpu_calc_masks,
 * freesasa_gpu_dots_count_dev / freesasa_gpu_dots_expand_dev, freesasa_gpu_dots_from_masks): which Shrake-Rupley test points
 * of every atom are exposed, as 16 bytes of mask per atom, and those points in space - what `gmx sasa -q` writes
 * (dots_kernels.h has the definitions).  The batch goes through the engine once, as any Shrake-Rupley batch does - areas,
 * counts and totals are freesasa_gpu_sr_batch_dev's bit for bit - with one more output of the tile kernel's store phase: the
 * mask it counted.  Dots are made from masks alone, with or without the engine in front: a scan of the popcounts in three
 * plain launches, then one lane per (atom, point) pair.  The trajectory topology entries (gpu_drivers.hip) call
 * masks_resident per shard.
 *
 * What the engine cannot make this way it refuses (run_batch_once, gpu_engine.hip): more than 128 test points, points that
 * are not unit vectors, FREESASA_AMD_SR_CAPS=0, a launch or a tile that runs the second arrangement, masks and the volume's
 * vectors in one batch.  A mask made any other way is never returned.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>
#include <vector>

#include "engine_internal.h"

using namespace sasa;

const char *masks_bad_args(const void *xyz, const void *radii, const int64_t *offsets, int n_structs, int n_points, const void *sasa, const void *masks)
{
    if (!xyz || !radii || !offsets || !sasa || !masks) return "null argument";
    if (n_structs <= 0) return "n_structs must be > 0";
    if (n_points <= 0) return "n_points must be > 0";
    if (offsets[0] != 0) return "offsets[0] must be 0";
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] < offsets[s]) return "offsets must be non-decreasing";
    if (offsets[n_structs] <= 0) return "empty batch";
    if (offsets[n_structs] > (int64_t)1 << 30) return "batch too large (max 2^30 atoms per call)";
    return nullptr;
}

/* what the scan and the expansion check of their sizes: 0, or the message */
static const char *dots_bad_sizes(long long n_atoms, int n_points)
{
    if (n_atoms <= 0) return "n_atoms must be > 0";
    if (n_atoms > (long long)1 << 30) return "too many atoms (max 2^30 per call)";
    if (n_points <= 0) return "n_points must be > 0";
    if (n_points > SR_CAP_POINTS_MAX) return "the exposure masks hold up to 128 test points";
    return nullptr;
}

int masks_resident(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                   double probe, int n_points, const double *unit_points, double *d_sasa, int *d_counts, double *d_totals,
                   unsigned *d_masks)
{
    c->err[0] = 0;
    if (const char *bad = masks_bad_args(d_xyz, d_radii, offsets, n_structs, n_points, d_sasa, d_masks)) return ctx_fail(c, "%s", bad);
    if ((uintptr_t)d_masks % 16) return ctx_fail(c, "the mask array must be aligned to 16 bytes (an atom's four words are one store)");
    if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
    std::vector<double> own;
    if (!unit_points) {
        own.resize(3 * (size_t)n_points);
        freesasa_gpu_test_points(n_points, own.data());
        unit_points = own.data();
    }
    /* (the request lives for this one batch: whatever way run_batch comes back, the next batch of the context is an ordinary one) */
    struct Request {
        freesasa_gpu_ctx *c;
        Request(freesasa_gpu_ctx *c_, unsigned *m) : c(c_) { c->sr_masks = m; }
        ~Request() { c->sr_masks = nullptr; }
    };
    const Request rq(c, d_masks);
    return run_batch(c, false, d_xyz, d_radii, offsets, n_structs, probe, n_points, unit_points, d_sasa, d_counts, d_totals);
}

/* the scan on the context's stream: dot_first [n_atoms + 1] from the masks; nothing is waited for (engine_internal.h: the
   interfaces' contact tables run scan and expansion too) */
int dots_count_resident(freesasa_gpu_ctx *c, const unsigned *d_masks, int64_t n_atoms, int n_points, int64_t *d_dot_first)
{
    DotsArgs a;
    memset(&a, 0, sizeof a);
    a.masks = d_masks; a.n_atoms = n_atoms; a.n_points = n_points; a.n_blocks = (n_atoms + DOTS_SCAN_B - 1) / DOTS_SCAN_B;
    if (ensure(c, c->dt_bsum, 8 * (size_t)a.n_blocks)) return -1;
    a.bsum = (int64_t *)c->dt_bsum.p; a.dot_first = d_dot_first;
    HIP_TRY(c, kl_dots_count(a, c->stream));
    return 0;
}

/* the unit points of n_points on the context's device (c->dt_unit), made and copied where it does not hold them yet.  It is
   the expansion's one host allocation: callers run it BEFORE they enqueue anything, so that a failure leaves nothing in flight. */
int dots_unit_ready(freesasa_gpu_ctx *c, int n_points)
{
    if (c->dt_unit_n == n_points) return 0;
    std::vector<double> u(3 * (size_t)n_points);
    freesasa_gpu_test_points(n_points, u.data());
    c->dt_unit_n = 0; /* (before the buffer is touched: ensure frees it before it allocates, and an allocation that fails leaves none) */
    if (ensure(c, c->dt_unit, 24 * (size_t)n_points)) return -1;
    HIP_TRY(c, hipMemcpy(c->dt_unit.p, u.data(), 24 * (size_t)n_points, hipMemcpyHostToDevice));
    c->dt_unit_n = n_points;
    return 0;
}

/* the expansion on the context's stream (dots_unit_ready first); nothing is waited for */
int dots_expand_resident(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, int64_t n_atoms, double probe, int n_points,
                                const unsigned *d_masks, const int64_t *d_dot_first, int64_t capacity, double *d_dot_xyz, int *d_dot_atom,
                                int *d_dot_point)
{
    if (c->dt_unit_n != n_points || !c->dt_unit.p) return ctx_fail(c, "internal error: the expansion's unit points are not on the device");
    DotsArgs a;
    memset(&a, 0, sizeof a);
    a.masks = d_masks; a.n_atoms = n_atoms; a.n_points = n_points; a.dot_first = const_cast<int64_t *>(d_dot_first);
    a.xyz = d_xyz; a.radii = d_radii; a.unit_pts = (const double *)c->dt_unit.p; a.probe = probe; a.inv_points = 1.0 / n_points; a.capacity = capacity;
    a.dot_xyz = d_dot_xyz; a.dot_atom = d_dot_atom; a.dot_point = d_dot_point;
    HIP_TRY(c, kl_dots_expand(a, c->stream));
    return 0;
}

extern "C" int freesasa_gpu_sr_masks_dev(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                                         int n_structs, double probe, int n_points, double *d_sasa, int *d_counts, double *d_totals,
                                         uint32_t *d_masks)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first) */
    return guarded_ctx(c, [&]() -> int {
        int rc = masks_resident(c, d_xyz, d_radii, offsets, n_structs, probe, n_points, nullptr, d_sasa, d_counts, d_totals, d_masks);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = ctx_fail(c, "stream synchronize failed"); /* (the call is synchronous) */
        if (rc) (void)hipStreamSynchronize(c->stream);
        return rc;
    });
}

extern "C" int freesasa_gpu_dots_count_dev(freesasa_gpu_ctx *c, const uint32_t *d_masks, long long n_atoms, int n_points,
                                           int64_t *d_dot_first, long long *n_dots_out)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1;
    return guarded_ctx(c, [&]() -> int {
        c->err[0] = 0;
        if (!d_masks || !d_dot_first || !n_dots_out) return ctx_fail(c, "null argument");
        if ((uintptr_t)d_masks % 16) return ctx_fail(c, "the mask array must be aligned to 16 bytes");
        if (const char *bad = dots_bad_sizes(n_atoms, n_points)) return ctx_fail(c, "%s", bad);
        if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
        int64_t D = 0;
        int rc = dots_count_resident(c, d_masks, n_atoms, n_points, d_dot_first);
        if (!rc && hipMemcpyAsync(&D, d_dot_first + n_atoms, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = ctx_fail(c, "device-to-host copy failed");
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "stream synchronize failed"); /* (D comes back to the host) */
        if (!rc) *n_dots_out = D;
        return rc;
    });
}

extern "C" int freesasa_gpu_dots_expand_dev(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, long long n_atoms, double probe,
                                            int n_points, const uint32_t *d_masks, const int64_t *d_dot_first, long long capacity,
                                            double *d_dot_xyz, int *d_dot_atom, int *d_dot_point)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1;
    return guarded_ctx(c, [&]() -> int {
        c->err[0] = 0;
        if (!d_xyz || !d_radii || !d_masks || !d_dot_first || (!d_dot_xyz && capacity > 0)) return ctx_fail(c, "null argument");
        if (const char *bad = dots_bad_sizes(n_atoms, n_points)) return ctx_fail(c, "%s", bad);
        if (capacity < 0) return ctx_fail(c, "capacity must be >= 0");
        if ((uintptr_t)d_masks % 16) return ctx_fail(c, "the mask array must be aligned to 16 bytes");
        if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
        int64_t D = 0;
        if (hipMemcpyAsync(&D, d_dot_first + n_atoms, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return ctx_fail(c, "device-to-host copy failed");
        if (D <= 0 || capacity == 0) return 0; /* (no dots, or nowhere to put one: nothing is launched) */
        if (dots_unit_ready(c, n_points)) return -1;
        int rc = dots_expand_resident(c, d_xyz, d_radii, n_atoms, probe, n_points, d_masks, d_dot_first, capacity, d_dot_xyz, d_dot_atom, d_dot_point);
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "stream synchronize failed");
        return rc;
    });
}

extern "C" int freesasa_gpu_calc_masks(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, double probe,
                                       int n_points, double *sasa_out, int *counts_out, double *totals_out, uint32_t *masks_out,
                                       int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (const char *bad = masks_bad_args(xyz, radii, offsets, n_structs, n_points, sasa_out, masks_out)) return set_err(err_out, err_len, bad);
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    const size_t n = (size_t)offsets[n_structs], ns = (size_t)n_structs;
    /* the batch as one chunk of the host-batch path, in place: its sizing, upload and failure epilogue; the masks here */
    BatchCall b;
    b.alg = 1; b.counts_out = counts_out; b.totals_out = totals_out;
    b.fallback = "GPU mask batch failed";
    Chunk h;
    h.ns = n_structs; h.n = n; h.off = offsets; h.xyz = xyz; h.radii = radii;
    const int rc = [&]() -> int {
        if (chunk_size(b, c, h) || ensure(c, c->dt_masks, 4 * SR_CAP_WORDS * n)) return -1;
        if (chunk_upload(c, h)) return -1;
        if (masks_resident(c, (const double *)c->h_xyz.p, (const double *)c->h_radii.p, offsets, n_structs, probe, n_points, nullptr,
                           (double *)c->h_sasa.p, counts_out ? (int *)c->h_counts.p : nullptr, totals_out ? (double *)c->h_totals.p : nullptr,
                           (unsigned *)c->dt_masks.p))
            return -1;
        if (hipMemcpyAsync(sasa_out, c->h_sasa.p, 8 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(masks_out, c->dt_masks.p, 4 * SR_CAP_WORDS * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (counts_out && hipMemcpyAsync(counts_out, c->h_counts.p, 4 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (totals_out && hipMemcpyAsync(totals_out, c->h_totals.p, 8 * ns, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
            return ctx_fail(c, "device-to-host copy failed");
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        return 0;
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}

/* the masks against what they may hold, on the host: no bit at or above n_points; their exposed points into *bits.  0, or the message in msg */
static int masks_popcount(const uint32_t *masks, long long n_atoms, int n_points, long long *bits, char *msg, size_t msg_len)
{
    long long sum = 0;
    for (long long i = 0; i < n_atoms; ++i)
        for (int w = 0; w < SR_CAP_WORDS; ++w) {
            const uint32_t m = masks[SR_CAP_WORDS * i + w];
            if (m & ~sr_cap_full_word(n_points, w)) {
                snprintf(msg, msg_len, "atom %lld: a mask bit at or above n_points (%d) is set", i, n_points);
                return -1;
            }
            sum += __builtin_popcount(m);
        }
    *bits = sum;
    return 0;
}

extern "C" int freesasa_gpu_masks_count(const uint32_t *masks, long long n_atoms, int n_points, long long *n_dots_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!masks || !n_dots_out) return set_err(err_out, err_len, "null argument");
    if (const char *bad = dots_bad_sizes(n_atoms, n_points)) return set_err(err_out, err_len, bad);
    char msg[120];
    if (masks_popcount(masks, n_atoms, n_points, n_dots_out, msg, sizeof msg)) return set_err(err_out, err_len, msg);
    return 0;
}

extern "C" int freesasa_gpu_dots_from_masks(const double *xyz, const double *radii, long long n_atoms, double probe, int n_points,
                                            const uint32_t *masks, long long n_dots, int64_t *dot_first_out, double *dot_xyz_out,
                                            int *dot_atom_out, int *dot_point_out, int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz || !radii || !masks || (!dot_xyz_out && n_dots > 0)) return set_err(err_out, err_len, "null argument");
    if (const char *bad = dots_bad_sizes(n_atoms, n_points)) return set_err(err_out, err_len, bad);
    if (n_dots < 0) return set_err(err_out, err_len, "n_dots must be >= 0");
    /* the masks against what the caller says of them, before a device is touched: no bit at or above n_points, n_dots bits in all */
    long long bits = 0;
    char msg[120];
    if (masks_popcount(masks, n_atoms, n_points, &bits, msg, sizeof msg)) return set_err(err_out, err_len, msg);
    if (bits != n_dots) {
        snprintf(msg, sizeof msg, "the masks hold %lld exposed points, n_dots says %lld", bits, n_dots);
        return set_err(err_out, err_len, msg);
    }
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    const size_t n = (size_t)n_atoms, D = (size_t)n_dots;
    BatchCall b;
    b.fallback = "GPU dots failed";
    const int rc = [&]() -> int {
        c->err[0] = 0;
        if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
        if (ensure(c, c->h_xyz, 24 * n) || ensure(c, c->h_radii, 8 * n) || ensure(c, c->dt_masks, 4 * SR_CAP_WORDS * n) ||
            ensure(c, c->dt_first, 8 * (n + 1)) || ensure(c, c->dt_xyz, 24 * D) || (dot_atom_out && ensure(c, c->dt_atom, 4 * D)) ||
            (dot_point_out && ensure(c, c->dt_point, 4 * D)) || (D && dots_unit_ready(c, n_points)))
            return -1;
        if (hipMemcpyAsync(c->h_xyz.p, xyz, 24 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->h_radii.p, radii, 8 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->dt_masks.p, masks, 4 * SR_CAP_WORDS * n, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return ctx_fail(c, "host-to-device copy failed");
        if (dots_count_resident(c, (const unsigned *)c->dt_masks.p, (int64_t)n, n_points, (int64_t *)c->dt_first.p)) return -1;
        if (D && dots_expand_resident(c, (const double *)c->h_xyz.p, (const double *)c->h_radii.p, (int64_t)n, probe, n_points,
                                      (const unsigned *)c->dt_masks.p, (const int64_t *)c->dt_first.p, (int64_t)D, (double *)c->dt_xyz.p,
                                      dot_atom_out ? (int *)c->dt_atom.p : nullptr, dot_point_out ? (int *)c->dt_point.p : nullptr))
            return -1;
        if ((dot_first_out && hipMemcpyAsync(dot_first_out, c->dt_first.p, 8 * (n + 1), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (D && hipMemcpyAsync(dot_xyz_out, c->dt_xyz.p, 24 * D, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (D && dot_atom_out && hipMemcpyAsync(dot_atom_out, c->dt_atom.p, 4 * D, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (D && dot_point_out && hipMemcpyAsync(dot_point_out, c->dt_point.p, 4 * D, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
            return ctx_fail(c, "device-to-host copy failed");
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        return 0;
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}
