/*
 * gpu_occupancy.hip — the residue contact occupancy map over a trajectory's interfaces (include/freesasa_gpu.h:
 * freesasa_gpu_contact_occupancy_open / _add_frames / _add_rows / _table / _table_free / _close / _error and
 * freesasa_gpu_calc_contact_occupancy).  Host code; the kernels are in gpu_kernels.hip (phase functions: occupancy_kernels.h).
 *
 * A handle holds a pooled context for its life, the system replicated for a chunk of frames_per_batch frames (radii and group ids on
 * the device, offsets, n_groups and res_first on the host) and the run table in one of two sets of device arrays.
 *
 *   add_frames   per chunk: the coordinates go up; iface_run (gpu_interfaces.hip) with the residue-residue contact stage, capacities
 *                that hold anything and no output arrays - the folded table stays in the context's buffers -; k_occ_keys makes the
 *                chunk's keys and frame boundaries of it; the merge
 *   add_rows     the caller's rows, validated on the host, go up chunk by chunk; the merge
 *   the merge    k_occ_first and the scan; N (the keys the run has not seen) and the frame boundaries come back - ONE stream
 *                synchronization -; the other set of arrays is sized for U + N rows; k_occ_rank, k_occ_accumulate; the sets swap
 *   table        k_occ_reverse over the current set, the arrays copied into host blocks of the library's
 *
 * Failure: what is found before the device is touched leaves the handle as it was; any later failure of an add poisons it - every
 * call but close and error then returns -1 with the first failure's message - so that no partially merged table is delivered.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "engine_internal.h"
#include "hostfault.h"

using namespace sasa;

struct freesasa_gpu_contact_occupancy {
    freesasa_gpu_ctx *c = nullptr;
    bool rows_only = false, poisoned = false;
    char err[640] = {0};
    int n = 0, G = 0, n_res = 0, resolution = 0, fpb = 0;
    double probe = 0;
    long long n_frames = 0, U = 0;
    int cur = 0;
    DevBuf tab[2];
    /* the system, replicated for a chunk: on the host what iface_run reads there, on the device the rest */
    std::vector<int64_t> offsets, res_first;
    std::vector<int32_t> n_groups;
    DevBuf d_xyz, d_radii, d_group, d_sasa, d_iso;
    /* a chunk's work: keys; flags and the scan's levels; pair_struct | pair_groups | pair_first; frame boundaries; (add_rows) counts | areas */
    DevBuf d_ck, d_fl, d_meta, d_ff, d_rows;
    std::vector<int32_t> h_meta;
    std::vector<int64_t> h_ff;
};

namespace {

typedef freesasa_gpu_contact_occupancy Occ;

const long long OCC_MAX_ROWS = 0x7fffffffLL;
const size_t OCC_ROW_BYTES = 8 * 9 + 4 * OCC_KEY; /* area [3] | frames | either | counts [2] | span [2] | keys [5] */

OccTable table_view(const DevBuf &b, long long cap)
{
    OccTable t;
    t.cap = cap;
    t.area = (double *)b.p;
    t.frames = (int64_t *)(t.area + 3 * cap);
    t.either = t.frames + cap;
    t.counts = t.either + cap;
    t.span = t.counts + 2 * cap;
    t.keys = (int *)(t.span + 2 * cap);
    return t;
}
long long table_cap(const DevBuf &b) { return (long long)(b.cap / OCC_ROW_BYTES); }

int occ_fail(Occ *o, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int occ_fail(Occ *o, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(o->err, sizeof o->err, fmt, ap);
    va_end(ap);
    return -1;
}
/* a failure behind the first touch of the device: nothing is left running, and the handle delivers nothing any more */
int occ_poison(Occ *o)
{
    (void)hipStreamSynchronize(o->c->stream);
    o->poisoned = true;
    return -1;
}
void free_buf(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

/* The merge of one chunk whose keys (ck), counts (cc), areas (ca) and frame boundaries (d_ff) are on the device or on their way there:
   F frames, Q > 0 rows, frame0 the run's number of the first.  counts_out (may be null): (-, Q_f) of every frame into its second
   column.  At its end the stream may still be running the rank and accumulate kernels, which read device memory only. */
int occ_merge(Occ *o, const int *ck, const int *cc, const double *ca, int F, long long Q, long long frame0, int64_t *counts_out)
{
    freesasa_gpu_ctx *c = o->c;
    hipStream_t st = c->stream;
    const size_t S = (size_t)ifr_scan_scratch(Q);
    if (ensure(c, o->d_fl, 4 * ((size_t)Q + 1 + S))) return occ_fail(o, "%s", c->err);
    OccArgs a;
    memset(&a, 0, sizeof a);
    a.n_rows = Q; a.n_frames = F; a.frame0 = frame0; a.n_old = o->U;
    a.ff = (const int64_t *)o->d_ff.p; a.ck = ck; a.cc = cc; a.ca = ca;
    a.fl = (int *)o->d_fl.p;
    a.old = table_view(o->tab[o->cur], table_cap(o->tab[o->cur]));
    int N = 0;
    hipError_t e = kl_occ_first(a, a.fl + Q + 1, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&N, a.fl + Q, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && counts_out) {
        o->h_ff.resize((size_t)F + 1);
        e = hipMemcpyAsync(o->h_ff.data(), o->d_ff.p, 8 * ((size_t)F + 1), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return occ_fail(o, "the search for a chunk's new keys failed: %s", hipGetErrorString(e));
    if (counts_out)
        for (int f = 0; f < F; ++f) counts_out[2 * f + 1] = o->h_ff[(size_t)f + 1] - o->h_ff[(size_t)f];
    const long long U = o->U + N;
    if (U > OCC_MAX_ROWS) return occ_fail(o, "the run table would have %lld rows: it holds up to 2^31 - 1", U);
    DevBuf &nb = o->tab[o->cur ^ 1];
    if (ensure(c, nb, OCC_ROW_BYTES * (size_t)U)) return occ_fail(o, "%s", c->err);
    a.n_new = U;
    a.next = table_view(nb, table_cap(nb));
    e = kl_occ_merge(a, st);
    if (e != hipSuccess) return occ_fail(o, "the merge of a chunk failed: %s", hipGetErrorString(e));
    o->cur ^= 1;
    o->U = U;
    return 0;
}

/* the first frame of frames f0 .. f0 + nf - 1 of the call that holds a coordinate that is not finite, or -1 */
long long first_bad_frame(const double *xyz, long long f0, int nf, int n)
{
    for (long long f = f0; f < f0 + nf; ++f) {
        const double *x = xyz + (size_t)f * 3 * (size_t)n;
        for (size_t i = 0; i < 3 * (size_t)n; ++i)
            if (!(x[i] - x[i] == 0)) return f;
    }
    return -1;
}

/* one chunk of add_frames: frames f0 .. f0 + nf - 1 of the call.  `r` is the caller's: it outlives the stream's work */
int occ_frames_chunk(Occ *o, const double *xyz, long long f0, int nf, int64_t *counts_out, IfaceRun &r)
{
    freesasa_gpu_ctx *c = o->c;
    hipStream_t st = c->stream;
    const size_t n = (size_t)o->n;
    c->err[0] = 0;
    hipError_t e = hipMemcpyAsync(o->d_xyz.p, xyz + (size_t)f0 * 3 * n, 24 * n * (size_t)nf, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return occ_fail(o, "the upload of frames failed: %s", hipGetErrorString(e));
    long long P = 0, M = 0, Cn = 0, D = 0, Q = 0;
    IfaceCall k;
    k.xyz = (const double *)o->d_xyz.p; k.radii = (const double *)o->d_radii.p; k.offsets = o->offsets.data(); k.n_structs = nf;
    k.group = (const int32_t *)o->d_group.p; k.n_groups = o->n_groups.data();
    k.alg = 1; k.probe = o->probe; k.resolution = o->resolution;
    k.sasa = (double *)o->d_sasa.p; k.iso = (double *)o->d_iso.p;
    k.whole = k.contacts = k.rescontacts = true;
    k.res_first = o->res_first.data(); k.n_res = nf * o->n_res;
    k.pair_capacity = k.atom_capacity = k.contact_capacity = k.dot_capacity = k.rescontact_capacity = 0x7fffffffffffffffLL;
    k.n_pairs = &P; k.n_pair_atoms = &M; k.n_contacts = &Cn; k.n_buried_dots = &D; k.n_rescontacts = &Q;
    k.out_dev = true;
    if (iface_run(c, k, r)) {
        const long long first = o->n_frames + f0, bad = first_bad_frame(xyz, f0, nf, o->n);
        if (bad >= 0) return occ_fail(o, "frame %lld of the run: %s", o->n_frames + bad, c->err);
        if (nf == 1) return occ_fail(o, "frame %lld of the run: %s", first, c->err);
        return occ_fail(o, "frames %lld .. %lld of the run: %s", first, first + nf - 1, c->err);
    }
    if (counts_out) {
        for (int f = 0; f < nf; ++f) counts_out[2 * f] = counts_out[2 * f + 1] = 0;
        for (int32_t s : r.pl.pair_struct) ++counts_out[2 * s];
    }
    if (Q == 0) return 0;
    if (Q > OCC_MAX_ROWS) return occ_fail(o, "frames %lld .. %lld of the run have %lld folded rows: a chunk takes up to 2^31 - 1",
                                          o->n_frames + f0, o->n_frames + f0 + nf - 1, Q);
    /* pair_struct [P] | pair_groups [2 P] | pair_first [nf + 1] */
    const size_t Pn = (size_t)P;
    o->h_meta.assign(3 * Pn + (size_t)nf + 1, 0);
    memcpy(o->h_meta.data(), r.pl.pair_struct.data(), 4 * Pn);
    memcpy(o->h_meta.data() + Pn, r.pl.pair_groups.data(), 8 * Pn);
    int32_t *pf = o->h_meta.data() + 3 * Pn;
    for (size_t p = 0; p < Pn; ++p) ++pf[r.pl.pair_struct[p] + 1];
    for (int f = 0; f < nf; ++f) pf[f + 1] += pf[f];
    if (ensure(c, o->d_meta, 4 * o->h_meta.size()) || ensure(c, o->d_ff, 8 * ((size_t)nf + 1)) || ensure(c, o->d_ck, 4 * OCC_KEY * (size_t)Q))
        return occ_fail(o, "%s", c->err);
    e = hipMemcpyAsync(o->d_meta.p, o->h_meta.data(), 4 * o->h_meta.size(), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return occ_fail(o, "the upload of a chunk's pairs failed: %s", hipGetErrorString(e));
    OccKeyArgs ka;
    memset(&ka, 0, sizeof ka);
    ka.n_rows = Q; ka.n_sides = 2 * P; ka.n_frames = nf; ka.n_res = o->n_res;
    ka.rc_off = r.qt.off; ka.rc_res = r.qt.res;
    ka.pair_struct = (const int *)o->d_meta.p; ka.pair_groups = ka.pair_struct + Pn; ka.pair_first = ka.pair_groups + 2 * Pn;
    ka.ck = (int *)o->d_ck.p; ka.ff = (int64_t *)o->d_ff.p;
    e = kl_occ_keys(ka, st);
    if (e != hipSuccess) return occ_fail(o, "the keys of a chunk failed: %s", hipGetErrorString(e));
    return occ_merge(o, ka.ck, r.qt.cnt, r.qt.area, nf, Q, o->n_frames + f0, counts_out);
}

/* key a strictly below key b, component by component (the host's twin of occ_cmp) */
bool key_below(const int32_t *a, const int32_t *b)
{
    for (int k = 0; k < OCC_KEY; ++k)
        if (a[k] != b[k]) return a[k] < b[k];
    return false;
}

/* what add_rows refuses, before anything goes up: 0, or -1 with the message (frames are the call's, rows the call's) */
int occ_bad_rows(Occ *o, int n_frames, const int64_t *ff, const int32_t *keys, const int32_t *counts, const double *area)
{
    if (n_frames < 0) return occ_fail(o, "n_frames must be >= 0");
    if (!ff) return occ_fail(o, "null argument");
    if (ff[0] != 0) return occ_fail(o, "frame_first[0] must be 0");
    for (int f = 0; f < n_frames; ++f) {
        if (ff[f + 1] < ff[f]) return occ_fail(o, "frame_first must be non-decreasing (frame %d)", f);
        if (ff[f + 1] - ff[f] > OCC_MAX_ROWS) return occ_fail(o, "frame %d has %lld rows: a chunk takes up to 2^31 - 1", f, (long long)(ff[f + 1] - ff[f]));
    }
    if (ff[n_frames] > 0 && (!keys || !counts || !area)) return occ_fail(o, "null argument");
    for (int f = 0; f < n_frames; ++f)
        for (int64_t t = ff[f]; t < ff[f + 1]; ++t) {
            const int32_t *k = keys + OCC_KEY * t;
            const long long row = (long long)(t - ff[f]);
            if (k[0] < 0 || k[0] >= k[1]) return occ_fail(o, "frame %d, row %lld: the groups must be 0 <= g < h (they are %d, %d)", f, row, k[0], k[1]);
            if (k[2] != 0 && k[2] != 1) return occ_fail(o, "frame %d, row %lld: side must be 0 or 1 (it is %d)", f, row, k[2]);
            if (k[3] < 0 || k[4] < 0) return occ_fail(o, "frame %d, row %lld: the residues must be >= 0 (they are %d, %d)", f, row, k[3], k[4]);
            if (t > ff[f] && !key_below(k - OCC_KEY, k)) return occ_fail(o, "frame %d, row %lld: the keys of a frame must be strictly ascending", f, row);
            if (counts[2 * t] < 1 || counts[2 * t + 1] < 1)
                return occ_fail(o, "frame %d, row %lld: both counts must be >= 1 (they are %d, %d)", f, row, counts[2 * t], counts[2 * t + 1]);
            if (!(area[t] - area[t] == 0)) return occ_fail(o, "frame %d, row %lld: the area is not finite", f, row);
        }
    return 0;
}

/* one chunk of add_rows: frames f0 .. f0 + nf - 1 of the call, Q > 0 rows from row t0 */
int occ_rows_chunk(Occ *o, long long f0, int nf, const int64_t *ff, const int32_t *keys, const int32_t *counts, const double *area)
{
    freesasa_gpu_ctx *c = o->c;
    hipStream_t st = c->stream;
    const int64_t t0 = ff[f0];
    const size_t Q = (size_t)(ff[f0 + nf] - t0);
    c->err[0] = 0;
    o->h_ff.resize((size_t)nf + 1);
    for (int f = 0; f <= nf; ++f) o->h_ff[(size_t)f] = ff[f0 + f] - t0;
    if (ensure(c, o->d_ff, 8 * ((size_t)nf + 1)) || ensure(c, o->d_ck, 4 * OCC_KEY * Q) || ensure(c, o->d_rows, 16 * Q)) return occ_fail(o, "%s", c->err);
    double *d_area = (double *)o->d_rows.p;
    int *d_cnt = (int *)(d_area + Q);
    hipError_t e = hipMemcpyAsync(o->d_ff.p, o->h_ff.data(), 8 * ((size_t)nf + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(o->d_ck.p, keys + OCC_KEY * t0, 4 * OCC_KEY * Q, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cnt, counts + 2 * t0, 8 * Q, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_area, area + t0, 8 * Q, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return occ_fail(o, "the upload of rows failed: %s", hipGetErrorString(e));
    return occ_merge(o, (const int *)o->d_ck.p, d_cnt, d_area, nf, (long long)Q, o->n_frames + f0, nullptr);
}

int occ_enter(Occ *o)
{
    if (!o) return -1;
    if (o->poisoned) return -1;
    o->err[0] = 0;
    if (hipSetDevice(o->c->device) != hipSuccess) return occ_fail(o, "hipSetDevice failed");
    return 0;
}

void table_release(freesasa_gpu_contact_occupancy_table_t *t)
{
    free(t->keys); free(t->frames); free(t->frames_either); free(t->counts); free(t->area); free(t->span); free(t->reverse);
    memset(t, 0, sizeof *t);
}

} /* namespace */

extern "C" freesasa_gpu_contact_occupancy *freesasa_gpu_contact_occupancy_open(const double *radii, int n_atoms, const int32_t *group, int n_groups,
                                                                               const int64_t *res_first, int n_res, double probe_radius,
                                                                               int resolution, int frames_per_batch, int device, char *err_out,
                                                                               int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    const bool rows_only = !radii && n_atoms == 0;
    char msg[200];
    if (!rows_only) {
        if (!radii || n_atoms <= 0) { set_err(err_out, err_len, !radii ? "null argument" : "n_atoms must be > 0"); return nullptr; }
        /* one frame as the batch of one structure: what the residue-residue contact entry refuses about it */
        const int64_t off[2] = {0, n_atoms};
        const int32_t ng[1] = {n_groups};
        IfaceCall k;
        k.xyz = radii; k.radii = radii; k.offsets = off; k.n_structs = 1; k.group = group; k.n_groups = ng;
        k.alg = 1; k.probe = probe_radius; k.resolution = resolution; k.res_first = res_first; k.n_res = n_res;
        if (iface_bad_rescontact_call(k, msg, sizeof msg)) { set_err(err_out, err_len, msg); return nullptr; }
        if (n_groups < 0 || n_groups > GRP_MAX_PER_STRUCT) {
            snprintf(msg, sizeof msg, "n_groups must be 0 .. %d (it is %d)", GRP_MAX_PER_STRUCT, n_groups);
            set_err(err_out, err_len, msg);
            return nullptr;
        }
        for (int i = 0; i < n_atoms; ++i)
            if (group[i] < -1 || group[i] >= n_groups) {
                snprintf(msg, sizeof msg, "atom %d has group id %d: ids are -1 (in no group) or 0 .. %d", i, group[i], n_groups - 1);
                set_err(err_out, err_len, msg);
                return nullptr;
            }
    }
    if (freesasa_gpu_device_count() <= 0) { set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path"); return nullptr; }
    Occ *o = nullptr;
    const int rc = guarded(err_out, err_len, [&]() -> int {
        o = new Occ();
        o->rows_only = rows_only;
        o->c = pool_get(device);
        if (!o->c) return set_err(err_out, err_len, "could not create a GPU context");
        freesasa_gpu_ctx *c = o->c;
        c->err[0] = 0;
        if (hipSetDevice(c->device) != hipSuccess) return set_err(err_out, err_len, "hipSetDevice failed");
        o->fpb = frames_per_batch;
        if (rows_only) {
            if (o->fpb <= 0) o->fpb = 256;
            return 0;
        }
        o->n = n_atoms; o->G = n_groups; o->n_res = n_res; o->resolution = resolution; o->probe = probe_radius;
        /* the drivers' rule on three times the atoms - the frame, its isolated groups, a pair structure's worth -, then iface_run's
           limits: 2^30 atoms and 2^27 tests of a call, chunk-wide residue numbers below 2^31 */
        long long fpb = frames_per_batch > 0 ? frames_per_batch : 1250000 / (3LL * n_atoms) + 1;
        const long long tests = (long long)n_groups * (n_groups - 1) / 2;
        const long long lim[] = {(1LL << 30) / (3LL * n_atoms), tests ? IF_MAX_TESTS / tests : fpb, 0x7fffffffLL / n_res, (1LL << 30) / (1 + n_groups)};
        for (long long l : lim) fpb = fpb > l ? l : fpb;
        o->fpb = fpb < 1 ? 1 : (int)fpb;
        const size_t FB = (size_t)o->fpb, n = (size_t)n_atoms;
        o->offsets.resize(FB + 1); o->n_groups.assign(FB, n_groups); o->res_first.resize(FB * (size_t)n_res + 1);
        for (size_t f = 0; f <= FB; ++f) o->offsets[f] = (int64_t)(f * n);
        for (size_t f = 0; f < FB; ++f)
            for (int r = 0; r < n_res; ++r) o->res_first[f * (size_t)n_res + (size_t)r] = (int64_t)(f * n) + res_first[r];
        o->res_first[FB * (size_t)n_res] = (int64_t)(FB * n);
        std::vector<double> rr(FB * n);
        std::vector<int32_t> gg(FB * n);
        for (size_t f = 0; f < FB; ++f) { memcpy(rr.data() + f * n, radii, 8 * n); memcpy(gg.data() + f * n, group, 4 * n); }
        if (ensure(c, o->d_xyz, 24 * FB * n) || ensure(c, o->d_radii, 8 * FB * n) || ensure(c, o->d_group, 4 * FB * n) ||
            ensure(c, o->d_sasa, 8 * FB * n) || ensure(c, o->d_iso, 8 * FB * n))
            return set_err(err_out, err_len, c->err);
        if (hipMemcpy(o->d_radii.p, rr.data(), 8 * FB * n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o->d_group.p, gg.data(), 4 * FB * n, hipMemcpyHostToDevice) != hipSuccess)
            return set_err(err_out, err_len, "the upload of the system failed");
        return 0;
    });
    if (rc) {
        if (o) freesasa_gpu_contact_occupancy_close(o);
        return nullptr;
    }
    return o;
}

extern "C" int freesasa_gpu_contact_occupancy_add_frames(freesasa_gpu_contact_occupancy *o, const double *xyz_frames, int n_frames,
                                                          int64_t *frame_counts_out)
{
    if (occ_enter(o)) return -1;
    if (o->rows_only) return occ_fail(o, "the accumulator was opened without a system: it takes rows, not frames");
    if (n_frames < 0) return occ_fail(o, "n_frames must be >= 0");
    if (n_frames > 0 && !xyz_frames) return occ_fail(o, "null argument");
    IfaceRun r; /* (before the guard: it outlives the stream's work, whatever ends the call) */
    char msg[200];
    int rc = 0;
    try {
        for (long long f0 = 0; f0 < n_frames && !rc; f0 += o->fpb) {
            const int nf = (int)(n_frames - f0 < o->fpb ? n_frames - f0 : o->fpb);
            r = IfaceRun();
            rc = occ_frames_chunk(o, xyz_frames, f0, nf, frame_counts_out ? frame_counts_out + 2 * f0 : nullptr, r);
            /* (the stream is idle behind the merge's synchronization but for kernels that read device memory only) */
        }
        if (!rc && hipStreamSynchronize(o->c->stream) != hipSuccess) rc = occ_fail(o, "stream synchronize failed");
    } catch (...) {
        rc = occ_fail(o, "%s", exception_text(msg, sizeof msg));
    }
    if (rc) return occ_poison(o);
    o->n_frames += n_frames;
    return 0;
}

extern "C" int freesasa_gpu_contact_occupancy_add_rows(freesasa_gpu_contact_occupancy *o, int n_frames, const int64_t *frame_first,
                                                        const int32_t *keys, const int32_t *counts, const double *area)
{
    if (occ_enter(o)) return -1;
    if (occ_bad_rows(o, n_frames, frame_first, keys, counts, area)) return -1;
    char msg[200];
    int rc = 0;
    try {
        /* chunks of up to frames_per_batch frames and 2^31 - 1 rows; frames without rows cost nothing */
        for (long long f0 = 0; f0 < n_frames && !rc;) {
            int nf = 1;
            while (nf < o->fpb && f0 + nf < n_frames && frame_first[f0 + nf + 1] - frame_first[f0] <= OCC_MAX_ROWS) ++nf;
            if (frame_first[f0 + nf] > frame_first[f0]) rc = occ_rows_chunk(o, f0, nf, frame_first, keys, counts, area);
            f0 += nf;
        }
        if (hipStreamSynchronize(o->c->stream) != hipSuccess && !rc) rc = occ_fail(o, "stream synchronize failed");
    } catch (...) {
        rc = occ_fail(o, "%s", exception_text(msg, sizeof msg));
    }
    if (rc) return occ_poison(o);
    o->n_frames += n_frames;
    return 0;
}

extern "C" int freesasa_gpu_contact_occupancy_table(freesasa_gpu_contact_occupancy *o, freesasa_gpu_contact_occupancy_table_t *out)
{
    if (occ_enter(o)) return -1;
    if (!out) return occ_fail(o, "null argument");
    memset(out, 0, sizeof *out);
    freesasa_gpu_ctx *c = o->c;
    hipStream_t st = c->stream;
    const size_t U = (size_t)o->U;
    out->n_frames = o->n_frames; out->n_rows = o->U;
    /* (a table without rows has blocks of one element: no array of it is null) */
    const size_t m = U ? U : 1;
    out->keys = (int32_t *)hf_malloc(4 * OCC_KEY * m); out->frames = (int64_t *)hf_malloc(8 * m); out->frames_either = (int64_t *)hf_malloc(8 * m);
    out->counts = (int64_t *)hf_malloc(16 * m); out->area = (double *)hf_malloc(24 * m); out->span = (int64_t *)hf_malloc(16 * m);
    out->reverse = (int32_t *)hf_malloc(4 * m);
    int rc = 0;
    if (!out->keys || !out->frames || !out->frames_either || !out->counts || !out->area || !out->span || !out->reverse) rc = occ_fail(o, "out of host memory");
    if (!rc && U) {
        c->err[0] = 0;
        if (ensure(c, o->d_fl, 4 * U)) rc = occ_fail(o, "%s", c->err);
        if (!rc) {
            OccArgs a;
            memset(&a, 0, sizeof a);
            a.n_new = o->U;
            a.next = table_view(o->tab[o->cur], table_cap(o->tab[o->cur]));
            a.reverse = (int *)o->d_fl.p;
            hipError_t e = kl_occ_reverse(a, st);
            const struct { void *dst; const void *src; size_t bytes; } cp[] = {
                {out->keys, a.next.keys, 4 * OCC_KEY * U}, {out->frames, a.next.frames, 8 * U}, {out->frames_either, a.next.either, 8 * U},
                {out->counts, a.next.counts, 16 * U}, {out->area, a.next.area, 24 * U}, {out->span, a.next.span, 16 * U}, {out->reverse, a.reverse, 4 * U}};
            for (const auto &x : cp)
                if (e == hipSuccess) e = hipMemcpyAsync(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost, st);
            const hipError_t e2 = hipStreamSynchronize(st); /* (whatever failed: nothing may write the blocks once they are freed) */
            if (e == hipSuccess) e = e2;
            if (e != hipSuccess) rc = occ_fail(o, "the copy of the run table failed: %s", hipGetErrorString(e));
        }
    }
    if (rc) table_release(out);
    return rc;
}

extern "C" void freesasa_gpu_contact_occupancy_table_free(freesasa_gpu_contact_occupancy_table_t *t)
{
    if (t) table_release(t);
}

extern "C" void freesasa_gpu_contact_occupancy_close(freesasa_gpu_contact_occupancy *o)
{
    if (!o) return;
    if (o->c) {
        (void)hipSetDevice(o->c->device);
        (void)hipStreamSynchronize(o->c->stream);
        for (DevBuf *b : {&o->tab[0], &o->tab[1], &o->d_xyz, &o->d_radii, &o->d_group, &o->d_sasa, &o->d_iso, &o->d_ck, &o->d_fl, &o->d_meta, &o->d_ff, &o->d_rows})
            free_buf(*b);
        o->c->shared_radii = false;
        pool_put(o->c);
    }
    delete o;
}

extern "C" const char *freesasa_gpu_contact_occupancy_error(const freesasa_gpu_contact_occupancy *o)
{
    return o ? o->err : "no accumulator";
}

extern "C" int freesasa_gpu_calc_contact_occupancy(const double *xyz_frames, int n_frames, const double *radii, int n_atoms, const int32_t *group,
                                                   int n_groups, const int64_t *res_first, int n_res, double probe_radius, int resolution,
                                                   int frames_per_batch, int64_t *frame_counts_out, freesasa_gpu_contact_occupancy_table_t *out,
                                                   int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!out || !radii || (n_frames > 0 && !xyz_frames)) return set_err(err_out, err_len, "null argument");
    if (n_frames < 0) return set_err(err_out, err_len, "n_frames must be >= 0");
    freesasa_gpu_contact_occupancy *o = freesasa_gpu_contact_occupancy_open(radii, n_atoms, group, n_groups, res_first, n_res, probe_radius, resolution,
                                                                            frames_per_batch, device, err_out, err_len);
    if (!o) return -1;
    const int rc = freesasa_gpu_contact_occupancy_add_frames(o, xyz_frames, n_frames, frame_counts_out) || freesasa_gpu_contact_occupancy_table(o, out) ? -1 : 0;
    if (rc) set_err(err_out, err_len, o->err);
    freesasa_gpu_contact_occupancy_close(o);
    return rc;
}
