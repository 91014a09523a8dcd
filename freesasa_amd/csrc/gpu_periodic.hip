/*
 * gpu_periodic.hip — periodic images (include/freesasa_gpu.h, freesasa_gpu_periodic_dev / freesasa_gpu_calc_periodic; the
 * FREESASA_GPU_FRAMES_PBC bit of the trajectory file drivers): every structure with an orthorhombic cell of its own, the
 * SASA of its atoms among their periodic images.  Host code; the kernels are in gpu_kernels.hip (phase functions and the
 * definition: pbc_kernels.h).  The same pipeline serves triclinic cells (freesasa_gpu_periodic_triclinic_dev /
 * freesasa_gpu_calc_periodic_triclinic, FREESASA_GPU_FRAMES_TRICLINIC; pbc_tri_kernels.h): a cell is then nine doubles on the
 * device - its six numbers and the three widths the host made of them (cell.c) -, count and emit are the triclinic kernels
 * and the check is of the widths; everything else, the orthorhombic path included, is what it was.
 *
 *   1. count      k_pbc_count: per atom the base of its images, per structure the image count and the max radius; those
 *                 come back to the host (the engine takes host offsets): the call's one synchronisation beyond run_batch's
 *   2. check      every edge against the structure's c = 2 (max radius + probe); the expanded batch against the engine's
 *                 2^30 atoms - before the engine runs
 *   3. emit       k_pbc_emit: the wrapped atoms, then their images, at each structure's expanded offset, radii per atom
 *   4. run_batch  the expanded batch: the tile kernels know nothing of cells
 *   5. collect    k_pbc_collect: the first n areas of every expanded structure into the caller's compact array
 *   6. totals     the totals kernels over the compact areas with the chunk table of the CALLER's offsets: the sum over the
 *                 real atoms in the order every batch's totals are formed in (a cell that makes no image gives the plain
 *                 run's totals bit for bit)
 *
 * Chain groups among periodic images (freesasa_gpu_groups_periodic_dev and its kin, the stage of
 * freesasa_gpu_trajectory_file_groups_periodic): the same pipeline over the chain-group entry's combined batch, at the end of this
 * file.
 *
 * periodic_resident is that pipeline for callers whose arrays are on the context's stream (the trajectory lanes,
 * gpu_drivers.hip); freesasa_gpu_calc_periodic brings host arrays to it with the host-batch path's sizing, upload and
 * failure epilogue (gpu_hostbatch.hip), as freesasa_gpu_calc_groups does.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "engine_internal.h"

using namespace sasa;

/* (engine_internal.h) */
double periodic_cutoff(const double *radii, int64_t n, double probe)
{
    double m = 0;
    for (int64_t i = 0; i < n; ++i)
        if (radii[i] > m) m = radii[i];
    return 2.0 * (m + probe);
}
int periodic_cell_bad(const double *cell, double c)
{
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(cell[a])) return -(a + 1);
        if (!(cell[a] >= c)) return a + 1;
    }
    return 0;
}

/* (engine_internal.h; periodic_cell6_bad is in cell.c) */
int periodic_widths_bad(const double *widths, double c)
{
    for (int a = 0; a < 3; ++a)
        if (!(widths[a] >= c)) return a + 1;
    return 0;
}
static const char *const CELL6_NAME[6] = {"ax", "bx", "by", "cx", "cy", "cz"};
/* the messages of a refused triclinic cell: its shape (bad: periodic_cell6_bad's) ... */
static void cell6_msg(char *msg, size_t len, int s, const double *h, int bad)
{
    const int k = bad < 0 ? -bad - 1 : bad - 1;
    if (bad < 0) snprintf(msg, len, "structure %d: entry %s of its cell is not finite", s, CELL6_NAME[k]);
    else snprintf(msg, len, "structure %d: entry %s of its cell is %.17g: ax, by and cz must be > 0", s, CELL6_NAME[k], h[k]);
}
/* ... and a width (bad: periodic_widths_bad's) */
static void width_msg(char *msg, size_t len, int s, const double *widths, int bad, double cut)
{
    snprintf(msg, len, "structure %d: width %c of its cell is %.17g, smaller than c = 2 (max radius + probe) = %.17g: "
                       "first-shell images do not suffice", s, "abc"[bad - 1], widths[bad - 1], cut);
}

static int cell_fail(freesasa_gpu_ctx *c, int s, const double *cell, int bad, double cut)
{
    const int a = bad < 0 ? -bad - 1 : bad - 1;
    if (bad < 0) return ctx_fail(c, "structure %d: edge %c of its cell is not finite", s, "xyz"[a]);
    return ctx_fail(c, "structure %d: edge %c of its cell is %.17g, shorter than c = 2 (max radius + probe) = %.17g: "
                       "first-shell images do not suffice", s, "xyz"[a], cell[a], cut);
}

/* the chunk table of the caller's offsets (run_batch_once makes the same of the offsets it is given), kept until they change:
   chunk_begin [nc] | chunk_len [nc] | chunk_struct [nc] | struct_chunk0 [ns + 1] in c->p_chunks */
static int compact_chunks(freesasa_gpu_ctx *c, const int64_t *offsets, int n_structs, PipeArgs &pa)
{
    const size_t ns1 = (size_t)n_structs + 1;
    if (c->p_offsets_host.size() != ns1 || memcmp(c->p_offsets_host.data(), offsets, 8 * ns1) != 0) {
        c->p_offsets_host.clear();
        std::vector<int> cs, cl, sc0(ns1);
        std::vector<int64_t> cb;
        for (int s = 0; s < n_structs; ++s) {
            sc0[s] = (int)cs.size();
            for (int64_t b = offsets[s]; b < offsets[s + 1]; b += SASA_BOUNDS_CHUNK) {
                const int64_t e = b + SASA_BOUNDS_CHUNK < offsets[s + 1] ? b + SASA_BOUNDS_CHUNK : offsets[s + 1];
                cs.push_back(s); cb.push_back(b); cl.push_back((int)(e - b));
            }
        }
        sc0[n_structs] = (int)cs.size();
        const size_t nc = cs.size();
        if (ensure(c, c->p_chunks, 16 * nc + 4 * ns1) || ensure(c, c->p_part, 8 * nc)) return -1;
        char *p = (char *)c->p_chunks.p;
        /* (synchronous copies out of vectors that end with this scope; the stream's earlier work does not read the table) */
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipMemcpy(p, cb.data(), 8 * nc, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(p + 8 * nc, cl.data(), 4 * nc, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(p + 12 * nc, cs.data(), 4 * nc, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(p + 16 * nc, sc0.data(), 4 * ns1, hipMemcpyHostToDevice));
        c->p_n_chunks = (int)nc;
        c->p_offsets_host.assign(offsets, offsets + ns1);
    }
    const size_t nc = (size_t)c->p_n_chunks;
    const char *p = (const char *)c->p_chunks.p;
    memset(&pa, 0, sizeof pa);
    pa.n_structs = n_structs; pa.n_atoms = (int)offsets[n_structs]; pa.n_chunks = (int)nc;
    pa.chunk_begin = (const int64_t *)p; pa.chunk_len = (const int *)(p + 8 * nc); pa.chunk_struct = (const int *)(p + 12 * nc);
    pa.struct_chunk0 = (const int *)(p + 16 * nc);
    return 0;
}

/* periodic_resident (tri false: cells [3 n_structs]) and periodic_resident_tri (tri: cells [9 n_structs]).  gx (chain groups
   among periodic images, groups_periodic_stage): the batch is a combined one - gx->n_cplx complexes, then their groups (and, for a
   trajectory shard with interface pairs, behind those the pair structures of every frame: gx->k_fixed); the host
   cells are the complexes' rows and are checked for them alone (a group's or a pair structure's max radius never exceeds its
   complex's), images_out
   is the complexes', and behind the engine runs the groups' fused finish in the collect's place (d_sasa and d_totals: null). */
static int resident(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                    int n_fixed, const double *cells, const double *d_cells, double probe, int resolution, const double *unit_points,
                    double *d_sasa, double *d_totals, int64_t *images_out, GpbcArgs *gx = nullptr)
{
    const size_t W = tri ? PBC_TRI_CELL : 3; /* doubles per cell */
    const int64_t n = offsets[n_structs];
    if (n <= 0) return ctx_fail(c, "empty batch");
    if (n > (int64_t)1 << 30) return ctx_fail(c, "the expanded batch is too large (max 2^30 atoms and images per call)");
    const size_t ns = (size_t)n_structs;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    /* offsets [ns + 1] | expanded offsets [ns + 1] | cells [W ns] | image counts [ns] | max radii [ns] */
    const size_t o_eoff = 8 * (ns + 1), o_cell = 2 * o_eoff, o_img = o_cell + 8 * W * ns, o_rmax = o_img + 8 * ns, meta_bytes = o_rmax + 8 * ns;
    if (ensure(c, c->p_meta, meta_bytes) || ensure(c, c->p_ibase, 4 * (size_t)n)) return -1;
    char *meta = (char *)c->p_meta.p;
    PipeArgs ta; /* (the totals' chunk table first: it goes up with copies that wait for the stream when the offsets are new) */
    if (d_totals && compact_chunks(c, offsets, n_structs, ta)) return -1;
    PbcTriArgs pt;
    memset(&pt, 0, sizeof pt);
    PbcArgs &pa = pt.b;
    pa.xyz = d_xyz; pa.radii = d_radii; pa.n_structs = n_structs; pa.n_atoms = n; pa.probe = probe;
    pa.n_fixed = n_fixed > 0 ? n_fixed : 0; pa.shared_radii = n_fixed > 0;
    pa.offsets = n_fixed > 0 ? nullptr : (const int64_t *)meta;
    (tri ? pt.cell9 : pa.cells) = d_cells ? d_cells : (const double *)(meta + o_cell);
    pa.ibase = (int *)c->p_ibase.p; pa.n_img = (int64_t *)(meta + o_img); pa.rmax = (double *)(meta + o_rmax);

    /* 1. count; the image counts and max radii back (the one synchronisation beyond run_batch's) */
    std::vector<int64_t> back(2 * ns), eoff(ns + 1); /* (declared before the copies that use them: they outlive the stream's reads) */
    if (n_fixed <= 0) HIP_TRY(c, hipMemcpyAsync(meta, offsets, 8 * (ns + 1), hipMemcpyHostToDevice, st));
    if (!d_cells) HIP_TRY(c, hipMemcpyAsync(meta + o_cell, cells, 8 * W * ns, hipMemcpyHostToDevice, st));
    HIP_TRY(c, tri ? kl_pbc_tri_count(pt, st) : kl_pbc_count(pa, st));
    HIP_TRY(c, hipMemcpyAsync(back.data(), meta + o_img, 16 * ns, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));

    /* 2. the checks that need the device's numbers, before the engine runs */
    eoff[0] = 0;
    for (size_t s = 0; s < ns; ++s) {
        const int64_t ns_atoms = offsets[s + 1] - offsets[s];
        if (ns_atoms > 0 && (!gx || s < (size_t)gx->n_cplx)) {
            double rmax;
            memcpy(&rmax, &back[ns + s], 8);
            const double cut = 2.0 * (rmax + probe);
            const int bad = tri ? periodic_widths_bad(cells + W * s + 6, cut) : periodic_cell_bad(cells + 3 * s, cut);
            if (bad && tri) {
                char msg[240];
                width_msg(msg, sizeof msg, (int)s, cells + W * s + 6, bad, cut);
                return ctx_fail(c, "%s", msg);
            }
            if (bad) return cell_fail(c, (int)s, cells + 3 * s, bad, cut);
        }
        if (back[s] < 0 || back[s] > 26 * ns_atoms) return ctx_fail(c, "structure %d: bad image count from the device", (int)s);
        eoff[s + 1] = eoff[s] + ns_atoms + back[s];
        if (images_out && (!gx || s < (size_t)gx->n_cplx)) images_out[s] = back[s];
    }
    const int64_t N = eoff[ns];
    if (gx && N > (int64_t)1 << 30)
        return ctx_fail(c, "the expanded batch is too large: %lld atoms of the complexes, %lld atoms of their groups and %lld images (max 2^30 together per call)",
                        (long long)gx->n_atoms, (long long)(n - gx->n_atoms), (long long)(N - n));
    if (N > (int64_t)1 << 30)
        return ctx_fail(c, "the expanded batch is too large: %lld atoms and %lld images (max 2^30 together per call)", (long long)n, (long long)(N - n));

    /* 3. emit */
    if (ensure(c, c->p_xyz, 24 * (size_t)N) || ensure(c, c->p_radii, 8 * (size_t)N) || ensure(c, c->p_sasa, 8 * (size_t)N)) return -1;
    pa.eoff = (const int64_t *)(meta + o_eoff); pa.exyz = (double *)c->p_xyz.p; pa.eradii = (double *)c->p_radii.p;
    HIP_TRY(c, hipMemcpyAsync(meta + o_eoff, eoff.data(), 8 * (ns + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(c, tri ? kl_pbc_tri_emit(pt, st) : kl_pbc_emit(pa, st));

    /* 4. the engine on the expanded batch (synchronous: eoff is no longer read when it returns) */
    std::vector<double> tp;
    if (alg == 1 && !unit_points) { tp = call_test_points(alg, resolution); unit_points = tp.data(); }
    const bool shared = c->shared_radii;
    c->shared_radii = false;
    const int rb = run_batch(c, alg == 0, (const double *)c->p_xyz.p, (const double *)c->p_radii.p, eoff.data(), n_structs, probe, resolution,
                             alg == 1 ? unit_points : nullptr, (double *)c->p_sasa.p, nullptr, nullptr);
    c->shared_radii = shared;
    if (rb) return -1;

    /* 5. collect, 6. totals over the real atoms */
    if (gx) { /* (collect and the groups' finish in one; the totals are groups_periodic_stage's) */
        gx->coff = (const int64_t *)meta; gx->eoff = (const int64_t *)(meta + o_eoff); gx->esasa = (const double *)c->p_sasa.p;
        HIP_TRY(c, kl_gpbc_finish(*gx, st));
        return 0;
    }
    pa.esasa = (const double *)c->p_sasa.p; pa.sasa = d_sasa;
    HIP_TRY(c, kl_pbc_collect(pa, st));
    if (d_totals) HIP_TRY(c, kl_totals(ta, ta.n_chunks, n_structs, d_sasa, (double *)c->p_part.p, d_totals, st));
    return 0;
}

/* (engine_internal.h) */
int periodic_resident(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                      int n_fixed, const double *cells, const double *d_cells, double probe, int resolution, const double *unit_points,
                      double *d_sasa, double *d_totals, int64_t *images_out)
{
    return resident(c, false, alg, d_xyz, d_radii, offsets, n_structs, n_fixed, cells, d_cells, probe, resolution, unit_points, d_sasa, d_totals, images_out);
}
int periodic_resident_tri(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets, int n_structs,
                          int n_fixed, const double *cells9, const double *d_cells9, double probe, int resolution, const double *unit_points,
                          double *d_sasa, double *d_totals, int64_t *images_out)
{
    return resident(c, true, alg, d_xyz, d_radii, offsets, n_structs, n_fixed, cells9, d_cells9, probe, resolution, unit_points, d_sasa, d_totals, images_out);
}

/* the six numbers of every structure's cell with their widths behind them: cells9 [9 n_structs] (a structure without atoms,
   whose cell is not checked, may get widths that are not numbers: no thread reads them for an atom) */
static void cells9_make(const double *cells6, int n_structs, std::vector<double> &cells9)
{
    cells9.resize((size_t)PBC_TRI_CELL * (size_t)n_structs);
    for (size_t s = 0; s < (size_t)n_structs; ++s) {
        memcpy(&cells9[PBC_TRI_CELL * s], cells6 + 6 * s, 48);
        (void)freesasa_gpu_cell_widths(cells6 + 6 * s, &cells9[PBC_TRI_CELL * s + 6]);
    }
}

/* the shape of every cell that has atoms, before the device is touched: 0, or -1 with the context's message (tri: cells is
   [6 n_structs]) */
static int cells_shape_check(freesasa_gpu_ctx *c, bool tri, const int64_t *offsets, int n_structs, const double *cells)
{
    for (int s = 0; s < n_structs; ++s) {
        if (offsets[s + 1] == offsets[s]) continue;
        if (tri) {
            const int bad = periodic_cell6_bad(cells + 6 * (size_t)s);
            if (bad) {
                char msg[240];
                cell6_msg(msg, sizeof msg, s, cells + 6 * (size_t)s, bad);
                return ctx_fail(c, "%s", msg);
            }
        } else {
            const int bad = periodic_cell_bad(cells + 3 * (size_t)s, 0.0);
            if (bad < 0) return cell_fail(c, s, cells + 3 * (size_t)s, bad, 0.0);
        }
    }
    return 0;
}

/* tri: cells is [6 n_structs] */
static int periodic_impl(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                         int n_structs, const double *cells, double probe, int resolution, double *d_sasa, double *d_totals,
                         int64_t *images_out)
{
    c->err[0] = 0;
    if (!d_xyz || !d_radii || !offsets || !cells || !d_sasa) return ctx_fail(c, "null argument");
    if (alg != 0 && alg != 1) return ctx_fail(c, "unknown algorithm %d", alg);
    if (n_structs <= 0) return ctx_fail(c, "n_structs must be > 0");
    if (resolution <= 0) return ctx_fail(c, "resolution must be > 0");
    if (offsets[0] != 0) return ctx_fail(c, "offsets[0] must be 0");
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] < offsets[s]) return ctx_fail(c, "offsets must be non-decreasing");
    std::vector<double> cells9;
    if (cells_shape_check(c, tri, offsets, n_structs, cells)) return -1;
    if (tri) cells9_make(cells, n_structs, cells9);
    if (resident(c, tri, alg, d_xyz, d_radii, offsets, n_structs, 0, tri ? cells9.data() : cells, nullptr, probe, resolution, nullptr, d_sasa, d_totals, images_out))
        return -1;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); /* (the call is synchronous) */
    return 0;
}

static int periodic_dev(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_xyz, const double *d_radii,
                        const int64_t *offsets, int n_structs, const double *cells, double probe_radius,
                        int resolution, double *d_sasa, double *d_totals, int64_t *images_out)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first) */
    return guarded_ctx(c, [&]() -> int {
        const int rc = periodic_impl(c, tri, alg, d_xyz, d_radii, offsets, n_structs, cells, probe_radius, resolution, d_sasa, d_totals, images_out);
        if (rc) (void)hipStreamSynchronize(c->stream);
        return rc;
    });
}

extern "C" int freesasa_gpu_periodic_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                         const int64_t *offsets, int n_structs, const double *cells, double probe_radius,
                                         int resolution, double *d_sasa, double *d_totals, int64_t *images_out)
{
    return periodic_dev(c, false, alg, d_xyz, d_radii, offsets, n_structs, cells, probe_radius, resolution, d_sasa, d_totals, images_out);
}
extern "C" int freesasa_gpu_periodic_triclinic_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                                   const int64_t *offsets, int n_structs, const double *cells6, double probe_radius,
                                                   int resolution, double *d_sasa, double *d_totals, int64_t *images_out)
{
    return periodic_dev(c, true, alg, d_xyz, d_radii, offsets, n_structs, cells6, probe_radius, resolution, d_sasa, d_totals, images_out);
}

/* what the host-array entries check before an array goes to a device: the sizes, then every structure's cell against its own
   radii; 0, or -1 with the message (tri: cells is [6 n_structs]) */
static int host_cells_check(bool tri, const double *radii, const int64_t *offsets, int n_structs, const double *cells, double probe_radius,
                            char *err_out, int err_len)
{
    if (offsets[0] != 0) return set_err(err_out, err_len, "offsets[0] must be 0");
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] < offsets[s]) return set_err(err_out, err_len, "offsets must be non-decreasing");
    if (offsets[n_structs] > (int64_t)1 << 30)
        return set_err(err_out, err_len, "the expanded batch is too large (max 2^30 atoms and images per call)");
    for (int s = 0; s < n_structs; ++s) {
        const int64_t ns_atoms = offsets[s + 1] - offsets[s];
        if (ns_atoms == 0) continue;
        const double cut = periodic_cutoff(radii + offsets[s], ns_atoms, probe_radius);
        if (tri) {
            const double *h = cells + 6 * (size_t)s;
            char msg[240];
            double widths[3];
            int bad = periodic_cell6_bad(h);
            if (bad) {
                cell6_msg(msg, sizeof msg, s, h, bad);
                return set_err(err_out, err_len, msg);
            }
            (void)freesasa_gpu_cell_widths(h, widths);
            if ((bad = periodic_widths_bad(widths, cut)) != 0) {
                width_msg(msg, sizeof msg, s, widths, bad, cut);
                return set_err(err_out, err_len, msg);
            }
            continue;
        }
        const double *cell = cells + 3 * (size_t)s;
        const int bad = periodic_cell_bad(cell, cut);
        if (bad) {
            char msg[240];
            const int a = bad < 0 ? -bad - 1 : bad - 1;
            if (bad < 0) snprintf(msg, sizeof msg, "structure %d: edge %c of its cell is not finite", s, "xyz"[a]);
            else snprintf(msg, sizeof msg, "structure %d: edge %c of its cell is %.17g, shorter than c = 2 (max radius + probe) = %.17g: "
                                           "first-shell images do not suffice", s, "xyz"[a], cell[a], cut);
            return set_err(err_out, err_len, msg);
        }
    }
    return 0;
}

/* tri: cells is [6 n_structs] */
static int calc_periodic(bool tri, const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                         const double *cells, int alg, double probe_radius, int resolution,
                         double *sasa_out, double *totals_out, int64_t *images_out,
                         int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz || !radii || !offsets || !cells || !sasa_out) return set_err(err_out, err_len, "null argument");
    if (n_structs <= 0 || offsets[n_structs] <= 0) return set_err(err_out, err_len, "empty batch");
    /* before an array is read or a device touched: the sizes, then every structure's cell against its own radii */
    if (host_cells_check(tri, radii, offsets, n_structs, cells, probe_radius, err_out, err_len)) return -1;
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    const size_t n = (size_t)offsets[n_structs];
    /* the batch as one chunk of the host-batch path, in place: its sizing, upload and failure epilogue */
    const BatchCall b;
    Chunk h;
    h.ns = n_structs; h.n = n; h.off = offsets; h.xyz = xyz; h.radii = radii;
    const int rc = [&]() -> int {
        if (chunk_size(b, c, h) || chunk_upload(c, h)) return -1;
        if (periodic_dev(c, tri, alg, (const double *)c->h_xyz.p, (const double *)c->h_radii.p, offsets, n_structs, cells,
                         probe_radius, resolution, (double *)c->h_sasa.p, totals_out ? (double *)c->h_totals.p : nullptr, images_out))
            return -1;
        if (hipMemcpyAsync(sasa_out, c->h_sasa.p, 8 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (totals_out && hipMemcpyAsync(totals_out, c->h_totals.p, 8 * (size_t)n_structs, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
            return ctx_fail(c, "device-to-host copy failed");
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        return 0;
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}

extern "C" int freesasa_gpu_calc_periodic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                          const double *cells, int alg, double probe_radius, int resolution,
                                          double *sasa_out, double *totals_out, int64_t *images_out,
                                          int device, char *err_out, int err_len)
{
    return calc_periodic(false, xyz, radii, offsets, n_structs, cells, alg, probe_radius, resolution, sasa_out, totals_out, images_out, device, err_out, err_len);
}
extern "C" int freesasa_gpu_calc_periodic_triclinic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                    const double *cells6, int alg, double probe_radius, int resolution,
                                                    double *sasa_out, double *totals_out, int64_t *images_out,
                                                    int device, char *err_out, int err_len)
{
    return calc_periodic(true, xyz, radii, offsets, n_structs, cells6, alg, probe_radius, resolution, sasa_out, totals_out, images_out, device, err_out, err_len);
}

/* ------------------------------------------------------------------ chain groups among periodic images
 * (freesasa_gpu_groups_periodic_dev and its kin; include/freesasa_gpu.h has the definition): the chain-group entry's cut
 * (gpu_groups.hip, groups_cut) makes the combined batch - the complexes, then every group as a structure -, the stage above
 * expands it, every group in the cell of its complex, and runs the engine ONCE over complexes, groups and all their images;
 * behind it pbc_kernels.h's fused finish reads every real atom's two areas out of the expanded batch, the totals kernels
 * reduce the compact combined areas and the gathered complex areas with the chunk table of the COMBINED offsets (the tables
 * run_batch left on the device describe the expanded batch), and k_grp_totals writes the table. */

/* (engine_internal.h) */
int groups_periodic_stage(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_cxyz, const double *d_cradii, const int64_t *comb,
                          const double *cells, const double *d_cells, GpbcArgs &x, double probe, int resolution,
                          const double *unit_points, double *d_ctot, double *d_ctot2, int64_t *images_out)
{
    const size_t W = tri ? PBC_TRI_CELL : 3;
    if (ensure(c, c->gp_cells, 8 * W * (size_t)x.n_comb)) return -1;
    x.W = (int)W; x.cells = d_cells; x.ccells = (double *)c->gp_cells.p;
    HIP_TRY(c, kl_gpbc_cells(x, c->stream));
    if (resident(c, tri, alg, d_cxyz, d_cradii, comb, x.n_comb, 0, cells, x.ccells, probe, resolution, unit_points, nullptr, nullptr, images_out, &x))
        return -1;
    PipeArgs ta;
    if (compact_chunks(c, comb, x.n_comb, ta)) return -1;
    HIP_TRY(c, kl_totals(ta, ta.n_chunks, x.n_comb, x.carea, (double *)c->p_part.p, d_ctot, c->stream));
    if (!d_ctot2) return 0;
    /* (interface pairs: the pair structures lie behind the others, and so do their chunks in the table; the finish writes no
       gathered area for a pair atom, so those chunks are KEPT OUT of this reduction - d_ctot2 is [n_cplx (1 + g_fixed)] - as
       shard_compute keeps them out for the run without cells) */
    int n_structs2 = x.n_comb, n_chunks2 = ta.n_chunks;
    if (x.k_fixed) {
        n_structs2 = x.n_cplx * (1 + x.g_fixed);
        int64_t k = 0;
        for (int s = 0; s < n_structs2; ++s) k += (comb[s + 1] - comb[s] + SASA_BOUNDS_CHUNK - 1) / SASA_BOUNDS_CHUNK;
        n_chunks2 = (int)k;
        ta.n_structs = n_structs2;
    }
    HIP_TRY(c, kl_totals(ta, n_chunks2, n_structs2, x.cgath, (double *)c->p_part.p, d_ctot2, c->stream));
    return 0;
}

/* (engine_internal.h) */
int groups_periodic_resident(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                             int n_structs, const int32_t *d_group, const int32_t *n_groups, const double *cells, double probe,
                             int resolution, const double *unit_points, double *d_sasa, double *d_iso, double *d_totals,
                             double *d_group_totals, int64_t *images_out)
{
    GrpArgs ga;
    std::vector<int64_t> comb;
    std::vector<int> cnt;
    if (groups_cut(c, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, ga, comb, cnt)) return -1;
    const int G = ga.n_groups;
    const size_t W = tri ? PBC_TRI_CELL : 3, NS = (size_t)n_structs + G;
    /* the complexes' cells behind the combined structures' (c->gp_cells) */
    if (ensure(c, c->gp_cells, 8 * W * (NS + (size_t)n_structs))) return -1;
    double *const d_cells = (double *)c->gp_cells.p + W * NS;
    HIP_TRY(c, hipMemcpyAsync(d_cells, cells, 8 * W * (size_t)n_structs, hipMemcpyHostToDevice, c->stream));
    GpbcArgs x;
    memset(&x, 0, sizeof x);
    x.n_cplx = n_structs; x.n_comb = (int)NS; x.gbase = ga.gbase;
    x.n_atoms = ga.n_atoms; x.n_all = comb[NS]; x.src = ga.src; x.key = ga.key;
    x.carea = (double *)c->g_sasa.p; x.cgath = (double *)c->g_gath.p; x.sasa = d_sasa; x.iso = d_iso;
    const bool gt = G > 0 && d_group_totals;
    if (groups_periodic_stage(c, tri, alg, (const double *)c->g_xyz.p, (const double *)c->g_radii.p, comb.data(), cells, d_cells, x, probe,
                              resolution, unit_points, (double *)c->g_tot.p, gt ? (double *)c->g_tot2.p : nullptr, images_out))
        return -1;
    ga.ctot = (const double *)c->g_tot.p; ga.ctot2 = (const double *)c->g_tot2.p; ga.totals = d_totals; ga.gtot = d_group_totals;
    if (d_totals || gt) HIP_TRY(c, kl_grp_totals(ga, c->stream));
    return 0;
}

/* tri: cells is [6 n_structs] */
static int groups_periodic_dev(freesasa_gpu_ctx *c, bool tri, int alg, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                               int n_structs, const int32_t *d_group, const int32_t *n_groups, const double *cells, double probe,
                               int resolution, double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals, int64_t *images_out)
{
    if (!c) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first) */
    return guarded_ctx(c, [&]() -> int {
        std::vector<double> cells9; /* (outlives the stream's read of it, on the way out after a failure too) */
        const int rc = [&]() -> int {
            c->err[0] = 0;
            if (!d_xyz || !d_radii || !offsets || !d_group || !n_groups || !cells || !d_sasa || !d_iso) return ctx_fail(c, "null argument");
            if (alg != 0 && alg != 1) return ctx_fail(c, "unknown algorithm %d", alg);
            if (n_structs <= 0) return ctx_fail(c, "n_structs must be > 0");
            if (resolution <= 0) return ctx_fail(c, "resolution must be > 0");
            if (offsets[0] != 0) return ctx_fail(c, "offsets[0] must be 0");
            for (int s = 0; s < n_structs; ++s)
                if (offsets[s + 1] < offsets[s]) return ctx_fail(c, "offsets must be non-decreasing");
            if (cells_shape_check(c, tri, offsets, n_structs, cells)) return -1;
            if (tri) cells9_make(cells, n_structs, cells9);
            if (groups_periodic_resident(c, tri, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, tri ? cells9.data() : cells, probe,
                                         resolution, nullptr, d_sasa, d_iso, d_totals, d_group_totals, images_out))
                return -1;
            HIP_TRY(c, hipStreamSynchronize(c->stream)); /* (the call is synchronous) */
            return 0;
        }();
        if (rc) (void)hipStreamSynchronize(c->stream);
        return rc;
    });
}

extern "C" int freesasa_gpu_groups_periodic_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                                const int64_t *offsets, int n_structs, const int32_t *d_group, const int32_t *n_groups,
                                                const double *cells, double probe_radius, int resolution, double *d_sasa, double *d_iso,
                                                double *d_totals, double *d_group_totals, int64_t *images_out)
{
    return groups_periodic_dev(c, false, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, cells, probe_radius, resolution, d_sasa,
                               d_iso, d_totals, d_group_totals, images_out);
}
extern "C" int freesasa_gpu_groups_periodic_triclinic_dev(freesasa_gpu_ctx *c, int alg, const double *d_xyz, const double *d_radii,
                                                          const int64_t *offsets, int n_structs, const int32_t *d_group,
                                                          const int32_t *n_groups, const double *cells6, double probe_radius, int resolution,
                                                          double *d_sasa, double *d_iso, double *d_totals, double *d_group_totals,
                                                          int64_t *images_out)
{
    return groups_periodic_dev(c, true, alg, d_xyz, d_radii, offsets, n_structs, d_group, n_groups, cells6, probe_radius, resolution, d_sasa,
                               d_iso, d_totals, d_group_totals, images_out);
}

/* tri: cells is [6 n_structs]; freesasa_gpu_calc_groups (gpu_groups.hip) with the cells */
static int calc_groups_periodic(bool tri, const double *xyz, const double *radii, const int64_t *offsets, int n_structs, const int32_t *group,
                                const int32_t *n_groups, const double *cells, int alg, double probe_radius, int resolution, double *sasa_out,
                                double *iso_out, double *totals_out, double *group_totals_out, int64_t *images_out, int device,
                                char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz || !radii || !offsets || !group || !n_groups || !cells || !sasa_out || !iso_out) return set_err(err_out, err_len, "null argument");
    if (n_structs <= 0 || offsets[n_structs] <= 0) return set_err(err_out, err_len, "empty batch");
    /* before an array is read or a device touched: the sizes, then every complex's cell against its own radii */
    if (host_cells_check(tri, radii, offsets, n_structs, cells, probe_radius, err_out, err_len)) return -1;
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    PoolLease lease(device);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) return set_err(err_out, err_len, "could not create a GPU context");
    const BatchCall b;
    GroupBatch g; /* (the grouped host batch: gpu_groups.hip) */
    g.xyz = xyz; g.radii = radii; g.offsets = offsets; g.n_structs = n_structs; g.group = group; g.n_groups = n_groups;
    g.sasa_out = sasa_out; g.iso_out = iso_out; g.totals_out = totals_out; g.group_totals_out = group_totals_out;
    const int rc = [&]() -> int {
        if (group_batch_upload(b, c, g)) return -1;
        if (groups_periodic_dev(c, tri, alg, g.d_xyz, g.d_radii, offsets, n_structs, g.d_group, n_groups, cells, probe_radius, resolution, g.d_sasa,
                                g.d_iso, g.d_totals, g.d_group_totals, images_out))
            return -1;
        if (group_batch_download(c, g)) return -1;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
        return 0;
    }();
    return rc ? set_err(err_out, err_len, chunk_failed(b, c)) : 0;
    });
}

extern "C" int freesasa_gpu_calc_groups_periodic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                 const int32_t *group, const int32_t *n_groups, const double *cells, int alg,
                                                 double probe_radius, int resolution, double *sasa_out, double *iso_out, double *totals_out,
                                                 double *group_totals_out, int64_t *images_out, int device, char *err_out, int err_len)
{
    return calc_groups_periodic(false, xyz, radii, offsets, n_structs, group, n_groups, cells, alg, probe_radius, resolution, sasa_out, iso_out,
                                totals_out, group_totals_out, images_out, device, err_out, err_len);
}
extern "C" int freesasa_gpu_calc_groups_periodic_triclinic(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                           const int32_t *group, const int32_t *n_groups, const double *cells6, int alg,
                                                           double probe_radius, int resolution, double *sasa_out, double *iso_out,
                                                           double *totals_out, double *group_totals_out, int64_t *images_out, int device,
                                                           char *err_out, int err_len)
{
    return calc_groups_periodic(true, xyz, radii, offsets, n_structs, group, n_groups, cells6, alg, probe_radius, resolution, sasa_out, iso_out,
                                totals_out, group_totals_out, images_out, device, err_out, err_len);
}
