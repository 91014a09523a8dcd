/*
 * gpu_ops.hip — device-side aggregates over per-atom areas (segments, atom classes, residues, selections: what the reference's
 * result tree adds up on the host, src/node.c:717-764, src/classifier.c:830-866, src/rsa.c:14-25) and the test hooks
 * that run the integer / exact parts of the Lee-Richards kernel on their own.  Host code; kernels in gpu_kernels.hip.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>
#include <string.h>
#include <utility>
#include <vector>

#include "engine_internal.h"
#include "select_program.h"

extern "C" int freesasa_gpu_segment_sums_dev(freesasa_gpu_ctx *c, const double *d_sasa, const int64_t *seg,
                                             int n_segs, double *d_out)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    c->err[0] = 0;
    if (!d_sasa || !seg || !d_out || n_segs <= 0) return ctx_fail(c, "bad argument");
    for (int k = 0; k < n_segs; ++k)
        if (seg[k + 1] < seg[k]) return ctx_fail(c, "segment offsets must be non-decreasing");
    HIP_TRY(c, hipSetDevice(c->device));
    if (ensure(c, c->seg, sizeof(int64_t) * ((size_t)n_segs + 1))) return -1;
    HIP_TRY(c, hipMemcpyAsync(c->seg.p, seg, sizeof(int64_t) * ((size_t)n_segs + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, kl_segment_sums(d_sasa, (const int64_t *)c->seg.p, n_segs, seg[n_segs] - seg[0] < (int64_t)64 * n_segs, d_out, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
    });
}

extern "C" int freesasa_gpu_class_sums_dev(freesasa_gpu_ctx *c, const double *d_sasa, const unsigned char *d_class,
                                           const int64_t *offsets, int n_structs, double *d_out)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    c->err[0] = 0;
    if (!d_sasa || !d_class || !offsets || !d_out || n_structs <= 0) return ctx_fail(c, "bad argument");
    for (int k = 0; k < n_structs; ++k)
        if (offsets[k + 1] < offsets[k]) return ctx_fail(c, "structure offsets must be non-decreasing");
    HIP_TRY(c, hipSetDevice(c->device));
    if (ensure(c, c->seg, sizeof(int64_t) * ((size_t)n_structs + 1))) return -1;
    HIP_TRY(c, hipMemcpyAsync(c->seg.p, offsets, sizeof(int64_t) * ((size_t)n_structs + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, kl_class_sums(d_sasa, d_class, (const int64_t *)c->seg.p, n_structs, d_out, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
    });
}

extern "C" int freesasa_gpu_residue_areas_dev(freesasa_gpu_ctx *c, const double *d_sasa, const unsigned char *d_class,
                                              const unsigned char *d_backbone, const int64_t *res_first, int n_res,
                                              const short *ref_row, const double *ref_table, int ref_rows,
                                              double *d_abs, double *d_rel)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    c->err[0] = 0;
    if (!d_sasa || !d_class || !d_backbone || !res_first || !d_abs || n_res <= 0) return ctx_fail(c, "bad argument");
    if (d_rel && (!ref_row || !ref_table || ref_rows <= 0)) return ctx_fail(c, "relative areas need the reference rows and table");
    for (int k = 0; k < n_res; ++k) {
        if (res_first[k + 1] < res_first[k]) return ctx_fail(c, "residue offsets must be non-decreasing");
        if (d_rel && ref_row[k] >= ref_rows) return ctx_fail(c, "reference row out of range");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    /* one staging buffer: offsets, reference table, reference rows */
    const size_t b_first = sizeof(int64_t) * ((size_t)n_res + 1);
    const size_t b_table = d_rel ? sizeof(double) * 5 * (size_t)ref_rows : 0;
    const size_t b_rows = d_rel ? sizeof(short) * (size_t)n_res : 0;
    if (ensure(c, c->seg, b_first + b_table + b_rows)) return -1;
    char *base = (char *)c->seg.p;
    HIP_TRY(c, hipMemcpyAsync(base, res_first, b_first, hipMemcpyHostToDevice, c->stream));
    if (d_rel) {
        HIP_TRY(c, hipMemcpyAsync(base + b_first, ref_table, b_table, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(base + b_first + b_table, ref_row, b_rows, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, kl_residue_areas(d_sasa, d_class, d_backbone, (const int64_t *)base, d_rel ? (const short *)(base + b_first + b_table) : nullptr,
                                d_rel ? (const double *)(base + b_first) : nullptr, d_abs, d_rel, n_res, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
    });
}

/* (engine_internal.h) the same kernel for callers whose residue arrays are on the device already: the file sweep's table */
int residue_areas_resident(freesasa_gpu_ctx *c, const double *d_sasa, const unsigned char *d_class, const unsigned char *d_backbone,
                           const int64_t *d_res_first, const short *d_ref_row, int n_res, double *d_abs, double *d_rel)
{
    if (!d_sasa || !d_class || !d_backbone || !d_res_first || !d_abs || n_res <= 0) return ctx_fail(c, "bad argument");
    const double *d_table = nullptr;
    if (d_ref_row) {
        if (!c->res_table.p) {
            const int rows = freesasa_ingest_residue_reference_table(nullptr);
            c->res_table_host.resize(5 * (size_t)rows); /* (lives in the context: the copy may run later) */
            freesasa_ingest_residue_reference_table(c->res_table_host.data());
            if (ensure(c, c->res_table, 8 * c->res_table_host.size())) return -1;
            if (hipMemcpyAsync(c->res_table.p, c->res_table_host.data(), 8 * c->res_table_host.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
                (void)hipFree(c->res_table.p);
                c->res_table = DevBuf();
                return ctx_fail(c, "upload of the reference areas failed");
            }
        }
        d_table = (const double *)c->res_table.p;
    }
    HIP_TRY(c, kl_residue_areas(d_sasa, d_class, d_backbone, d_res_first, d_ref_row, d_table, d_abs, d_ref_row ? d_rel : nullptr, n_res, c->stream));
    return 0;
}

/* ------------------------------------------------------------------ selection areas (select_kernels.h) */

/* (engine_internal.h) */
int select_resident(freesasa_gpu_ctx *c, const freesasa_ingest_selection *sel, sasa::SelArgs &sa)
{
    int n_words = 0, flags = 0;
    const freesasa_sel_word *prog = (const freesasa_sel_word *)freesasa_ingest_selection_program(sel, &n_words, &flags);
    const int S = freesasa_ingest_selection_count(sel);
    if (S < 1 || n_words < 1 || sa.n_atoms <= 0 || sa.n_structs <= 0 || sa.n_res <= 0) return ctx_fail(c, "bad argument");
    DevBuf *B = c->parse;
    const size_t cells = (size_t)sa.n_structs * (size_t)S;
    if (ensure(c, B[PBUF_SEL_PROG], sizeof(freesasa_sel_word) * (size_t)n_words) || ensure(c, B[PBUF_SEL_BITS], 8 * (size_t)sa.n_atoms) ||
        ensure(c, B[PBUF_SEL_OUT], 16 * cells))
        return -1;
    /* (the program lives in the set, which outlives the call: the copy may run later) */
    HIP_TRY(c, hipMemcpyAsync(B[PBUF_SEL_PROG].p, prog, sizeof(freesasa_sel_word) * (size_t)n_words, hipMemcpyHostToDevice, c->stream));
    sa.prog = (const freesasa_sel_word *)B[PBUF_SEL_PROG].p; sa.n_words = n_words; sa.flags = flags; sa.n_sel = S;
    sa.bits = (uint64_t *)B[PBUF_SEL_BITS].p;
    sa.area = (double *)B[PBUF_SEL_OUT].p; sa.count = (long long *)(sa.area + cells);
    HIP_TRY(c, kl_sel_mask(sa, c->stream));
    HIP_TRY(c, kl_sel_sums(sa, c->stream));
    return 0;
}

extern "C" int freesasa_gpu_select_batch(const freesasa_ingest_batch *b, const freesasa_ingest_selection *sel, const double *sasa,
                                         double *area_out, long long *atoms_out, unsigned long long *bits_out, int device,
                                         char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!b || !sel || !sasa || !area_out || !atoms_out) return set_err(err_out, err_len, "null argument");
    const int S = freesasa_ingest_selection_count(sel), ns = b->n_structs;
    const int64_t n = b->n_atoms, R = b->n_residues;
    if (ns < 0 || n < 0 || R < 0 || (n > 0 && (R == 0 || ns == 0))) return set_err(err_out, err_len, "inconsistent batch");
    for (int k = 0; k < ns; ++k)
        if (b->offsets[k + 1] < b->offsets[k]) return set_err(err_out, err_len, "structure offsets must be non-decreasing");
    for (int64_t r = 0; r < R; ++r)
        if (b->res_first[r + 1] < b->res_first[r]) return set_err(err_out, err_len, "residue offsets must be non-decreasing");
    if (ns > 0 && (b->offsets[0] != 0 || b->offsets[ns] != n || (R > 0 && (b->res_first[0] != 0 || b->res_first[R] != n))))
        return set_err(err_out, err_len, "inconsistent batch");
    for (size_t k = 0; k < (size_t)ns * (size_t)S; ++k) { area_out[k] = 0; atoms_out[k] = 0; }
    if (n == 0) return 0; /* (nothing to select from: freesasa_ingest_select gives 0 as well) */
    if (freesasa_gpu_device_count() <= 0) return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
        std::vector<uint64_t> keys((size_t)n); /* (declared before the lease: freed after its stream is idle) */
        sel_pack_atom_keys(b->atom_name, b->atom_symbol, n, keys.data());
        PoolLease lease(device);
        freesasa_gpu_ctx *c = lease.c;
        if (!c) return set_err(err_out, err_len, "could not create a GPU context");
        c->err[0] = 0;
        const int rc = [&]() -> int {
            HIP_TRY(c, hipSetDevice(c->device));
            DevBuf *B = c->parse;
            const size_t b_off = 8 * ((size_t)ns + 1), b_first = 8 * ((size_t)R + 1);
            if (ensure(c, c->h_sasa, 8 * (size_t)n) || ensure(c, c->seg, b_off + b_first) || ensure(c, B[PBUF_ATOM_KEYS], 8 * (size_t)n) ||
                ensure(c, B[PBUF_SEL_LABELS], 14 * (size_t)R))
                return -1;
            char *seg = (char *)c->seg.p, *lab = (char *)B[PBUF_SEL_LABELS].p;
            hipStream_t st = c->stream;
            HIP_TRY(c, hipMemcpyAsync(c->h_sasa.p, sasa, 8 * (size_t)n, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(seg, b->offsets, b_off, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(seg + b_off, b->res_first, b_first, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(B[PBUF_ATOM_KEYS].p, keys.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(lab, b->res_name, 4 * (size_t)R, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(lab + 4 * (size_t)R, b->res_chain, 4 * (size_t)R, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(lab + 8 * (size_t)R, b->res_number, 6 * (size_t)R, hipMemcpyHostToDevice, st));
            sasa::SelArgs sa;
            memset(&sa, 0, sizeof sa);
            sa.akey = (const uint64_t *)B[PBUF_ATOM_KEYS].p;
            sa.offsets = (const int64_t *)seg; sa.n_structs = ns; sa.n_atoms = n;
            sa.res_first = (const int64_t *)(seg + b_off); sa.n_res = R; sa.n_res_dev = 0;
            sa.name_h = (const uint32_t *)lab; sa.chain_h = (const uint32_t *)(lab + 4 * (size_t)R); sa.number_h = (const uint16_t *)(lab + 8 * (size_t)R);
            sa.sasa = (const double *)c->h_sasa.p;
            if (select_resident(c, sel, sa)) return -1;
            const size_t cells = (size_t)ns * (size_t)S;
            HIP_TRY(c, hipMemcpyAsync(area_out, sa.area, 8 * cells, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(atoms_out, sa.count, 8 * cells, hipMemcpyDeviceToHost, st));
            if (bits_out) HIP_TRY(c, hipMemcpyAsync(bits_out, sa.bits, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            return 0;
        }();
        if (rc) { (void)hipStreamSynchronize(c->stream); return set_err(err_out, err_len, c->err[0] ? c->err : "selection areas failed"); }
        return 0;
    });
}

/* ------------------------------------------------------------------ test hooks of the L&R kernel's integer parts */

/* The neighbor sets the Lee-Richards kernel finds (ref: freesasa_nb_new with radii + probe, src/nb.c:524-557, what
 * tests/test_nb.c checks): per atom, in original order, the number of neighbors and, if d_nb is given, the first
 * nb_cap of them (original atom indices, in order of discovery).  Device pointers; d_nb may be NULL. */
extern "C" int freesasa_gpu_lr_neighbors_dev(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                                             int n_structs, double probe, int *d_nn, int *d_nb, int nb_cap)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    if (!d_nn || (d_nb && nb_cap <= 0)) return ctx_fail(c, "bad argument");
    const int64_t n = offsets && n_structs > 0 ? offsets[n_structs] : 0;
    if (n <= 0) return ctx_fail(c, "empty batch");
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first, as for every synchronous entry) */
    if (hipSetDevice(c->device) != hipSuccess || ensure(c, c->h_sasa, 8 * (size_t)n)) return -1;
    struct Hooks { /* (taken off the context on every way out) */
        freesasa_gpu_ctx *c;
        ~Hooks() { c->dbg_nn = c->dbg_nb = nullptr; c->dbg_cap = 0; }
    } hooks{c};
    c->dbg_nn = d_nn; c->dbg_nb = d_nb; c->dbg_cap = nb_cap;
    return run_batch(c, true, d_xyz, d_radii, offsets, n_structs, probe, 20, nullptr, (double *)c->h_sasa.p, nullptr, nullptr);
    });
}

/* The exposed arc length of n_sets sets of arcs (start, end pairs in [0, 2 pi], set k = arcs first[k] .. first[k+1]),
 * computed on the device by the arc union and sweep of the Lee-Richards kernel (ref: exposed_arc_length,
 * src/sasa_lr.c:389-408, and its KATs :455-475).  Host arrays; at most 64 sets. */
extern "C" int freesasa_gpu_arc_union_dev(freesasa_gpu_ctx *c, const double *arcs, const int *first, int n_sets, double *out)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    if (!arcs || !first || !out || n_sets <= 0 || n_sets > 64) return ctx_fail(c, "bad argument");
    const int total = first[n_sets];
    /* the arc pass feeds the union in the order of the arcs' mid-points (the neighbors' directions) */
    std::vector<double> sorted(2 * (size_t)(total > 0 ? total : 1));
    for (int k = 0; k < n_sets; ++k) {
        std::vector<std::pair<double, double>> v;
        for (int i = first[k]; i < first[k + 1]; ++i) v.emplace_back(arcs[2 * i], arcs[2 * i + 1]);
        std::stable_sort(v.begin(), v.end(), [](const std::pair<double, double> &x, const std::pair<double, double> &y) {
            return x.first + x.second < y.first + y.second; });
        for (size_t i = 0; i < v.size(); ++i) { sorted[2 * (first[k] + i)] = v[i].first; sorted[2 * (first[k] + i) + 1] = v[i].second; }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t b_arcs = sizeof(double) * sorted.size(), b_first = sizeof(int) * ((size_t)n_sets + 1);
    if (ensure(c, c->seg, b_arcs + b_first + 8 * 64 + 64)) return -1;
    char *base = (char *)c->seg.p;
    HIP_TRY(c, hipMemcpyAsync(base, sorted.data(), b_arcs, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(base + b_arcs, first, b_first, hipMemcpyHostToDevice, c->stream));
    double *d_out = (double *)(base + ((b_arcs + b_first + 15) & ~(size_t)15));
    HIP_TRY(c, kl_arc_kat((const double *)base, (const int *)(base + b_arcs), n_sets, d_out, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)n_sets, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
    });
}

/* ------------------------------------------------------------------ test hooks: device-only arithmetic and lane primitives (kat_kernels.h) */

extern "C" int freesasa_gpu_kat_elementwise_dev(freesasa_gpu_ctx *c, int op, const double *a, const double *b, const double *in_c, long long n,
                                                double k, double *out0, double *out1)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    c->err[0] = 0;
    const int arrays = sasa::kat_ew_arrays(op);
    if (!arrays) return ctx_fail(c, "unknown op %d", op);
    if (n < 1 || n > KAT_EW_MAX) return ctx_fail(c, "n must be 1 .. %d", KAT_EW_MAX);
    const double *in[3] = {a, b, in_c};
    double *out[2] = {out0, out1};
    for (int j = 0; j < 3; ++j)
        if ((arrays >> j & 1) && !in[j]) return ctx_fail(c, "null argument");
    for (int j = 0; j < 2; ++j)
        if ((arrays >> (4 + j) & 1) && !out[j]) return ctx_fail(c, "null argument");
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first, as for every synchronous entry) */
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(double) * (size_t)n;
    if (ensure(c, c->seg, 5 * bytes)) return -1;
    double *d[5];
    for (int j = 0; j < 5; ++j) d[j] = (double *)c->seg.p + (size_t)j * (size_t)n;
    for (int j = 0; j < 3; ++j)
        if (arrays >> j & 1) HIP_TRY(c, hipMemcpyAsync(d[j], in[j], bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, kl_kat_elementwise(op, d[0], d[1], d[2], k, d[3], d[4], (int)n, c->stream));
    for (int j = 0; j < 2; ++j)
        if (arrays >> (4 + j) & 1) HIP_TRY(c, hipMemcpyAsync(out[j], d[3 + j], bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
    });
}

extern "C" int freesasa_gpu_kat_wave_dev(freesasa_gpu_ctx *c, int op, const uint64_t *in, int rows, uint64_t *out)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    c->err[0] = 0;
    if (op < 0 || op >= sasa::KAT_WAVE_OPS) return ctx_fail(c, "unknown op %d", op);
    if (rows < 1 || rows > KAT_WAVE_ROWS_MAX) return ctx_fail(c, "rows must be 1 .. %d", KAT_WAVE_ROWS_MAX);
    if (!in || !out) return ctx_fail(c, "null argument");
    if (const char *why = sasa::kat_wave_refusal(op, (const unsigned long long *)in, rows)) return ctx_fail(c, "%s", why);
    if (freesasa_gpu_wait(c)) return -1;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = 8 * (size_t)rows * LR2_LANES;
    if (ensure(c, c->seg, 2 * bytes)) return -1;
    unsigned long long *d_in = (unsigned long long *)c->seg.p, *d_out = d_in + (size_t)rows * LR2_LANES;
    HIP_TRY(c, hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, kl_kat_wave(op, d_in, d_out, rows, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
    });
}

/* ------------------------------------------------------------------ test hook: the cell sort on its own (include/freesasa_gpu.h) */

static_assert(FREESASA_GPU_CELL_SORT_STATUS_WORDS == sasa::ST_WORDS, "the hook hands out every status word");
static_assert(sizeof(sasa::GridS) == 48 && sizeof(sasa::SortIdx) == 16 && sizeof(sasa::Quad) == 32, "the records the hook's header describes");

extern "C" long long freesasa_gpu_cell_sort_cap(freesasa_gpu_ctx *c, long long n_atoms, int n_structs, long long cells_cap)
{
    if (!c || n_atoms < 1 || n_atoms > 1LL << 30 || n_structs < 1 || cells_cap < 0) return -1;
    if (cells_cap > 0) return cells_cap;
    /* (a batch in flight raises what the context has seen when it is collected: collected here, as the hook collects it, the
       two name the same number) */
    if (freesasa_gpu_wait(c)) return -1;
    return batch_cells_cap(c, (int)n_atoms, n_structs);
}

/* One pass of the cell sort in the arrangement the caller names, by the engine's own launches (cell_sort_enqueue), and
 * everything it wrote down to the caller's arrays.  Whatever the status words say, nothing is redone and the context learns
 * nothing: judge_status (gpu_engine.hip) is not asked. */
extern "C" int freesasa_gpu_cell_sort_dev(freesasa_gpu_ctx *c, const double *d_xyz, const double *d_radii, const int64_t *offsets,
                                          int n_structs, double probe, int arrangement, long long cells_cap, long long table_cells,
                                          int shared_radii, int32_t *status, int32_t *occ_stride, void *grid, int64_t *ncells, double *sq, void *s_idx,
                                          int32_t *cell_start, uint64_t *cell_tbl, int32_t *cell_first)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    c->err[0] = 0;
    if (!d_xyz || !d_radii || !offsets || !status || !occ_stride || !grid || !ncells || !sq || !s_idx) return ctx_fail(c, "null argument");
    if (n_structs <= 0) return ctx_fail(c, "n_structs must be > 0");
    if (offsets[0] != 0) return ctx_fail(c, "offsets[0] must be 0");
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] < offsets[s]) return ctx_fail(c, "offsets must be non-decreasing");
    const int64_t n64 = offsets[n_structs];
    if (n64 <= 0) return ctx_fail(c, "empty batch");
    if (n64 > (int64_t)1 << 30) return ctx_fail(c, "batch too large (max 2^30 atoms per call)");
    if (arrangement < 0 || arrangement > 2) return ctx_fail(c, "unknown arrangement %d (0: general pipeline, 1: k_sort_struct with the dense table, 2: with the compact table)", arrangement);
    if (arrangement == 2 ? !cell_tbl || !cell_first : !cell_start) return ctx_fail(c, "null argument");
    if (cells_cap < 0) return ctx_fail(c, "cells_cap must not be negative");
    if (cells_cap > c->max_cells) return ctx_fail(c, "cells_cap is beyond the %lld cells a context holds", c->max_cells);
    if (shared_radii != 0 && shared_radii != 1) return ctx_fail(c, "shared_radii must be 0 or 1");
    const int n = (int)n64;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first, as for every synchronous entry) */
    HIP_TRY(c, hipSetDevice(c->device));
    struct Radii { /* (put back on every way out) */
        freesasa_gpu_ctx *c;
        bool was;
        ~Radii() { c->shared_radii = was; }
    } radii{c, c->shared_radii};
    c->shared_radii = shared_radii != 0;
    const long long cap = cells_cap > 0 ? cells_cap : batch_cells_cap(c, n, n_structs);
    /* (everything below is copied into the caller's arrays by this number) */
    if (table_cells != cap) return ctx_fail(c, "the table arrays are sized for %lld cells, the pass takes %lld (freesasa_gpu_cell_sort_cap)", table_cells, cap);
    const size_t nb = (size_t)n, ns = (size_t)n_structs;
    hipStream_t st = c->stream;
    sasa::PipeArgs pa;
    int rc = cell_sort_enqueue(c, d_xyz, d_radii, offsets, n_structs, n, probe, -1, 0, arrangement != 0, arrangement == 2, cap, true, pa);
    if (!rc) {
        bool ok = hipMemcpyAsync(status, pa.status, sizeof(int) * (size_t)sasa::ST_WORDS, hipMemcpyDeviceToHost, st) == hipSuccess &&
                  hipMemcpyAsync(grid, pa.grid, sizeof(sasa::GridS) * ns, hipMemcpyDeviceToHost, st) == hipSuccess &&
                  hipMemcpyAsync(ncells, pa.ncells, 8 * ns, hipMemcpyDeviceToHost, st) == hipSuccess &&
                  hipMemcpyAsync(sq, pa.sq, 32 * nb, hipMemcpyDeviceToHost, st) == hipSuccess &&
                  hipMemcpyAsync(s_idx, pa.s_idx, 16 * nb, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (ok && arrangement == 2)
            ok = hipMemcpyAsync(cell_tbl, pa.cell_tbl, 8 * ((size_t)(cap >> 5) + 2), hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipMemcpyAsync(cell_first, pa.cell_first, 4 * (nb + ns + 2), hipMemcpyDeviceToHost, st) == hipSuccess;
        else if (ok)
            ok = hipMemcpyAsync(cell_start, pa.cell_start, 4 * ((size_t)cap + 2), hipMemcpyDeviceToHost, st) == hipSuccess;
        if (!ok) rc = ctx_fail(c, "could not read the cell sort's arrays back");
    }
    /* (nothing is left running on the stream, whatever failed) */
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = ctx_fail(c, "could not read the cell sort's arrays back");
    if (rc) return -1;
    *occ_stride = pa.occ_stride; /* (as a context without history: the density samples are part of what is checked) */
    return 0;
    });
}
