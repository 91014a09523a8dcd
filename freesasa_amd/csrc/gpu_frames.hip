/*
 * gpu_frames.hip — the frame source of the trajectory drivers (FrameSource, engine_internal.h): the ONE place that knows where
 * the frames of a run come from - raw fp64 frames (in host memory or in a file), raw fp32 frames, a DCD, an AMBER NetCDF, a
 * GROMACS XTC or a GROMACS TRR file (include/freesasa_gpu.h has the formats; dcd.c, netcdf.c, xtc.c and trr.c read their
 * headers).  The driver (gpu_drivers.hip) opens a source, asks it for the frames of the file and the sizes of a shard, and
 * calls read (host: the shard's bytes into page-locked memory, checked) and to_frames (device: compact fp64 frames in
 * c->h_xyz) per shard.  Raw, DCD and NetCDF frames lie at a constant stride; XTC and TRR shards are cut by the index of the
 * file, and share the rule of their box.  Host code; kernels in gpu_kernels.hip.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "engine_internal.h"

/* What open needs to know of a container: its bit of frames_f32 and the bit's number, how the messages call it, why it takes
   no header_bytes and whether it says so BEFORE the bits that exclude it are looked at, and what it lacks when it has no cell.
   In the order of the bits: of several that are set the highest speaks, and names the lowest it excludes. */
struct FrameContainer {
    int bit, no;
    FrameSource::Kind kind;
    const char *a_file, *name, *no_header;
    bool header_first;
    const char *no_cell;
};
static const FrameContainer containers[4] = {
    {FREESASA_GPU_FRAMES_DCD, 2, FrameSource::DCD, "a DCD file", "DCD", "the byte of its first frame comes from its header", true,
     "periodic images need a DCD file with a unit-cell record per frame: this one has none"},
    {FREESASA_GPU_FRAMES_NETCDF, 5, FrameSource::NETCDF, "an AMBER NetCDF file", "NetCDF", "the byte of its first record comes from its header", false,
     "periodic images need a NetCDF file with the variables cell_lengths and cell_angles: this one has no cell"},
    {FREESASA_GPU_FRAMES_XTC, 6, FrameSource::XTC, "an XTC file", "XTC", "its frames are found by their headers", false,
     "periodic images need an XTC file with a box: the box of this one's first frame is all zero"},
    {FREESASA_GPU_FRAMES_TRR, 7, FrameSource::TRR, "a TRR file", "TRR", "its frames are found by their headers", false,
     "periodic images need a TRR file with a box: this one's first coordinate frame has none, or one that is all zero"}};

/* A shard behind its in_bytes bytes, in the staging and on the device (c->g_xyz) alike, every part at a multiple of 8: its cells
   (periodic runs: cell_bytes per frame) | extra: one descriptor per frame of an XTC shard, the byte of every frame's x[0] within
   a TRR shard (one int64 per frame) - up to here the one copy from the host - | XTC: group count and status per frame (in the
   staging: where they come down to) | the group records (at a multiple of 16) | with `keep` the fp32 frames xtc_unpack writes
   (without: kl_widen_f32's input, c->h_counts) | end */
struct ShardLayout { size_t cells, extra, count, rec, f32, end; };
static ShardLayout shard_layout(size_t in_bytes, size_t nf, size_t frame_atoms, size_t cell_bytes, bool keep)
{
    ShardLayout a;
    a.cells = (in_bytes + 7) & ~(size_t)7;
    a.extra = a.cells + cell_bytes * nf;
    a.count = a.extra + sizeof(freesasa_gpu_xtc_frame) * nf;
    a.rec = (a.count + 8 * nf + 15) & ~(size_t)15;
    a.f32 = a.rec + sizeof(sasa::XtcRec) * frame_atoms * nf;
    a.end = a.f32 + (keep ? 12 * frame_atoms * nf : 0);
    return a;
}

/* ------------------------------------------------------------------ open */

/* the header of a container, or the index of its frames: the stride or the index, the byte of frame 0, what the file says of
   its atoms and its cell.  The index arrays are freed on every path; what allocates runs inside guarded(). */
int FrameSource::read_header(const char *path, int *file_atoms, bool *has_cell, char *err_out, int err_len)
{
    int64_t *offsets = nullptr;
    long long indexed_frames = 0;
    if (kind == DCD) {
        if (freesasa_gpu_dcd_info_read(path, &dcd, err_out, err_len)) return -1;
        first = dcd.first_frame; stride = (size_t)dcd.frame_bytes; *file_atoms = dcd.n_atoms; *has_cell = dcd.has_cell != 0;
    } else if (kind == NETCDF) {
        if (freesasa_gpu_nc_info_read(path, &nc, err_out, err_len)) return -1;
        first = nc.first_record; stride = (size_t)nc.record_bytes; *file_atoms = nc.n_atoms; *has_cell = nc.has_cell != 0;
    } else if (kind == XTC) {
        freesasa_gpu_xtc_info x = {};
        if (freesasa_gpu_xtc_index_read(path, &x, &offsets, err_out, err_len)) return -1;
        indexed_frames = x.n_frames; *file_atoms = x.n_atoms; *has_cell = x.has_box != 0;
    } else {
        freesasa_gpu_trr_info t = {};
        if (freesasa_gpu_trr_index_read(path, &t, &offsets, err_out, err_len)) return -1;
        indexed_frames = t.n_frames; *file_atoms = t.n_atoms; *has_cell = t.has_box != 0; real_bytes = t.real_bytes;
    }
    if (!offsets) return 0;
    const int rc = guarded(err_out, err_len, [&]() -> int { off.assign(offsets, offsets + indexed_frames + 1); return 0; });
    if (kind == XTC) freesasa_gpu_xtc_index_free(offsets);
    else freesasa_gpu_trr_index_free(offsets);
    return rc;
}

int FrameSource::open(const char *path, int frames_f32, long long header_bytes, long long frame_atoms, char *err_out, int err_len)
{
    const bool images = (frames_f32 & FREESASA_GPU_FRAMES_PBC) != 0;
    if (images && !(frames_f32 & (FREESASA_GPU_FRAMES_DCD | FREESASA_GPU_FRAMES_NETCDF | FREESASA_GPU_FRAMES_XTC | FREESASA_GPU_FRAMES_TRR)))
        return set_err(err_out, err_len, "bit 3 of frames_f32 (periodic images) needs bit 2 (a DCD file), bit 5 (an AMBER NetCDF file), bit 6 (an XTC file) or bit 7 (a TRR file): raw frame files carry no cell");
    if ((frames_f32 & FREESASA_GPU_FRAMES_TRICLINIC) && !images)
        return set_err(err_out, err_len, "bit 4 of frames_f32 (triclinic cells) needs bit 3 (periodic images) and bit 2 (a DCD file), bit 5 (an AMBER NetCDF file), bit 6 (an XTC file) or bit 7 (a TRR file)");
    kind = (frames_f32 & FREESASA_GPU_FRAMES_F32) ? RAW_F32 : RAW_F64;
    fa = (size_t)frame_atoms; first = header_bytes; stride = (kind == RAW_F32 ? 12 : 24) * fa;
    for (int k = 3; k >= 0 && !con; --k)
        if (frames_f32 & containers[k].bit) con = &containers[k];
    if (!con) return 0;
    /* a container says for itself where its frames are and what they are: before a device is touched or an output file opened */
    char msg[200], no_header[200];
    snprintf(no_header, sizeof no_header, "header_bytes must be 0 with %s: %s", con->a_file, con->no_header);
    if (con->header_first && header_bytes != 0) return set_err(err_out, err_len, no_header);
    if (frames_f32 & FREESASA_GPU_FRAMES_F32) {
        snprintf(msg, sizeof msg, "bit 0 of frames_f32 (raw fp32 frames) and bit %d (%s) exclude each other%s", con->no, con->a_file,
                 con->kind == TRR ? ": the file says its own precision" : "");
        return set_err(err_out, err_len, msg);
    }
    for (const FrameContainer *o = containers; o < con; ++o)
        if (frames_f32 & o->bit) {
            snprintf(msg, sizeof msg, "bit %d of frames_f32 (%s) and bit %d (%s) exclude each other", o->no, o->a_file, con->no, con->a_file);
            return set_err(err_out, err_len, msg);
        }
    if (header_bytes != 0) return set_err(err_out, err_len, no_header);
    kind = con->kind;
    int file_atoms = 0;
    bool has_cell = false;
    if (read_header(path, &file_atoms, &has_cell, err_out, err_len)) return -1;
    if (file_atoms != frame_atoms) {
        snprintf(msg, sizeof msg, "the %s file holds %d atoms per frame, the run expects %lld", con->name, file_atoms, frame_atoms);
        return set_err(err_out, err_len, msg);
    }
    if (images) {
        if (!has_cell) return set_err(err_out, err_len, con->no_cell);
        pbc = true;
        tri = (frames_f32 & FREESASA_GPU_FRAMES_TRICLINIC) != 0;
    }
    return 0;
}

void FrameSource::open_memory(const double *frames, size_t frame_atoms)
{
    kind = RAW_F64; mem = frames; fa = frame_atoms; stride = 24 * fa;
}

long long FrameSource::frames_in_file(long long file_bytes) const
{
    return indexed() ? (long long)off.size() - 1 : (file_bytes - first) / (long long)stride;
}
int FrameSource::head_f32() const
{
    return (kind == RAW_F32 ? FREESASA_GPU_FRAMES_F32 : 0) | (con ? con->bit : 0) | (pbc ? FREESASA_GPU_FRAMES_PBC : 0) | (tri ? FREESASA_GPU_FRAMES_TRICLINIC : 0);
}

/* ------------------------------------------------------------------ sizes */

void FrameSource::plan(size_t n_atoms, bool with_index, long long n_frames, int frames_per_batch, const double *radii, double probe)
{
    n = n_atoms; gather = with_index; FB = (size_t)frames_per_batch;
    cut = pbc ? periodic_cutoff(radii, (int64_t)n_atoms, probe) : 0;
    mem_pinned = mem && host_pinned(mem);
    max_bytes = indexed() ? 0 : stride * FB;
    for (long long f0 = 0; indexed() && f0 < n_frames; f0 += frames_per_batch) {
        const size_t b = shard_bytes(f0, n_frames - f0 < frames_per_batch ? n_frames - f0 : frames_per_batch);
        if (b > max_bytes) max_bytes = b;
    }
}
size_t FrameSource::shard_bytes(long long f0, long long nf) const
{
    return indexed() ? (size_t)(off[(size_t)(f0 + nf)] - off[(size_t)f0]) : stride * (size_t)nf;
}
static ShardLayout layout_of(const FrameSource &s, size_t in_bytes, size_t nf)
{
    return shard_layout(in_bytes, nf, s.fa, s.pbc ? 8 * s.cell_doubles() : 0, s.gather);
}
size_t FrameSource::up_bytes(size_t in_bytes, size_t nf) const
{
    const ShardLayout at = layout_of(*this, in_bytes, nf);
    return kind == XTC ? at.count : kind == TRR ? at.extra + 8 * nf : pbc ? at.extra : in_bytes;
}
size_t FrameSource::xyz_bytes() const
{
    if (kind <= RAW_F32 && !gather) return 0; /* (raw frames without an index go where the engine, or kl_widen_f32, reads them) */
    return kind == XTC ? layout_of(*this, max_bytes, FB).end : up_bytes(max_bytes, FB);
}
const double *FrameSource::host_cells(const freesasa_gpu_ctx *c, size_t in_bytes) const
{
    return (const double *)((const char *)c->stage_in + layout_of(*this, in_bytes, 0).cells);
}
const double *FrameSource::dev_cells(const freesasa_gpu_ctx *c, size_t in_bytes) const
{
    return (const double *)((const char *)c->g_xyz.p + layout_of(*this, in_bytes, 0).cells);
}

/* ------------------------------------------------------------------ read + check (host) */

/* every record marker of the DCD frames [0, nf) at `bytes`: 6 per frame, 2 more with a cell record, 2 more with a 4th dimension.
   Returns the first frame with a wrong one, or -1. */
static long long dcd_damaged_frame(const freesasa_gpu_dcd_info &d, const char *bytes, long long nf)
{
    auto word = [&](uint32_t v) { return d.big_endian ? __builtin_bswap32(v) : v; };
    const uint32_t cell = word(48), plane = word(4u * (uint32_t)d.n_atoms);
    for (long long f = 0; f < nf; ++f) {
        const char *p = bytes + f * d.frame_bytes;
        uint32_t w[2];
        if (d.has_cell) {
            memcpy(&w[0], p, 4); memcpy(&w[1], p + 52, 4);
            if (w[0] != cell || w[1] != cell) return f;
            p += 56;
        }
        for (int k = 0; k < 3 + d.has_4d; ++k, p += d.plane_bytes) {
            memcpy(&w[0], p, 4); memcpy(&w[1], p + d.plane_bytes - 4, 4);
            if (w[0] != plane || w[1] != plane) return f;
        }
    }
    return -1;
}

/* The descriptors of the XTC frames [f0, f0 + nf) at `bytes` (xtc.c: every header checked again as it lies in the staging - the
   device trusts the descriptors for its bounds - and against the index: a frame must be as long as the index pass found it).
   Returns -1, or the first frame that fails, the reason in why. */
static long long xtc_descriptors(const int64_t *off, const char *bytes, long long nf, int frame_atoms, freesasa_gpu_xtc_frame *desc, char *why, size_t why_len)
{
    for (long long f = 0; f < nf; ++f) {
        long long frame_bytes = 0;
        const long long at = off[f] - off[0], len = off[f + 1] - off[f];
        if (freesasa_gpu_xtc_frame_desc(bytes + at, len, frame_atoms, at + FREESASA_GPU_XTC_HEADER, &desc[f], &frame_bytes, why, (int)why_len)) return f;
        if (frame_bytes != len) { snprintf(why, why_len, "its header is not the one the index was made from"); return f; }
    }
    return -1;
}

/* The frames [f0, f0 + nf) of a TRR file at `bytes` (trr.c): EVERY header of the shard checked again as it lies in the staging -
   the device trusts x_off for its bounds - and against the index: a frame's stretch begins with a record that holds coordinates,
   the records behind it hold none, and they end where the index says the next frame begins.  x_off[nf]: the byte of every
   frame's x[0] within the shard.  Returns -1, or the first frame that fails, the reason in why. */
static long long trr_descriptors(const int64_t *off, const char *bytes, long long nf, int frame_atoms, int real_bytes, int64_t *x_off, char *why, size_t why_len)
{
    for (long long f = 0; f < nf; ++f) {
        long long at = off[f] - off[0];
        const long long end = off[f + 1] - off[0];
        for (bool first = true; at < end; first = false) {
            freesasa_gpu_trr_record r;
            if (freesasa_gpu_trr_frame_desc(bytes + at, end - at, frame_atoms, real_bytes, at, &r, why, (int)why_len)) return f;
            if (first != (r.has_x != 0)) { snprintf(why, why_len, "its headers are not the ones the index was made from"); return f; }
            if (first) x_off[f] = r.x_off;
            at += r.record_bytes; /* (<= end: the record lies within what is left) */
        }
    }
    return -1;
}

/* the orthorhombic rule of every container: the edges are finite and reach cut; they are the cell then */
static bool ortho_edges_bad(const double len[3], double cut, double *cell, char *why, size_t why_len)
{
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(len[k])) { snprintf(why, why_len, "edge %c of its cell is not finite", "xyz"[k]); return true; }
        if (!(len[k] >= cut)) {
            snprintf(why, why_len, "edge %c of its cell is %.9g, shorter than c = 2 (max radius + probe) = %.9g", "xyz"[k], len[k], cut);
            return true;
        }
        cell[k] = len[k];
    }
    return false;
}

/* A decoded cell h[6] of a frame: its shape, and its three widths - made here, into h[6 .. 8] - against cut.  edge: A, B, C as the
   file holds them, for the reason.  false, or true with the reason in why. */
static bool tri_cell_bad(double *h, const double edge[3], double cut, char *why, size_t why_len)
{
    const int shape = periodic_cell6_bad(h);
    if (shape) { /* (an edge that is not positive: everything else the decoder has refused) */
        snprintf(why, why_len, "edge %c of its cell is %.9g: not positive", shape == 1 ? 'A' : shape == 3 ? 'B' : 'C', edge[shape == 1 ? 0 : shape == 3 ? 1 : 2]);
        return true;
    }
    (void)freesasa_gpu_cell_widths(h, h + 6);
    const int bad = periodic_widths_bad(h + 6, cut);
    if (bad) snprintf(why, why_len, "width %c of its cell is %.9g, smaller than c = 2 (max radius + probe) = %.9g", "abc"[bad - 1], h[6 + bad - 1], cut);
    return bad != 0;
}

/* The cell of ONE frame from its box, for XTC and TRR frames alike: nine numbers in nm as doubles - each what the file holds,
   widened -, GROMACS' lower triangle - rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz) -, each element b * 10.0. */
static bool box_cell_bad(const double b[9], bool tri, double cut, double *cell, char *why, size_t why_len)
{
    bool zero = true;
    for (int k = 0; k < 9; ++k) zero = zero && b[k] == 0.0;
    if (zero) { snprintf(why, why_len, "its box is all zero: the frame carries no cell"); return true; }
    const int upper[3] = {1, 2, 5}, lower[3] = {3, 6, 7};
    for (int k = 0; k < 3; ++k)
        if (b[upper[k]] != 0.0) {
            snprintf(why, why_len, "element [%d][%d] of its box is %.9g: a box must be lower-triangular", upper[k] / 3, upper[k] % 3, b[upper[k]]);
            return true;
        }
    const double len[3] = {b[0] * 10.0, b[4] * 10.0, b[8] * 10.0};
    if (!tri) {
        for (int k = 0; k < 3; ++k)
            if (b[lower[k]] != 0.0) {
                snprintf(why, why_len, "its cell is not orthorhombic (element [%d][%d] of its box is %.9g): triclinic cells need bit 4", lower[k] / 3, lower[k] % 3, b[lower[k]]);
                return true;
            }
        return ortho_edges_bad(len, cut, cell, why, why_len);
    }
    const int at[6] = {0, 3, 4, 6, 7, 8};
    for (int k = 0; k < 6; ++k) {
        cell[k] = b[at[k]] * 10.0;
        if (!isfinite(cell[k])) { snprintf(why, why_len, "element [%d][%d] of its box is not finite", at[k] / 3, at[k] % 3); return true; }
    }
    return tri_cell_bad(cell, len, cut, why, why_len);
}

/* The cell of frame f of the shard at `bytes`, whose frames begin at off[0 .. ] (indexed kinds; their headers are checked).
   Orthorhombic runs: the edges into cell[3]; triclinic runs: the six numbers of the cell and, behind them, its three widths
   into cell[9].  false, or true with the reason periodic images are not offered for this frame in why: a shape the run does
   not take, an edge that is not finite, an edge or a width below cut. */
static bool frame_cell_bad(const FrameSource &s, const int64_t *off, const char *bytes, long long f, double *cell, char *why, size_t why_len)
{
    double b[9];
    if (s.kind == FrameSource::DCD) {
        /* 6 doubles in the file's byte order, CHARMM's A, gamma, B, beta, alpha, C - the angles as cosines or as degrees */
        double v[6];
        for (int k = 0; k < 6; ++k) {
            uint64_t w;
            memcpy(&w, bytes + f * s.dcd.frame_bytes + 4 + 8 * k, 8);
            if (s.dcd.big_endian) w = __builtin_bswap64(w);
            memcpy(&v[k], &w, 8);
        }
        const double edge[3] = {v[0], v[2], v[5]};
        if (s.tri) return freesasa_gpu_cell_from_dcd(v, cell, why, (int)why_len) || tri_cell_bad(cell, edge, s.cut, why, why_len);
        const int ang[3] = {1, 3, 4};
        for (int k = 0; k < 3; ++k)
            if (!(fabs(v[ang[k]]) <= 1e-6 || fabs(v[ang[k]] - 90.0) <= 1e-4)) {
                snprintf(why, why_len, "its cell is not orthorhombic (angle field %.9g): triclinic cells are not offered", v[ang[k]]);
                return true;
            }
        return ortho_edges_bad(edge, s.cut, cell, why, why_len);
    }
    if (s.kind == FrameSource::NETCDF) {
        /* three edge lengths and alpha, beta, gamma, big-endian doubles, the angles ALWAYS degrees (a 0 is not a right angle here) */
        double len[3], deg[3];
        freesasa_gpu_nc_cell_record(&s.nc, bytes, f, len, deg);
        if (s.tri) return freesasa_gpu_cell_from_lengths_angles(len, deg, cell, why, (int)why_len) || tri_cell_bad(cell, len, s.cut, why, why_len);
        for (int k = 0; k < 3; ++k)
            if (!(fabs(deg[k] - 90.0) <= 1e-4)) {
                snprintf(why, why_len, "its cell is not orthorhombic (angle %s is %.9g degrees): triclinic cells need bit 4", k == 0 ? "alpha" : k == 1 ? "beta" : "gamma", deg[k]);
                return true;
            }
        return ortho_edges_bad(len, s.cut, cell, why, why_len);
    }
    const long long at = off[f] - off[0];
    if (s.kind == FrameSource::XTC) { /* nine floats in nm */
        float bf[9];
        freesasa_gpu_xtc_frame_box(bytes + at, bf);
        for (int k = 0; k < 9; ++k) b[k] = (double)bf[k];
    } else { /* nine reals in nm; a frame without a box carries no cell */
        freesasa_gpu_trr_record r;
        if (freesasa_gpu_trr_frame_desc(bytes + at, off[f + 1] - off[f], 0, 0, at, &r, why, (int)why_len)) return true;
        if (r.box_off < 0) { snprintf(why, why_len, "it has no box: the frame carries no cell"); return true; }
        freesasa_gpu_trr_box(bytes + r.box_off, r.real_bytes, b);
    }
    return box_cell_bad(b, s.tri, s.cut, cell, why, why_len);
}

int FrameSource::read(freesasa_gpu_ctx *c, long long f0, int nf, size_t in_bytes, const void **src) const
{
    *src = mem ? mem + 3 * fa * (size_t)f0 : nullptr;
    if (*src && mem_pinned) return 0; /* the caller's array is page-locked: no staging */
    /* (an XTC shard: behind what goes up, the place its frames' status comes down to) */
    if (ensure_pinned(c, &c->stage_in, &c->stage_in_cap, up_bytes(in_bytes, (size_t)nf) + (kind == XTC ? 8 * (size_t)nf : 0))) return -1;
    char *stage = (char *)c->stage_in;
    if (*src) memcpy(stage, *src, in_bytes);
    else if (!pread_all(file.fd, stage, in_bytes, indexed() ? (long long)off[(size_t)f0] : first + (long long)stride * f0))
        return ctx_fail(c, "could not read frames %lld..%lld of the frame file", f0, f0 + nf - 1);
    *src = stage;
    const ShardLayout at = layout_of(*this, in_bytes, (size_t)nf);
    const int64_t *o = indexed() ? off.data() + f0 : nullptr;
    char why[200] = "a record marker is not what the header implies";
    const long long bad = kind == DCD ? dcd_damaged_frame(dcd, stage, nf)
                        : kind == XTC ? xtc_descriptors(o, stage, nf, (int)fa, (freesasa_gpu_xtc_frame *)(stage + at.extra), why, sizeof why)
                        : kind == TRR ? trr_descriptors(o, stage, nf, (int)fa, real_bytes, (int64_t *)(stage + at.extra), why, sizeof why) : -1;
    if (bad >= 0) return ctx_fail(c, "frame %lld of the %s file is damaged: %s", f0 + bad, con->name, why);
    /* periodic images: every cell decoded and checked, behind the bytes */
    for (long long f = 0; pbc && f < nf; ++f)
        if (frame_cell_bad(*this, o, stage, f, (double *)(stage + at.cells) + cell_doubles() * (size_t)f, why, sizeof why))
            return ctx_fail(c, "frame %lld of the %s file: %s", f0 + f, con->name, why);
    return 0;
}

/* ------------------------------------------------------------------ to frames (device) */

/* The decode of the XTC frames that lie on the device with their descriptors, for the driver's shards and for the test hook
   freesasa_gpu_xtc_decode_dev alike: scan, then unpack, on the context's stream, then the frames' (groups, status) pairs down
   to `status` (page-locked, 2 n_frames words); returns when they are there. */
static int xtc_decode(freesasa_gpu_ctx *c, const sasa::XtcArgs &xa, int32_t *status)
{
    if (kl_xtc_scan(xa, c->stream) != hipSuccess || kl_xtc_unpack(xa, c->stream) != hipSuccess) return ctx_fail(c, "XTC decode launch failed");
    if (hipMemcpyAsync(status, xa.count, 8 * (size_t)xa.n_frames, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return ctx_fail(c, "could not read the status of the XTC frames");
    return 0;
}
static sasa::XtcArgs xtc_args(char *g, const ShardLayout &at, int frame_atoms, int nf, void *frames)
{
    return {frame_atoms, nf, (const uint32_t *)g, (const freesasa_gpu_xtc_frame *)(g + at.extra), (sasa::XtcRec *)(g + at.rec), (int32_t *)(g + at.count), (float *)frames};
}

int FrameSource::to_frames(freesasa_gpu_ctx *c, const sasa::TrajArgs &ta, long long f0, int nf, size_t in_bytes, const void *src) const
{
    const ShardLayout at = layout_of(*this, in_bytes, (size_t)nf);
    const bool f32 = kind == RAW_F32 || kind == XTC;
    void *d_in = xyz_bytes() ? c->g_xyz.p : (f32 ? c->h_counts.p : c->h_xyz.p);
    char *const g = (char *)d_in;
    const int32_t *index = gather ? ta.index : nullptr;
    double *xyz = (double *)c->h_xyz.p;
    /* (periodic images: the shard's cells behind its bytes, in the same copy; an XTC or a TRR shard: its descriptors too) */
    const size_t up = up_bytes(in_bytes, (size_t)nf);
    if (hipMemcpyAsync(d_in, src, up, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ctx_fail(c, "host-to-device copy failed");
    /* a container's bytes as they lie in the file, made into compact fp64 frames (de-planarized, byte-swapped, widened,
       gathered) by one kernel */
    if (kind == DCD) {
        const sasa::TrajDcdArgs da = {(int)n, nf, index, dcd.frame_bytes, dcd.x_off, dcd.plane_bytes};
        return kl_traj_gather_dcd(da, d_in, dcd.big_endian != 0, xyz, c->stream) != hipSuccess ? ctx_fail(c, "DCD gather launch failed") : 0;
    }
    if (kind == NETCDF) {
        const sasa::TrajNcArgs na = {(int)n, nf, index, nc.record_bytes, nc.coord_off};
        return kl_traj_gather_nc(na, d_in, xyz, c->stream) != hipSuccess ? ctx_fail(c, "NetCDF gather launch failed") : 0;
    }
    if (kind == TRR) {
        const sasa::TrajTrrArgs ra = {(int)n, nf, index, (const int64_t *)(g + at.extra)};
        return kl_traj_gather_trr(ra, d_in, real_bytes == 8, xyz, c->stream) != hipSuccess ? ctx_fail(c, "TRR gather launch failed") : 0;
    }
    if (kind == XTC) {
        /* scan, then unpack: raw fp32 frames where the raw fp32 path has them - and the frames' status down BEFORE the engine sees
           them: what a damaged stream leaves of a frame is not a frame (one more synchronisation per shard; the other lanes' shards
           fill the device meanwhile) */
        int32_t *status = (int32_t *)((char *)c->stage_in + up);
        d_in = gather ? (void *)(g + at.f32) : c->h_counts.p;
        if (xtc_decode(c, xtc_args(g, at, (int)fa, nf, d_in), status)) return -1;
        for (int f = 0; f < nf; ++f)
            if (const int st = status[2 * f + 1])
                return ctx_fail(c, "frame %lld of the XTC file is damaged: %s", f0 + f,
                                st & sasa::XTC_ST_BITS ? "its stream ends before its atoms do" : st & sasa::XTC_ST_ATOMS ? "a group of its stream runs past its atoms"
                                : st & sasa::XTC_ST_SMALLIDX ? "smallidx leaves 9 .. 72 in its stream" : "its stream unpacks to a value outside its range");
    }
    /* full frames up as they were read: one kernel drops the solvent and widens fp32 */
    if (gather && kl_traj_gather(ta, d_in, f32, xyz, c->stream) != hipSuccess) return ctx_fail(c, "gather launch failed");
    if (!gather && f32 && kl_widen_f32((const float *)d_in, xyz, (long long)(3 * n * (size_t)nf), c->stream) != hipSuccess) return ctx_fail(c, "widening launch failed");
    return 0;
}

/* ------------------------------------------------------------------ test hook: the XTC decode on its own (include/freesasa_gpu.h) */

/* what freesasa_gpu_xtc_decode_dev refuses before it touches a device: host only */
extern "C" int freesasa_gpu_xtc_decode_check(const void *bytes, long long len, int n_frames, int n_atoms, const int32_t *rec, const int32_t *count,
                                             const float *out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!bytes || !rec || !count || !out) return set_err(err_out, err_len, "xtc_decode: null argument");
    if (n_frames < 1) return set_err(err_out, err_len, "xtc_decode: n_frames must be at least 1");
    if (n_atoms < 1) return set_err(err_out, err_len, "xtc_decode: n_atoms must be at least 1");
    if (len < 1) return set_err(err_out, err_len, "xtc_decode: len must be at least 1");
    if ((long long)n_frames * n_atoms > 0x7fffffffLL) return set_err(err_out, err_len, "xtc_decode: n_frames * n_atoms does not fit an int");
    return 0;
}

extern "C" int freesasa_gpu_xtc_decode_dev(freesasa_gpu_ctx *c, const void *bytes, long long len, int n_frames, int n_atoms, int32_t *rec,
                                           int32_t *count, float *out)
{
    if (!c) return -1;
    return guarded_ctx(c, [&]() -> int {
    c->err[0] = 0;
    if (freesasa_gpu_xtc_decode_check(bytes, len, n_frames, n_atoms, rec, count, out, c->err, (int)sizeof c->err)) return -1;
    if (freesasa_gpu_wait(c)) return -1; /* (batches submitted asynchronously come first, as for every synchronous entry) */
    /* an XTC shard without cells whose fp32 frames stay in c->g_xyz; in the staging its bytes, descriptors and status */
    const size_t nf = (size_t)n_frames, slots = nf * (size_t)n_atoms;
    const ShardLayout at = shard_layout((size_t)len, nf, (size_t)n_atoms, 0, true);
    if (ensure_pinned(c, &c->stage_in, &c->stage_in_cap, at.count + 8 * nf)) return -1;
    char *stage = (char *)c->stage_in;
    memcpy(stage, bytes, (size_t)len);
    memset(stage + len, 0, at.extra - (size_t)len);
    freesasa_gpu_xtc_frame *desc = (freesasa_gpu_xtc_frame *)(stage + at.extra);
    long long pos = 0;
    for (int f = 0; f < n_frames; ++f) {
        char why[200];
        long long frame_bytes = 0;
        if (freesasa_gpu_xtc_frame_desc(stage + pos, len - pos, n_atoms, pos + FREESASA_GPU_XTC_HEADER, &desc[f], &frame_bytes, why, (int)sizeof why))
            return ctx_fail(c, "frame %d of the XTC bytes: %s", f, why);
        pos += frame_bytes;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (ensure(c, c->g_xyz, at.end)) return -1;
    char *g = (char *)c->g_xyz.p;
    const sasa::XtcArgs xa = xtc_args(g, at, n_atoms, n_frames, g + at.f32);
    HIP_TRY(c, hipMemcpyAsync(g, stage, at.count, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(xa.count, 0xff, 8 * nf, c->stream));
    HIP_TRY(c, hipMemsetAsync(xa.rec, 0, sizeof(sasa::XtcRec) * slots, c->stream));
    HIP_TRY(c, hipMemsetAsync(xa.out, 0xff, 12 * slots, c->stream));
    int32_t *status = (int32_t *)(stage + at.count);
    int rc = xtc_decode(c, xa, status);
    if (!rc && (hipMemcpyAsync(rec, xa.rec, sizeof(sasa::XtcRec) * slots, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipMemcpyAsync(out, xa.out, 12 * slots, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
        rc = ctx_fail(c, "could not read the XTC records and frames back");
    /* (nothing is left running on the stream, whatever failed) */
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ctx_fail(c, "could not read the XTC records and frames back");
    if (rc) return -1;
    memcpy(count, status, 8 * nf);
    return 0;
    });
}
