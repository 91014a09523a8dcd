/*
 * netcdf.c — the header of an AMBER NetCDF trajectory (convention 1.0, `.nc` as sander / pmemd / cpptraj / OpenMM / MDAnalysis
 * write it), read on the host for the trajectory file drivers (include/freesasa_gpu.h, freesasa_gpu_nc_info_read;
 * gpu_frames.hip).  The file is NetCDF classic: uncompressed, big-endian, and every frame is one RECORD at a constant byte
 * stride, so all the drivers need from it is where a record's coordinates (and its cell) lie: the records themselves go to the
 * device as they are in the file (traj_kernels.h, traj_gather_nc).
 *
 * The file (every integer big-endian, 32 bits unless said otherwise):
 *     'C' 'D' 'F' version        1: classic, 2: 64-bit offset (a variable's begin is 8 bytes)
 *     numrecs                    0xFFFFFFFF: streaming
 *     dim_list gatt_list var_list    each ABSENT (two zero words) or [tag | nelems | elements]; tags 0x0A, 0x0C, 0x0B
 *     name   = length, the bytes, padded to 4
 *     dim    = name, length (0: the record dimension)
 *     attr   = name, nc_type, nelems, the values padded to 4
 *     var    = name, ndims, dimid[ndims], the variable's attribute list, nc_type, vsize, begin
 *     nc_type / bytes: BYTE 1/1, CHAR 2/1, SHORT 3/2, INT 4/4, FLOAT 5/4, DOUBLE 6/8
 * A record variable is one whose first dimension is the record dimension; a record is the record variables' vsize (each
 * padded to 4) one behind the other - with exactly ONE record variable its unpadded size - and record 0 begins at the smallest
 * begin among them: variable v of frame f lies at begin_v + f * record size.
 * The frame count is what the FILE SIZE holds (numrecs is stale after a crash and 0xFFFFFFFF while streaming: reported, never
 * trusted); a tail that is not a whole record is ignored.  Plain C, no allocation; the parser reads the first 64 KiB of the file
 * into a buffer of its own and no byte outside it, whatever the file holds.
 */
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/freesasa_gpu.h"

#define NC_HEADER_MAX 65536
#define NC_SIZE_MAX ((uint64_t)1 << 48)
enum { NC_DIMENSION = 0x0A, NC_VARIABLE = 0x0B, NC_ATTRIBUTE = 0x0C, NC_CHAR = 2, NC_FLOAT = 5, NC_DOUBLE = 6 };

/* the header as far as it was read, and the place the grammar has reached; `why` once something is wrong */
typedef struct {
    const unsigned char *p;
    size_t len, pos;
    long long file_size;
    const char *why;
} nc_cur;

static int nc_bad(nc_cur *c, const char *why)
{
    if (!c->why) c->why = why;
    return -1;
}
/* the header ends here and the grammar does not: the file is short, or its header is longer than what the parser reads */
static int nc_short(nc_cur *c)
{
    return nc_bad(c, c->file_size > (long long)c->len ? "the NetCDF header is longer than 64 KiB: AMBER trajectories' are below 2 KiB"
                                                      : "the NetCDF header ends before its grammar does: the file is truncated");
}
static int nc_u32(nc_cur *c, uint32_t *v)
{
    if (c->len - c->pos < 4) return nc_short(c);
    const unsigned char *q = c->p + c->pos;
    *v = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
    c->pos += 4;
    return 0;
}
/* what a count of the header asks for does not fit into what was read: it points outside the file (`outside`), or the header is
   longer than what the parser reads */
static int nc_beyond(nc_cur *c, uint64_t bytes, const char *outside)
{
    return bytes > (uint64_t)c->file_size - c->pos ? nc_bad(c, outside) : nc_short(c);
}
/* `bytes` bytes and their padding to 4, all within the buffer: their place */
static int nc_skip(nc_cur *c, uint64_t bytes, const char *outside, size_t *at)
{
    const uint64_t padded = (bytes + 3) & ~(uint64_t)3;
    if (padded > (uint64_t)(c->len - c->pos)) return nc_beyond(c, padded, outside);
    if (at) *at = c->pos;
    c->pos += (size_t)padded;
    return 0;
}
static int nc_name(nc_cur *c, size_t *at, uint32_t *n)
{
    if (nc_u32(c, n)) return -1;
    return nc_skip(c, *n, "a name length of the NetCDF header points outside the file", at);
}
static int nc_is(const nc_cur *c, size_t at, uint32_t n, const char *name) { return n == strlen(name) && memcmp(c->p + at, name, n) == 0; }

/* the head of a list: its tag or ABSENT; *nelems elements of at least `least` bytes each follow */
static int nc_list(nc_cur *c, uint32_t tag, uint32_t least, const char *wrong, const char *count, uint32_t *nelems)
{
    uint32_t t;
    if (nc_u32(c, &t) || nc_u32(c, nelems)) return -1;
    if (t == 0) return *nelems ? nc_bad(c, wrong) : 0;
    if (t != tag) return nc_bad(c, wrong);
    if (*nelems > (c->len - c->pos) / least) return nc_beyond(c, (uint64_t)*nelems * least, count);
    return 0;
}
static uint32_t nc_type_bytes(uint32_t t) { return t == 1 || t == 2 ? 1 : t == 3 ? 2 : t == 4 || t == 5 ? 4 : t == 6 ? 8 : 0; }

/* dimension k of the dimension list at `dims` (its head is behind it: the walk has been made once and fits) */
static void nc_dim(const nc_cur *c, size_t dims, uint32_t k, size_t *name_at, uint32_t *name_n, uint32_t *length)
{
    nc_cur w = *c;
    w.pos = dims;
    for (uint32_t d = 0; d <= k; ++d)
        if (nc_name(&w, name_at, name_n) || nc_u32(&w, length)) { *name_n = 0; *length = 0; return; }
}

/* one attribute list.  conventions: look for the CHAR attribute Conventions (1: AMBER among its tokens, 2: AMBERRESTART);
   scale: look for scale_factor (1: it is 1, 2: it is something else) */
static int nc_attrs(nc_cur *c, int *conventions, int *scale)
{
    uint32_t n;
    if (nc_list(c, NC_ATTRIBUTE, 12, "an attribute list of the NetCDF header does not begin with its tag", "an attribute count of the NetCDF header points outside the file", &n)) return -1;
    for (uint32_t k = 0; k < n; ++k) {
        size_t name, val;
        uint32_t len, type, nelems;
        if (nc_name(c, &name, &len) || nc_u32(c, &type) || nc_u32(c, &nelems)) return -1;
        const uint32_t esz = nc_type_bytes(type);
        if (!esz) return nc_bad(c, "an attribute of the NetCDF header has an unknown nc_type");
        if (nc_skip(c, (uint64_t)nelems * esz, "an attribute's value count of the NetCDF header points outside the file", &val)) return -1;
        if (conventions && type == NC_CHAR && nc_is(c, name, len, "Conventions")) {
            if (!*conventions) *conventions = -1; /* (present, AMBER not yet seen) */
            for (uint32_t b = 0; b < nelems;) {
                uint32_t e = b;
                while (e < nelems && c->p[val + e] != ',' && c->p[val + e] != ' ' && c->p[val + e] != 0) ++e;
                if (e - b == 5 && memcmp(c->p + val + b, "AMBER", 5) == 0 && *conventions != 2) *conventions = 1;
                if (e - b == 12 && memcmp(c->p + val + b, "AMBERRESTART", 12) == 0) *conventions = 2;
                b = e + 1;
            }
        }
        if (scale && nc_is(c, name, len, "scale_factor")) {
            *scale = 2;
            if (nelems == 1 && type == NC_FLOAT) {
                static const unsigned char one[4] = {0x3f, 0x80, 0, 0};
                if (memcmp(c->p + val, one, 4) == 0) *scale = 1;
            } else if (nelems == 1 && type == NC_DOUBLE) {
                static const unsigned char one[8] = {0x3f, 0xf0, 0, 0, 0, 0, 0, 0};
                if (memcmp(c->p + val, one, 8) == 0) *scale = 1;
            }
        }
    }
    return 0;
}

/* what the parser keeps of a variable it knows by name */
typedef struct {
    int seen, rec;
    uint32_t ndims, dimid[3], type;
    long long begin;
} nc_var;

static int nc_parse(nc_cur *c, freesasa_gpu_nc_info *out)
{
    if (c->len < 4) return nc_bad(c, "not a NetCDF file: it is shorter than 4 bytes");
    if (memcmp(c->p, "\x89HDF", 4) == 0)
        return nc_bad(c, "a NetCDF-4 (HDF5) file: only NetCDF classic is read - convert with `nccopy -k classic` or `cpptraj`");
    if (memcmp(c->p, "CDF", 3) != 0) return nc_bad(c, "not a NetCDF file: it does not begin with CDF");
    if (c->p[3] == 5) return nc_bad(c, "a CDF-5 (64-bit data) file: only NetCDF classic, versions 1 and 2, is read");
    if (c->p[3] != 1 && c->p[3] != 2) return nc_bad(c, "not a NetCDF classic file: the version byte behind CDF is neither 1 nor 2");
    out->version = c->p[3];
    c->pos = 4;
    uint32_t numrecs, n_dims, n_vars;
    if (nc_u32(c, &numrecs)) return -1;
    out->n_frames_header = numrecs == 0xFFFFFFFFu ? -1 : (long long)numrecs;

    if (nc_list(c, NC_DIMENSION, 8, "the dimension list of the NetCDF header does not begin with its tag", "the dimension count of the NetCDF header points outside the file", &n_dims)) return -1;
    const size_t dims = c->pos;
    long long recdim = -1;
    for (uint32_t d = 0; d < n_dims; ++d) {
        size_t at;
        uint32_t n, length;
        if (nc_name(c, &at, &n) || nc_u32(c, &length)) return -1;
        if (length == 0 && recdim < 0) recdim = d;
    }
    int conventions = 0;
    if (nc_attrs(c, &conventions, NULL)) return -1;

    if (nc_list(c, NC_VARIABLE, 20, "the variable list of the NetCDF header does not begin with its tag", "the variable count of the NetCDF header points outside the file", &n_vars)) return -1;
    nc_var coord = {0}, lengths = {0}, angles = {0}, tim = {0}, vel = {0};
    long long n_rec = 0, first = -1;
    uint64_t rec_sum = 0, rec_single = 0;
    int scale = 0, begin_outside = 0;
    for (uint32_t v = 0; v < n_vars; ++v) {
        size_t name;
        uint32_t len, ndims, type, vsize, b_hi = 0, b_lo;
        if (nc_name(c, &name, &len) || nc_u32(c, &ndims)) return -1;
        if (ndims > (c->len - c->pos) / 4) return nc_beyond(c, 4 * (uint64_t)ndims, "a variable's dimension count of the NetCDF header points outside the file");
        nc_var *known = nc_is(c, name, len, "coordinates") ? &coord : nc_is(c, name, len, "cell_lengths") ? &lengths : nc_is(c, name, len, "cell_angles") ? &angles
                      : nc_is(c, name, len, "time") ? &tim : nc_is(c, name, len, "velocities") ? &vel : NULL;
        if (known && known->seen) return nc_bad(c, "a variable of the NetCDF header occurs twice");
        int rec = 0;
        uint64_t unpadded = 1;
        for (uint32_t k = 0; k < ndims; ++k) {
            uint32_t id;
            if (nc_u32(c, &id)) return -1;
            if (id >= n_dims) return nc_bad(c, "a dimid of the NetCDF header points outside the dimension list");
            if (k == 0 && (long long)id == recdim) rec = 1;
            else if (rec) { /* (a record variable's size without its padding: the record size when it is the only one) */
                size_t at;
                uint32_t n, length;
                nc_dim(c, dims, id, &at, &n, &length);
                unpadded = length && unpadded > NC_SIZE_MAX / length ? NC_SIZE_MAX : unpadded * length; /* (saturates far above any file) */
            }
            if (known && k < 3) known->dimid[k] = id;
        }
        if (nc_attrs(c, NULL, known == &coord ? &scale : NULL) || nc_u32(c, &type) || nc_u32(c, &vsize)) return -1;
        if (!nc_type_bytes(type)) return nc_bad(c, "a variable of the NetCDF header has an unknown nc_type");
        if (out->version == 2 && nc_u32(c, &b_hi)) return -1;
        if (nc_u32(c, &b_lo)) return -1;
        const uint64_t begin = ((uint64_t)b_hi << 32) | b_lo;
        if (begin > (uint64_t)c->file_size) { begin_outside = 1; continue; } /* (said once the grammar has ended: a cut header is a cut header) */
        if (rec) {
            ++n_rec;
            rec_sum += vsize;
            rec_single = unpadded * nc_type_bytes(type);
            if (first < 0 || (long long)begin < first) first = (long long)begin;
        }
        if (known) { known->seen = 1; known->rec = rec; known->ndims = ndims; known->type = type; known->begin = (long long)begin; }
    }
    if (begin_outside) return nc_bad(c, "a variable's begin of the NetCDF header points outside the file");
    if (first >= 0 && (long long)c->pos > first) return nc_bad(c, "a record variable's begin of the NetCDF header points into the header");

    if (!conventions) return nc_bad(c, "the NetCDF file has no global attribute Conventions (text): not an AMBER trajectory");
    if (conventions == 2) return nc_bad(c, "the NetCDF file's Conventions name AMBERRESTART: a restart file, not a trajectory");
    if (conventions != 1) return nc_bad(c, "the NetCDF file's Conventions do not name AMBER: not an AMBER trajectory");
    if (!coord.seen) return nc_bad(c, "the NetCDF file has no variable `coordinates`");
    size_t at = 0;
    uint32_t n = 0, atoms = 0, three = 0;
    if (coord.ndims == 3) { nc_dim(c, dims, coord.dimid[2], &at, &n, &three); nc_dim(c, dims, coord.dimid[1], &at, &n, &atoms); }
    if (coord.type != NC_FLOAT || coord.ndims != 3 || !coord.rec || !nc_is(c, at, n, "atom") || three != 3)
        return nc_bad(c, "the variable `coordinates` of the NetCDF file is not NC_FLOAT over (the record dimension, atom, a dimension of length 3)");
    if (scale == 2) return nc_bad(c, "the variable `coordinates` of the NetCDF file has a scale_factor other than 1: not offered");
    if (atoms == 0) return nc_bad(c, "the dimension `atom` of the NetCDF file is 0: it must be > 0");
    if (atoms > 0x7fffffffu / 12) return nc_bad(c, "the dimension `atom` of the NetCDF file is too large: a frame's coordinates must stay below 2^31 bytes");
    nc_var *const cellv[2] = {&lengths, &angles};
    for (int k = 0; k < 2; ++k) {
        if (!cellv[k]->seen) continue;
        three = 0;
        if (cellv[k]->ndims == 2) nc_dim(c, dims, cellv[k]->dimid[1], &at, &n, &three);
        if (cellv[k]->type != NC_DOUBLE || cellv[k]->ndims != 2 || !cellv[k]->rec || three != 3)
            return nc_bad(c, k ? "the variable `cell_angles` of the NetCDF file is not NC_DOUBLE over (the record dimension, a dimension of length 3)"
                               : "the variable `cell_lengths` of the NetCDF file is not NC_DOUBLE over (the record dimension, a dimension of length 3)");
    }
    const uint64_t record = n_rec == 1 ? rec_single : rec_sum;
    out->n_atoms = (int32_t)atoms;
    out->has_cell = lengths.seen && angles.seen;
    out->has_time = tim.seen && tim.rec;
    out->has_velocities = vel.seen && vel.rec;
    out->first_record = first;
    out->record_bytes = (long long)record;
    out->coord_off = coord.begin - first;
    out->lengths_off = out->has_cell ? lengths.begin - first : -1;
    out->angles_off = out->has_cell ? angles.begin - first : -1;
    /* what the drivers and the kernel rely on: 32-bit words, and every variable they read inside its record */
    if (record == 0 || record > NC_SIZE_MAX) return nc_bad(c, "the record size the NetCDF header implies is 0 or beyond 2^48 bytes");
    if ((record & 3) || (out->coord_off & 3) || (out->has_cell && ((out->lengths_off | out->angles_off) & 3)))
        return nc_bad(c, "the record size or a variable's begin of the NetCDF header is not a multiple of 4 bytes");
    if ((uint64_t)out->coord_off + 12ull * atoms > record || (out->has_cell && ((uint64_t)out->lengths_off + 24 > record || (uint64_t)out->angles_off + 24 > record)))
        return nc_bad(c, "a variable of the NetCDF file does not lie within one record: a vsize or a begin of the header is damaged");
    out->n_frames = (c->file_size - first) / (long long)record;
    if (out->n_frames <= 0) return nc_bad(c, "the NetCDF file holds no whole record");
    return 0;
}

int freesasa_gpu_nc_info_read(const char *path, freesasa_gpu_nc_info *out, char *err, int err_len)
{
    unsigned char buf[NC_HEADER_MAX];
    struct stat st;
    nc_cur c;
    memset(&c, 0, sizeof c);
    if (err && err_len > 0) err[0] = 0;
    if (!path || !out) c.why = "null argument";
    else {
        memset(out, 0, sizeof *out);
        const int fd = open(path, O_RDONLY);
        if (fd < 0) c.why = "cannot open the NetCDF file";
        else if (fstat(fd, &st) != 0) c.why = "cannot stat the NetCDF file";
        else {
            c.file_size = (long long)st.st_size;
            const size_t want = c.file_size < NC_HEADER_MAX ? (size_t)c.file_size : NC_HEADER_MAX;
            while (c.len < want) {
                const ssize_t r = pread(fd, buf + c.len, want - c.len, (off_t)c.len);
                if (r <= 0) break;
                c.len += (size_t)r;
            }
            if (c.len < want) c.why = "cannot read the NetCDF file";
        }
        if (fd >= 0) close(fd);
    }
    c.p = buf;
    if (!c.why && nc_parse(&c, out) == 0) return 0;
    if (out) memset(out, 0, sizeof *out);
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", c.why ? c.why : "the NetCDF header is damaged");
    return -1;
}

void freesasa_gpu_nc_cell_record(const freesasa_gpu_nc_info *info, const void *records, long long f, double lengths_out[3], double angles_out[3])
{
    const unsigned char *rec = (const unsigned char *)records + f * info->record_bytes;
    for (int k = 0; k < 6; ++k) {
        const unsigned char *q = rec + (k < 3 ? info->lengths_off + 8 * k : info->angles_off + 8 * (k - 3));
        unsigned char b[8];
        memcpy(b, q, 8);
        uint64_t w = 0;
        for (int j = 0; j < 8; ++j) w = (w << 8) | b[j];
        memcpy(k < 3 ? &lengths_out[k] : &angles_out[k - 3], &w, 8);
    }
}
