/*
 * trr.c — the records of a GROMACS TRR trajectory, found and checked on the host for the trajectory file drivers
 * (include/freesasa_gpu.h, freesasa_gpu_trr_info_read, freesasa_gpu_trr_index_read, freesasa_gpu_trr_frame_desc;
 * gpu_frames.hip).  A TRR record is UNCOMPRESSED, in single or double precision, and holds whichever of box, virial,
 * pressure, coordinates, velocities and forces its writer chose for that step (nstxout, nstvout, nstfout): records have no
 * common stride and need not hold coordinates at all.  The host does what the header says: ONE pass over the headers gives the
 * byte offset of every record WITH coordinates (the index, by which shards are cut - the records without lie between them and
 * go up unread) and checks every header; per frame of a shard a descriptor says where x[0] and the box lie.  The bytes go to
 * the device as they are in the file (traj_kernels.h, traj_gather_trr).
 *
 * A record, every value XDR (big-endian, 4-byte units):
 *     int magic = 1993 | int 13 | int 12 | 12 bytes "GMX_trn_file" |
 *     int ir_size, e_size, box_size, vir_size, pres_size, top_size, sym_size, x_size, v_size, f_size, natoms, step, nre |
 *     real t | real lambda | box[9] | vir[9] | pres[9] | x[3 natoms] | v[3 natoms] | f[3 natoms]
 * each part of the body present only when its size is not 0.  real is 4 or 8 bytes for the whole record: box_size / 9 when
 * box_size != 0, else the first non-zero of x_size, v_size, f_size divided by 3 natoms.  The header is 84 bytes in single
 * and 92 in double precision.  Plain C; the index pass does one read of at most 92 bytes per record (and one of frame 0's
 * box) and allocates nothing but the array of offsets.
 */
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/freesasa_gpu.h"

static int trr_fail(int fd, char *err, int err_len, const char *msg)
{
    if (fd >= 0) close(fd);
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", msg);
    return -1;
}

static int trr_read(int fd, void *buf, size_t bytes, long long off)
{
    char *p = (char *)buf;
    while (bytes) {
        const ssize_t r = pread(fd, p, bytes, (off_t)off);
        if (r <= 0) return -1;
        p += r; off += r; bytes -= (size_t)r;
    }
    return 0;
}

static uint32_t trr_word(const unsigned char *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
static int32_t trr_int(const unsigned char *p) { return (int32_t)trr_word(p); }

int freesasa_gpu_trr_frame_desc(const void *header, long long avail, int n_atoms, int real_bytes, long long base,
                                freesasa_gpu_trr_record *out, char *why, int why_len)
{
    const unsigned char *h = (const unsigned char *)header;
    static const char *const size_name[13] = {"ir_size", "e_size", "box_size", "vir_size", "pres_size", "top_size", "sym_size",
                                              "x_size", "v_size", "f_size", "natoms", "step", "nre"};
#define TRR_WHY(...) do { if (why && why_len > 0) snprintf(why, (size_t)why_len, __VA_ARGS__); return -1; } while (0)
    if (avail < 4) TRR_WHY("the file ends inside its header");
    const int32_t magic = trr_int(h);
    if (magic != 1993) TRR_WHY("its magic number is %d, not 1993: not a TRR record", (int)magic);
    if (avail < 24) TRR_WHY("the file ends inside its header");
    if (trr_int(h + 4) != 13 || trr_int(h + 8) != 12 || memcmp(h + 12, "GMX_trn_file", 12) != 0)
        TRR_WHY("its version string is not 13, 12, \"GMX_trn_file\"");
    if (avail < FREESASA_GPU_TRR_HEADER_MIN) TRR_WHY("the file ends inside its header");
    long long w[13]; /* the 13 integers, in the header's order */
    for (int k = 0; k < 13; ++k) w[k] = trr_int(h + 24 + 4 * k);
    const int unused[4] = {0, 1, 5, 6};
    for (int k = 0; k < 4; ++k)
        if (w[unused[k]] != 0) TRR_WHY("its %s is %lld: records with such a part are not offered", size_name[unused[k]], w[unused[k]]);
    const long long natoms = w[10];
    if (natoms <= 0) TRR_WHY("it holds %lld atoms", natoms);
    /* the width of a real: from the box, else from the first of x, v, f that is there (integer division: what does not divide
       fails the check of the sizes below) */
    const long long width = w[2] != 0 ? w[2] / 9 : w[7] != 0 ? w[7] / (3 * natoms) : w[8] != 0 ? w[8] / (3 * natoms) : w[9] / (3 * natoms);
    if (width != 4 && width != 8) TRR_WHY("its reals are %lld bytes wide: neither 4 (single) nor 8 (double precision)", width);
    const int of9[3] = {2, 3, 4}, of3n[3] = {7, 8, 9};
    for (int k = 0; k < 3; ++k)
        if (w[of9[k]] != 0 && w[of9[k]] != 9 * width) TRR_WHY("its %s is %lld, not 9 reals of %lld bytes", size_name[of9[k]], w[of9[k]], width);
    for (int k = 0; k < 3; ++k)
        if (w[of3n[k]] != 0 && w[of3n[k]] != 3 * natoms * width)
            TRR_WHY("its %s is %lld, not 3 x %lld atoms x %lld bytes", size_name[of3n[k]], w[of3n[k]], natoms, width);
    if (n_atoms > 0 && natoms != n_atoms) TRR_WHY("it holds %lld atoms, record 0 holds %d", natoms, n_atoms);
    if (real_bytes > 0 && width != real_bytes) TRR_WHY("its reals are %lld bytes wide, record 0's are %d: files that mix precisions are not offered", width, real_bytes);
    const long long header_bytes = FREESASA_GPU_TRR_HEADER_MIN + 2 * width;
    if (avail < header_bytes) TRR_WHY("the file ends inside its header");
    const long long record_bytes = header_bytes + w[2] + w[3] + w[4] + w[7] + w[8] + w[9];
    if (record_bytes > avail) TRR_WHY("the file ends inside its body: the record is %lld bytes long, %lld are left", record_bytes, avail);
    if (out) {
        memset(out, 0, sizeof *out);
        out->n_atoms = (int32_t)natoms;
        out->real_bytes = (int32_t)width;
        out->has_box = w[2] != 0; out->has_x = w[7] != 0; out->has_v = w[8] != 0; out->has_f = w[9] != 0;
        out->record_bytes = record_bytes;
        out->box_off = w[2] ? base + header_bytes : -1;
        out->x_off = w[7] ? base + header_bytes + w[2] + w[3] + w[4] : -1;
    }
    return 0;
#undef TRR_WHY
}

void freesasa_gpu_trr_box(const void *box, int real_bytes, double box_out[9])
{
    const unsigned char *p = (const unsigned char *)box;
    for (int k = 0; k < 9; ++k) {
        if (real_bytes == 8) {
            const uint64_t u = ((uint64_t)trr_word(p + 8 * k) << 32) | trr_word(p + 8 * k + 4);
            memcpy(&box_out[k], &u, 8);
        } else {
            const uint32_t u = trr_word(p + 4 * k);
            float v;
            memcpy(&v, &u, 4);
            box_out[k] = (double)v;
        }
    }
}

void freesasa_gpu_trr_index_free(int64_t *offsets) { free(offsets); }

int freesasa_gpu_trr_index_read(const char *path, freesasa_gpu_trr_info *out, int64_t **offsets_out, char *err, int err_len)
{
    unsigned char h[FREESASA_GPU_TRR_HEADER_MIN + 16];
    char why[200], msg[280];
    struct stat st;
    if (err && err_len > 0) err[0] = 0;
    if (offsets_out) *offsets_out = NULL;
    if (!path || !out) return trr_fail(-1, err, err_len, "null argument");
    memset(out, 0, sizeof *out);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return trr_fail(-1, err, err_len, "cannot open the TRR file");
    if (fstat(fd, &st) != 0) return trr_fail(fd, err, err_len, "cannot stat the TRR file");
    const long long size = (long long)st.st_size;
    int64_t *offs = NULL;
    long long cap = 0, nf = 0, nrec = 0, at = 0, max_bytes = 0, last = 0;
    while (at < size) {
        const long long avail = size - at, want = avail < (long long)sizeof h ? avail : (long long)sizeof h;
        freesasa_gpu_trr_record r;
        memset(h, 0, sizeof h);
        if (trr_read(fd, h, (size_t)want, at)) { free(offs); return trr_fail(fd, err, err_len, "cannot read the TRR file"); }
        if (freesasa_gpu_trr_frame_desc(h, avail, nrec ? out->n_atoms : 0, nrec ? out->real_bytes : 0, at, &r, why, (int)sizeof why)) {
            snprintf(msg, sizeof msg, "record %lld of the TRR file: %s", nrec, why);
            free(offs);
            return trr_fail(fd, err, err_len, msg);
        }
        if (nrec == 0) { out->n_atoms = r.n_atoms; out->real_bytes = r.real_bytes; }
        out->has_velocities |= r.has_v;
        out->has_forces |= r.has_f;
        if (r.has_x) {
            if (nf == 0 && r.has_box) { /* does the first coordinate frame's box hold anything? */
                unsigned char raw[72];
                double box[9];
                if (trr_read(fd, raw, (size_t)(9 * r.real_bytes), r.box_off)) { free(offs); return trr_fail(fd, err, err_len, "cannot read the TRR file"); }
                freesasa_gpu_trr_box(raw, r.real_bytes, box);
                for (int k = 0; k < 9; ++k) out->has_box |= box[k] != 0.0;
            }
            if (nf && at - last > max_bytes) max_bytes = at - last;
            last = at;
            if (offsets_out) {
                if (nf + 2 > cap) {
                    cap = cap ? 2 * cap : 1024;
                    int64_t *grown = (int64_t *)realloc(offs, sizeof(int64_t) * (size_t)cap);
                    if (!grown) { free(offs); return trr_fail(fd, err, err_len, "out of memory for the TRR frame index"); }
                    offs = grown;
                }
                offs[nf] = at;
            }
            ++nf;
        }
        at += r.record_bytes;
        ++nrec;
    }
    if (nf == 0) {
        snprintf(msg, sizeof msg, "the TRR file holds no coordinate frame: none of its %lld records has coordinates", nrec);
        free(offs);
        return trr_fail(fd, err, err_len, msg);
    }
    close(fd);
    if (at - last > max_bytes) max_bytes = at - last;
    if (offsets_out) { offs[nf] = at; *offsets_out = offs; }
    out->n_frames = nf;
    out->n_records = nrec;
    out->max_frame_bytes = max_bytes;
    return 0;
}

int freesasa_gpu_trr_info_read(const char *path, freesasa_gpu_trr_info *out, char *err, int err_len)
{
    return freesasa_gpu_trr_index_read(path, out, NULL, err, err_len);
}
