/*
 * xtc.c — the frames of a GROMACS XTC trajectory, found and checked on the host for the trajectory file drivers
 * (include/freesasa_gpu.h, freesasa_gpu_xtc_info_read, freesasa_gpu_xtc_index_read, freesasa_gpu_xtc_frame_desc;
 * gpu_frames.hip).  An XTC frame is COMPRESSED: a 92-byte header and one bit stream of packed integers whose length the
 * header names, so frames have no common stride.  The host does what needs no bit of the stream: ONE pass over the headers
 * gives the byte offset of every frame (the index, by which shards are cut) and checks every header; per frame of a shard a
 * descriptor of 64 bytes says where the stream lies and how its integers are packed.  The streams go to the device as they
 * are in the file and are decoded there (xtc_kernels.h).
 *
 * A frame, every value XDR (big-endian, 4 bytes):
 *     int magic = 1995 | int natoms | int step | float time | float box[3][3] (nm, row-major) | int natoms | float precision |
 *     int minint[3] | int maxint[3] | int smallidx | int bytecount | bytecount bytes, padded to a multiple of 4
 * The stream starts 92 bytes into the frame; the next frame follows the padding.  Magic 2023 (64-bit bytecount) and frames of
 * 9 atoms or fewer (uncompressed floats) are refused.  Plain C; the index pass does one read of 92 bytes per frame and
 * allocates nothing but the array of offsets.
 */
#include <fcntl.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/freesasa_gpu.h"

static int xtc_fail(int fd, char *err, int err_len, const char *msg)
{
    if (fd >= 0) close(fd);
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", msg);
    return -1;
}

static int xtc_read(int fd, void *buf, size_t bytes, long long off)
{
    char *p = (char *)buf;
    while (bytes) {
        const ssize_t r = pread(fd, p, bytes, (off_t)off);
        if (r <= 0) return -1;
        p += r; off += r; bytes -= (size_t)r;
    }
    return 0;
}

static int32_t xtc_int(const unsigned char *p) { return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]); }
static float xtc_float(const unsigned char *p)
{
    const uint32_t w = (uint32_t)xtc_int(p);
    float v;
    memcpy(&v, &w, 4);
    return v;
}

/* the smallest b <= 32 with 2^b > s */
static int xtc_sizeofint(uint32_t s)
{
    int b = 0;
    while (b < 32 && (1ULL << b) <= s) ++b;
    return b;
}

int freesasa_gpu_xtc_frame_desc(const void *header, long long avail, int n_atoms, long long stream_off, freesasa_gpu_xtc_frame *out,
                                long long *frame_bytes_out, char *why, int why_len)
{
    const unsigned char *h = (const unsigned char *)header;
#define XTC_WHY(...) do { if (why && why_len > 0) snprintf(why, (size_t)why_len, __VA_ARGS__); return -1; } while (0)
    if (avail < 8) XTC_WHY("the file ends inside its header");
    const int32_t magic = xtc_int(h), natoms = xtc_int(h + 4);
    if (magic == 2023) XTC_WHY("its magic number is 2023: the XTC variant with 64-bit byte counts (very large systems) is not offered");
    if (magic != 1995) XTC_WHY("its magic number is %d, not 1995: not an XTC frame", (int)magic);
    if (natoms <= 9) XTC_WHY("it holds %d atoms: frames of 9 atoms or fewer are uncompressed floats, which are not offered", (int)natoms);
    if (avail < FREESASA_GPU_XTC_HEADER) XTC_WHY("the file ends inside its header");
    const int32_t natoms2 = xtc_int(h + 52);
    if (natoms2 != natoms) XTC_WHY("its two atom counts differ: %d and %d", (int)natoms, (int)natoms2);
    if (n_atoms > 0 && natoms != n_atoms) XTC_WHY("it holds %d atoms, frame 0 holds %d", (int)natoms, n_atoms);
    const float precision = xtc_float(h + 56);
    if (!isfinite(precision) || !(precision > 0)) XTC_WHY("its precision is %.9g: it must be finite and > 0", (double)precision);
    freesasa_gpu_xtc_frame d;
    memset(&d, 0, sizeof d);
    for (int k = 0; k < 3; ++k) {
        const int32_t lo = xtc_int(h + 60 + 4 * k), hi = xtc_int(h + 72 + 4 * k);
        if (lo > hi) XTC_WHY("minint %d exceeds maxint %d in dimension %c", (int)lo, (int)hi, "xyz"[k]);
        const long long size = (long long)hi - lo + 1;
        if (size > 0xffffffffLL) XTC_WHY("dimension %c spans all 2^32 integers", "xyz"[k]);
        d.minint[k] = lo;
        d.sizeint[k] = (uint32_t)size;
    }
    const int32_t smallidx = xtc_int(h + 84), bytecount = xtc_int(h + 88);
    if (smallidx < 9 || smallidx > 72) XTC_WHY("its smallidx is %d, outside 9 .. 72", (int)smallidx);
    if (bytecount < 0) XTC_WHY("its byte count is %d: negative", (int)bytecount);
    if (bytecount >= (1 << 28)) XTC_WHY("its byte count is %d: streams of 2^28 bytes and more are not offered", (int)bytecount);
    const long long frame_bytes = FREESASA_GPU_XTC_HEADER + (((long long)bytecount + 3) & ~3LL);
    if (frame_bytes > avail) XTC_WHY("its byte count %d runs past the end of the file", (int)bytecount);
    if ((d.sizeint[0] | d.sizeint[1] | d.sizeint[2]) > 0xffffffu) {
        d.bitsize = 0;
        for (int k = 0; k < 3; ++k) d.bitsizeint[k] = xtc_sizeofint(d.sizeint[k]);
    } else {
        /* the bit length of the product of the three sizes (< 2^72) */
        unsigned __int128 p = (unsigned __int128)d.sizeint[0] * d.sizeint[1] * d.sizeint[2];
        int b = 0;
        while (p) { ++b; p >>= 1; }
        d.bitsize = b;
    }
    d.stream_off = stream_off;
    d.bytecount = bytecount;
    d.smallidx = smallidx;
    d.inv_precision = (float)(1.0 / (double)precision);
    if (out) *out = d;
    if (frame_bytes_out) *frame_bytes_out = frame_bytes;
    return 0;
#undef XTC_WHY
}

void freesasa_gpu_xtc_frame_box(const void *header, float box_out[9])
{
    for (int k = 0; k < 9; ++k) box_out[k] = xtc_float((const unsigned char *)header + 16 + 4 * k);
}

void freesasa_gpu_xtc_index_free(int64_t *offsets) { free(offsets); }

int freesasa_gpu_xtc_index_read(const char *path, freesasa_gpu_xtc_info *out, int64_t **offsets_out, char *err, int err_len)
{
    unsigned char h[FREESASA_GPU_XTC_HEADER];
    char why[200], msg[280];
    struct stat st;
    if (err && err_len > 0) err[0] = 0;
    if (offsets_out) *offsets_out = NULL;
    if (!path || !out) return xtc_fail(-1, err, err_len, "null argument");
    memset(out, 0, sizeof *out);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return xtc_fail(-1, err, err_len, "cannot open the XTC file");
    if (fstat(fd, &st) != 0) return xtc_fail(fd, err, err_len, "cannot stat the XTC file");
    const long long size = (long long)st.st_size;
    if (size == 0) return xtc_fail(fd, err, err_len, "the XTC file holds no frame");
    int64_t *offs = NULL;
    long long cap = 0, nf = 0, at = 0, max_bytes = 0;
    while (at < size) {
        const long long avail = size - at, want = avail < FREESASA_GPU_XTC_HEADER ? avail : FREESASA_GPU_XTC_HEADER;
        long long frame_bytes = 0;
        freesasa_gpu_xtc_frame d;
        memset(h, 0, sizeof h);
        if (xtc_read(fd, h, (size_t)want, at)) { free(offs); return xtc_fail(fd, err, err_len, "cannot read the XTC file"); }
        if (freesasa_gpu_xtc_frame_desc(h, avail, nf ? out->n_atoms : 0, FREESASA_GPU_XTC_HEADER, &d, &frame_bytes, why, (int)sizeof why)) {
            snprintf(msg, sizeof msg, "frame %lld of the XTC file: %s", nf, why);
            free(offs);
            return xtc_fail(fd, err, err_len, msg);
        }
        if (nf == 0) {
            out->n_atoms = xtc_int(h + 4);
            out->precision = xtc_float(h + 56);
            for (int k = 0; k < 9; ++k) out->has_box |= xtc_float(h + 16 + 4 * k) != 0.0f;
        }
        if (offsets_out) {
            if (nf + 2 > cap) {
                cap = cap ? 2 * cap : 1024;
                int64_t *grown = (int64_t *)realloc(offs, sizeof(int64_t) * (size_t)cap);
                if (!grown) { free(offs); return xtc_fail(fd, err, err_len, "out of memory for the XTC frame index"); }
                offs = grown;
            }
            offs[nf] = at;
        }
        if (frame_bytes > max_bytes) max_bytes = frame_bytes;
        at += frame_bytes;
        ++nf;
    }
    close(fd);
    if (offsets_out) { offs[nf] = at; *offsets_out = offs; }
    out->n_frames = nf;
    out->max_frame_bytes = max_bytes;
    return 0;
}

int freesasa_gpu_xtc_info_read(const char *path, freesasa_gpu_xtc_info *out, char *err, int err_len)
{
    return freesasa_gpu_xtc_index_read(path, out, NULL, err, err_len);
}
