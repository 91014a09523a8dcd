/*
 * dcd.c — the header of a DCD trajectory (CHARMM, NAMD, OpenMM, LAMMPS), read on the host for the trajectory file drivers
 * (include/freesasa_gpu.h, freesasa_gpu_dcd_info_read; gpu_frames.hip).  A DCD is uncompressed fp32 and every frame has
 * the same byte stride, so all the drivers need from it is WHERE a frame's x, y and z planes lie: the planes themselves go to
 * the device as they are in the file (traj_kernels.h, traj_gather_dcd).
 *
 * The file: Fortran records, each between two equal int32 byte counts, every integer in the file's byte order.
 *     1   [84 | "CORD" | icntrl[0..19] | 84]        0 NSET, 8 fixed atoms, 10 unit cell per frame, 11 4th dimension per
 *                                                   frame, 19 CHARMM version (0: X-PLOR, which has neither)
 *     2   [m | NTITLE | 80 NTITLE bytes | m]        m = 4 + 80 NTITLE
 *     3   [4 | NATOM | 4]
 *     per frame   [48 | 6 doubles | 48] with a unit cell, then [4N | N floats | 4N] for x, y, z and, with a 4th dimension,
 *                 once more.
 * The frame count is what the FILE SIZE holds (NSET is often 0 or stale: reported, never trusted); a tail that is not a whole
 * frame is ignored.  Plain C, no allocation.
 */
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/freesasa_gpu.h"

static int dcd_fail(int fd, char *err, int err_len, const char *msg)
{
    if (fd >= 0) close(fd);
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", msg);
    return -1;
}

static int dcd_read(int fd, void *buf, size_t bytes, long long off)
{
    char *p = (char *)buf;
    while (bytes) {
        const ssize_t r = pread(fd, p, bytes, (off_t)off);
        if (r <= 0) return -1;
        p += r; off += r; bytes -= (size_t)r;
    }
    return 0;
}

static uint32_t dcd_swap(uint32_t w) { return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24); }

/* word k of a little-endian host's view of the buffer, in the file's byte order */
static int32_t dcd_word(const unsigned char *p, int big)
{
    uint32_t w;
    memcpy(&w, p, 4);
    return (int32_t)(big ? dcd_swap(w) : w);
}

int freesasa_gpu_dcd_info_read(const char *path, freesasa_gpu_dcd_info *out, char *err, int err_len)
{
    static const char short_msg[] = "the file is shorter than the DCD header";
    unsigned char h[92], t[8], a[12];
    char msg[160];
    struct stat st;
    if (err && err_len > 0) err[0] = 0;
    if (!path || !out) return dcd_fail(-1, err, err_len, "null argument");
    memset(out, 0, sizeof *out);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return dcd_fail(-1, err, err_len, "cannot open the DCD file");
    if (fstat(fd, &st) != 0) return dcd_fail(fd, err, err_len, "cannot stat the DCD file");
    const long long size = (long long)st.st_size;
    if (size < 8 || dcd_read(fd, h, 8, 0)) return dcd_fail(fd, err, err_len, short_msg);
    const uint32_t w0 = (uint32_t)dcd_word(h, 0), w1 = (uint32_t)dcd_word(h + 4, 0);
    if ((w0 == 84u && w1 == 0u) || (w0 == 0u && w1 == 0x54000000u))
        return dcd_fail(fd, err, err_len, "64-bit record markers are not supported");
    if (w0 != 84u && w0 != 0x54000000u)
        return dcd_fail(fd, err, err_len, "not a DCD file: the first word is neither 84 nor 84 in the other byte order");
    const int big = w0 != 84u;
    if (memcmp(h + 4, "CORD", 4) != 0) return dcd_fail(fd, err, err_len, "not a DCD file: CORD is missing behind the first record marker");
    if (size < 92 || dcd_read(fd, h, 92, 0)) return dcd_fail(fd, err, err_len, short_msg);
    if (dcd_word(h + 88, big) != 84) return dcd_fail(fd, err, err_len, "the record markers of the DCD header's first record do not match");
    int32_t icntrl[20];
    for (int k = 0; k < 20; ++k) icntrl[k] = dcd_word(h + 8 + 4 * k, big);
    /* the title record */
    if (size < 100 || dcd_read(fd, t, 8, 92)) return dcd_fail(fd, err, err_len, short_msg);
    const long long m = dcd_word(t, big), ntitle = dcd_word(t + 4, big);
    if (ntitle < 0 || m != 4 + 80 * ntitle) return dcd_fail(fd, err, err_len, "the title record of the DCD header is damaged: its marker is not 4 + 80 NTITLE");
    if (size < 96 + m + 4 + 12 || dcd_read(fd, t, 4, 96 + m) || dcd_read(fd, a, 12, 100 + m)) return dcd_fail(fd, err, err_len, short_msg);
    if (dcd_word(t, big) != m) return dcd_fail(fd, err, err_len, "the record markers of the DCD header's title record do not match");
    if (dcd_word(a, big) != 4 || dcd_word(a + 8, big) != 4) return dcd_fail(fd, err, err_len, "the record markers of the DCD header's atom-count record do not match");
    close(fd);
    const long long natom = dcd_word(a + 4, big);
    if (icntrl[8] != 0) {
        snprintf(msg, sizeof msg, "DCD files with fixed atoms are not supported (the header names %d): from the second frame on they hold the free atoms only", icntrl[8]);
        return dcd_fail(-1, err, err_len, msg);
    }
    if (natom <= 0) {
        snprintf(msg, sizeof msg, "NATOM of the DCD header is %lld: it must be > 0", natom);
        return dcd_fail(-1, err, err_len, msg);
    }
    if (natom > (0x7fffffffLL - 8) / 4) return dcd_fail(-1, err, err_len, "NATOM of the DCD header is too large: a coordinate record must stay below 2^31 bytes");
    out->n_atoms = (int32_t)natom;
    out->n_frames_header = icntrl[0];
    out->big_endian = big;
    out->charmm_version = icntrl[19];
    out->has_cell = icntrl[19] != 0 && icntrl[10] != 0; /* (X-PLOR, version 0: neither record, whatever the words say) */
    out->has_4d = icntrl[19] != 0 && icntrl[11] != 0;
    out->first_frame = 112 + m;
    out->plane_bytes = (int32_t)(4 * natom + 8);
    out->x_off = 56 * out->has_cell + 4;
    out->frame_bytes = 56LL * out->has_cell + (3LL + out->has_4d) * out->plane_bytes;
    out->n_frames = (size - out->first_frame) / out->frame_bytes;
    if (out->n_frames <= 0) return dcd_fail(-1, err, err_len, "the DCD file holds no whole frame");
    return 0;
}
