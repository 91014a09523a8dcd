/* TESTS ONLY: xtc_scan and xtc_unpack (freesasa_amd/csrc/xtc_kernels.h) driven on the CPU in the launch shapes of kl_xtc_scan and
 * kl_xtc_unpack (gpu_kernels.hip): per frame a workgroup of XTC_SCAN_B lanes that stage a window of the stream, then lane 0 walks
 * it, until the walk is done; then workgroups of XTC_UNPACK_B threads over n_frames * n_atoms slots.  The descriptors come from
 * the frames' headers through freesasa_gpu_xtc_frame_desc (xtc.c), as the driver makes them.  With -DXTC_EMU_MAIN a stand-alone
 * program (tests/emu/xtc_emu_check, built with AddressSanitizer + UBSan): every frame of the files of argv, one line per frame
 *     frame <k> status <s> groups <g> records <fnv1a of the group records> xyz <fnv1a of the frame's fp32 output>
 * or "refused <message>" for a header the host refuses.  Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../freesasa_amd/csrc/xtc_kernels.h"

using namespace sasa;

/* `bytes`: n_frames whole frames one behind the other, in a buffer of EXACTLY len bytes (4-byte aligned).  rec [n_frames * n_atoms * 4],
   count [n_frames * 2], out [n_frames * n_atoms * 3].  Returns 0, or -1 - k for a header of frame k the host refuses (why). */
extern "C" int emu_xtc_shard(const void *bytes, long long len, int n_frames, int n_atoms, int32_t *rec, int32_t *count, float *out, char *why, int why_len)
{
    if (!bytes || ((uintptr_t)bytes & 3) || n_frames < 1 || n_atoms < 1) return -1000000;
    std::vector<freesasa_gpu_xtc_frame> desc((size_t)n_frames);
    long long at = 0;
    for (int f = 0; f < n_frames; ++f) {
        long long frame_bytes = 0;
        if (freesasa_gpu_xtc_frame_desc((const char *)bytes + at, len - at, n_atoms, at + FREESASA_GPU_XTC_HEADER, &desc[(size_t)f], &frame_bytes, why, why_len)) return -1 - f;
        at += frame_bytes;
    }
    const XtcArgs a = {n_atoms, n_frames, (const uint32_t *)bytes, desc.data(), (XtcRec *)rec, count, out};
    for (int f = 0; f < n_frames; ++f) {
        uint32_t win[XTC_WIN + 1];
        memset(win, 0xee, sizeof win); /* (what a window does not load is not the stream's) */
        XtcScanState st;
        xtc_scan_init(a, f, st);
        win[XTC_WIN] = 0;
        for (int rounds = 0; !st.done; ++rounds) {
            if (rounds > (1 << 22)) return -2000000; /* (the window moves on every round) */
            for (int lane = 0; lane < XTC_SCAN_B; ++lane) xtc_scan_stage(a, f, st, win, lane);
            xtc_scan_walk(a, f, st, win);
        }
    }
    const int64_t blocks = ((int64_t)n_frames * n_atoms + XTC_UNPACK_B - 1) / XTC_UNPACK_B;
    for (int64_t blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < XTC_UNPACK_B; ++t) xtc_unpack(a, blk * XTC_UNPACK_B + t);
    return 0;
}

#ifdef XTC_EMU_MAIN
static unsigned long long fnv1a(const void *p, size_t bytes)
{
    unsigned long long h = 1469598103934665603ULL;
    for (size_t q = 0; q < bytes; ++q) h = (h ^ ((const unsigned char *)p)[q]) * 1099511628211ULL;
    return h;
}

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; ++k) {
        freesasa_gpu_xtc_info info;
        int64_t *offs = NULL;
        char err[300];
        if (freesasa_gpu_xtc_index_read(argv[k], &info, &offs, err, (int)sizeof err)) {
            printf("refused %s\n", err);
            continue;
        }
        /* frame by frame, each in a buffer of exactly its size: a read past a frame's bytes is a sanitizer report */
        FILE *fp = fopen(argv[k], "rb");
        const size_t n = (size_t)info.n_atoms;
        std::vector<int32_t> rec(4 * n), count(2);
        std::vector<float> out(3 * n);
        for (long long f = 0; fp && f < info.n_frames; ++f) {
            const size_t bytes = (size_t)(offs[f + 1] - offs[f]);
            uint32_t *buf = (uint32_t *)malloc(bytes);
            if (!buf || fseek(fp, (long)offs[f], SEEK_SET) != 0 || fread(buf, 1, bytes, fp) != bytes) { printf("frame %lld unread\n", f); free(buf); continue; }
            memset(rec.data(), 0, 16 * n);
            memset(out.data(), 0xff, 12 * n);
            count[0] = count[1] = -1;
            const int rc = emu_xtc_shard(buf, (long long)bytes, 1, info.n_atoms, rec.data(), count.data(), out.data(), err, (int)sizeof err);
            if (rc) printf("frame %lld refused %s\n", f, err);
            else printf("frame %lld status %d groups %d records %016llx xyz %016llx\n", f, count[1], count[0],
                        fnv1a(rec.data(), 16 * (size_t)(count[0] > 0 ? count[0] : 0)), fnv1a(out.data(), 12 * n));
            free(buf);
        }
        if (fp) fclose(fp);
        freesasa_gpu_xtc_index_free(offs);
    }
    return 0;
}
#endif
