/* TESTS ONLY: the TRR header walker (freesasa_amd/csrc/trr.c) in a stand-alone program, built with AddressSanitizer + UBSan
 * (Makefile, tests/emu/trr_check).  One line per path of argv:
 *     ok <n_atoms> <n_frames> <n_records> <real_bytes> <max_frame_bytes> <has_box> <has_velocities> <has_forces> <offsets ...>
 *     refused <message>
 * Exit status 0 unless a sanitizer ends it.  Never linked into the product. */
#include <stdio.h>

#include "../../include/freesasa_gpu.h"

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; ++k) {
        freesasa_gpu_trr_info d, d2;
        int64_t *offs = NULL;
        char err[300];
        if (freesasa_gpu_trr_index_read(argv[k], &d, &offs, err, (int)sizeof err)) {
            printf("refused %s\n", err);
            /* (the same with nowhere to put the message, and with 8 bytes for it) */
            (void)freesasa_gpu_trr_info_read(argv[k], &d2, NULL, 0);
            (void)freesasa_gpu_trr_info_read(argv[k], &d2, err, 8);
            continue;
        }
        printf("ok %d %lld %lld %d %lld %d %d %d", (int)d.n_atoms, (long long)d.n_frames, (long long)d.n_records, (int)d.real_bytes,
               (long long)d.max_frame_bytes, (int)d.has_box, (int)d.has_velocities, (int)d.has_forces);
        for (long long f = 0; f <= d.n_frames; ++f) printf(" %lld", (long long)offs[f]);
        printf("\n");
        freesasa_gpu_trr_index_free(offs);
    }
    return 0;
}
