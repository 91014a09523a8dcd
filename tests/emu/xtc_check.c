/* TESTS ONLY: the XTC header walker (freesasa_amd/csrc/xtc.c) in a stand-alone program, built with AddressSanitizer + UBSan
 * (Makefile, tests/emu/xtc_check).  One line per path of argv:
 *     ok <n_atoms> <n_frames> <max_frame_bytes> <precision as a hexadecimal float> <has_box> <the offset behind the last frame>
 *     refused <message>
 * Exit status 0 unless a sanitizer ends it.  Never linked into the product. */
#include <stdio.h>

#include "../../include/freesasa_gpu.h"

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; ++k) {
        freesasa_gpu_xtc_info d;
        int64_t *offs = NULL;
        char err[300];
        if (freesasa_gpu_xtc_index_read(argv[k], &d, &offs, err, (int)sizeof err)) {
            printf("refused %s\n", err);
            continue;
        }
        printf("ok %d %lld %lld %a %d %lld\n", (int)d.n_atoms, (long long)d.n_frames, (long long)d.max_frame_bytes, (double)d.precision, (int)d.has_box,
               (long long)offs[d.n_frames]);
        freesasa_gpu_xtc_index_free(offs);
    }
    return 0;
}
