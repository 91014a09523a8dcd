/* TESTS ONLY: the DCD header parser (freesasa_amd/csrc/dcd.c) in a stand-alone program, built with AddressSanitizer + UBSan
 * (Makefile, tests/emu/dcd_check).  One line per path of argv:
 *     ok <n_atoms> <n_frames> <n_frames_header> <first_frame> <frame_bytes> <x_off> <plane_bytes> <big_endian> <has_cell> <has_4d> <charmm_version>
 *     refused <message>
 * Exit status 0 unless a sanitizer ends it.  Never linked into the product. */
#include <stdio.h>

#include "../../include/freesasa_gpu.h"

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; ++k) {
        freesasa_gpu_dcd_info d;
        char err[256];
        if (freesasa_gpu_dcd_info_read(argv[k], &d, err, (int)sizeof err))
            printf("refused %s\n", err);
        else
            printf("ok %d %lld %lld %lld %lld %d %d %d %d %d %d\n", (int)d.n_atoms, (long long)d.n_frames, (long long)d.n_frames_header,
                   (long long)d.first_frame, (long long)d.frame_bytes, (int)d.x_off, (int)d.plane_bytes, (int)d.big_endian, (int)d.has_cell,
                   (int)d.has_4d, (int)d.charmm_version);
    }
    return 0;
}
