/* TESTS ONLY: the AMBER NetCDF header parser (freesasa_amd/csrc/netcdf.c) and the cell decoding behind it (cell.c) in a
 * stand-alone program, built with AddressSanitizer + UBSan (Makefile, tests/emu/nc_check).  One line per path of argv:
 *     ok <n_atoms> <n_frames> <n_frames_header> <first_record> <record_bytes> <coord_off> <lengths_off> <angles_off> <version> <has_cell> <has_time> <has_velocities>
 *     refused <message>
 * and with a cell, behind an ok line, one line per frame (the numbers as hexadecimal floats):
 *     cell <f> <a> <b> <c> <alpha> <beta> <gamma> ok <ax> <bx> <by> <cx> <cy> <cz> | cell <f> <six numbers> refused <reason>
 * The records are read into a buffer of exactly their size.  Exit status 0 unless a sanitizer ends it.  Never linked into the
 * product. */
#include <stdio.h>
#include <stdlib.h>

#include "../../include/freesasa_gpu.h"

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; ++k) {
        freesasa_gpu_nc_info d;
        char err[256];
        if (freesasa_gpu_nc_info_read(argv[k], &d, err, (int)sizeof err)) {
            printf("refused %s\n", err);
            continue;
        }
        printf("ok %d %lld %lld %lld %lld %lld %lld %lld %d %d %d %d\n", (int)d.n_atoms, (long long)d.n_frames, (long long)d.n_frames_header,
               (long long)d.first_record, (long long)d.record_bytes, (long long)d.coord_off, (long long)d.lengths_off, (long long)d.angles_off,
               (int)d.version, (int)d.has_cell, (int)d.has_time, (int)d.has_velocities);
        if (!d.has_cell || d.n_frames * d.record_bytes > (64LL << 20)) continue;
        const size_t bytes = (size_t)(d.n_frames * d.record_bytes);
        char *records = malloc(bytes);
        FILE *fp = fopen(argv[k], "rb");
        if (records && fp && fseek(fp, (long)d.first_record, SEEK_SET) == 0 && fread(records, 1, bytes, fp) == bytes)
            for (long long f = 0; f < d.n_frames; ++f) {
                double len[3], deg[3], h[6];
                char why[256];
                freesasa_gpu_nc_cell_record(&d, records, f, len, deg);
                printf("cell %lld %a %a %a %a %a %a", f, len[0], len[1], len[2], deg[0], deg[1], deg[2]);
                if (freesasa_gpu_cell_from_lengths_angles(len, deg, h, why, (int)sizeof why)) printf(" refused %s\n", why);
                else printf(" ok %a %a %a %a %a %a\n", h[0], h[1], h[2], h[3], h[4], h[5]);
            }
        if (fp) fclose(fp);
        free(records);
    }
    return 0;
}
