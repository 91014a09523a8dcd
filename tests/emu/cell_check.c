/* TESTS ONLY: the host arithmetic of triclinic cells (freesasa_amd/csrc/cell.c) in a stand-alone program, built with
 * AddressSanitizer + UBSan (Makefile, tests/emu/cell_check).  argv holds cell records of six numbers each (A, gamma, B, beta,
 * alpha, C); one line per record, the numbers as hexadecimal floats:
 *     ok <ax> <bx> <by> <cx> <cy> <cz> widths <d_a> <d_b> <d_c> | ok <six numbers> widths refused
 *     refused <message>
 * Every record is decoded a second time with a reason buffer of 8 bytes, and once with none.  Exit status 0 unless a sanitizer
 * ends it.  Never linked into the product. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/freesasa_gpu.h"

int main(int argc, char **argv)
{
    for (int k = 1; k + 5 < argc; k += 6) {
        double rec[6], h[6], h2[6], d[3];
        char why[256], tiny[8];
        for (int j = 0; j < 6; ++j) rec[j] = strtod(argv[k + j], NULL);
        const int rc = freesasa_gpu_cell_from_dcd(rec, h, why, (int)sizeof why);
        if (freesasa_gpu_cell_from_dcd(rec, h2, tiny, (int)sizeof tiny) != rc || freesasa_gpu_cell_from_dcd(rec, h2, NULL, 0) != rc ||
            (rc && strncmp(why, tiny, sizeof tiny - 1) != 0) || (!rc && memcmp(h, h2, sizeof h) != 0)) {
            printf("inconsistent\n");
            continue;
        }
        if (rc) {
            printf("refused %s\n", why);
            continue;
        }
        printf("ok %a %a %a %a %a %a widths", h[0], h[1], h[2], h[3], h[4], h[5]);
        if (freesasa_gpu_cell_widths(h, d)) printf(" refused\n");
        else printf(" %a %a %a\n", d[0], d[1], d[2]);
    }
    return 0;
}
