/* TESTS ONLY: the host loader's parsers (freesasa_amd/csrc/ingest.c) in a stand-alone program, built with AddressSanitizer +
 * UBSan (Makefile, tests/emu/ingest_check).  argv: an option set, then paths.  Every file is read into a block of EXACTLY its
 * size - no terminator, nothing behind the last byte that a parser may look at - and all of them are parsed as one batch of
 * texts by one thread.  One line per path:
 *     <status> <atoms> <residues>
 * Exit status 0 unless a sanitizer ends it (a read of the byte behind a text does).  Never linked into the product. */
#include <stdio.h>
#include <stdlib.h>

#include "../../include/freesasa_ingest.h"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const int options = atoi(argv[1]), n = argc - 2;
    char **texts = malloc(sizeof *texts * (size_t)(n ? n : 1));
    size_t *lens = malloc(sizeof *lens * (size_t)(n ? n : 1));
    if (!texts || !lens) return 2;
    for (int k = 0; k < n; ++k) {
        FILE *f = fopen(argv[k + 2], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        texts[k] = malloc((size_t)size); /* (an empty file: a block of no bytes) */
        if (!texts[k] || (size > 0 && fread(texts[k], 1, (size_t)size, f) != (size_t)size)) return 2;
        lens[k] = (size_t)size;
        fclose(f);
    }
    freesasa_ingest_batch b;
    if (freesasa_ingest_pdb_texts((const char *const *)texts, lens, n, options, 1, &b)) return 3;
    for (int k = 0; k < n; ++k)
        printf("%d %lld %lld\n", (int)b.status[k], (long long)(b.offsets[k + 1] - b.offsets[k]), (long long)(b.res_offsets[k + 1] - b.res_offsets[k]));
    freesasa_ingest_free(&b);
    for (int k = 0; k < n; ++k) free(texts[k]);
    free(texts);
    free(lens);
    return 0;
}
