/* select_program.h — the compiled form of a selection set (freesasa_ingest_selection, include/freesasa_ingest.h): what
 * select.c writes and select_kernels.h runs.  Never installed.  Plain C: select.c includes it.
 *
 * A set of up to SEL_MAX_SELECTIONS commands is ONE postfix program of 16-byte words.  An atom's thread runs it from the
 * first word to the last with a stack of bits: a test pushes its result, and / or take two bits and leave one, not flips
 * the top, "end of selection k" takes the top as bit k of the atom's mask word.  Everything select.c decides from the
 * command alone is decided when the program is written: ids are upper-cased and packed into integer keys (byte k =
 * character k; a field trimmed the way select.c trimmed() trims it compares with the key by integer compares), range
 * bounds are numbers, and what select.c skips with a warning (valid_id, the type checks of select_range) is SEL_OP_FALSE.
 * What depends on the structure stays an operand: the open ends of "resi -N" / "resi N-".
 */
#ifndef FREESASA_AMD_SELECT_PROGRAM_H
#define FREESASA_AMD_SELECT_PROGRAM_H

#include <stdint.h>

#define SEL_MAX_SELECTIONS 64 /* one 64-bit mask word per atom */
#define SEL_MAX_WORDS 4096    /* words of one set's program (64 KiB) */
#define SEL_MAX_DEPTH 64      /* the bit stack is one 64-bit register */

enum {
    SEL_OP_FALSE = 0,   /* push 0 (an item select.c ignores with a warning, or an id no field can hold) */
    SEL_OP_NAME,        /* push: trimmed atom name == key (a | b << 32) */
    SEL_OP_SYMBOL,      /* ... element symbol */
    SEL_OP_RESN,        /* ... residue name */
    SEL_OP_RESI,        /* ... residue number field, as a string */
    SEL_OP_CHAIN,       /* push: first byte of the chain label == a */
    SEL_OP_RESI_RANGE,  /* push: a <= atoi(residue number) <= b (a, b: int) */
    SEL_OP_RESI_OPEN_L, /* push: atoi(number of the structure's FIRST atom's residue) <= atoi(residue number) <= b */
    SEL_OP_RESI_OPEN_R, /* push: a <= atoi(residue number) <= atoi(number of the structure's LAST atom's residue) */
    SEL_OP_CHAIN_RANGE, /* push: a <= (signed char) first byte of the chain label <= b */
    SEL_OP_AND, SEL_OP_OR, SEL_OP_NOT,
    SEL_OP_END          /* pop into bit a of the mask word */
};
enum { SEL_FLAG_RESI_RANGE = 1, /* the program holds a resi range: atoi of the number field is needed */
       SEL_FLAG_OPEN = 2 };     /* ... an open one: the structure's first and last residue numbers are needed */

typedef struct freesasa_sel_word { uint32_t op, a, b, c; } freesasa_sel_word;

/* (the program of a set: freesasa_ingest_selection_program, include/freesasa_ingest.h) */

/* An atom's 8-byte key: name (4 bytes) | symbol (2 bytes) | 0 0, from the arrays of a freesasa_ingest_batch */
static inline void sel_pack_atom_keys(const char *atom_name, const char *atom_symbol, int64_t n, uint64_t *out)
{
    for (int64_t i = 0; i < n; ++i) {
        uint64_t k = 0;
        for (int q = 0; q < 4; ++q) k |= (uint64_t)(unsigned char)atom_name[4 * i + q] << (8 * q);
        for (int q = 0; q < 2; ++q) k |= (uint64_t)(unsigned char)atom_symbol[2 * i + q] << (32 + 8 * q);
        out[i] = k;
    }
}

#endif
