/*
 * select_kernels.h — phase functions of the selection areas (freesasa_gpu_select_batch, freesasa_gpu_sweep_files_select,
 * include/freesasa_gpu.h): run a compiled selection set (select_program.h; select.c writes it) for every atom of a batch,
 * then sum the per-atom areas under each selection's mask, per structure.
 *
 * Written like group_kernels.h: every function is one thread's share of a phase, so that a -DSASA_EMU build can drive
 * them on the CPU (tests/emu/emu_select.cpp); the __global__ wrappers and kl_sel_* launchers are in gpu_kernels.hip.
 *
 * What an atom is compared by is what select.c atom_field / resnum read: its own name and element symbol, and the number,
 * chain and name labels of the RESIDUE it belongs to - those of the residue's first atom, also where the atom's own
 * residue-name columns differ.  No float atomics: every area is formed in one fixed order, that of class_phase0 /
 * class_phase1 (sasa_kernels.h), so that a selection's area equals, bit for bit, element [1] of the class sums with the
 * selection's 0/1 mask as class.
 */
#ifndef FREESASA_AMD_SELECT_KERNELS_H
#define FREESASA_AMD_SELECT_KERNELS_H

#include "sasa_kernels.h"
#include "select_program.h"

namespace sasa {

#define SEL_B 256 /* threads per workgroup of sel_mask */
#define SEL_G 8   /* selections one workgroup of sel_sums carries per pass over the areas: 8 sums and 8 counts in registers;
                     a set of 64 reads the structure's areas and mask words 8 times (from L2 after the first) */

struct SelArgs {
    const freesasa_sel_word *prog; /* the set's program: the same address for every lane */
    int n_words, flags, n_sel;
    const uint64_t *akey;          /* [n_atoms] name (4 bytes) | symbol (2 bytes) | 0 0 */
    const int64_t *offsets;        /* [n_structs + 1] */
    int n_structs;
    int64_t n_atoms;
    const int64_t *res_first;      /* [n_res + 1] first atom of every residue, batch-wide */
    int64_t n_res, n_res_dev;      /* residues < n_res_dev have their labels in the *_d arrays (the device parser's), the
                                      others, counted from n_res_dev, in the *_h arrays (a loaded batch's) */
    const uint32_t *name_d, *chain_d, *name_h, *chain_h; /* four bytes per residue */
    const uint16_t *number_d, *number_h;                 /* six bytes per residue */
    uint64_t *bits;                /* [n_atoms] bit k: selection k holds the atom */
    const double *sasa;            /* [n_atoms] */
    double *area;                  /* [n_structs * n_sel] */
    long long *count;              /* [n_structs * n_sel] selected atoms */
};

SASA_D bool sel_is_space(unsigned c) { return c == ' ' || (c - 9u) < 5u; } /* isspace of the C locale */

/* select.c trimmed() on a field of w bytes held in an integer (byte k = character k, zero above w): leading blanks off,
   then up to the first blank, NUL or the field's end - as a key of the same packing */
SASA_D uint64_t sel_trim(uint64_t f, int w)
{
    int i = 0;
    while (i < w && (f & 0xffu) != 0 && sel_is_space((unsigned)(f & 0xffu))) { f >>= 8; ++i; }
    uint64_t k = 0;
    for (int n = 0; i < w && (f & 0xffu) != 0 && !sel_is_space((unsigned)(f & 0xffu)); ++i, ++n) { k |= (f & 0xffu) << (8 * n); f >>= 8; }
    return k;
}

/* atoi of the six-byte number field (select.c resnum: the field with a NUL behind it) */
SASA_D int sel_atoi6(uint64_t f)
{
    int i = 0;
    while (i < 6 && sel_is_space((unsigned)(f & 0xffu))) { f >>= 8; ++i; }
    bool neg = false;
    if (i < 6 && ((f & 0xffu) == '-' || (f & 0xffu) == '+')) { neg = (f & 0xffu) == '-'; f >>= 8; ++i; }
    int v = 0;
    for (; i < 6 && (unsigned)((f & 0xffu) - '0') <= 9u; ++i) { v = v * 10 + (int)((f & 0xffu) - '0'); f >>= 8; }
    return neg ? -v : v;
}

/* the last k in [0, n) with first[k] <= i (n >= 1, first[0] <= i): the structure / residue of atom i; empty ones are passed over */
SASA_D int64_t sel_last_le(const int64_t *first, int64_t n, int64_t i)
{
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

SASA_D uint64_t sel_number_of(const SelArgs &a, int64_t r)
{
    const bool dev = r < a.n_res_dev;
    const uint16_t *q = dev ? a.number_d + 3 * r : a.number_h + 3 * (r - a.n_res_dev);
    return (uint64_t)q[0] | ((uint64_t)q[1] << 16) | ((uint64_t)q[2] << 32);
}

/* sel_mask, one thread per atom: the program over the atom's fields, a bit stack in a register, one 64-bit word out.
   The words are read through a.prog + w with w alike in every lane; the branches on the opcode and on a.flags are uniform. */
SASA_D void sel_mask_atom(const SelArgs &a, int64_t i)
{
    if (i >= a.n_atoms) return;
    const int64_t r = sel_last_le(a.res_first, a.n_res, i);
    const bool dev = r < a.n_res_dev;
    const int64_t rr = dev ? r : r - a.n_res_dev;
    const uint32_t rname = dev ? a.name_d[rr] : a.name_h[rr], rchain = dev ? a.chain_d[rr] : a.chain_h[rr];
    const uint64_t number = sel_number_of(a, r), key = a.akey[i];
    const uint64_t k_name = sel_trim(key & 0xffffffffu, 4), k_symbol = sel_trim((key >> 32) & 0xffffu, 2);
    const uint64_t k_resn = sel_trim(rname, 4), k_resi = sel_trim(number, 6);
    const uint32_t chain0 = rchain & 0xffu;
    const int chain_code = (int)(signed char)chain0; /* (select.c compares the plain char's code) */
    int resi = 0, first = 0, last = 0;
    if (a.flags & SEL_FLAG_RESI_RANGE) resi = sel_atoi6(number);
    if (a.flags & SEL_FLAG_OPEN) {
        const int64_t s = sel_last_le(a.offsets, a.n_structs, i);
        first = sel_atoi6(sel_number_of(a, sel_last_le(a.res_first, a.n_res, a.offsets[s])));
        last = sel_atoi6(sel_number_of(a, sel_last_le(a.res_first, a.n_res, a.offsets[s + 1] - 1)));
    }
    uint64_t st = 0, out = 0;
    for (int w = 0; w < a.n_words; ++w) {
        const freesasa_sel_word q = a.prog[w];
        const uint64_t k = (uint64_t)q.a | ((uint64_t)q.b << 32);
        bool m = false;
        switch (q.op) {
        case SEL_OP_AND: { const uint64_t t = st & 1u; st >>= 1; st &= t | ~(uint64_t)1; continue; }
        case SEL_OP_OR: { const uint64_t t = st & 1u; st >>= 1; st |= t; continue; }
        case SEL_OP_NOT: st ^= 1u; continue;
        case SEL_OP_END: out |= (st & 1u) << (q.a & 63u); st >>= 1; continue;
        case SEL_OP_NAME: m = k_name == k; break;
        case SEL_OP_SYMBOL: m = k_symbol == k; break;
        case SEL_OP_RESN: m = k_resn == k; break;
        case SEL_OP_RESI: m = k_resi == k; break;
        case SEL_OP_CHAIN: m = chain0 == q.a; break;
        case SEL_OP_RESI_RANGE: m = resi >= (int)q.a && resi <= (int)q.b; break;
        case SEL_OP_RESI_OPEN_L: m = resi >= first && resi <= (int)q.b; break;
        case SEL_OP_RESI_OPEN_R: m = resi >= (int)q.a && resi <= last; break;
        case SEL_OP_CHAIN_RANGE: m = chain_code >= (int)q.a && chain_code <= (int)q.b; break;
        default: break; /* SEL_OP_FALSE */
        }
        st = (st << 1) | (m ? 1u : 0u);
    }
    a.bits[i] = out;
}

/* sel_sums, SASA_TOT_B threads per (structure s, selections g0 .. g0 + SEL_G - 1): as class_phase0, every thread takes a
   contiguous chunk of the structure's atoms and sums it left to right - here under SEL_G masks at once -, then, as
   class_phase1, one thread per selection adds the partials left to right.  part [SEL_G * SASA_TOT_B], cnt alike. */
SASA_D void sel_sums_phase0(const SelArgs &a, double *part, int *cnt, int s, int g0, int tid)
{
    const int64_t b = a.offsets[s], e = a.offsets[s + 1];
    const int64_t per = (e - b + SASA_TOT_B - 1) / SASA_TOT_B;
    const int64_t lo = b + tid * per, hi = lo + per < e ? lo + per : e;
    double t[SEL_G];
    int c[SEL_G];
    for (int q = 0; q < SEL_G; ++q) { t[q] = 0; c[q] = 0; }
    for (int64_t i = lo; i < hi; ++i) {
        const double v = a.sasa[i];
        const unsigned w = (unsigned)((a.bits[i] >> g0) & ((1u << SEL_G) - 1u));
        for (int q = 0; q < SEL_G; ++q)
            if ((w >> q) & 1u) { t[q] += v; ++c[q]; }
    }
    for (int q = 0; q < SEL_G; ++q) { part[q * SASA_TOT_B + tid] = t[q]; cnt[q * SASA_TOT_B + tid] = c[q]; }
}
SASA_D void sel_sums_phase1(const SelArgs &a, const double *part, const int *cnt, int s, int g0, int tid)
{
    if (tid >= SEL_G || g0 + tid >= a.n_sel) return;
    double t = 0;
    long long c = 0;
    for (int k = 0; k < SASA_TOT_B; ++k) { t += part[tid * SASA_TOT_B + k]; c += cnt[tid * SASA_TOT_B + k]; }
    a.area[(int64_t)s * a.n_sel + g0 + tid] = t;
    a.count[(int64_t)s * a.n_sel + g0 + tid] = c;
}

} /* namespace sasa */

#endif
