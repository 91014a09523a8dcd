/*
 * ifsweep_kernels.h — the file sweep's interfaces between chain groups (freesasa_gpu_sweep_files_interfaces, gpu_sweep.hip): the
 * little device work that lets the interface tables leave the device labelled and compact.  Phase functions, shared by the HIP
 * kernels (gpu_kernels.hip: k_ifs_side_class, k_ifs_res_rows) and their CPU emulation (tests/emu/emu_ifsweep.cpp, -DSASA_EMU).
 *
 *   ifs_side_class  one thread per pair-structure atom m: the class of its input atom, a byte gather.  The class sums of the
 *                   2 P sides are then the class-sum kernel's (class_phase0 / class_phase1, sasa_kernels.h) over pair_buried with
 *                   side_offsets as the structures' offsets: the order of the adds is that kernel's, not restated here.
 *   ifs_res_rows    one thread per residue row r of the per-residue table: its side (the last q with res_off[q] <= r: sides
 *                   without a row are ties, and the last of them is the one that holds r), the side's pair and its structure s,
 *                   the structure's first residue (the lower bound of offsets[s] in res_first: a structure without atoms between
 *                   two others has no residue and moves no bound), then the residue's place in ITS structure and its 14 label
 *                   bytes - from the device parser's planes below n_res_dev, from the host parser's behind them.
 *
 * Neither lets a workgroup wait for another, neither adds a floating-point number.  Every thread writes its own outputs only.
 */
#ifndef FREESASA_AMD_IFSWEEP_KERNELS_H
#define FREESASA_AMD_IFSWEEP_KERNELS_H

#include "sasa_kernels.h"

namespace sasa {

#define IFS_B 256 /* threads per workgroup of both kernels */

struct IfsClassArgs {
    int64_t n_pair_atoms;      /* M */
    const int *pair_atom;      /* [M] input atom of every pair-structure atom */
    const unsigned char *cls;  /* [n_atoms] class of every input atom */
    unsigned char *pcls;       /* [M] */
};

SASA_D void ifs_side_class(const IfsClassArgs &a, int64_t m)
{
    if (m >= a.n_pair_atoms) return;
    a.pcls[m] = a.cls[a.pair_atom[m]];
}

struct IfsRowArgs {
    int64_t n_rows;              /* R */
    int64_t n_sides;             /* 2 P */
    const int64_t *res_off;      /* [2 P + 1] rows per side */
    const int *pair_struct;      /* [P] */
    const int64_t *offsets;      /* [n_structs + 1] */
    const int64_t *res_first;    /* [n_res + 1] first atom of every residue of the batch */
    int64_t n_res, n_res_dev;    /* residues of the batch; how many of them the device parser made */
    const int *res_index;        /* [R] residue of the batch */
    /* label planes: names, 4 bytes | chains, 4 bytes | numbers, 6 bytes as 2-byte units */
    const uint32_t *name_d, *chain_d; const uint16_t *number_d; /* [n_res_dev] */
    const uint32_t *name_h, *chain_h; const uint16_t *number_h; /* [n_res - n_res_dev] */
    int *res_local;              /* [R] the residue's place among the residues of its structure */
    uint32_t *name, *chain; uint16_t *number; /* [R] */
};

SASA_D void ifs_res_rows(const IfsRowArgs &a, int64_t r)
{
    if (r >= a.n_rows) return;
    int64_t lo = 0, hi = a.n_sides - 1; /* the last side q with res_off[q] <= r (res_off[0] = 0 <= r) */
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.res_off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    const int s = a.pair_struct[lo >> 1];
    const int64_t at = a.offsets[s];
    int64_t b = 0, e = a.n_res; /* the first residue j with res_first[j] >= at */
    while (b < e) {
        const int64_t mid = (b + e) >> 1;
        if (a.res_first[mid] < at) b = mid + 1;
        else e = mid;
    }
    const int64_t j = a.res_index[r];
    a.res_local[r] = (int)(j - b);
    const uint32_t *name = a.name_d, *chain = a.chain_d;
    const uint16_t *number = a.number_d;
    int64_t q = j;
    if (j >= a.n_res_dev) { name = a.name_h; chain = a.chain_h; number = a.number_h; q = j - a.n_res_dev; }
    a.name[r] = name[q];
    a.chain[r] = chain[q];
    a.number[3 * r] = number[3 * q];
    a.number[3 * r + 1] = number[3 * q + 1];
    a.number[3 * r + 2] = number[3 * q + 2];
}

} /* namespace sasa */

#endif
