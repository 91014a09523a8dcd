/*
 * group_kernels.h — phase functions of the chain-group entry (freesasa_gpu_groups_dev, include/freesasa_gpu.h): count
 * and validate the atoms of every group, cut the groups out of their structures into one combined batch in a stable
 * order, and give the isolated areas back in input order.  The SASA of the combined batch is the ordinary pipeline
 * (sasa_kernels.h, lr2_kernels.h, sr_caps.h), unchanged.
 *
 * Written like sasa_kernels.h: every function is one thread's (or, for grp_rank_struct, one wave's) share of a phase,
 * so that a -DSASA_EMU build can drive them on the CPU; the __global__ wrappers and kl_grp_* launchers are in
 * gpu_kernels.hip, the host side in gpu_groups.hip.
 *
 * Combined batch: the n input atoms first, as they are (the complex structures), then the G isolated structures in
 * structure-major group order k = gbase[s] + g, each holding the atoms of its group in their input order.  Derived atom
 * j >= n is input atom src[j - n].  Integer atomics only (the per-group counts); no float atomics anywhere: every area
 * and every sum is formed in one fixed order.
 */
#ifndef FREESASA_AMD_GROUP_KERNELS_H
#define FREESASA_AMD_GROUP_KERNELS_H

#include "sasa_kernels.h"
#include "lr2_kernels.h" /* (the wave primitives LR2_BALLOT / LR2_SHFL / LR2_RANK / LR2_POPC64, and their SASA_EMU forms) */

namespace sasa {

#define GRP_B 256 /* threads per workgroup of the per-atom phases */

struct GrpArgs {
    /* input, device */
    const double *xyz;      /* [3 n] */
    const double *radii;    /* [n] */
    const int32_t *group;   /* [n] group id of each atom, local to its structure; -1: in no group */
    const int64_t *offsets; /* [n_structs + 1] */
    const int64_t *gbase;   /* [n_structs + 1] first group of each structure in structure-major order (prefix of n_groups) */
    int n_structs, n_atoms, n_groups; /* n_groups: G, the groups of the whole batch */
    /* workspace */
    int *key;    /* [n] gbase[s] + g, or -1 */
    int *count;  /* [G + 2] atoms per group; [G]: a bad id was seen (1), [G + 1]: 1 + the last atom index with a bad id */
    int *cursor; /* [G] next combined-batch index of each group (the host sets it to n + the group's first) */
    double *cxyz, *cradii; /* [3 N], [N] the combined batch, N = n + n_iso */
    int *src;    /* [n_iso] input atom of each isolated atom */
    int n_iso;
    /* results of the combined batch and what is made of them */
    const double *csasa;  /* [N] */
    const double *ctot;   /* [n_structs + G] per combined structure */
    const double *ctot2;  /* [n_structs + G] per combined structure, over cgath */
    double *cgath;        /* [N] complex area of every combined atom (j < n: its own; j >= n: its source atom's) */
    double *sasa, *iso;   /* [n] caller's outputs */
    double *totals;       /* [n_structs] or null */
    double *gtot;         /* [3 G] or null */
};

/* structure of atom i: the last s with offsets[s] <= i (atoms of empty structures do not exist) */
SASA_D int grp_struct_of(const GrpArgs &a, int64_t i)
{
    int lo = 0, hi = a.n_structs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* Phase 1, one thread per atom (every lane of a wave takes part: the counts are added once per distinct group of the
 * wave, by the first lane holding it): the atom's key, the group's count, bad ids into the status words. */
SASA_D void grp_count_atom(const GrpArgs &a, int i, int lane)
{
    const bool in = i < a.n_atoms;
    int k = -1;
    if (in) {
        const int s = grp_struct_of(a, i);
        const int g = a.group[i];
        const int64_t ng = a.gbase[s + 1] - a.gbase[s];
        if (g < -1 || (int64_t)g >= ng) {
            a.count[a.n_groups] = 1;
            SASA_ATOMIC_MAX_GLB(&a.count[a.n_groups + 1], i + 1);
        } else if (g >= 0) {
            k = (int)(a.gbase[s] + g);
        }
        a.key[i] = k;
    }
    unsigned long long pending = LR2_BALLOT(k >= 0);
    while (pending) {
        const int leader = __builtin_ctzll(pending);
        const int k0 = LR2_SHFL(k, leader);
        const unsigned long long m = LR2_BALLOT(k == k0);
        if (lane == leader) SASA_ATOMIC_ADD_GLB(&a.count[k0], (int)LR2_POPC64(m));
        pending &= ~m;
    }
}

/* Phase 2, ONE WAVE PER STRUCTURE: its atoms 64 at a time, in order; every group of the structure is this wave's alone,
 * so a group's running position needs no atomics.  The position of the group met last stays in a register (lane 0
 * keeps the array up to date when the group changes): a structure made of a few chains touches the array a few times.
 * Each atom of a group goes to cursor + its rank among the lanes of its group: xyz, radius and its own index. */
SASA_D void grp_rank_struct(const GrpArgs &a, int s, int lane)
{
    const int64_t b = a.offsets[s], e = a.offsets[s + 1];
    int ck = -1, cpos = 0; /* the group met last and its next position (alike in every lane) */
    for (int64_t i0 = b; i0 < e; i0 += 64) {
        const int64_t i = i0 + lane;
        const int k = i < e ? a.key[i] : -1;
        unsigned long long pending = LR2_BALLOT(k >= 0);
        while (pending) {
            const int k0 = LR2_SHFL(k, __builtin_ctzll(pending));
            const unsigned long long m = LR2_BALLOT(k == k0);
            if (k0 != ck) {
                int p = 0;
                if (lane == 0) { /* (one lane reads and writes the array: program order on the same address) */
                    if (ck >= 0) a.cursor[ck] = cpos;
                    p = a.cursor[k0];
                }
                cpos = LR2_SHFL(p, 0);
                ck = k0;
            }
            if (k == k0) {
                const int j = cpos + (int)LR2_RANK(m, lane);
                a.cxyz[3 * (int64_t)j] = a.xyz[3 * i];
                a.cxyz[3 * (int64_t)j + 1] = a.xyz[3 * i + 1];
                a.cxyz[3 * (int64_t)j + 2] = a.xyz[3 * i + 2];
                a.cradii[j] = a.radii[i];
                a.src[j - a.n_atoms] = (int)i;
            }
            cpos += (int)LR2_POPC64(m);
            pending &= ~m;
        }
    }
}

/* Phase 3, one thread per combined atom t: the complex areas to the caller, the isolated ones back to input order,
 * and the complex area of every isolated atom beside it (cgath: what the group's complex total is summed from). */
SASA_D void grp_finish_atom(const GrpArgs &a, int64_t t)
{
    const int64_t n = a.n_atoms;
    if (t < n) {
        const double v = a.csasa[t];
        a.sasa[t] = v;
        a.cgath[t] = v;
        if (a.key[t] < 0) a.iso[t] = v;
    } else if (t < n + a.n_iso) {
        const int i = a.src[t - n];
        a.iso[i] = a.csasa[t];
        a.cgath[t] = a.csasa[i];
    }
}

/* Phase 4, one thread per group / structure: totals, and per group (isolated, complex, buried = isolated - complex) */
SASA_D void grp_totals_item(const GrpArgs &a, int k)
{
    if (a.totals && k < a.n_structs) a.totals[k] = a.ctot[k];
    if (a.gtot && k < a.n_groups) {
        const double t0 = a.ctot[a.n_structs + k], t1 = a.ctot2[a.n_structs + k];
        a.gtot[3 * (int64_t)k] = t0;
        a.gtot[3 * (int64_t)k + 1] = t1;
        a.gtot[3 * (int64_t)k + 2] = t0 - t1;
    }
}

} /* namespace sasa */

#endif
