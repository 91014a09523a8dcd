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
    double *sasa, *iso;   /* [n] caller's outputs (either may be null: the file sweep wants neither, gpu_sweep.hip) */
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
        if (a.sasa) a.sasa[t] = v;
        a.cgath[t] = v;
        if (a.iso && a.key[t] < 0) a.iso[t] = v;
    } else if (t < n + a.n_iso) {
        const int i = a.src[t - n];
        if (a.iso) a.iso[i] = a.csasa[t];
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

/* ------------------------------------------------------------------ group ids made on the device
 * (freesasa_gpu_chain_group_ids, freesasa_gpu_sweep_files_groups): what freesasa_ingest_chain_groups (select.c) makes of a
 * loaded batch's chain labels, made of residue boundaries and labels that are on the device - the device parser's residues
 * first, a loaded batch's behind them, as SelArgs has them.  The spec is parsed on the host by select.c's own code
 * (freesasa_ingest_chain_groups_parse); its labels come sorted by their value as a word so that a residue finds its own in
 * log2(n_lab) steps. */

#define GID_MAX_PER_STRUCT 65535
#define GID_MAX_LABELS 4096
#define GID_EGROUP 8 /* FREESASA_INGEST_EGROUP (gpu_groups.hip asserts it) */
#ifdef SASA_EMU
#define GID_FENCE() ((void)0)
#else
#define GID_FENCE() __threadfence()
#endif

struct GidArgs {
    const int64_t *offsets;      /* [n_structs + 1] atoms */
    int n_structs;
    const int64_t *res_first;    /* [n_res + 1] first atom of every residue, batch-wide (n_res 0: one entry) */
    int64_t n_res, n_res_dev;    /* residues < n_res_dev have their label in chain_d, the others, counted from n_res_dev, in chain_h */
    const uint32_t *chain_d, *chain_h;
    const int32_t *status;       /* [n_structs] the loader's status */
    const uint32_t *lab;         /* [n_lab] the spec's labels, ascending; n_lab 0: separate chains */
    const int32_t *lab_group;    /* [n_lab] */
    int n_lab, n_spec_groups;
    int32_t *group;              /* [n_atoms] */
    int32_t *n_groups, *group_status; /* [n_structs] */
};

/* the first k in [0, n] with first[k] >= v (first has n + 1 entries, ascending): a structure's residues are those between
   the bounds of its first atom and of its end; a residue without atoms on the border belongs to nobody it matters to */
SASA_D int64_t gid_lower(const int64_t *first, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (first[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
/* strncmp over 4 bytes as equality of words: nothing behind a label's first NUL counts */
SASA_D uint32_t gid_canon(uint32_t l)
{
    if (!(l & 0xffu)) return 0;
    if (!(l & 0xff00u)) return l & 0xffu;
    if (!(l & 0xff0000u)) return l & 0xffffu;
    return l;
}

/* ONE WAVE PER STRUCTURE, its residues 64 at a time in order.  Separate chains: a residue that holds atoms starts a group
 * when its 4 label bytes differ from those of the residue with atoms before it - the lane below it, or, for the step's first
 * one, the label carried over from the step before; a lane's group is the running number plus the starts up to its own.
 * Spec: every lane looks its label up, marks it present (present [GID_MAX_LABELS / 32], the wave's own: LDS) and takes its
 * group; a structure that misses one of the labels has all its ids put back to -1.  A lane writes the ids of its residue's
 * atoms itself. */
SASA_D void gid_struct(const GidArgs &a, unsigned *present, int s, int lane)
{
    const int64_t b = a.offsets[s], e = a.offsets[s + 1];
    const int st = a.status[s];
    const bool separate = a.n_lab == 0;
    int ng = separate ? 0 : a.n_spec_groups, gs = st;
    bool bad = st != 0;
    if (st == 0) {
        const int words = (a.n_lab + 31) >> 5;
        for (int w = lane; w < words; w += 64) present[w] = 0;
        LR2_SYNC();
        const int64_t r0 = gid_lower(a.res_first, a.n_res, b), r1 = gid_lower(a.res_first, a.n_res, e);
        int run = 0;          /* groups so far, the label of the last residue with atoms (alike in every lane) */
        bool have = false;
        uint32_t carry = 0;
        for (int64_t rb = r0; rb < r1; rb += 64) {
            const int64_t r = rb + lane;
            int64_t a0 = 0, a1 = 0;
            if (r < r1) { a0 = a.res_first[r]; a1 = a.res_first[r + 1]; }
            const bool has = a1 > a0;
            uint32_t lbl = 0;
            if (has) lbl = r < a.n_res_dev ? a.chain_d[r] : a.chain_h[r - a.n_res_dev];
            int g = -1;
            if (separate) {
                const unsigned long long hm = LR2_BALLOT(has);
                const unsigned long long below = hm & ((1ull << lane) - 1ull);
                const uint32_t pl = (uint32_t)LR2_SHFL((int)lbl, below ? 63 - __builtin_clzll(below) : 0);
                const bool start = has && (below ? lbl != pl : (!have || lbl != carry));
                const unsigned long long sm = LR2_BALLOT(start);
                g = run + (int)LR2_POPC64(sm & ((2ull << lane) - 1ull)) - 1;
                run += (int)LR2_POPC64(sm);
                const uint32_t last = (uint32_t)LR2_SHFL((int)lbl, hm ? 63 - __builtin_clzll(hm) : 0);
                if (hm) { carry = last; have = true; }
            } else if (has) {
                const uint32_t key = gid_canon(lbl);
                int lo = 0, hi = a.n_lab - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (a.lab[mid] < key) lo = mid + 1;
                    else hi = mid;
                }
                if (a.lab[lo] == key) {
                    SASA_ATOMIC_OR_LDS(&present[lo >> 5], 1u << (lo & 31));
                    g = a.lab_group[lo];
                }
            }
            for (int64_t i = a0; i < a1; ++i) a.group[i] = g;
        }
        if (separate) {
            bad = run > GID_MAX_PER_STRUCT;
            ng = bad ? 0 : run;
        } else {
            LR2_SYNC();
            bool miss = false;
            for (int w = lane; w < words; w += 64) {
                const int nb = a.n_lab - 32 * w;
                miss = miss || present[w] != (nb >= 32 ? 0xffffffffu : (1u << nb) - 1u);
            }
            bad = LR2_BALLOT(miss) != 0;
        }
        if (bad) gs = GID_EGROUP;
    }
    if (bad) {
        GID_FENCE(); /* (the ids written above, by other lanes, are in memory before these go over them) */
        for (int64_t i = b + lane; i < e; i += 64) a.group[i] = -1;
    }
    if (lane == 0) { a.n_groups[s] = ng; a.group_status[s] = gs; }
}

/* The label of every group of a batch cut by separate chains, one thread per group: that of the residue of the group's first
 * atom in the combined batch (coffsets: the combined batch's offsets, [n_structs + n_groups + 1]; src as in GrpArgs). */
struct GidLabelArgs {
    const int64_t *coffsets;
    const int *src;
    int n_structs, n_groups;
    int64_t n_atoms;
    const int64_t *res_first;
    int64_t n_res, n_res_dev;
    const uint32_t *chain_d, *chain_h;
    uint32_t *label;             /* [n_groups] */
};
SASA_D void gid_label_item(const GidLabelArgs &a, int k)
{
    if (k >= a.n_groups) return;
    const int64_t p0 = a.coffsets[a.n_structs + k], p1 = a.coffsets[a.n_structs + k + 1];
    uint32_t l = 0;
    if (p1 > p0 && a.n_res > 0) {
        const int64_t i = a.src[p0 - a.n_atoms];
        int64_t lo = 0, hi = a.n_res - 1; /* the last residue that begins at or before atom i */
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (a.res_first[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        l = lo < a.n_res_dev ? a.chain_d[lo] : a.chain_h[lo - a.n_res_dev];
    }
    a.label[k] = l;
}

} /* namespace sasa */

#endif
