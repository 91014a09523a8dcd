/*
 * pbc_kernels.h — phase functions of PERIODIC IMAGES (freesasa_gpu_periodic_dev / freesasa_gpu_calc_periodic and the
 * FREESASA_GPU_FRAMES_PBC bit of the trajectory file drivers, include/freesasa_gpu.h): a stage in front of the engine that
 * makes of every structure and its orthorhombic cell an EXPANDED structure - the atoms wrapped into the cell, then the
 * images of them that can be a neighbour of a wrapped atom - and a stage behind it that gives the areas of the real atoms
 * back.  The tile kernels see an ordinary batch with per-atom radii and are unchanged.
 *
 * The definition (the tests pin it; tests/pbc_ref.py restates it in numpy).  n atoms, cell L = (Lx, Ly, Lz), probe p,
 * c = 2 (max radius of the structure + p): the largest distance at which two of its atoms can be neighbours.
 *   requirement   L finite and L[a] >= c on every axis: first-shell images then suffice (an atom's own image and any
 *                 second-shell image lie at >= c, and the neighbour predicate is strict).  The host refuses anything else.
 *   wrap          w[i][a] = x[i][a] - L[a] * floor(x[i][a] / L[a]), fp64, no fma (the build has -ffp-contract=off)
 *   images        on axis a atom i admits shift 0 always, +1 when w[i][a] < c, -1 when w[i][a] > L[a] - c (L[a] < 2c: both
 *                 can hold); its images are the admitted (sx, sy, sz) != (0, 0, 0), at w[i] + s L with radius r[i]: 0 .. 26
 *   expanded      the n wrapped atoms in input order, then the images by atom ascending and, within an atom, by
 *                 code = 9 (sx + 1) + 3 (sy + 1) + (sz + 1) ascending
 *   result        atom i's periodic area is the engine's area of atom i of the expanded structure
 * Coordinates in [0, L) further than c from every face: floor is 0, w == x bit for bit, no image - the expanded batch IS
 * the batch.
 *
 *   pbc_count_struct   ONE WORKGROUP of PBC_B threads PER STRUCTURE: the structure's max radius (an LDS reduction; max is
 *                      exact in any order), then its atoms PBC_B at a time, in order: every thread the image count of its
 *                      atom, an inclusive scan within each wave64 (shuffles), the waves' sums through LDS, a running base
 *                      every thread holds alike - so the base of an atom's images is fixed and in the order above, with no
 *                      atomics.  Out: the base of every atom, the image count and the max radius of every structure.
 *   pbc_emit_atom      one thread per atom: the wrapped atom to its place, its images one behind the other from its base on
 *                      (each lane writes its own images; whether a slot-major emit would be faster has not been measured).
 *                      The wrap is RECOMPUTED here, not stored: three divisions per atom against 24 bytes written and read.
 *   pbc_collect_atom   one thread per real atom: its area out of the expanded batch's into the compact [sum n] array.
 * Totals over the real atoms are the engine's own totals kernels over the compact areas (no float atomics; nothing depends
 * on launch shape, shard cut or device list).
 *
 * One workgroup per structure suits trajectory shards of hundreds of frames and batches of many structures; for ONE
 * structure of 1e6 atoms it is slow (a single CU walks it).  That is accepted: there is no multi-workgroup scan here.
 *
 * Triclinic cells: pbc_tri_kernels.h, beside this file (nothing here changes for them).  Chain groups among periodic images
 * (freesasa_gpu_groups_periodic_dev, freesasa_gpu_trajectory_file_groups_periodic): the two phases at the end of this file.
 * Not offered: cells smaller than c; a cell for raw fp32 / fp64 frame files or the memory trajectory
 * entries (callers pass frames as a batch to freesasa_gpu_calc_periodic); skipping the
 * area computation of the image atoms (their areas are computed and dropped); file or cache sweeps (a PDB CRYST1 record is a
 * crystallographic cell with symmetry: another feature).
 *
 * Written like traj_kernels.h and select_kernels.h: every function is one thread's share of a phase, so that a -DSASA_EMU
 * build can drive them on the CPU (tests/emu/emu_pbc.cpp: the PBC_B threads of a workgroup as fibers in lock step); the
 * __global__ wrappers and kl_pbc_* launchers are in gpu_kernels.hip, the host side in gpu_periodic.hip.
 */
#ifndef FREESASA_AMD_PBC_KERNELS_H
#define FREESASA_AMD_PBC_KERNELS_H

#include "sasa_kernels.h"
#include "lr2_kernels.h" /* (LR2_SHFL and its SASA_EMU form) */

namespace sasa {

#define PBC_B 256 /* threads per workgroup of every phase */
#define PBC_WAVES (PBC_B / 64)
#ifdef SASA_EMU
#define PBC_BARRIER() sasa_emu::wave_sync()
#else
#define PBC_BARRIER() __syncthreads()
#endif

struct PbcArgs {
    /* the batch as the caller has it, device */
    const double *xyz;      /* [3 n] */
    const double *radii;    /* [n]; shared_radii: [n_fixed], the same for every structure (trajectory frames) */
    const int64_t *offsets; /* [n_structs + 1]; NULL: every structure holds n_fixed atoms */
    const double *cells;    /* [3 n_structs] */
    int n_structs, n_fixed, shared_radii;
    int64_t n_atoms;
    double probe;
    /* pbc_count_struct's results */
    int *ibase;             /* [n] images of the atoms before it in its structure */
    int64_t *n_img;         /* [n_structs] */
    double *rmax;           /* [n_structs] (0 for a structure without atoms) */
    /* the expanded batch */
    const int64_t *eoff;    /* [n_structs + 1]: eoff[s + 1] - eoff[s] = atoms + images of structure s */
    double *exyz, *eradii;  /* [3 N], [N] */
    const double *esasa;    /* [N] */
    double *sasa;           /* [n] */
};

SASA_D int64_t pbc_begin(const PbcArgs &a, int s) { return a.offsets ? a.offsets[s] : (int64_t)s * a.n_fixed; }
/* structure of atom i: the last s with begin(s) <= i (atoms of empty structures do not exist) */
SASA_D int pbc_struct_of(const PbcArgs &a, int64_t i)
{
    if (!a.offsets) return (int)(i / a.n_fixed);
    int lo = 0, hi = a.n_structs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
SASA_D double pbc_radius(const PbcArgs &a, int64_t i, int64_t b) { return a.radii[a.shared_radii ? i - b : i]; }

SASA_D double pbc_wrap(double x, double L) { return x - L * floor(x / L); }
/* the admitted shifts of one axis, bit s + 1 for shift s: 2 | (w < c ? 4 : 0) | (w > L - c ? 1 : 0) */
SASA_D unsigned pbc_admit(double w, double L, double c) { return 2u | (w < c ? 4u : 0u) | (w > L - c ? 1u : 0u); }
SASA_D int pbc_bits3(unsigned m) { return (int)((m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u)); }

/* the wrap and the three masks of atom i of a structure with cell L and cutoff c */
SASA_D void pbc_atom(const double *xyz, int64_t i, const double *L, double c, double *w, unsigned *m)
{
    for (int k = 0; k < 3; ++k) {
        w[k] = pbc_wrap(xyz[3 * i + k], L[k]);
        m[k] = pbc_admit(w[k], L[k], c);
    }
}

/* One workgroup per structure s; lds_d [PBC_B] doubles, lds_w [PBC_WAVES] ints.  Every thread of the workgroup calls this
   with the same s and runs the same number of steps (the barriers are in uniform control flow). */
SASA_D void pbc_count_struct(const PbcArgs &a, double *lds_d, int *lds_w, int s, int tid)
{
    const int64_t b = pbc_begin(a, s), e = pbc_begin(a, s + 1);
    const int lane = tid & 63, wave = tid >> 6;
    /* the structure's max radius */
    double m = 0;
    for (int64_t i = b + tid; i < e; i += PBC_B) {
        const double r = pbc_radius(a, i, b);
        if (r > m) m = r;
    }
    lds_d[tid] = m;
    PBC_BARRIER();
    for (int st = PBC_B / 2; st > 0; st >>= 1) {
        if (tid < st && lds_d[tid + st] > lds_d[tid]) lds_d[tid] = lds_d[tid + st];
        PBC_BARRIER();
    }
    m = lds_d[0];
    const double c = 2.0 * (m + a.probe);
    const double L[3] = {a.cells[3 * (int64_t)s], a.cells[3 * (int64_t)s + 1], a.cells[3 * (int64_t)s + 2]};
    int64_t base = 0; /* images of the atoms before this step (alike in every thread) */
    for (int64_t i0 = b; i0 < e; i0 += PBC_B) {
        const int64_t i = i0 + tid;
        int cnt = 0;
        if (i < e) {
            double w[3];
            unsigned mk[3];
            pbc_atom(a.xyz, i, L, c, w, mk);
            cnt = pbc_bits3(mk[0]) * pbc_bits3(mk[1]) * pbc_bits3(mk[2]) - 1;
        }
        int incl = cnt; /* inclusive scan over the wave's 64 lanes */
        for (int d = 1; d < 64; d <<= 1) {
            const int below = LR2_SHFL(incl, lane >= d ? lane - d : lane);
            if (lane >= d) incl += below;
        }
        if (lane == 63) lds_w[wave] = incl;
        PBC_BARRIER();
        int before = 0, step = 0;
        for (int k = 0; k < PBC_WAVES; ++k) {
            const int t = lds_w[k];
            if (k < wave) before += t;
            step += t;
        }
        if (i < e) a.ibase[i] = (int)(base + before + incl - cnt);
        base += step;
        PBC_BARRIER(); /* (lds_w is written again in the next step) */
    }
    if (tid == 0) { a.n_img[s] = base; a.rmax[s] = m; }
}

/* one thread per atom t of the batch */
SASA_D void pbc_emit_atom(const PbcArgs &a, int64_t t)
{
    if (t >= a.n_atoms) return;
    const int s = pbc_struct_of(a, t);
    const int64_t b = pbc_begin(a, s), n = pbc_begin(a, s + 1) - b;
    const double c = 2.0 * (a.rmax[s] + a.probe), r = pbc_radius(a, t, b);
    const double L[3] = {a.cells[3 * (int64_t)s], a.cells[3 * (int64_t)s + 1], a.cells[3 * (int64_t)s + 2]};
    double w[3];
    unsigned mk[3];
    pbc_atom(a.xyz, t, L, c, w, mk);
    int64_t j = a.eoff[s] + (t - b);
    a.exyz[3 * j] = w[0]; a.exyz[3 * j + 1] = w[1]; a.exyz[3 * j + 2] = w[2];
    a.eradii[j] = r;
    j = a.eoff[s] + n + a.ibase[t];
    for (int sx = 0; sx < 3; ++sx) {
        if (!((mk[0] >> sx) & 1u)) continue;
        for (int sy = 0; sy < 3; ++sy) {
            if (!((mk[1] >> sy) & 1u)) continue;
            for (int sz = 0; sz < 3; ++sz) {
                if (!((mk[2] >> sz) & 1u) || (sx == 1 && sy == 1 && sz == 1)) continue;
                a.exyz[3 * j] = w[0] + (double)(sx - 1) * L[0];
                a.exyz[3 * j + 1] = w[1] + (double)(sy - 1) * L[1];
                a.exyz[3 * j + 2] = w[2] + (double)(sz - 1) * L[2];
                a.eradii[j] = r;
                ++j;
            }
        }
    }
}

/* one thread per atom t of the batch */
SASA_D void pbc_collect_atom(const PbcArgs &a, int64_t t)
{
    if (t >= a.n_atoms) return;
    const int s = pbc_struct_of(a, t);
    a.sasa[t] = a.esasa[a.eoff[s] + (t - pbc_begin(a, s))];
}

/* ------------------------------------------------------------------ chain groups among periodic images
 * (freesasa_gpu_groups_periodic_dev and its kin, freesasa_gpu_trajectory_file_groups_periodic; host side: gpu_periodic.hip).
 * The COMBINED batch of the chain-group entries - the n_cplx complexes first, then every group as a structure of its own
 * (group_kernels.h; per frame: traj_kernels.h) - goes through the stage above as any batch, every group structure in the cell
 * of its complex.  Two phases are the groups' own:
 *
 *   gpbc_cell_struct    one thread per combined structure: the W doubles of its complex's cell (3, or PBC_TRI_CELL) to its own
 *                       row.  A trajectory's cells are on the device per frame, so this is a kernel and no host loop.
 *   gpbc_finish_atom    one thread per combined atom: collect and the groups' finish in one - the atom's area out of the
 *                       EXPANDED batch into the compact combined areas (what the totals of complexes and isolated groups are
 *                       summed from), a complex atom's to the caller (and as its isolated area when it is in no group), an
 *                       isolated atom's to its source atom's isolated area, and beside it the source atom's COMPLEX area, read
 *                       out of the complex's expanded structure (cgath: what a group's complex total is summed from).  No
 *                       thread reads what another writes.
 *
 * Which complex a group structure k >= n_cplx belongs to: the last s with gbase[s] <= k - n_cplx (the batch entries; a complex
 * without groups is never the last), or (k - n_cplx) / g_fixed (a shard's frames, each with the same groups).  Which atom an
 * isolated atom t >= n_atoms comes from: src[t - n_atoms] (the batch entries), or atom src[j] of frame f with
 * t - n_atoms = f n_iso_fixed + j (a shard's frames).
 *
 * INTERFACE PAIRS among periodic images (freesasa_gpu_trajectory_file_interfaces_periodic and its kin): a shard's combined batch
 * is frames | isolated groups | PAIR STRUCTURES (traj_kernels.h, traj_pair_cut), k_fixed of them per frame behind the n_cplx g_fixed
 * groups: n_comb = n_cplx (1 + g_fixed + k_fixed) structures, n_all = n_cplx (n_fixed + n_iso_fixed + n_pair) atoms.  Pair
 * structure k belongs to frame (k - n_cplx (1 + g_fixed)) / k_fixed and gets that frame's cell row; a pair atom t >= pair_first
 * has its area read out of the expanded batch into the compact combined areas AND NOTHING ELSE: it has no source atom to write
 * an isolated area to and no complex area to gather.  The pair part of cgath is therefore NEVER WRITTEN, and the host keeps the
 * pair structures' chunks out of the reduction of cgath (gpu_periodic.hip, groups_periodic_stage - as the non-periodic run does
 * with grp_chunks).  k_fixed = 0: no pairs, every byte what it was.  Only a shard's frames (gbase NULL) have pairs. */
struct GpbcArgs {
    int n_cplx, n_comb;     /* complexes; combined structures: the complexes and all their groups */
    const int64_t *coff;    /* [n_comb + 1] the combined batch's offsets */
    const int64_t *eoff;    /* [n_comb + 1] the expanded batch's */
    const int64_t *gbase;   /* [n_cplx + 1] first group of every complex; NULL: g_fixed groups per complex */
    int g_fixed;
    int k_fixed;            /* (gbase NULL) pair structures per complex, behind all the groups; 0: none */
    int64_t pair_first;     /* (k_fixed > 0) the first pair atom of the combined batch: n_atoms + n_cplx n_iso_fixed */
    /* gpbc_cell_struct */
    int W;                  /* doubles per cell */
    const double *cells;    /* [W n_cplx] */
    double *ccells;         /* [W n_comb] */
    /* gpbc_finish_atom */
    int64_t n_atoms, n_all; /* atoms of the complexes, atoms of the combined batch */
    const int *src;         /* [n_all - n_atoms]; a shard's frames: [n_iso_fixed], the topology's */
    int n_fixed, n_iso_fixed; /* a shard's frames: atoms of a frame, those of them with an id >= 0; else 0 */
    const int *key;         /* [n_atoms] < 0: in no group; a shard's frames: [n_fixed], the topology's ids */
    const double *esasa;    /* [eoff[n_comb]] */
    double *carea;          /* [n_all] the compact combined areas */
    double *cgath;          /* [n_all] the complex area of every combined atom (the pair part: never written, never read) */
    double *sasa, *iso;     /* [n_atoms]; either may be null */
};

/* the last s in [0, n) with first[s] <= v */
SASA_D int gpbc_last_le(const int64_t *first, int n, int64_t v)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
SASA_D int gpbc_complex_of(const GpbcArgs &a, int k)
{
    if (k < a.n_cplx) return k;
    if (a.k_fixed && k >= a.n_cplx * (1 + a.g_fixed)) return (k - a.n_cplx * (1 + a.g_fixed)) / a.k_fixed; /* (a pair structure) */
    return a.gbase ? gpbc_last_le(a.gbase, a.n_cplx, (int64_t)(k - a.n_cplx)) : (k - a.n_cplx) / a.g_fixed;
}

/* one thread per combined structure k */
SASA_D void gpbc_cell_struct(const GpbcArgs &a, int k)
{
    if (k >= a.n_comb) return;
    const int s = gpbc_complex_of(a, k);
    for (int w = 0; w < a.W; ++w) a.ccells[(int64_t)a.W * k + w] = a.cells[(int64_t)a.W * s + w];
}

/* one thread per combined atom t.  No thread reads what another writes: every thread reads esasa, the offsets and the
   topology's tables, which no thread writes, and writes carea[t] and cgath[t] of its own t, sasa[t] (a complex atom) or
   iso[i] of its one source atom i (an isolated atom: an atom is in one group at most; an atom in no group is written by its
   complex atom's thread); a pair atom's thread writes carea[t] alone. */
SASA_D void gpbc_finish_atom(const GpbcArgs &a, int64_t t)
{
    if (t >= a.n_all) return;
    const int k = gpbc_last_le(a.coff, a.n_comb, t); /* (atoms of empty structures do not exist) */
    const double v = a.esasa[a.eoff[k] + (t - a.coff[k])];
    a.carea[t] = v;
    if (t < a.n_atoms) {
        if (a.sasa) a.sasa[t] = v;
        a.cgath[t] = v;
        if (a.iso && a.key[a.n_fixed ? t % a.n_fixed : t] < 0) a.iso[t] = v;
        return;
    }
    if (a.k_fixed && t >= a.pair_first) return; /* (a pair atom: no isolated area, no gathered complex area) */
    const int s = gpbc_complex_of(a, k);
    int64_t i;
    if (a.n_fixed) {
        const int64_t q = t - a.n_atoms, f = q / a.n_iso_fixed;
        i = f * a.n_fixed + a.src[q - f * a.n_iso_fixed];
    } else {
        i = a.src[t - a.n_atoms];
    }
    if (a.iso) a.iso[i] = v;
    a.cgath[t] = a.esasa[a.eoff[s] + (i - a.coff[s])];
}

} /* namespace sasa */

#endif
