/*
 * pbc_tri_kernels.h — phase functions of PERIODIC IMAGES IN A TRICLINIC CELL (freesasa_gpu_periodic_triclinic_dev /
 * freesasa_gpu_calc_periodic_triclinic and the FREESASA_GPU_FRAMES_TRICLINIC bit of the trajectory file drivers,
 * include/freesasa_gpu.h): the stage of pbc_kernels.h with the geometry of a general cell.  What is behind the engine
 * (pbc_collect_atom) and everything about offsets, radii, bases and the expanded batch is pbc_kernels.h's, unchanged; the
 * orthorhombic phase functions, PbcArgs and their kernels are not touched by this header.
 *
 * The definition (the tests pin it; tests/pbc_tri_ref.py restates it in numpy).  A cell is six numbers
 * h = (ax, bx, by, cx, cy, cz): the lower-triangular box matrix with rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz).
 * fp64, every operation rounded on its own (the build has -ffp-contract=off), in exactly the order written.
 *   widths        d_c = cz;  d_b = by * (cz / sqrt(cy*cy + cz*cz));  t = bx*cy - by*cx;
 *                 d_a = ax * ((by*cz) / sqrt(((by*cz)*(by*cz) + (bx*cz)*(bx*cz)) + t*t))
 *                 the distances between opposite faces; made ONCE per structure ON THE HOST (freesasa_gpu_cell_widths) and
 *                 handed to the device behind the six numbers: the device takes no square root.  A right-angled cell: the edges.
 *   requirement   the six numbers finite, ax, by, cz > 0, every width >= c = 2 (max radius of the structure + probe).  Shifts
 *                 in {-1, 0, 1}^3 then suffice: two points whose k-th fractional coordinates differ by D are at least
 *                 |D| d_k apart, and the neighbour predicate is strict.  The host refuses anything else.  The cell need not
 *                 be reduced.
 *   fractional    of a point p:  fc = p_z / cz;  fb = (p_y - fc*cy) / by;  fa = ((p_x - fc*cx) - fb*bx) / ax
 *   wrap          n = floor(f) of the input atom:
 *                 w_x = ((x - nc*cx) - nb*bx) - na*ax;  w_y = (y - nc*cy) - nb*by;  w_z = z - nc*cz
 *   images        g = the fractional coordinates of w, by the same formulas (not f - n).  Axis k admits shift 0 always, +1
 *                 when g_k * d_k < c, -1 when (1.0 - g_k) * d_k < c; an atom's images are the admitted
 *                 (sa, sb, sc) != (0, 0, 0), 0 .. 26, at
 *                 x = ((w_x + sc*cx) + sb*bx) + sa*ax;  y = (w_y + sc*cy) + sb*by;  z = w_z + sc*cz   with the atom's radius
 *   expanded      the n wrapped atoms in input order, then the images by atom ascending and, within an atom, by
 *                 code = 9 (sa + 1) + 3 (sb + 1) + (sc + 1) ascending
 *   result        atom i's periodic area is the engine's area of atom i of the expanded structure
 * On (Lx, 0, Ly, 0, 0, Lz) this is pbc_kernels.h's expansion (the tests hold the two to the same bytes on their batch).
 *
 *   pbc_tri_count_struct   pbc_count_struct with this geometry: one workgroup of PBC_B threads per structure, the max radius
 *                          by an LDS reduction, then the wave64 shuffle scan and the waves' sums through LDS; no atomics.
 *   pbc_tri_emit_atom      one thread per atom: the wrapped atom, then its images from its base on.  Wrap and fractional
 *                          coordinates are RECOMPUTED here as in pbc_emit_atom, not stored by the count: six fp64 divisions per
 *                          atom (each a reciprocal estimate and a few fma steps on this device, no instruction of its own)
 *                          against 24 to 48 bytes per atom written by one kernel and read by the next, and a buffer of 24 n
 *                          bytes more.  That choice has not been measured.
 *   (collect)              pbc_collect_atom on PbcTriArgs::b
 *
 * Written like pbc_kernels.h: every function is one thread's share of a phase, so that a -DSASA_EMU build can drive them on
 * the CPU (tests/emu/emu_pbc_tri.cpp); the __global__ wrappers and kl_pbc_tri_* launchers are in gpu_kernels.hip, the host
 * side in gpu_periodic.hip.
 */
#ifndef FREESASA_AMD_PBC_TRI_KERNELS_H
#define FREESASA_AMD_PBC_TRI_KERNELS_H

#include "pbc_kernels.h"

namespace sasa {

#define PBC_TRI_CELL 9 /* doubles per structure: ax, bx, by, cx, cy, cz, then the widths d_a, d_b, d_c */

struct PbcTriArgs {
    PbcArgs b;           /* the batch, the count's results and the expanded batch as pbc_kernels.h has them; b.cells is not read */
    const double *cell9; /* [PBC_TRI_CELL n_structs] */
};

/* the fractional coordinates (a, b, c) of the point p in the cell h */
SASA_D void pbc_tri_frac(const double *p, const double *h, double *f)
{
    f[2] = p[2] / h[5];
    f[1] = (p[1] - f[2] * h[4]) / h[2];
    f[0] = ((p[0] - f[2] * h[3]) - f[1] * h[1]) / h[0];
}

/* the wrap and the three masks (a, b, c; bit s + 1 for shift s) of atom i of a structure with cell h, widths d and cutoff c */
SASA_D void pbc_tri_atom(const double *xyz, int64_t i, const double *h, const double *d, double c, double *w, unsigned *m)
{
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double f[3], g[3];
    pbc_tri_frac(p, h, f);
    const double na = floor(f[0]), nb = floor(f[1]), nc = floor(f[2]);
    w[0] = ((p[0] - nc * h[3]) - nb * h[1]) - na * h[0];
    w[1] = (p[1] - nc * h[4]) - nb * h[2];
    w[2] = p[2] - nc * h[5];
    pbc_tri_frac(w, h, g);
    for (int k = 0; k < 3; ++k) m[k] = 2u | (g[k] * d[k] < c ? 4u : 0u) | ((1.0 - g[k]) * d[k] < c ? 1u : 0u);
}

/* One workgroup per structure s; lds_d [PBC_B] doubles, lds_w [PBC_WAVES] ints.  Every thread of the workgroup calls this
   with the same s and runs the same number of steps (the barriers are in uniform control flow). */
SASA_D void pbc_tri_count_struct(const PbcTriArgs &t, double *lds_d, int *lds_w, int s, int tid)
{
    const PbcArgs &a = t.b;
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
    double h[PBC_TRI_CELL];
    for (int k = 0; k < PBC_TRI_CELL; ++k) h[k] = t.cell9[PBC_TRI_CELL * (int64_t)s + k];
    int64_t base = 0; /* images of the atoms before this step (alike in every thread) */
    for (int64_t i0 = b; i0 < e; i0 += PBC_B) {
        const int64_t i = i0 + tid;
        int cnt = 0;
        if (i < e) {
            double w[3];
            unsigned mk[3];
            pbc_tri_atom(a.xyz, i, h, h + 6, c, w, mk);
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
            const int v = lds_w[k];
            if (k < wave) before += v;
            step += v;
        }
        if (i < e) a.ibase[i] = (int)(base + before + incl - cnt);
        base += step;
        PBC_BARRIER(); /* (lds_w is written again in the next step) */
    }
    if (tid == 0) { a.n_img[s] = base; a.rmax[s] = m; }
}

/* one thread per atom i of the batch */
SASA_D void pbc_tri_emit_atom(const PbcTriArgs &t, int64_t i)
{
    const PbcArgs &a = t.b;
    if (i >= a.n_atoms) return;
    const int s = pbc_struct_of(a, i);
    const int64_t b = pbc_begin(a, s), n = pbc_begin(a, s + 1) - b;
    const double c = 2.0 * (a.rmax[s] + a.probe), r = pbc_radius(a, i, b);
    double h[PBC_TRI_CELL];
    for (int k = 0; k < PBC_TRI_CELL; ++k) h[k] = t.cell9[PBC_TRI_CELL * (int64_t)s + k];
    double w[3];
    unsigned mk[3];
    pbc_tri_atom(a.xyz, i, h, h + 6, c, w, mk);
    int64_t j = a.eoff[s] + (i - b);
    a.exyz[3 * j] = w[0]; a.exyz[3 * j + 1] = w[1]; a.exyz[3 * j + 2] = w[2];
    a.eradii[j] = r;
    j = a.eoff[s] + n + a.ibase[i];
    for (int sa = 0; sa < 3; ++sa) {
        if (!((mk[0] >> sa) & 1u)) continue;
        for (int sb = 0; sb < 3; ++sb) {
            if (!((mk[1] >> sb) & 1u)) continue;
            for (int sc = 0; sc < 3; ++sc) {
                if (!((mk[2] >> sc) & 1u) || (sa == 1 && sb == 1 && sc == 1)) continue;
                const double fa = (double)(sa - 1), fb = (double)(sb - 1), fc = (double)(sc - 1);
                a.exyz[3 * j] = ((w[0] + fc * h[3]) + fb * h[1]) + fa * h[0];
                a.exyz[3 * j + 1] = (w[1] + fc * h[4]) + fb * h[2];
                a.exyz[3 * j + 2] = w[2] + fc * h[5];
                a.eradii[j] = r;
                ++j;
            }
        }
    }
}

} /* namespace sasa */

#endif
