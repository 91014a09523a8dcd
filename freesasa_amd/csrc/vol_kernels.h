/*
 * vol_kernels.h — phase functions of the MOLECULAR VOLUME (freesasa_gpu_sr_volume_dev / freesasa_gpu_calc_volume and the
 * volume output of the trajectory topology entries, include/freesasa_gpu.h): the volume enclosed by the solvent-accessible
 * surface of every structure of a batch, made of the Shrake-Rupley test points by the divergence theorem - what
 * `gmx sasa -tv` prints per frame, in the same formulation:
 *
 *     V = (1/3) sum_i a_i ( (x_i - o) . E_i + R_i n_i ),    E_i = sum over atom i's exposed points of u_k,  a_i = 4 pi R_i^2 / N
 *
 * (every exposed point stands for a_i of surface at x_i + R_i u_k with outward normal u_k; o is any fixed point).
 *
 * The definition (the tests pin it; tests/volume_ref.py restates it in numpy).  fp64, every operation rounded on its own (the
 * build has -ffp-contract=off).  Structure s, atoms b .. e-1, probe p, N test points u_k (freesasa_gpu_test_points):
 *   radius        R_i = r_i + p
 *   exposure      what the engine decides for the areas: t = u_k * R_i; t += x_i; the point is covered iff for some other atom
 *                 j  dx^2 + dy^2 + dz^2 <= R_j * R_j.  n_i is the engine's `counts` output.
 *   E_i           from (0, 0, 0); for k = 0 .. N-1 ascending, if point k is exposed, += u_k component by component.  Made in
 *                 the tile kernel's store phase (sr_caps_store<true>, sr_caps.h): the mask of covered points never leaves
 *                 the LDS.  evec[3i .. 3i+2].
 *   origin        per axis o_s = (min_i x_i + max_i x_i) * 0.5 over the structure's atoms (one atom: o = x exactly; the volume
 *                 moves with the structure, only the rounding of x - o differs)
 *   per atom      a = (4.0 * PI * R_i * R_i) / N;  d = x_i - o_s;  t = d_x * E_x + d_y * E_y + d_z * E_z, left to right;
 *                 v_i = (a * (t + R_i * (double) n_i)) / 3.0
 *   volume        V_s = the engine's totals kernels (kl_totals: totals_chunk_phase0 / 1, totals_struct) over v: deterministic
 *                 and independent of launch shape, like the area totals.  A structure without atoms: 0.
 *
 *   vol_origin_phase0 / 1   ONE WORKGROUP of SASA_TOT_B threads PER STRUCTURE: every thread the min and max of its atoms
 *                           (b + tid, b + tid + B, ...), then three threads fold the B partials of their axis (min and max
 *                           are exact in any order).  A structure without atoms gets (0, 0, 0).
 *   vol_atom                one thread per atom: v_i.
 *
 * Offered where the third arrangement of the Shrake-Rupley kernel runs (sr_caps.h): <= SR_CAP_POINTS_MAX = 128 unit test
 * points, a table of cap masks, neighbour lists within its limits; everything else is refused by the engine with a message
 * (gpu_engine.hip: sr_caps_shape is the one place that decides).  Not offered: Lee-Richards volume; density (mass over V: the
 * batch holds no masses); volume among periodic images (the surface is not closed within the cell).
 *
 * Written like pbc_kernels.h: every function is one thread's share of a phase, so that a -DSASA_EMU build can drive them on
 * the CPU (tests/emu/emu_volume.cpp); the __global__ wrappers and kl_vol_* launchers are in gpu_kernels.hip, the host side in
 * gpu_volume.hip.
 */
#ifndef FREESASA_AMD_VOL_KERNELS_H
#define FREESASA_AMD_VOL_KERNELS_H

#include "sasa_kernels.h"

namespace sasa {

#define VOL_B 256 /* threads per workgroup of vol_atom */

struct VolArgs {
    const double *xyz;      /* [3 n] */
    const double *radii;    /* [n]; shared_radii: ONE structure's, the same for every structure (trajectory frames) */
    const int64_t *offsets; /* [n_structs + 1] */
    int n_structs, shared_radii, n_points;
    int64_t n_atoms;
    double probe;
    const int *counts;      /* [n] exposed points per atom */
    const double *evec;     /* [3 n] */
    double *origin;         /* [3 n_structs] */
    double *vol;            /* [n] */
};

/* structure of atom i: the last s with offsets[s] <= i (atoms of empty structures do not exist) */
SASA_D int vol_struct_of(const VolArgs &a, int64_t i)
{
    int lo = 0, hi = a.n_structs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* part: [6][SASA_TOT_B] doubles of LDS (min x, y, z, max x, y, z) */
SASA_D void vol_origin_phase0(const VolArgs &a, double *part, int s, int tid)
{
    const int64_t b = a.offsets[s], e = a.offsets[s + 1];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = b + tid; i < e; i += SASA_TOT_B)
        for (int k = 0; k < 3; ++k) {
            const double x = a.xyz[3 * i + k];
            lo[k] = fmin(x, lo[k]); hi[k] = fmax(x, hi[k]);
        }
    for (int k = 0; k < 3; ++k) { part[k * SASA_TOT_B + tid] = lo[k]; part[(3 + k) * SASA_TOT_B + tid] = hi[k]; }
}
SASA_D void vol_origin_phase1(const VolArgs &a, const double *part, int s, int tid)
{
    if (tid >= 3) return;
    if (a.offsets[s + 1] <= a.offsets[s]) { a.origin[3 * (int64_t)s + tid] = 0; return; }
    double lo = part[tid * SASA_TOT_B], hi = part[(3 + tid) * SASA_TOT_B];
    for (int t = 1; t < SASA_TOT_B; ++t) { lo = fmin(part[tid * SASA_TOT_B + t], lo); hi = fmax(part[(3 + tid) * SASA_TOT_B + t], hi); }
    a.origin[3 * (int64_t)s + tid] = (lo + hi) * 0.5;
}

/* one thread per atom i of the batch */
SASA_D void vol_atom(const VolArgs &a, int64_t i)
{
    if (i >= a.n_atoms) return;
    const int s = vol_struct_of(a, i);
    const double R = a.radii[a.shared_radii ? i - a.offsets[s] : i] + a.probe;
    const double *o = a.origin + 3 * (int64_t)s, *E = a.evec + 3 * i, *x = a.xyz + 3 * i;
    const double ar = (4.0 * SASA_PI * R * R) / a.n_points;
    const double dx = x[0] - o[0], dy = x[1] - o[1], dz = x[2] - o[2];
    double t = dx * E[0];
    t += dy * E[1];
    t += dz * E[2];
    a.vol[i] = (ar * (t + R * (double)a.counts[i])) / 3.0;
}

} /* namespace sasa */

#endif
