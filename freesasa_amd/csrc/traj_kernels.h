/*
 * traj_kernels.h — phase functions of the trajectory drivers' TOPOLOGY (freesasa_gpu_trajectory_topology,
 * freesasa_gpu_trajectory_file_topology, include/freesasa_gpu.h): the frames of a shard are one structure n atoms long,
 * repeated; what says which frame atom is which topology atom, where its residues begin, what class an atom has and which
 * selections hold it is the same for every frame and lives once per lane on the device.  Per shard, behind the tile kernels:
 *
 *   traj_gather        out[f][i] = in[f][index[i]], fp32 input widened on the way (before the engine sees the frames)
 *   traj_residue       the six per-residue areas of every (frame, residue), as residue_areas (sasa_kernels.h)
 *   traj_class_phase0  the three class sums of every frame, as class_phase0 / class_phase1
 *   traj_sel_phase0/1  the selection areas of every frame, as sel_sums_phase0 / sel_sums_phase1 (select_kernels.h)
 *
 * Atom i of frame f is element f * n + i of the shard's per-atom areas and reads the per-topology arrays at i.  Every sum
 * takes its atoms in the order of the function it is named after - the same chunks of SASA_TOT_B, left to right, the
 * partials left to right, no float atomics - so a frame's numbers are, bit for bit, what those kernels give on that frame
 * as a structure of its own.
 *
 * Written like select_kernels.h: every function is one thread's share of a phase, so that a -DSASA_EMU build can drive them
 * on the CPU (tests/emu/emu_traj.cpp); the __global__ wrappers and kl_traj_* launchers are in gpu_kernels.hip.
 */
#ifndef FREESASA_AMD_TRAJ_KERNELS_H
#define FREESASA_AMD_TRAJ_KERNELS_H

#include "sasa_kernels.h"
#include "select_kernels.h"

namespace sasa {

#define TRAJ_B 256 /* threads per workgroup of traj_gather and traj_residue */

struct TrajArgs {
    int n;                    /* atoms of the topology = atoms of a frame as the engine sees it */
    int n_frames;             /* frames of this shard */
    int frame_atoms;          /* atoms of an INPUT frame (>= n) */
    const int32_t *index;     /* [n] topology atom i is input atom index[i] */
    int n_res;
    const int64_t *res_first; /* [n_res + 1] first atom of every residue, within the topology (res_first[0] = 0) */
    const unsigned char *cls, *bb; /* [n] */
    const uint64_t *bits;     /* [n] bit k: selection k holds the atom (sel_mask_atom on the topology, once) */
    int n_sel;
    const double *sasa;       /* [n_frames * n] */
    double *cls_out;          /* [n_frames * 3] */
    double *res_out;          /* [n_frames * n_res * 6] */
    double *sel_out;          /* [n_frames * n_sel] */
    long long *sel_count;     /* [n_frames * n_sel] selected atoms (the same for every frame) */
};

/* traj_gather, one thread per COORDINATE of the compact frames (3 * n_frames * n): consecutive lanes write consecutive
   doubles; three lanes share an input atom, and a monotonic index reads as coalesced as the solute lies in the frame. */
template <class T>
SASA_D void traj_gather(const TrajArgs &a, const T *in, double *out, int64_t t)
{
    const int64_t total = 3 * (int64_t)a.n_frames * a.n;
    if (t >= total) return;
    const int64_t atom = t / 3;
    const int comp = (int)(t - 3 * atom);
    const int64_t f = atom / a.n;
    const int i = (int)(atom - f * a.n);
    out[t] = (double)in[3 * (f * a.frame_atoms + a.index[i]) + comp];
}

/* traj_residue, one thread per (frame, residue): residue_areas' loop with the areas of frame f and the flags of the topology */
SASA_D void traj_residue(const TrajArgs &a, int64_t t)
{
    if (t >= (int64_t)a.n_frames * a.n_res) return;
    const int64_t f = t / a.n_res;
    const int r = (int)(t - f * a.n_res);
    const double *sasa = a.sasa + f * a.n;
    double total = 0, mc = 0, sc = 0, polar = 0, apolar = 0, unknown = 0;
    for (int64_t i = a.res_first[r]; i < a.res_first[r + 1]; ++i) {
        const double v = sasa[i];
        total += v;
        if (a.bb[i]) mc += v; else sc += v;
        const int c = a.cls[i];
        if (c == 0) apolar += v;
        else if (c == 1) polar += v;
        else unknown += v;
    }
    double *o = a.res_out + 6 * t;
    o[0] = total; o[1] = mc; o[2] = sc; o[3] = polar; o[4] = apolar; o[5] = unknown;
}

/* SASA_TOT_B threads per frame: class_phase0 with offsets[f] = f * n and the class of atom i - f * n; then class_phase1 */
SASA_D void traj_class_phase0(const TrajArgs &a, double *part, int f, int tid)
{
    const int64_t b = (int64_t)f * a.n, e = b + a.n;
    const int64_t per = (e - b + SASA_TOT_B - 1) / SASA_TOT_B;
    const int64_t lo = b + tid * per, hi = lo + per < e ? lo + per : e;
    double t0 = 0, t1 = 0, t2 = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const double v = a.sasa[i];
        const int c = a.cls[i - b];
        if (c == 0) t0 += v;
        else if (c == 1) t1 += v;
        else t2 += v;
    }
    part[3 * tid] = t0; part[3 * tid + 1] = t1; part[3 * tid + 2] = t2;
}

/* SASA_TOT_B threads per (frame, selections g0 .. g0 + SEL_G - 1): sel_sums_phase0 / sel_sums_phase1 in the same way */
SASA_D void traj_sel_phase0(const TrajArgs &a, double *part, int *cnt, int f, int g0, int tid)
{
    const int64_t b = (int64_t)f * a.n, e = b + a.n;
    const int64_t per = (e - b + SASA_TOT_B - 1) / SASA_TOT_B;
    const int64_t lo = b + tid * per, hi = lo + per < e ? lo + per : e;
    double t[SEL_G];
    int c[SEL_G];
    for (int q = 0; q < SEL_G; ++q) { t[q] = 0; c[q] = 0; }
    for (int64_t i = lo; i < hi; ++i) {
        const double v = a.sasa[i];
        const unsigned w = (unsigned)((a.bits[i - b] >> g0) & ((1u << SEL_G) - 1u));
        for (int q = 0; q < SEL_G; ++q)
            if ((w >> q) & 1u) { t[q] += v; ++c[q]; }
    }
    for (int q = 0; q < SEL_G; ++q) { part[q * SASA_TOT_B + tid] = t[q]; cnt[q * SASA_TOT_B + tid] = c[q]; }
}
SASA_D void traj_sel_phase1(const TrajArgs &a, const double *part, const int *cnt, int f, int g0, int tid)
{
    if (tid >= SEL_G || g0 + tid >= a.n_sel) return;
    double t = 0;
    long long c = 0;
    for (int k = 0; k < SASA_TOT_B; ++k) { t += part[tid * SASA_TOT_B + k]; c += cnt[tid * SASA_TOT_B + k]; }
    a.sel_out[(int64_t)f * a.n_sel + g0 + tid] = t;
    a.sel_count[(int64_t)f * a.n_sel + g0 + tid] = c;
}

} /* namespace sasa */

#endif
