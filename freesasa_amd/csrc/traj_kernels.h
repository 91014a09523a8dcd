/*
 * traj_kernels.h — phase functions of the trajectory drivers' TOPOLOGY (freesasa_gpu_trajectory_topology,
 * freesasa_gpu_trajectory_file_topology, include/freesasa_gpu.h): the frames of a shard are one structure n atoms long,
 * repeated; what says which frame atom is which topology atom, where its residues begin, what class an atom has and which
 * selections hold it is the same for every frame and lives once per lane on the device.  Per shard, behind the tile kernels:
 *
 *   traj_gather        out[f][i] = in[f][index[i]], fp32 input widened on the way (before the engine sees the frames)
 *   traj_gather_dcd    the same from the bytes of DCD frames: planar x[] | y[] | z[] records of fp32, either byte order
 *   traj_gather_nc     the same from the bytes of AMBER NetCDF records: big-endian fp32, atom by atom, at a record stride
 *   traj_gather_trr    the same from the bytes of GROMACS TRR records: big-endian fp32 or fp64 in nm, each frame at its own byte
 *   traj_residue       the six per-residue areas of every (frame, residue), as residue_areas (sasa_kernels.h)
 *   traj_class_phase0  the three class sums of every frame, as class_phase0 / class_phase1
 *   traj_sel_phase0/1  the selection areas of every frame, as sel_sums_phase0 / sel_sums_phase1 (select_kernels.h)
 *   traj_group_*       chain groups per frame: the isolated structures behind the frames, as group_kernels.h
 *   traj_pair_*        interfaces between chain groups per frame: the pair structures behind the isolated ones, six doubles a pair
 *   traj_pair_res      ... and their per-residue table: four doubles per (frame, segment of a side that lies in one residue)
 *   traj_stats         run statistics: a shard's partial (mean, M2, min, max) of every column of the outputs asked for (at the end)
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

/* traj_gather_dcd: the frames of a shard as they lie in a DCD file (dcd.c has the layout) -> the compact fp64 frames.  Each
   frame is frame_bytes long and holds, from byte x_off on, three planes plane_bytes apart: x[], y[], z[] of ALL its atoms as
   fp32, with record markers (and, in front or behind, a unit cell and a 4th dimension) between them that no thread reads.
   One thread per output coordinate, t -> (f, i, comp) as in traj_gather: consecutive lanes write consecutive doubles; lanes
   t, t + 3, t + 6, ... read consecutive floats of one plane when the index is monotonic.  index NULL: the identity (the
   plain drivers, or a topology that is the whole frame).  Every offset is a multiple of 4 and in general not of 8 (an odd
   atom count makes plane_bytes an odd multiple of 4): 4-byte loads only, `in` is the shard's bytes as 32-bit words.  SWAP: the
   file is big-endian - a build of its own, not a branch per lane.  This is traj_gather AND the widening for DCD input. */
struct TrajDcdArgs {
    int n;                /* atoms of a frame as the engine sees it */
    int n_frames;         /* frames of this shard */
    const int32_t *index; /* [n] output atom i is the file's atom index[i]; NULL: i */
    int64_t frame_bytes;  /* the file's stride from frame to frame */
    int x_off;            /* byte of x[0] within a frame */
    int plane_bytes;      /* from x[k] to y[k] to z[k] */
};
template <bool SWAP>
SASA_D void traj_gather_dcd(const TrajDcdArgs &a, const uint32_t *in, double *out, int64_t t)
{
    const int64_t total = 3 * (int64_t)a.n_frames * a.n;
    if (t >= total) return;
    const int64_t atom = t / 3;
    const int comp = (int)(t - 3 * atom);
    const int64_t f = atom / a.n;
    const int i = (int)(atom - f * a.n);
    const int64_t byte = f * a.frame_bytes + a.x_off + (int64_t)comp * a.plane_bytes + 4 * (int64_t)(a.index ? a.index[i] : i);
    uint32_t w = in[byte >> 2];
    if (SWAP) w = (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24);
    float v;
    memcpy(&v, &w, 4);
    out[t] = (double)v;
}

/* traj_gather_nc: the frames of a shard as they lie in an AMBER NetCDF file (netcdf.c has the layout) -> the compact fp64
   frames.  Each frame is one record of record_bytes; from byte coord_off on it holds x, y, z of ALL its atoms as big-endian fp32,
   atom by atom; what else the record holds (time, cell, velocities, forces) no thread reads.  One thread per output coordinate,
   t -> (f, i, comp) as in traj_gather: with the identity index (index NULL) consecutive lanes read consecutive words and write
   consecutive doubles.  Every offset is a multiple of 4 and in general not of 8 (37 atoms without a time variable: records of
   444 bytes): 4-byte loads only, `in` is the shard's bytes as 32-bit words.  The file is always big-endian: the swap is not a
   template flag.  This is traj_gather AND the widening for NetCDF input. */
struct TrajNcArgs {
    int n;                /* atoms of a frame as the engine sees it */
    int n_frames;         /* frames of this shard */
    const int32_t *index; /* [n] output atom i is the file's atom index[i]; NULL: i */
    int64_t record_bytes; /* the file's stride from frame to frame */
    int64_t coord_off;    /* byte of atom 0's x within a record */
};
SASA_D void traj_gather_nc(const TrajNcArgs &a, const uint32_t *in, double *out, int64_t t)
{
    const int64_t total = 3 * (int64_t)a.n_frames * a.n;
    if (t >= total) return;
    const int64_t atom = t / 3;
    const int comp = (int)(t - 3 * atom);
    const int64_t f = atom / a.n;
    const int i = (int)(atom - f * a.n);
    const int64_t byte = f * a.record_bytes + a.coord_off + 12 * (int64_t)(a.index ? a.index[i] : i) + 4 * comp;
    uint32_t w = in[byte >> 2];
    w = (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24);
    float v;
    memcpy(&v, &w, 4);
    out[t] = (double)v;
}

/* traj_gather_trr: the frames of a shard as they lie in a GROMACS TRR file (trr.c has the layout) -> the compact fp64 frames.
   Records have no common stride and some hold no coordinates: x_off[f] is the byte of frame f's x[0] within the shard, made
   on the host from the checked headers; from there x, y, z of ALL the frame's atoms lie atom by atom as big-endian reals in
   nm.  One thread per output coordinate, t -> (f, i, comp) as in traj_gather: with the identity index (index NULL)
   consecutive lanes read consecutive reals and write consecutive doubles.  Every offset is a multiple of 4 and in general
   not of 8 (x[0] of a double record with a box: byte 164): 4-byte loads only, `in` is the shard's bytes as 32-bit words - a
   double is two of them, the high word first.  DOUBLE: the file's precision - a build of its own, not a branch per lane.
   out = (double) real * 10.0 (nm to Angstrom): exact for a float, one rounding for a double, so both precisions give the
   frames of a raw fp64 file that holds (double) x_nm * 10.0.  This is traj_gather AND the widening for TRR input. */
struct TrajTrrArgs {
    int n;                /* atoms of a frame as the engine sees it */
    int n_frames;         /* frames of this shard */
    const int32_t *index; /* [n] output atom i is the file's atom index[i]; NULL: i */
    const int64_t *x_off; /* [n_frames] byte of x[0] of every frame within the shard (a multiple of 4) */
};
SASA_D uint32_t traj_bswap32(uint32_t w) { return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24); }
template <bool DOUBLE>
SASA_D void traj_gather_trr(const TrajTrrArgs &a, const uint32_t *in, double *out, int64_t t)
{
    const int64_t total = 3 * (int64_t)a.n_frames * a.n;
    if (t >= total) return;
    const int64_t atom = t / 3;
    const int comp = (int)(t - 3 * atom);
    const int64_t f = atom / a.n;
    const int i = (int)(atom - f * a.n);
    const int64_t real = 3 * (int64_t)(a.index ? a.index[i] : i) + comp; /* of the frame's x[] */
    const int64_t word = (a.x_off[f] >> 2) + (DOUBLE ? 2 * real : real);
    const uint32_t hi = traj_bswap32(in[word]);
    double v;
    if (DOUBLE) {
        const uint64_t u = ((uint64_t)hi << 32) | traj_bswap32(in[word + 1]);
        memcpy(&v, &u, 8);
    } else {
        float s;
        memcpy(&s, &hi, 4);
        v = (double)s;
    }
    out[t] = v * 10.0;
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

/* ------------------------------------------------------------------ chain groups per frame
 * (freesasa_gpu_trajectory_groups / _trajectory_file_groups): every frame in its complex and every group of it cut out as a
 * structure of its own, in ONE batch per shard.  The topology's cut into its groups is the same for every frame: the host
 * makes it once per run (traj_group_cut: src, gfirst), a lane uploads src once.  The combined batch of a shard of nf frames:
 *
 *     atoms  [0, nf n)                          the nf complex frames, where the plain path has them
 *            nf n + f n_iso + gfirst[g] ...     the isolated structure of group g of frame f: its atoms in input order
 *     structures  f < nf: frame f;  nf + f G + g: group g of frame f
 *
 * which is, structure for structure and atom for atom, the combined batch freesasa_gpu_groups_dev (group_kernels.h) makes of
 * the nf frames given as a batch of nf structures with the ids repeated - so the engine's areas and totals, the totals
 * kernels over cgath (the same chunk tables) and the columns below are that entry's, bit for bit.  No float atomics. */

struct TrajGroupArgs {
    int n, n_iso, n_groups;   /* atoms of the topology, those of them with an id >= 0, groups */
    int n_frames;             /* frames of this shard */
    const int32_t *group;     /* [n] group id of every atom of the topology, -1: in no group */
    const int32_t *src;       /* [n_iso] topology atom of every isolated atom: group-major, input order within a group */
    const double *radii;      /* [n] the topology's radii */
    double *xyz;              /* [3 n_frames (n + n_iso)] the combined batch: the compact frames first (gather: in and out) */
    double *cradii;           /* [n_frames (n + n_iso)] its per-atom radii */
    const double *csasa;      /* [n_frames (n + n_iso)] its areas */
    double *cgath;            /* [n_frames (n + n_iso)] the complex area of every combined atom */
    double *iso;              /* [n_frames n] every atom's area in its isolated group, frame-major input order; or null */
    const double *ctot, *ctot2; /* [n_frames (1 + n_groups)] per combined structure: over csasa (the engine's), over cgath */
    double *out;              /* [n_frames n_groups 3] isolated, complex, buried */
};

/* The cut, on the host, once per run: gfirst [n_groups + 1] (prefix of the groups' atom counts) and src [atoms with an id
   >= 0] - the order grp_rank_struct (group_kernels.h) produces for a one-structure batch.  Returns n_iso, or -1 with the first
   atom whose id is < -1 or >= n_groups in *bad_atom. */
inline int64_t traj_group_cut(const int32_t *group, int64_t n, int n_groups, int64_t *gfirst, int32_t *src, int64_t *bad_atom)
{
    for (int g = 0; g <= n_groups; ++g) gfirst[g] = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (group[i] < -1 || group[i] >= n_groups) { *bad_atom = i; return -1; }
        if (group[i] >= 0) ++gfirst[group[i] + 1];
    }
    for (int g = 0; g < n_groups; ++g) gfirst[g + 1] += gfirst[g];
    for (int64_t i = 0; i < n; ++i)
        if (group[i] >= 0) src[gfirst[group[i]]++] = (int32_t)i; /* (gfirst[g] runs up to gfirst[g + 1] ...) */
    for (int g = n_groups; g > 0; --g) gfirst[g] = gfirst[g - 1]; /* (... and is put back) */
    gfirst[0] = 0;
    return gfirst[n_groups];
}

/* traj_group_radii, one thread per combined atom: n_frames copies of the n radii, then n_frames copies of the n_iso permuted
   ones.  Once per lane and shard length: the radii do not change over the run. */
SASA_D void traj_group_radii(const TrajGroupArgs &a, int64_t t)
{
    const int64_t nc = (int64_t)a.n_frames * a.n;
    if (t < nc) a.cradii[t] = a.radii[t % a.n];
    else if (t < nc + (int64_t)a.n_frames * a.n_iso) a.cradii[t] = a.radii[a.src[(t - nc) % a.n_iso]];
}

/* traj_group_gather, one thread per COORDINATE of the isolated part (3 n_frames n_iso): consecutive lanes write consecutive
   doubles behind the compact frames and read them through src (three lanes share an atom). */
SASA_D void traj_group_gather(const TrajGroupArgs &a, int64_t t)
{
    if (t >= 3 * (int64_t)a.n_frames * a.n_iso) return;
    const int64_t atom = t / 3;
    const int comp = (int)(t - 3 * atom);
    const int64_t f = atom / a.n_iso;
    const int j = (int)(atom - f * a.n_iso);
    a.xyz[3 * (int64_t)a.n_frames * a.n + t] = a.xyz[3 * (f * a.n + a.src[j]) + comp];
}

/* traj_group_finish, one thread per combined atom: grp_finish_atom with the frame arithmetic (the complex areas stay where the
   engine wrote them: the driver reads csasa[f n + i]). */
SASA_D void traj_group_finish(const TrajGroupArgs &a, int64_t t)
{
    const int64_t nc = (int64_t)a.n_frames * a.n;
    if (t < nc) {
        const double v = a.csasa[t];
        a.cgath[t] = v;
        if (a.iso && a.group[t % a.n] < 0) a.iso[t] = v;
    } else if (t < nc + (int64_t)a.n_frames * a.n_iso) {
        const int64_t q = t - nc, f = q / a.n_iso;
        const int64_t i = f * a.n + a.src[q - f * a.n_iso];
        if (a.iso) a.iso[i] = a.csasa[t];
        a.cgath[t] = a.csasa[i];
    }
}

/* traj_group_totals, one thread per (frame, group): grp_totals_item's three columns */
SASA_D void traj_group_totals(const TrajGroupArgs &a, int64_t t)
{
    if (t >= (int64_t)a.n_frames * a.n_groups) return;
    const double t0 = a.ctot[a.n_frames + t], t1 = a.ctot2[a.n_frames + t];
    a.out[3 * t] = t0;
    a.out[3 * t + 1] = t1;
    a.out[3 * t + 2] = t0 - t1;
}

/* ------------------------------------------------------------------ interfaces between chain groups per frame
 * (freesasa_gpu_trajectory_interfaces / _trajectory_file_interfaces): the groups' run with, behind the isolated structures, the
 * PAIR STRUCTURE of every pair (g, h) the caller names, g < h - group g's atoms in input order, then group h's - of every frame.
 * The pairs are the same for every frame: the host makes pfirst, pside and psrc once per run (traj_pair_cut), a lane uploads
 * them once.  The combined batch of a shard of nf frames, with n_pair = the sum over the pairs of |g| + |h|:
 *
 *     atoms  [0, nf n)                                   the nf complex frames                            } as the groups'
 *            nf n + f n_iso + gfirst[g] ...              the isolated structure of group g of frame f     } run has them
 *            nf (n + n_iso) + f n_pair + pfirst[k] ...   the pair structure of pair k of frame f: side g, then side h
 *     structures  f | nf + f G + g | nf (1 + G) + f K + k
 *
 * There is no contact screen: a pair that does not touch in a frame has its structure and its row all the same.  Behind the
 * engine a side's area in the pair is the sum of its atoms' areas in the order of totals_phase0 / totals_phase1 (k_totals over
 * the 2 K nf sides, which are consecutive in the batch: side_off), whatever the side's size; the row of (frame, pair) is the
 * six doubles of iface_finish_row (iface_kernels.h).  No float atomics, no workgroup waits for another. */

struct TrajPairArgs {
    int n, n_iso, n_pair;     /* atoms of the topology, of a frame's isolated structures, of a frame's pair structures */
    int n_groups, n_pairs;    /* G, K */
    int n_frames;             /* frames of this shard */
    const int32_t *pairs;     /* [2 K] g, h of every pair */
    const int64_t *pside;     /* [2 K + 1] where every side begins within a frame's pair part: pside[2 k] = pfirst[k] */
    const int32_t *psrc;      /* [n_pair] topology atom of every pair-structure atom */
    const double *radii;      /* [n] the topology's radii */
    double *xyz;              /* [3 n_frames (n + n_iso + n_pair)] the combined batch: the compact frames first (gather: in and out) */
    double *cradii;           /* [n_frames (n + n_iso + n_pair)] its per-atom radii */
    int64_t *side_off;        /* [2 K n_frames + 1] where every side of the shard begins in the combined batch */
    const double *ctot;       /* [n_frames (1 + G + K)] the engine's totals per combined structure */
    const double *inpair;     /* [2 K n_frames] every side's area in its pair structure */
    double *out;              /* [n_frames K 6] iso_g, iso_h, in_pair_g, in_pair_h, buried_g, buried_h */
};

/* The pairs' cut, on the host, once per run, from the groups' (traj_group_cut): pfirst [K + 1] (prefix of the pair structures'
   atom counts), pside [2 K + 1] (every side's begin, pside[2 K] = n_pair) and psrc [n_pair].  Returns n_pair.  The pairs are
   checked by the caller (0 <= g < h < G). */
inline int64_t traj_pair_cut(const int32_t *pairs, int n_pairs, const int64_t *gfirst, const int32_t *src, int64_t *pfirst, int64_t *pside,
                             int32_t *psrc)
{
    int64_t m = 0;
    for (int k = 0; k < n_pairs; ++k) {
        pfirst[k] = m;
        for (int q = 0; q < 2; ++q) {
            const int g = pairs[2 * k + q];
            pside[2 * k + q] = m;
            for (int64_t j = gfirst[g]; j < gfirst[g + 1]; ++j) {
                if (psrc) psrc[m] = src[j];
                ++m;
            }
        }
    }
    pfirst[n_pairs] = pside[2 * n_pairs] = m;
    return m;
}

/* traj_pair_radii, one thread per pair-structure atom of the shard: n_frames copies of the n_pair permuted radii behind the
   groups' part.  Once per lane and shard length, like traj_group_radii. */
SASA_D void traj_pair_radii(const TrajPairArgs &a, int64_t t)
{
    if (t >= (int64_t)a.n_frames * a.n_pair) return;
    a.cradii[(int64_t)a.n_frames * ((int64_t)a.n + a.n_iso) + t] = a.radii[a.psrc[t % a.n_pair]];
}

/* traj_pair_sides, one thread per boundary (2 K n_frames + 1): side j of frame f begins at nf (n + n_iso) + f n_pair + pside[j];
   the last boundary is f = n_frames, j = 0.  Once per lane and shard length, with the radii. */
SASA_D void traj_pair_sides(const TrajPairArgs &a, int64_t t)
{
    const int64_t per = 2 * (int64_t)a.n_pairs;
    if (t > per * a.n_frames) return;
    const int64_t f = t / per;
    a.side_off[t] = (int64_t)a.n_frames * ((int64_t)a.n + a.n_iso) + f * a.n_pair + a.pside[t - f * per];
}

/* traj_pair_gather, one thread per COORDINATE of the pair part (3 n_frames n_pair): consecutive lanes write consecutive doubles
   behind the isolated structures and read the compact frames through psrc (three lanes share an atom): traj_group_gather's shape. */
SASA_D void traj_pair_gather(const TrajPairArgs &a, int64_t t)
{
    if (t >= 3 * (int64_t)a.n_frames * a.n_pair) return;
    const int64_t atom = t / 3;
    const int comp = (int)(t - 3 * atom);
    const int64_t f = atom / a.n_pair;
    const int j = (int)(atom - f * a.n_pair);
    a.xyz[3 * (int64_t)a.n_frames * ((int64_t)a.n + a.n_iso) + t] = a.xyz[3 * (f * a.n + a.psrc[j]) + comp];
}

/* traj_pair_rows, one thread per (frame, pair): iface_finish_row's six doubles - the isolated totals are the engine's totals of
   the frame's isolated structures (column 0 of the groups' output), buried = isolated - in the pair, one subtraction */
SASA_D void traj_pair_rows(const TrajPairArgs &a, int64_t t)
{
    if (t >= (int64_t)a.n_frames * a.n_pairs) return;
    const int64_t f = t / a.n_pairs;
    const int k = (int)(t - f * a.n_pairs);
    const double *iso = a.ctot + a.n_frames + f * a.n_groups;
    const double ig = iso[a.pairs[2 * k]], ih = iso[a.pairs[2 * k + 1]];
    const double pg = a.inpair[2 * t], ph = a.inpair[2 * t + 1];
    double *o = a.out + 6 * t;
    o[0] = ig; o[1] = ih; o[2] = pg; o[3] = ph; o[4] = ig - pg; o[5] = ih - ph;
}

/* ------------------------------------------------------------------ per-residue interface tables per frame
 * (freesasa_gpu_trajectory_interface_residues / _trajectory_file_interface_residues): the interfaces' run with, per frame, a
 * DENSE table [S, 4].  A SEGMENT is a maximal run of consecutive atoms of ONE side of a frame's pair part whose topology atoms
 * lie in one residue: a head at every side's begin and wherever the residue changes.  Empty residues are never found, a residue
 * split over two groups gives a segment on each side it occurs on, atoms in no group are in no side, an empty side has no
 * segment, and a group named in several pairs has its residues once per pair.  The segments are the same for every frame: the
 * host makes them once per run (traj_pair_res_cut), a lane uploads seg_first and seg_iso once.  Per frame f and segment s, over
 * the pair-part positions m in [seg_first[s], seg_first[s + 1]):
 *
 *     iso_res       the sum of the engine's areas of those atoms in their ISOLATED group of frame f - a side of group g lies
 *                   there in the same order, so the segment is contiguous from seg_iso[s] = gfirst[g] + (seg_first[s] - pside[side])
 *     in_pair_res   the sum of the engine's areas of the pair-structure atoms m of frame f
 *     buried_res    iso_res - in_pair_res, one subtraction
 *     in_interface  1.0 if buried_res > min_buried (strict), else 0.0 - its mean over a run is the residue's OCCUPANCY
 *
 * Both sums are taken one addition at a time in atom order from 0.0; there is no fma (contraction is off in the function
 * itself, as in traj_stats).  No float atomics, no workgroup waits for another, no LDS. */

struct TrajPairResArgs {
    int n, n_iso, n_pair;     /* atoms of the topology, of a frame's isolated structures, of a frame's pair structures */
    int n_seg;                /* S */
    int n_frames;             /* frames of this shard */
    const int64_t *seg_first; /* [S + 1] every segment's begin within a frame's pair part; seg_first[S] = n_pair */
    const int64_t *seg_iso;   /* [S] its first atom's place within a frame's isolated part */
    const double *csasa;      /* [n_frames (n + n_iso + n_pair)] the combined batch's areas */
    double min_buried;
    double *out;              /* [n_frames S 4] iso_res, in_pair_res, buried_res, in_interface */
};

/* The segments, on the host, once per run, behind traj_pair_cut: seg_first [S + 1], seg_res [S] (the residue, counted within the
   structure), seg_side [S] (0 .. 2 K - 1) and seg_iso [S]; any of them may be NULL (a first call counts).  res_first [n_res + 1]
   is the structure's, rebased to it.  An atom's residue is the last r < n_res with res_first[r] <= atom: within a side the
   topology atoms ascend (input order), so r only walks forward.  Returns S (<= n_pair). */
inline int64_t traj_pair_res_cut(const int32_t *pairs, int n_pairs, const int64_t *gfirst, const int64_t *pside, const int32_t *psrc,
                                 const int64_t *res_first, int64_t n_res, int64_t *seg_first, int32_t *seg_res, int32_t *seg_side, int64_t *seg_iso)
{
    int64_t S = 0;
    for (int j = 0; j < 2 * n_pairs; ++j) {
        int64_t r = 0, last = -1;
        for (int64_t m = pside[j]; m < pside[j + 1]; ++m) {
            while (r + 1 < n_res && res_first[r + 1] <= psrc[m]) ++r;
            if (m == pside[j] || r != last) {
                if (seg_first) seg_first[S] = m;
                if (seg_res) seg_res[S] = (int32_t)r;
                if (seg_side) seg_side[S] = j;
                if (seg_iso) seg_iso[S] = gfirst[pairs[j]] + (m - pside[j]);
                ++S;
            }
            last = r;
        }
    }
    if (seg_first) seg_first[S] = pside[2 * n_pairs];
    return S;
}

#define TRAJ_PRES_U 8 /* atoms a thread loads ahead of its additions */

/* traj_pair_res, one thread per (frame, segment), as traj_residue has one per (frame, residue): consecutive lanes take consecutive
   segments of one frame, whose atoms lie one behind the other in both parts, and write consecutive rows.  The order of the
   additions is the definition, so a segment is never split over lanes; what keeps a LONG segment (a chain under one residue
   label, a lipid) from costing its length in memory latencies is that TRAJ_PRES_U atoms of both parts are loaded before the first
   of them is added - sixteen loads of a thread are in flight together, the additions stay in atom order (traj_stats does the same
   with its frames). */
SASA_D void traj_pair_res(const TrajPairResArgs &a, int64_t t)
{
#ifndef SASA_EMU
#pragma clang fp contract(off) /* (the emulation is built with -ffp-contract=off; so is the library - this holds whatever the flags) */
#endif
    if (t >= (int64_t)a.n_frames * a.n_seg) return;
    const int64_t f = t / a.n_seg;
    const int64_t s = t - f * a.n_seg;
    const int64_t b = a.seg_first[s], len = a.seg_first[s + 1] - b;
    const double *iso = a.csasa + (int64_t)a.n_frames * a.n + f * a.n_iso + a.seg_iso[s];
    const double *pr = a.csasa + (int64_t)a.n_frames * ((int64_t)a.n + a.n_iso) + f * a.n_pair + b;
    double si = 0.0, sp = 0.0;
    int64_t m = 0;
    for (; m + TRAJ_PRES_U <= len; m += TRAJ_PRES_U) {
        double vi[TRAJ_PRES_U], vp[TRAJ_PRES_U];
        for (int q = 0; q < TRAJ_PRES_U; ++q) { vi[q] = iso[m + q]; vp[q] = pr[m + q]; }
        for (int q = 0; q < TRAJ_PRES_U; ++q) { si += vi[q]; sp += vp[q]; }
    }
    for (; m < len; ++m) { si += iso[m]; sp += pr[m]; }
    const double buried = si - sp;
    double *o = a.out + 4 * t;
    o[0] = si; o[1] = sp; o[2] = buried; o[3] = buried > a.min_buried ? 1.0 : 0.0;
}

/* ------------------------------------------------------------------ run statistics
 * (freesasa_gpu_trajectory_stats and its kin, include/freesasa_gpu.h): a shard's PARTIAL of every output statistics are asked
 * for - per column of the output's block a[n_frames][width] of fp64 the mean, M2 = sum (a - mean)^2, the smallest and the
 * largest value.  The blocks are where the kernels before this one wrote them; a small table of segments says which block a
 * column of the partial belongs to.  One thread per column, ONE launch per shard: consecutive lanes take consecutive columns,
 * so every frame's row is read coalesced; the frame loop is serial in the thread, because its order is the definition - the
 * frames of a column are never split over lanes, and the second pass re-reads the block (a shard's areas were just written).
 * Every operation is rounded on its own: the square is a multiplication of its own, never fused into the add (contraction is
 * switched off in the function itself). */

#define TRAJ_STAT_SEGS 9 /* the drivers' table of outputs has nine rows with statistics */
#define TRAJ_STAT_U 8    /* rows a thread loads ahead of its additions */
struct TrajStatSeg {
    const double *src;    /* the output's block [n_frames][width] */
    int64_t width, first; /* ... and its first column of the partial */
};
struct TrajStatsArgs {
    int n_frames;   /* frames of this shard */
    int n_seg;
    int64_t W;      /* columns of the partial: the sum of the segments' widths */
    TrajStatSeg seg[TRAJ_STAT_SEGS];
    double *out;    /* [4][W]: mean, M2, min, max */
};

SASA_D void traj_stats(const TrajStatsArgs &a, int64_t t)
{
#ifndef SASA_EMU
#pragma clang fp contract(off) /* (the emulation is built with -ffp-contract=off; so is the library - this holds whatever the flags) */
#endif
    if (t >= a.W) return;
    int k = 0;
    while (k + 1 < a.n_seg && t >= a.seg[k + 1].first) ++k;
    const int64_t w = a.seg[k].width;
    const double *col = a.seg[k].src + (t - a.seg[k].first);
    /* TRAJ_STAT_U rows are loaded before the first of them is added: the loads of a thread are in flight together (a load per
       add would wait out the memory's latency n_frames times), the additions stay in frame order */
    const int nf = a.n_frames;
    double s = 0, lo = col[0], hi = col[0];
    int f = 0;
    for (; f + TRAJ_STAT_U <= nf; f += TRAJ_STAT_U) {
        double v[TRAJ_STAT_U];
        for (int q = 0; q < TRAJ_STAT_U; ++q) v[q] = col[(int64_t)(f + q) * w];
        for (int q = 0; q < TRAJ_STAT_U; ++q) {
            s += v[q];
            lo = v[q] < lo ? v[q] : lo;
            hi = v[q] > hi ? v[q] : hi;
        }
    }
    for (; f < nf; ++f) {
        const double v = col[(int64_t)f * w];
        s += v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    const double mean = s / (double)nf;
    double m2 = 0;
    for (f = 0; f + TRAJ_STAT_U <= nf; f += TRAJ_STAT_U) {
        double v[TRAJ_STAT_U];
        for (int q = 0; q < TRAJ_STAT_U; ++q) v[q] = col[(int64_t)(f + q) * w];
        for (int q = 0; q < TRAJ_STAT_U; ++q) {
            const double d = v[q] - mean;
            const double sq = d * d;
            m2 += sq;
        }
    }
    for (; f < nf; ++f) {
        const double d = col[(int64_t)f * w] - mean;
        const double sq = d * d;
        m2 += sq;
    }
    a.out[t] = mean; a.out[a.W + t] = m2; a.out[2 * a.W + t] = lo; a.out[3 * a.W + t] = hi;
}

} /* namespace sasa */

#endif
