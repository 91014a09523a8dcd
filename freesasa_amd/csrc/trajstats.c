/*
 * trajstats.c — the host side of the trajectory drivers' run statistics (include/freesasa_gpu.h, "RUN STATISTICS"): the
 * layout of a statistics word and the merge of the shards' partials.  Plain C without allocation and without a GPU call,
 * compiled with -ffp-contract=off like all of the library: every operation of the merge is rounded on its own, in the order
 * written - the tests hold it to the same formulas in numpy bit for bit.
 */
#include <math.h>
#include <stddef.h>

#include "../../include/freesasa_gpu.h"

long long freesasa_gpu_traj_stats_width(int stats, long long n_atoms, long long n_res, long long n_sel, long long n_groups,
                                        long long *first_out)
{
    /* the drivers' table of outputs, in its order */
    const int bit[7] = {FREESASA_GPU_STATS_TOTALS, FREESASA_GPU_STATS_ATOMS, FREESASA_GPU_STATS_ISOLATED, FREESASA_GPU_STATS_CLASSES,
                        FREESASA_GPU_STATS_RESIDUES, FREESASA_GPU_STATS_SELECTIONS, FREESASA_GPU_STATS_GROUPS};
    const long long width[7] = {1, n_atoms, n_atoms, 3, 6 * n_res, n_sel, 3 * n_groups};
    long long W = 0;
    if (stats < 0 || stats > 127 || n_atoms < 0 || n_res < 0 || n_sel < 0 || n_groups < 0) return -1;
    for (int k = 0; k < 7; ++k) {
        if (first_out) first_out[k] = stats & bit[k] ? W : -1;
        if (stats & bit[k]) W += width[k];
    }
    return W;
}

/* ... with the two outputs of the interface entries behind the groups: pairs [6 K] | interface residues [4 S] */
long long freesasa_gpu_traj_stats_width_pairs(int stats, long long n_atoms, long long n_res, long long n_sel, long long n_groups,
                                              long long n_pairs, long long n_segments, long long *first_out)
{
    const int bit[9] = {FREESASA_GPU_STATS_TOTALS, FREESASA_GPU_STATS_ATOMS, FREESASA_GPU_STATS_ISOLATED, FREESASA_GPU_STATS_CLASSES,
                        FREESASA_GPU_STATS_RESIDUES, FREESASA_GPU_STATS_SELECTIONS, FREESASA_GPU_STATS_GROUPS, FREESASA_GPU_STATS_PAIRS,
                        FREESASA_GPU_STATS_PAIR_RESIDUES};
    const long long width[9] = {1, n_atoms, n_atoms, 3, 6 * n_res, n_sel, 3 * n_groups, 6 * n_pairs, 4 * n_segments};
    long long W = 0;
    if (stats < 0 || stats > 511 || n_atoms < 0 || n_res < 0 || n_sel < 0 || n_groups < 0 || n_pairs < 0 || n_segments < 0) return -1;
    for (int k = 0; k < 9; ++k) {
        if (first_out) first_out[k] = stats & bit[k] ? W : -1;
        if (stats & bit[k]) W += width[k];
    }
    return W;
}

int freesasa_gpu_traj_stats_merge(const double *parts, const long long *frames_per_part, long long n_parts, long long width,
                                  double *out, long long *frames_total_out)
{
    if (!parts || !frames_per_part || !out || n_parts < 1 || width < 1) return -1;
    for (long long k = 0; k < n_parts; ++k)
        if (frames_per_part[k] < 1) return -1;
    const size_t W = (size_t)width;
    double *mean = out, *m2 = out + W, *lo = out + 2 * W, *hi = out + 3 * W;
    for (size_t q = 0; q < 4 * W; ++q) out[q] = parts[q];
    long long n = frames_per_part[0];
    for (long long k = 1; k < n_parts; ++k) {
        const double *b = parts + 4 * W * (size_t)k;
        const long long nb = frames_per_part[k], t = n + nb;
        const double r = (double)nb / (double)t, w = (double)n * r;
        for (size_t j = 0; j < W; ++j) {
            const double d = b[j] - mean[j];
            mean[j] += d * r;
            m2[j] = (m2[j] + b[W + j]) + (d * d) * w;
            if (b[2 * W + j] < lo[j]) lo[j] = b[2 * W + j];
            if (b[3 * W + j] > hi[j]) hi[j] = b[3 * W + j];
        }
        n = t;
    }
    for (size_t j = 0; j < W; ++j) m2[j] = sqrt(m2[j] / (double)n);
    if (frames_total_out) *frames_total_out = n;
    return 0;
}
