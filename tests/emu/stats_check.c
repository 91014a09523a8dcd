/* TESTS ONLY: the merge of the run statistics' partials and the layout of a statistics word (freesasa_amd/csrc/trajstats.c) in a
 * stand-alone program, built with AddressSanitizer + UBSan (Makefile, tests/emu/stats_check).  It makes the partials of seeded
 * columns with the two-pass loop of the definition, merges them - shards 3 3 1, one shard, one frame per shard, a sub-range -
 * and holds the result to a two-pass over all frames within 1e-12 relative, the error returns to -1 with `out` untouched and
 * the widths to their sums.  Prints one line per case; exit status 0 when all hold and no sanitizer ends it.  Never linked
 * into the product. */
#include <math.h>
#include <stdio.h>

#include "../../include/freesasa_gpu.h"

#define F 7
#define W 5

static double a[F][W];

static void partial(int f0, int nf, double *p /* [4][W] */)
{
    for (int j = 0; j < W; ++j) {
        double s = 0, lo = a[f0][j], hi = a[f0][j], m2 = 0;
        for (int f = f0; f < f0 + nf; ++f) {
            s += a[f][j];
            if (a[f][j] < lo) lo = a[f][j];
            if (a[f][j] > hi) hi = a[f][j];
        }
        const double mean = s / nf;
        for (int f = f0; f < f0 + nf; ++f) {
            const double d = a[f][j] - mean;
            m2 += d * d;
        }
        p[j] = mean; p[W + j] = m2; p[2 * W + j] = lo; p[3 * W + j] = hi;
    }
}

static int close_to(double got, double want) { return fabs(got - want) <= 1e-12 * fabs(want) + 1e-12; }

/* the merge of the cut against the two-pass loop over frames [f0, f0 + the cut's frames) */
static int check_cut(const char *name, int f0, const long long *cut, int n_parts)
{
    double parts[F][4 * W], out[4 * W], whole[4 * W];
    long long total = 0, frames = 0;
    int at = f0, bad = 0;
    for (int k = 0; k < n_parts; ++k) { partial(at, (int)cut[k], parts[k]); at += (int)cut[k]; total += cut[k]; }
    if (freesasa_gpu_traj_stats_merge(&parts[0][0], cut, n_parts, W, out, &frames) || frames != total) bad = 1;
    partial(f0, (int)total, whole);
    for (int j = 0; j < W && !bad; ++j)
        if (!close_to(out[j], whole[j]) || !close_to(out[W + j], sqrt(whole[W + j] / (double)total)) || out[2 * W + j] != whole[2 * W + j] ||
            out[3 * W + j] != whole[3 * W + j])
            bad = 1;
    printf("%s %s\n", name, bad ? "FAILED" : "ok");
    return bad;
}

int main(void)
{
    unsigned long long x = 20261019ULL;
    for (int f = 0; f < F; ++f)
        for (int j = 0; j < W; ++j) {
            x = x * 6364136223846793005ULL + 1442695040888963407ULL;
            /* column 0 constant, column 1 all zero, the others area-like */
            a[f][j] = j == 0 ? 42.5 : j == 1 ? 0.0 : 50.0 + (double)(x >> 11) / 9007199254740992.0;
        }
    int bad = 0;
    const long long c331[3] = {3, 3, 1}, c7[1] = {7}, c1[7] = {1, 1, 1, 1, 1, 1, 1}, c31[2] = {3, 1};
    bad |= check_cut("shards-3-3-1", 0, c331, 3);
    bad |= check_cut("one-shard", 0, c7, 1);
    bad |= check_cut("one-frame-per-shard", 0, c1, 7);
    bad |= check_cut("sub-range-1-3", 3, c31, 2);
    {   /* a constant column: std exactly 0, min == max == mean */
        double parts[3][4 * W], out[4 * W];
        partial(0, 3, parts[0]); partial(3, 3, parts[1]); partial(6, 1, parts[2]);
        const int rc = freesasa_gpu_traj_stats_merge(&parts[0][0], c331, 3, W, out, NULL);
        const int ok = !rc && out[0] == 42.5 && out[W] == 0.0 && out[2 * W] == 42.5 && out[3 * W] == 42.5 && out[1] == 0.0 && out[W + 1] == 0.0;
        printf("constant-column %s\n", ok ? "ok" : "FAILED");
        bad |= !ok;
    }
    {   /* error returns: out untouched */
        double parts[4 * W] = {0}, out[1] = {-7.0};
        const long long one[1] = {1}, zero[1] = {0};
        const int ok = freesasa_gpu_traj_stats_merge(parts, one, 0, W, out, NULL) == -1 && freesasa_gpu_traj_stats_merge(parts, zero, 1, W, out, NULL) == -1 &&
                       freesasa_gpu_traj_stats_merge(parts, one, 1, 0, out, NULL) == -1 && freesasa_gpu_traj_stats_merge(NULL, one, 1, W, out, NULL) == -1 &&
                       out[0] == -7.0;
        printf("error-returns %s\n", ok ? "ok" : "FAILED");
        bad |= !ok;
    }
    {   /* the layout of a statistics word */
        long long first[7];
        const int ok = freesasa_gpu_traj_stats_width(127, 602, 76, 10, 2, first) == 1 + 602 + 602 + 3 + 456 + 10 + 6 && first[0] == 0 && first[1] == 1 &&
                       first[2] == 603 && first[3] == 1205 && first[4] == 1208 && first[5] == 1664 && first[6] == 1674 &&
                       freesasa_gpu_traj_stats_width(FREESASA_GPU_STATS_ATOMS | FREESASA_GPU_STATS_RESIDUES, 602, 76, 0, 0, first) == 602 + 456 &&
                       first[0] == -1 && first[1] == 0 && first[4] == 602 && freesasa_gpu_traj_stats_width(128, 1, 0, 0, 0, NULL) == -1 &&
                       freesasa_gpu_traj_stats_width(0, 1, 0, 0, 0, NULL) == 0;
        printf("widths %s\n", ok ? "ok" : "FAILED");
        bad |= !ok;
    }
    return bad;
}
