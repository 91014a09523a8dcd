/* TESTS ONLY: the run statistics' phase function (freesasa_amd/csrc/traj_kernels.h, traj_stats) driven thread by thread on the
 * CPU, as k_traj_stats launches it: one thread per column of a shard's partial, over a table of segments.  Never linked into
 * the product. */
#include <stdint.h>
#include <string.h>

#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

/* blocks [n_seg]: block k is [n_frames][width[k]] doubles; out [4][W], W = the sum of the widths.  Returns W, or -1. */
extern "C" long long emu_traj_stats(const double *const *blocks, const long long *width, int n_seg, int n_frames, double *out)
{
    if (!blocks || !width || !out || n_seg < 1 || n_seg > TRAJ_STAT_SEGS || n_frames < 1) return -1;
    TrajStatsArgs a;
    memset(&a, 0, sizeof a);
    a.n_frames = n_frames; a.n_seg = n_seg; a.out = out;
    for (int k = 0; k < n_seg; ++k) {
        if (!blocks[k] || width[k] < 1) return -1;
        a.seg[k].src = blocks[k]; a.seg[k].width = width[k]; a.seg[k].first = a.W;
        a.W += width[k];
    }
    /* whole workgroups of 64, as the launcher's grid: the threads behind the last column must return */
    for (int64_t t = 0; t < (a.W + 63) / 64 * 64; ++t) traj_stats(a, t);
    return a.W;
}
