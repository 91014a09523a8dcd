/* TESTS ONLY: traj_gather_trr (freesasa_amd/csrc/traj_kernels.h) driven thread by thread on the CPU, in the launch shape of
 * kl_traj_gather_trr (gpu_kernels.hip): workgroups of TRAJ_B threads over 3 * n_frames * n output coordinates.  `shard`: the
 * bytes of a run of whole records; the table of x_off is made from their headers by trr.c, as the driver makes it
 * (gpu_frames.hip, trr_descriptors).  Never linked into the product. */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "freesasa_gpu.h"
#include "freesasa_ingest.h"
#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

/* -> the number of records with coordinates among the `bytes` bytes at shard (their frames into out[frames][n][3], as far as
   max_frames reaches), -1: a bad argument, -2: a header that trr.c refuses */
extern "C" long long emu_traj_gather_trr(const void *shard, long long bytes, const int32_t *index, int n, long long max_frames, double *out)
{
    if (!shard || !out || n < 1 || bytes < 1 || ((uintptr_t)shard & 3)) return -1;
    std::vector<int64_t> x_off;
    int n_atoms = 0, real_bytes = 0;
    for (long long at = 0; at < bytes;) {
        freesasa_gpu_trr_record r;
        if (freesasa_gpu_trr_frame_desc((const char *)shard + at, bytes - at, n_atoms, real_bytes, at, &r, nullptr, 0)) return -2;
        n_atoms = r.n_atoms; real_bytes = r.real_bytes;
        if (r.has_x) x_off.push_back(r.x_off);
        at += r.record_bytes;
    }
    if (x_off.empty() || (long long)x_off.size() > max_frames) return (long long)x_off.size();
    if (index) {
        for (int i = 0; i < n; ++i)
            if (index[i] < 0 || index[i] >= n_atoms) return -1;
    } else if (n != n_atoms) return -1;
    const TrajTrrArgs a = {n, (int)x_off.size(), index, x_off.data()};
    const int64_t blocks = (3 * (int64_t)a.n_frames * n + TRAJ_B - 1) / TRAJ_B;
    for (int64_t blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < TRAJ_B; ++t) {
            if (real_bytes == 8) traj_gather_trr<true>(a, (const uint32_t *)shard, out, blk * TRAJ_B + t);
            else traj_gather_trr<false>(a, (const uint32_t *)shard, out, blk * TRAJ_B + t);
        }
    return (long long)x_off.size();
}
