/* TESTS ONLY: traj_gather_nc (freesasa_amd/csrc/traj_kernels.h) driven thread by thread on the CPU, in the launch shape of
 * kl_traj_gather_nc (gpu_kernels.hip): workgroups of TRAJ_B threads over 3 * n_frames * n output coordinates.  `records`: the
 * bytes of the file from its first record on.  Never linked into the product. */
#include <stdint.h>
#include <string.h>

#include "freesasa_ingest.h"
#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

extern "C" int emu_traj_gather_nc(const void *records, int n_frames, long long record_bytes, long long coord_off, const int32_t *index, int n, double *out)
{
    if (!records || !out || n < 1 || n_frames < 1 || ((uintptr_t)records & 3) || (record_bytes & 3) || (coord_off & 3)) return -1;
    const TrajNcArgs a = {n, n_frames, index, (int64_t)record_bytes, (int64_t)coord_off};
    const int64_t blocks = (3 * (int64_t)n_frames * n + TRAJ_B - 1) / TRAJ_B;
    for (int64_t blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < TRAJ_B; ++t) traj_gather_nc(a, (const uint32_t *)records, out, blk * TRAJ_B + t);
    return 0;
}
