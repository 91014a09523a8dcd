/* TESTS ONLY: traj_gather_dcd (freesasa_amd/csrc/traj_kernels.h) driven thread by thread on the CPU, in the launch shape of
 * kl_traj_gather_dcd (gpu_kernels.hip): workgroups of TRAJ_B threads over 3 * n_frames * n output coordinates, the byte-swapping
 * build for a big-endian file.  `frames`: the bytes of the file from its first frame on.  Never linked into the product. */
#include <stdint.h>
#include <string.h>

#include "freesasa_ingest.h"
#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

extern "C" int emu_traj_gather_dcd(const void *frames, int n_frames, long long frame_bytes, int x_off, int plane_bytes, int big_endian,
                                   const int32_t *index, int n, double *out)
{
    if (!frames || !out || n < 1 || n_frames < 1 || ((uintptr_t)frames & 3) || (frame_bytes & 3) || (x_off & 3) || (plane_bytes & 3)) return -1;
    const TrajDcdArgs a = {n, n_frames, index, (int64_t)frame_bytes, x_off, plane_bytes};
    const int64_t blocks = (3 * (int64_t)n_frames * n + TRAJ_B - 1) / TRAJ_B;
    for (int64_t blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < TRAJ_B; ++t) {
            if (big_endian) traj_gather_dcd<true>(a, (const uint32_t *)frames, out, blk * TRAJ_B + t);
            else traj_gather_dcd<false>(a, (const uint32_t *)frames, out, blk * TRAJ_B + t);
        }
    return 0;
}
