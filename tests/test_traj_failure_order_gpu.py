"""Which failure a trajectory run reports (gpu_drivers.hip, TrajRun::shard_failed): the failure of its LOWEST failed shard, however
its lanes are scheduled.  A DCD file whose every cell record is triclinic, read without the triclinic bit, is refused in every
shard - always "at frame 0", with one lane, with three, and with a shard per frame."""
import numpy as np
import pytest

import freesasa_amd as fa
from test_dcd import write_dcd
from test_dcd_gpu import coil  # noqa: F401 (fixture)
from test_pbc_tri_gpu import frame_records, patch_records

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("devices, fpb", [([0], 2), ([0, 0, 0], 1), ([0, 0, 0], 2)])
def test_a_file_refused_in_every_shard_is_refused_at_frame_0(coil, tmp_path, devices, fpb):
    frames, radii = coil
    dcd = tmp_path / "frames.dcd"
    write_dcd(dcd, frames, cell=True)
    patch_records(dcd, frame_records(True))
    for k in range(8):                  # (eight runs: with "whichever lane fails first" a later shard's frame came up by chance)
        with pytest.raises(RuntimeError, match="frame 0 of the DCD file") as e:
            fa.trajectory_file(dcd, radii, str(tmp_path / "t"), str(tmp_path / "s"), done_path=str(tmp_path / f"done{k}"), alg=fa.SHRAKE_RUPLEY,
                               resolution=100, frames_per_batch=fpb, dcd=True, pbc=True, devices=devices)
        assert "orthorhombic" in str(e.value)
