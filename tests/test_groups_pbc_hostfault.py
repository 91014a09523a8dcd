"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through chain groups among periodic images: the
n-th host allocation of the four batch entries and of the file entry fails, n = 1, 2, ...; every call fails with -1 and a message
or succeeds with the un-faulted bytes, and the call after the walk gives them bit for bit."""
import os

import numpy as np
import pytest

import freesasa_amd as fa
import groups_pbc_ref as gr
from freesasa_amd import ingest
from test_dcd import write_dcd
from test_hostfault import walk
from test_pbc_gpu import patch_cells

pytestmark = pytest.mark.gpu


def _bytes(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got)


def _walk(run):
    want = _bytes(run())

    def call():
        try:
            got = run()
        except RuntimeError as e:
            return False, str(e).split(": ", 1)[1]
        assert _bytes(got) == want
        return True, ""

    fired, failed = walk(call)
    assert _bytes(run()) == want
    return fired, failed


@pytest.mark.parametrize("tri", [False, True])
def test_the_host_array_entries_survive_every_allocation_failing(tri):
    xyz, radii, offsets, group, n_groups, cells = gr.batch()
    if tri:
        cells = gr.triclinic_cells(cells)
    entry = fa.calc_groups_periodic_triclinic if tri else fa.calc_groups_periodic
    fired, failed = _walk(lambda: entry(xyz, radii, offsets, group, n_groups, cells, probe=gr.PROBE))
    assert fired >= 5 and failed >= 5, (fired, failed)      # the offsets and bases, the counts, the combined offsets, the cells' checks, the engine's own


@pytest.mark.parametrize("tri", [False, True])
def test_the_device_pointer_entries_survive_every_allocation_failing(tri):
    import torch
    xyz, radii, offsets, group, n_groups, cells = gr.batch()
    if tri:
        cells = gr.triclinic_cells(cells)
    dev = torch.device("cuda:0")
    n, G = len(radii), int(n_groups.sum())
    d_xyz, d_r, d_g = torch.from_numpy(xyz).to(dev), torch.from_numpy(radii).to(dev), torch.from_numpy(group).to(dev)
    d_sasa, d_iso = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    d_tot, d_gt = torch.empty(5, dtype=torch.float64, device=dev), torch.empty(3 * G, dtype=torch.float64, device=dev)
    ctx = fa.GpuContext(0)

    def run():
        entry = ctx.groups_periodic_triclinic if tri else ctx.groups_periodic
        images = entry(d_xyz.data_ptr(), d_r.data_ptr(), offsets, d_g.data_ptr(), n_groups, cells, d_sasa.data_ptr(), d_iso.data_ptr(),
                       d_tot.data_ptr(), d_gt.data_ptr(), probe=gr.PROBE)
        return d_sasa.cpu().numpy(), d_iso.cpu().numpy(), d_tot.cpu().numpy(), d_gt.cpu().numpy(), images

    try:
        fired, failed = _walk(run)
    finally:
        ctx.close()
    assert fired >= 5 and failed >= 5, (fired, failed)


def test_the_file_entry_survives_every_allocation_failing(tmp_path):
    b = ingest.load_pdb_files([os.path.join(gr.PDB, "2jo4.pdb")])
    ids = np.asarray(b.chain_groups(separate_chains=True)[0], dtype=np.int32)
    x0 = np.asarray(b.xyz, dtype=np.float64).reshape(-1, 3)
    rng = np.random.default_rng(3)
    frames = (x0[None] + rng.uniform(-0.3, 0.3, (3,) + x0.shape)).astype(np.float32)
    ext = np.ceil(x0.max(0) - x0.min(0)) + 6.0
    path = tmp_path / "frames.dcd"
    write_dcd(path, frames, cell=True)
    patch_cells(path, [tuple(float(v) for v in ext)] * 3)
    p = {k: str(tmp_path / k) for k in ("totals", "sasa", "iso", "groups")}

    def run():
        done, n_frames, _ = fa.trajectory_file_groups_periodic(path, b, p["totals"], sasa_path=p["sasa"], group=ids, n_groups=4,
                                                               group_areas_path=p["groups"], isolated_path=p["iso"], frames_per_batch=2,
                                                               dcd=True, probe=gr.PROBE, devices=[0])
        assert done and n_frames == 3
        return [np.fromfile(p[k], dtype=np.uint8) for k in p]

    fired, failed = _walk(run)
    assert fired >= 5 and failed >= 5, (fired, failed)
