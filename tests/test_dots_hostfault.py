"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the mask and dot entries: the n-th host
allocation or thread creation of calc_dots (freesasa_gpu_calc_masks, freesasa_gpu_dots_from_masks) and of
freesasa_gpu_trajectory_masks fails, n = 1, 2, ...; every call fails with a message or succeeds with the un-faulted numbers, and
the call after the walk gives them bit for bit."""
import numpy as np
import pytest

import freesasa_amd as fa
import volume_ref as vr
from test_hostfault import walk
from test_volume_gpu import system  # noqa: F401 (the trajectory tests' topology and frames)

pytestmark = pytest.mark.gpu


def test_calc_dots_survives_every_allocation_failing():
    xyz, radii, offsets = vr.batch()
    want = fa.calc_dots(xyz, radii, offsets, n_points=100, with_index=True)

    def call():
        try:
            got = fa.calc_dots(xyz, radii, offsets, n_points=100, with_index=True)
        except RuntimeError as e:
            return False, str(e)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        return True, ""

    fired, failed = walk(call)
    assert fired >= 1 and failed >= 1, (fired, failed)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fa.calc_dots(xyz, radii, offsets, n_points=100, with_index=True), want))


def test_calc_dots_at_alternating_point_counts_survives_every_allocation_failing():
    """33, 100, 33 points on one pooled context: the expansion's unit points change hands, and their buffer grows, inside the walk"""
    xyz, radii, offsets = vr.batch()
    want = {N: fa.calc_dots(xyz, radii, offsets, n_points=N, with_index=True) for N in (33, 100)}

    def call():
        try:
            got = [(N, fa.calc_dots(xyz, radii, offsets, n_points=N, with_index=True)) for N in (33, 100, 33)]
        except RuntimeError as e:
            return False, str(e)
        assert all(a.tobytes() == b.tobytes() for N, g in got for a, b in zip(g, want[N]))
        return True, ""

    fired, failed = walk(call)
    assert fired >= 3 and failed >= 3, (fired, failed)
    for N in (33, 100, 33):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fa.calc_dots(xyz, radii, offsets, n_points=N, with_index=True), want[N]))


def test_a_failed_growth_of_the_unit_points_leaves_the_context_good_for_the_earlier_point_count():
    """the n-th DEVICE allocation of an expansion at 100 points fails on a context that has expanded at 33: the unit points' buffer
    has to grow (1246 -> 2400 bytes) and is freed before it is allocated anew.  The call fails with a message; the expansion at 33
    points behind it - the point count the context held - gives the dots it gave before, as does the one at 100."""
    import torch
    import dots_ref as dr
    rng = np.random.default_rng(9)
    n = 700
    xyz, radii = rng.uniform(-50, 50, (n, 3)), rng.uniform(1.0, 2.0, n)
    masks = {N: dr.random_masks(rng, n, N) for N in (33, 100)}
    want = {N: dr.dots(xyz, radii, 1.4, fa.test_points(N), masks[N]) for N in (33, 100)}
    dev = "cuda:0"
    d_xyz, d_r = torch.from_numpy(xyz.reshape(-1)).to(dev), torch.from_numpy(radii).to(dev)
    d_masks = {N: torch.from_numpy(masks[N].view(np.int32)).to(dev) for N in (33, 100)}
    d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def expand(ctx, N):
        D = ctx.dots_count(d_masks[N].data_ptr(), n, d_first.data_ptr(), n_points=N)
        d_dx = torch.full((D, 3), float("nan"), dtype=torch.float64, device=dev)
        d_da, d_dp = (torch.full((D,), -7, dtype=torch.int32, device=dev) for _ in range(2))
        ctx.dots_expand(d_xyz.data_ptr(), d_r.data_ptr(), n, d_masks[N].data_ptr(), d_first.data_ptr(), D, d_dx.data_ptr(), d_da.data_ptr(),
                        d_dp.data_ptr(), probe=1.4, n_points=N)
        got = (d_dx.cpu().numpy(), d_da.cpu().numpy(), d_dp.cpu().numpy())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want[N])), N

    L = fa.lib()
    failures = 0
    try:
        for k in range(1, 20):
            ctx = fa.GpuContext(0)                  # a fresh context: its buffers are allocated in these calls
            try:
                expand(ctx, 33)
                L.freesasa_gpu_test_fail_after(k)
                try:
                    expand(ctx, 100)
                    ok = True
                except RuntimeError as e:
                    ok = False
                    assert str(e).split(": ", 1)[1], "a failure without a message"
                L.freesasa_gpu_test_fail_after(0)
                expand(ctx, 33)                     # the point count the context held before the failure
                expand(ctx, 100)
            finally:
                L.freesasa_gpu_test_fail_after(0)
                ctx.close()
            if ok:
                break
            failures += 1
        assert failures >= 1, failures              # (the unit points' buffer, at the least)
    finally:
        L.freesasa_gpu_test_fail_after(0)


def test_trajectory_masks_survive_every_allocation_failing(system):
    one, full32, index, _ = system
    frames = full32.astype(np.float64)
    kw = dict(atom_index=index, alg=fa.SHRAKE_RUPLEY, resolution=100, frames_per_batch=3, devices=[0, 0], masks=True)
    want = fa.trajectory_topology(frames, one, **kw)

    def call():
        try:
            got = fa.trajectory_topology(frames, one, **kw)
        except RuntimeError as e:
            return False, str(e)
        assert got.masks.tobytes() == want.masks.tobytes() and got.totals.tobytes() == want.totals.tobytes()
        return True, ""

    fired, failed = walk(call)
    assert fired >= 3 and failed >= 3, (fired, failed)
    assert fa.trajectory_topology(frames, one, **kw).masks.tobytes() == want.masks.tobytes()
