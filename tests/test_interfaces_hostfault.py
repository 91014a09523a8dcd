"""Host-side failure injection (tests/test_hostfault.py has the hook and the bar) through the interface entries: the n-th host
allocation of calc_interfaces (freesasa_gpu_calc_interface_pairs, freesasa_gpu_calc_interfaces) fails, n = 1, 2, ...; every call
fails with a message or succeeds with the un-faulted bytes, and the call after the walk gives them bit for bit."""
import numpy as np
import pytest

import freesasa_amd as fa
import interfaces_ref as ir
from test_hostfault import walk

pytestmark = pytest.mark.gpu


def _bytes(got):
    return b"".join(a.tobytes() for a in (got.sasa, got.iso, got.totals, got.group_totals, got.pair_struct, got.pair_groups, got.pair_areas,
                                          got.side_offsets, got.pair_atom, got.pair_buried))


@pytest.mark.parametrize("alg", [fa.LEE_RICHARDS, fa.SHRAKE_RUPLEY])
def test_calc_interfaces_survives_every_allocation_failing(alg):
    xyz, radii, offsets, group, n_groups = (np.array(a) for a in ir.edge_batch()[:5])
    kw = dict(alg=alg, resolution=20 if alg == fa.LEE_RICHARDS else 100, per_atom=True)
    want = _bytes(fa.calc_interfaces(xyz, radii, offsets, group, n_groups, **kw))

    def call():
        try:
            got = fa.calc_interfaces(xyz, radii, offsets, group, n_groups, **kw)
        except RuntimeError as e:
            return False, str(e).split(": ", 1)[1]
        assert _bytes(got) == want
        return True, ""

    fired, failed = walk(call)
    assert fired >= 5 and failed >= 5, (fired, failed)     # the plan's arrays, the flags, the counts, the test points, the engine's own
    assert _bytes(fa.calc_interfaces(xyz, radii, offsets, group, n_groups, **kw)) == want
