"""What the interface entries (include/freesasa_gpu.h: freesasa_gpu_interfaces_dev, _interface_residues_dev, _interface_contacts_dev,
_interface_residue_contacts_dev and the four freesasa_gpu_calc_interface* forms with capacities) owe their callers whatever their
tables hold: the counts set before a capacity is refused, the required arrays alone, the host form of the residue entry against
its device form, and the empty cases - no pair, no residue row, no buried point, no folded row - on a structure of two atoms.

The entries are called through lib() as C callers call them (the Python wrappers raise where these tests look at what was
written).  Every array handed in, on the device or on the host, is filled with -7 and has GUARD elements behind it.  Nothing is
compared to a tolerance: counts are integers, and arrays are held byte for byte to another call of the same library.  Shrake-Rupley
at 33 points on tests/interface_residue_contacts_ref.py's batch, whose sizes come from the restatement.  Reads nothing outside the
repository."""
import ctypes as C

import numpy as np
import pytest

import interface_residue_contacts_ref as qr
import interface_residues_ref as rr
from test_groups_gpu import LR, SR, RES
from test_interface_residues_gpu import Run as ResidueRun
from test_interfaces_gpu import GUARD, _dev, _guarded

pytestmark = pytest.mark.gpu

KINDS = ("interfaces", "residues", "contacts", "rescontacts")
FORMS = ("dev", "host")
ENTRY = {("interfaces", "dev"): "freesasa_gpu_interfaces_dev", ("interfaces", "host"): "freesasa_gpu_calc_interfaces",
         ("residues", "dev"): "freesasa_gpu_interface_residues_dev", ("residues", "host"): "freesasa_gpu_calc_interface_residues",
         ("contacts", "dev"): "freesasa_gpu_interface_contacts_dev", ("contacts", "host"): "freesasa_gpu_calc_interface_contacts",
         ("rescontacts", "dev"): "freesasa_gpu_interface_residue_contacts_dev",
         ("rescontacts", "host"): "freesasa_gpu_calc_interface_residue_contacts"}
# the capacities and the counts of a kind, in the order of its signature; a capacity's count is the one at its place
CAPS = {"interfaces": ("pair", "atom"), "residues": ("pair", "atom", "res"), "contacts": ("pair", "atom", "contact", "dot"),
        "rescontacts": ("pair", "atom", "contact", "dot", "rescontact")}
COUNTS = {"interfaces": "PM", "residues": "PMR", "contacts": "PMCD", "rescontacts": "PMCDQ"}
GROUP_ARRAYS = ("sasa", "iso", "totals", "gt")
PAIR_ARRAYS = ("ps", "pg", "areas", "so", "pa", "pb")
STAGE_ARRAYS = {"interfaces": (), "residues": ("ro", "ri", "ra", "rar"), "contacts": ("cf", "cp", "cn", "ca", "bm", "dp"),
                "rescontacts": ("cf", "cp", "cn", "ca", "bm", "dp")}
FOLD_ARRAYS = ("qo", "qr", "qc", "qa", "qv")
REQUIRED = {"interfaces": ("areas",), "residues": ("areas", "rar"), "contacts": ("areas",), "rescontacts": ("areas", "qa")}
i32, i64, f64 = np.int32, np.int64, np.float64
# name: (dtype, elements the caller's array holds for the capacities k, elements a good call with the counts n writes)
ARRAYS = {
    "ps": (i32, lambda k: k["pair"], lambda n: n["P"]), "pg": (i32, lambda k: 2 * k["pair"], lambda n: 2 * n["P"]),
    "areas": (f64, lambda k: 6 * k["pair"], lambda n: 6 * n["P"]), "so": (i64, lambda k: 2 * k["pair"] + 1, lambda n: 2 * n["P"] + 1),
    "pa": (i32, lambda k: k["atom"], lambda n: n["M"]), "pb": (f64, lambda k: k["atom"], lambda n: n["M"]),
    "ro": (i64, lambda k: 2 * k["pair"] + 1, lambda n: 2 * n["P"] + 1), "ri": (i32, lambda k: k["res"], lambda n: n["R"]),
    "ra": (i32, lambda k: k["res"], lambda n: n["R"]), "rar": (f64, lambda k: 3 * k["res"], lambda n: 3 * n["R"]),
    "cf": (i64, lambda k: k["atom"] + 1, lambda n: n["M"] + 1 if n["P"] else 1), "cp": (i32, lambda k: k["contact"], lambda n: n["C"]),
    "cn": (i32, lambda k: k["contact"], lambda n: n["C"]), "ca": (f64, lambda k: k["contact"], lambda n: n["C"]),
    "bm": (i32, lambda k: 4 * k["atom"], lambda n: 4 * n["M"]), "dp": (i32, lambda k: k["dot"], lambda n: n["D"]),
    "qo": (i64, lambda k: 2 * k["pair"] + 1, lambda n: 2 * n["P"] + 1), "qr": (i32, lambda k: 2 * k["rescontact"], lambda n: 2 * n["Q"]),
    "qc": (i32, lambda k: 2 * k["rescontact"], lambda n: 2 * n["Q"]), "qa": (f64, lambda k: k["rescontact"], lambda n: n["Q"]),
    "qv": (i32, lambda k: k["rescontact"], lambda n: n["Q"]),
}


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0, "no HIP device: the GPU tests cannot run"
    return freesasa_amd


@pytest.fixture(scope="module")
def batch():
    b = qr.rescontacts_batch()
    return tuple(np.array(a) for a in b[:5]) + (np.array(b[6]),)      # (copies: the restatement's own arrays stay read-only)


@pytest.fixture(scope="module")
def sizes():
    """the counts of the batch at 33 points, from the restatement: P, M, C, D, Q (R is asked of a good call: it depends on the areas)"""
    ps, _, _, pa = qr.batch_table()
    c, f = qr.batch_contacts(33), qr.batch_fold(33)
    return dict(P=len(ps), M=len(pa), C=len(c["contact_partner"]), D=len(c["dot_partner"]), Q=len(f["rescontact_area"]))


def _names(kind):
    return PAIR_ARRAYS + STAGE_ARRAYS[kind] + (FOLD_ARRAYS if kind == "rescontacts" else ())


def _caps_for(kind, n, R=None):
    """the capacities that hold exactly what the counts n ask for (res: R rows, or - R unknown - the M a table can have)"""
    full = dict(pair=n["P"], atom=n["M"], res=n["M"] if R is None else R, contact=n["C"], dot=n["D"], rescontact=n["Q"])
    return {k: full[k] for k in CAPS[kind]}


class Call:
    """one call of an entry through lib(): ret, msg, counts {letter: value, -7 where the entry wrote none} and raw {name: the
    caller's array without its guard, None where a null pointer was handed in}; the guards are checked, and after a good call
    that nothing was written beyond the rows the counts speak of"""

    def __init__(self, fa, ctx, kind, form, batch, caps, resolution=33, alg=SR, optional=True, min_buried=0.0):
        xyz, r, offs, group, ng, rf = batch
        xyz, r = np.ascontiguousarray(xyz, f64).reshape(-1), np.ascontiguousarray(r, f64)
        offs, rf = np.ascontiguousarray(offs, i64), np.ascontiguousarray(rf, i64)
        group, ng = np.ascontiguousarray(group, i32), np.ascontiguousarray(ng, i32)
        n, ns, G = len(r), len(offs) - 1, int(ng.sum())
        dev = form == "dev"
        names = _names(kind)
        size = {k: ARRAYS[k][1](caps) for k in names}
        size.update(sasa=n, iso=n, totals=ns, gt=3 * G)
        kinds = {k: ARRAYS[k][0] for k in names}
        kinds.update({k: f64 for k in GROUP_ARRAYS})
        wanted = [k for k in GROUP_ARRAYS + names
                  if optional or k in REQUIRED[kind] or (dev and k in ("sasa", "iso"))]      # (the device forms need sasa and iso)
        if dev:
            import torch
            tk = {i32: torch.int32, i64: torch.int64, f64: torch.float64}
            keep = [_dev(xyz), _dev(r), _dev(group, i32)]
            out = {k: _guarded(size[k], tk[kinds[k]], -7.0 if kinds[k] is f64 else -7) for k in wanted}
            ptr = {k: v.data_ptr() for k, v in out.items()}
            x_, r_, g_ = (t.data_ptr() for t in keep)
        else:
            out = {k: np.full(size[k] + GUARD, -7, kinds[k]) for k in wanted}
            ptr = dict(out)
            x_, r_, g_ = xyz, r, group
        p = lambda k: ptr.get(k)
        cnt = {c: C.c_longlong(-7) for c in COUNTS[kind]}
        cap_list, cnt_list = [caps[k] for k in CAPS[kind]], [C.byref(cnt[c]) for c in COUNTS[kind]]
        residues = [rf, len(rf) - 1] if kind == "residues" else []
        args = ([alg] if dev else []) + [x_, r_, offs, ns, g_, ng] + residues + ([] if dev else [alg]) + [qr.PROBE, resolution]
        args += ([min_buried] if kind == "residues" else []) + [p(k) for k in GROUP_ARRAYS] + cap_list[:4] + cnt_list[:4]
        args += [p(k) for k in PAIR_ARRAYS + STAGE_ARRAYS[kind]]
        if kind == "rescontacts":
            args += [rf, len(rf) - 1, cap_list[4], cnt_list[4]] + [p(k) for k in FOLD_ARRAYS]
        err = C.create_string_buffer(512)
        args = [ctx._h] + args if dev else args + [-1, err, 512]
        fn = getattr(fa.lib(), ENTRY[kind, form])
        assert len(args) == len(fn.argtypes), ENTRY[kind, form]
        conv = []
        for a, t in zip(args, fn.argtypes):
            if isinstance(a, np.ndarray):
                a = a.ctypes.data if t is C.c_void_p else a.ctypes.data_as(t)
            conv.append(a)
        self.ret = fn(*conv)
        self.msg = ctx.error() if dev else err.value.decode()
        self.counts = {c: int(v.value) for c, v in cnt.items()}
        host = {k: v.cpu().numpy() if dev else v for k, v in out.items()}
        for k, v in host.items():
            assert len(v) == size[k] + GUARD and np.all(v[size[k]:] == -7), f"the guard behind {k} was written"
        self.raw = {k: host[k][:size[k]] if k in host else None for k in GROUP_ARRAYS + names}
        self.names = names
        if self.ret == 0:
            full = dict(dict.fromkeys("RCDQ", 0), **self.counts)
            self.out = {}
            for k in names:
                if self.raw[k] is not None:
                    used = ARRAYS[k][2](full)
                    assert used <= size[k] and np.all(self.raw[k][used:] == -7), f"{k} was written beyond its rows"
                    self.out[k] = self.raw[k][:used]

    def tables_untouched(self):
        """none of the caller's pair, atom, residue, contact or dot arrays was written"""
        return all(np.all(self.raw[k] == -7) for k in self.names if self.raw[k] is not None)


def _good(fa, ctx, kind, form, batch, sizes):
    """a call whose capacities hold exactly what it delivers, and those capacities"""
    caps = _caps_for(kind, sizes)
    good = Call(fa, ctx, kind, form, batch, caps)
    assert good.ret == 0, good.msg
    if kind == "residues":                                                 # (the first call: the M rows a table can have; now R)
        assert 0 < good.counts["R"] <= sizes["M"]
        caps = _caps_for(kind, sizes, good.counts["R"])
        again = Call(fa, ctx, kind, form, batch, caps)
        assert again.ret == 0 and again.counts == good.counts and all(again.out[k].tobytes() == good.out[k].tobytes() for k in good.out)
        good = again
    assert all(good.counts[c] == sizes[c] for c in good.counts if c != "R"), good.counts
    return good, caps


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_counts_are_set_before_a_capacity_is_refused(fa, batch, sizes, kind, form):
    ctx = fa.GpuContext(0)
    try:
        good, caps = _good(fa, ctx, kind, form, batch, sizes)
        for word, letter in zip(CAPS[kind], COUNTS[kind]):
            short = dict(caps)
            short[word] -= 1
            assert short[word] >= 0
            bad = Call(fa, ctx, kind, form, batch, short)
            assert bad.ret == -1, (word, bad.ret)
            assert f"{word}_capacity {short[word]} is too small" in bad.msg and str(good.counts[letter]) in bad.msg, bad.msg
            assert bad.counts == good.counts, (word, bad.counts, good.counts)
            assert bad.tables_untouched(), word
        after = Call(fa, ctx, kind, form, batch, caps)                          # the call after the refused ones
        assert after.ret == 0 and after.counts == good.counts
        assert all(after.out[k].tobytes() == good.out[k].tobytes() for k in good.out)
    finally:
        ctx.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_required_arrays_only(fa, batch, sizes, kind, form):
    ctx = fa.GpuContext(0)
    try:
        good, caps = _good(fa, ctx, kind, form, batch, sizes)
        bare_caps = dict(caps, atom=0)
        bare_caps.update({k: 0 for k in ("contact", "dot") if k in caps})
        bare = Call(fa, ctx, kind, form, batch, bare_caps, optional=False)
    finally:
        ctx.close()
    assert bare.ret == 0, bare.msg
    assert bare.counts == good.counts
    given = [k for k, v in bare.raw.items() if v is not None]
    assert sorted(given) == sorted(REQUIRED[kind] + (("sasa", "iso") if form == "dev" else ()))
    for k in REQUIRED[kind]:
        assert len(good.out[k]) > 0 and bare.out[k].tobytes() == good.out[k].tobytes(), k
    if form == "dev":
        for k in ("sasa", "iso"):
            assert not np.any(good.raw[k] == -7) and bare.raw[k].tobytes() == good.raw[k].tobytes(), k


@pytest.mark.parametrize("alg", [LR, SR])
def test_the_residue_entrys_host_form_gives_its_device_forms_bytes(fa, alg):
    b = rr.residue_edge_batch()
    xyz, r, offs, group, ng, rf = tuple(np.array(a) for a in b[:5]) + (np.array(b[6]),)
    ps, _, _, pa = rr.edge_table()
    P, M = len(ps), len(pa)
    ctx = fa.GpuContext(0)
    try:
        run = ResidueRun(ctx, alg, xyz, r, offs, group, ng, rf, P, M, M)
    finally:
        ctx.close()
    assert run.error is None, run.error
    got = fa.calc_interfaces(xyz, r, offs, group, ng, alg=alg, resolution=RES[alg], per_atom=True, res_first=rf)
    assert (got.n_pairs, len(got.pair_atom), got.n_res_rows) == (run.P, run.M, run.R) and run.R > 0
    names = ("sasa", "iso", "totals", "group_totals", "pair_struct", "pair_groups", "pair_areas", "side_offsets", "pair_atom", "pair_buried",
             "res_offsets", "res_index", "res_atoms", "res_areas")
    for k, dev in zip(names, (run.sasa, run.iso, run.totals, run.gt, run.ps, run.pg, run.areas, run.so, run.pa, run.pb, run.ro, run.ri,
                              run.ra, run.rar)):
        host = getattr(got, k)
        assert host.dtype == dev.dtype and host.size == dev.size and host.tobytes() == dev.tobytes(), k
    assert b"".join(getattr(got, k).tobytes() for k in names) == run.bytes()


TWO = (np.array([1.5, 1.5]), np.array([0, 2]), np.array([0, 1], np.int32), np.array([2], np.int32), np.array([0, 1, 2]))
FAR, TOUCHING = np.array([[0.0, 0, 0], [50.0, 0, 0]]), np.array([[0.0, 0, 0], [0, 3.0, 0]])
ROOMY = dict(pair=2, atom=4, res=4, contact=4, dot=400, rescontact=4)


def _two(fa, ctx, kind, form, xyz, resolution, **kw):
    run = Call(fa, ctx, kind, form, (xyz,) + TWO, {k: ROOMY[k] for k in CAPS[kind]}, resolution=resolution, **kw)
    assert run.ret == 0, run.msg
    return run


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_two_atoms_far_apart_and_touching(fa, kind, form):
    """P == 0: side_offsets [1], res_offsets [1], contact_first [1] and rescontact_offsets [1] are 0 and nothing else of the tables
    is written; touching at one test point: no buried point (D_b == 0: contact_first [M + 1] zeros, the masks delivered), no folded
    row (Q == 0: rescontact_offsets [2 P + 1] zeros), and with a min_buried no residue reaches no residue row (R == 0)"""
    ctx = fa.GpuContext(0)
    try:
        far = _two(fa, ctx, kind, form, FAR, 100)
        dry = _two(fa, ctx, kind, form, TOUCHING, 1, min_buried=1e300)
        wet = _two(fa, ctx, kind, form, TOUCHING, 100)
    finally:
        ctx.close()
    assert all(v == 0 for v in far.counts.values()), far.counts
    for k in far.names:
        if k in ("so", "ro", "cf", "qo"):
            assert np.array_equal(far.out[k], [0]) and np.all(far.raw[k][1:] == -7), k
        else:
            assert np.all(far.raw[k] == -7), k
    for run in (far, dry, wet):
        assert not any(np.any(run.raw[k] == -7) for k in GROUP_ARRAYS)
    assert (dry.counts["P"], dry.counts["M"]) == (1, 2) and all(dry.counts[c] == 0 for c in dry.counts if c not in "PM"), dry.counts
    assert np.array_equal(dry.out["ps"], [0]) and np.array_equal(dry.out["pg"], [0, 1]) and np.array_equal(dry.out["so"], [0, 1, 2])
    assert np.array_equal(dry.out["pa"], [0, 1]) and not np.any(dry.out["areas"] == -7) and not np.any(dry.out["pb"] == -7)
    if kind == "residues":
        assert np.array_equal(dry.out["ro"], [0, 0, 0]) and all(np.all(dry.raw[k] == -7) for k in ("ri", "ra", "rar"))
        assert wet.counts["R"] == 2 and np.array_equal(wet.out["ro"], [0, 1, 2]) and np.array_equal(wet.out["ri"], [0, 1])
    if kind in ("contacts", "rescontacts"):
        assert np.array_equal(dry.out["cf"], [0, 0, 0]) and np.array_equal(dry.out["bm"], [0] * 8)
        assert all(np.all(dry.raw[k] == -7) for k in ("cp", "cn", "ca", "dp"))
        assert wet.counts["C"] == 2 and wet.counts["D"] > 0 and np.array_equal(wet.out["cf"], [0, 1, 2]) and np.array_equal(wet.out["cp"], [1, 0])
        assert wet.out["cn"].sum() == wet.counts["D"] == len(wet.out["dp"]) and np.any(wet.out["bm"] != 0)
    if kind == "rescontacts":
        assert np.array_equal(dry.out["qo"], [0, 0, 0]) and all(np.all(dry.raw[k] == -7) for k in ("qr", "qc", "qa", "qv"))
        assert wet.counts["Q"] == 2 and np.array_equal(wet.out["qo"], [0, 1, 2]) and np.array_equal(wet.out["qv"], [1, 0])
        assert wet.out["qa"].tobytes() == wet.out["ca"].tobytes()


def test_two_atoms_through_the_pair_entries(fa):
    r, offs, group, ng, _ = TWO
    ctx = fa.GpuContext(0)
    try:
        for xyz, want in ((FAR, (0, 0)), (TOUCHING, (1, 2))):
            ps, pg = np.full(2 + GUARD, -7, np.int32), np.full(4 + GUARD, -7, np.int32)
            d_x, d_r, d_g = _dev(xyz.reshape(-1)), _dev(r), _dev(group, np.int32)
            counts = ctx.interface_pairs(d_x.data_ptr(), d_r.data_ptr(), offs, d_g.data_ptr(), ng, 2, ps, pg, alg=SR, resolution=100)
            host = fa.interface_pairs(xyz, r, offs, group, ng, alg=SR, resolution=100)
            P = want[0]
            assert counts == want + (1, P) and (host.n_pairs, host.n_pair_atoms, host.n_tests, host.n_candidates) == counts
            assert np.array_equal(ps[:P], [0] * P) and np.array_equal(pg[:2 * P], [0, 1] * P) and np.all(ps[P:] == -7) and np.all(pg[2 * P:] == -7)
            assert np.array_equal(host.pair_struct, [0] * P) and np.array_equal(host.pair_groups.reshape(-1), [0, 1] * P)
    finally:
        ctx.close()
