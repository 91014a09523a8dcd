"""Interfaces between chain groups in the file sweep on the device (freesasa_gpu_sweep_files_interfaces, include/freesasa_gpu.h):
the interface pipeline of the batch entries run once per batch of the sweep on the residues, labels, classes and group ids the
sweep holds on the device, and two kernels of its own (csrc/ifsweep_kernels.h) that let the tables leave the device labelled.

The bar is the long way round, file by file: ingest.load_files -> chain_groups -> calc_interfaces(per_atom=True, res_first=...)
-> GpuContext.class_sums over (pair_buried, atom_class[pair_atom], side_offsets).  Everything must be equal bit for bit: an atom's
area does not depend on what else rides in its batch, the pair areas are sums over the sides in a fixed order, the residue sums
are taken in strict atom order, and the class sums are the class-sum kernel's over the same numbers - equality is derived, not
measured.  The first six outputs are sweep_files_groups' own."""
import ctypes as C
import os

import numpy as np
import pytest

import freesasa_amd as fa
from freesasa_amd import ingest
from test_device_parser import MUST_PARSE
from test_groups_sweep_gpu import DEV, REFUSED, SWEEP_FILES, bits64, cif_text, fixture, _free_device_memory

pytestmark = pytest.mark.gpu

CRLF = "2jo4_crlf.pdb"
FILES = SWEEP_FILES + ["3bzd_trimmed.pdb", CRLF]
# separate chains, as the long way alone finds them (a CPU estimate with a 6 A cut on the fixtures agrees)
PAIRS = {"2jo4.pdb": 6, "1a0q.pdb": 1, "3bzd_trimmed.pdb": 1, CRLF: 6}


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    """the fixtures, and 2jo4.pdb with CRLF line ends in a form the device parser refuses, so that a multi-chain file whose
    residues and labels come from the host parser rides in a batch with device-parsed ones.  (CRLF alone does not do it: the
    device parser reads such files itself, and refuses syn_crlf.pdb for its exponents.  So the copy also writes the first x
    coordinate that fits as an exponent, 12.345 as 12345e-3 - the same double through strtod, and the host parser's to read.)"""
    d = tmp_path_factory.mktemp("ifsweep")
    with open(fixture("2jo4.pdb"), "rb") as fh:
        lines = fh.read().split(b"\n")
    assert not any(b"\r" in ln for ln in lines)
    for k, ln in enumerate(lines):
        if ln.startswith(b"ATOM") and float(ln[30:38]) > 0:
            new = b"%8s" % (b"%de-3" % round(float(ln[30:38]) * 1000))
            assert len(new) == 8 and float(new) == float(ln[30:38])
            lines[k] = ln[:30] + new + ln[38:]
            break
    else:
        raise AssertionError("no coordinate to rewrite")
    crlf = os.path.join(str(d), CRLF)
    with open(crlf, "wb") as fh:
        fh.write(b"\r\n".join(lines))
    return [crlf if n == CRLF else fixture(n) for n in FILES]


def long_way_of(file_paths, alg, res, kw, min_buried):
    """per file: None (group status not 0), or what the long way gives of the file alone"""
    import torch
    dev = torch.device("cuda:0")
    ctx = fa.GpuContext(0)
    out = []
    for p in file_paths:
        b = ingest.load_files([p])
        g, n, st = b.chain_groups(kw.get("spec"), separate_chains=kw.get("separate_chains", False))
        if st[0] != 0:
            out.append(dict(status=int(st[0])))
            continue
        r = fa.calc_interfaces(b.xyz, b.radii, b.offsets, g, n, alg, resolution=res, device=0, per_atom=True, res_first=b.res_first,
                               min_buried=min_buried)
        P = r.n_pairs
        cls = np.zeros((P, 2, 3))
        if P:
            d_b = torch.from_numpy(np.ascontiguousarray(r.pair_buried)).to(dev)
            d_c = torch.from_numpy(np.ascontiguousarray(b.atom_class[r.pair_atom])).to(dev)
            d_o = torch.empty(6 * P, dtype=torch.float64, device=dev)
            ctx.class_sums(d_b.data_ptr(), d_c.data_ptr(), r.side_offsets, d_o.data_ptr())
            torch.cuda.synchronize()
            cls = d_o.cpu().numpy().reshape(P, 2, 3)
        out.append(dict(status=0, groups=r.pair_groups, atoms=np.diff(r.side_offsets).reshape(P, 2).astype(np.int32), areas=r.pair_areas, cls=cls,
                        res_offsets=r.res_offsets, res_index=r.res_index, res_atoms=r.res_atoms, res_areas=r.res_areas,
                        number=[b.res_number[i] for i in r.res_index], chain=[b.res_chain[i] for i in r.res_index],
                        names=[b.res_name[i] for i in r.res_index]))
    return out


_LONG = {}


def long_way(paths, alg, res, key, min_buried):
    kw = dict(separate_chains=True) if key == "separate" else dict(spec=key)
    if (alg, res, key, min_buried) not in _LONG:
        _LONG[(alg, res, key, min_buried)] = long_way_of(paths, alg, res, kw, min_buried)
    return kw, _LONG[(alg, res, key, min_buried)]


def same_as_the_long_way(got, want, names):
    gstatus, istatus, gt, t = got[4], got[5], got[6], got[7]
    assert t.n_files == len(names) and t.pair_offsets[0] == 0 and t.pair_offsets[-1] == t.n_pairs
    assert t.res_offsets[0] == 0 and t.res_offsets[-1] == t.n_res_rows
    gchain, pchain = gt.chain, t.pair_chain
    name, number, chain = t.res_name, t.res_number, t.res_chain
    for k, w in enumerate(want):
        s = t.file(k)
        assert istatus[k] == w["status"] == gstatus[k], (names[k], istatus[k], gstatus[k], w["status"])
        if w["status"]:
            assert s.start == s.stop, names[k]
            continue
        P = len(w["groups"])
        assert s.stop - s.start == P, (names[k], s, P)
        assert np.array_equal(t.pair_groups[s], w["groups"]), names[k]
        assert np.array_equal(t.pair_atoms[s], w["atoms"]), names[k]
        assert np.array_equal(bits64(t.pair_areas[s]), bits64(w["areas"])), names[k]
        assert np.array_equal(bits64(t.pair_class_buried[s]), bits64(w["cls"])), names[k]
        g0 = gt.file(k).start
        for p in range(P):
            assert pchain[s.start + p] == (gchain[g0 + w["groups"][p, 0]], gchain[g0 + w["groups"][p, 1]]), names[k]
        if P == 0:
            continue
        r0 = int(t.res_offsets[2 * s.start])
        rows = slice(r0, int(t.res_offsets[2 * s.stop]))
        assert np.array_equal(t.res_offsets[2 * s.start:2 * s.stop + 1] - r0, w["res_offsets"]), names[k]
        assert np.array_equal(t.res_index[rows], w["res_index"]), names[k]
        assert np.array_equal(t.res_atoms[rows], w["res_atoms"]), names[k]
        assert np.array_equal(bits64(t.res_areas[rows]), bits64(w["res_areas"])), names[k]
        assert name[rows] == w["names"] and number[rows] == w["number"] and chain[rows] == w["chain"], names[k]


@pytest.mark.parametrize("alg, res, min_buried", [(fa.LEE_RICHARDS, 20, 0.0), (fa.LEE_RICHARDS, 20, 1.0), (fa.SHRAKE_RUPLEY, 100, 0.0)],
                         ids=["lr20", "lr20-min1", "sr100"])
@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["one", "three"])
@pytest.mark.parametrize("batch_atoms", [0, 3000])
@pytest.mark.parametrize("parser", ["host", "device"])
def test_sweep_files_interfaces_equals_the_long_way(paths, parser, batch_atoms, devices, alg, res, min_buried):
    kw, want = long_way(paths, alg, res, "separate", min_buried)
    # the guard against an empty test: the pairs the long way alone finds
    count = {n: (len(w["groups"]) if not w["status"] else -1) for n, w in zip(FILES, want)}
    for n, p in PAIRS.items():
        assert count[n] == p, (n, count[n])
    assert count["3gnn.pdb"] >= 3
    assert sum(c > 0 for c in count.values()) >= 5 and sum(c == 0 for c in count.values()) >= 8, count
    assert sum(len(w["res_index"]) for w in want if not w["status"]) > 100
    opt = DEV if parser == "device" else 0
    fa.sweep_parse_stats()
    got = fa.sweep_files_interfaces(paths, separate_chains=True, alg=alg, resolution=res, ingest_options=opt, batch_atoms=batch_atoms,
                                    devices=devices, n_threads=4, residues=True, min_buried=min_buried)
    on_device, by_host = fa.sweep_parse_stats()
    if parser == "device":      # the device-built residues and labels were what was tested, and the CRLF copy went to the host parser
        assert on_device >= len(MUST_PARSE) and by_host >= len(REFUSED) + 1
        fa.sweep_files_interfaces([paths[FILES.index(CRLF)]], separate_chains=True, ingest_options=opt)
        assert fa.sweep_parse_stats() == (0, 1)
    groups = fa.sweep_files_groups(paths, separate_chains=True, alg=alg, resolution=res, ingest_options=opt, batch_atoms=batch_atoms,
                                   devices=devices, n_threads=4)
    for x, y, what in zip(groups[:5], got[:5], ("totals", "class sums", "atoms", "status", "group status")):
        assert np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(x, y), what
    for f in ("group_offsets", "group_atoms", "chain_raw", "areas"):
        assert getattr(groups[5], f).tobytes() == getattr(got[6], f).tobytes(), f
    same_as_the_long_way(got, want, FILES)
    # without the residue rows: the same pairs and no rows
    bare = fa.sweep_files_interfaces(paths, separate_chains=True, alg=alg, resolution=res, ingest_options=opt, batch_atoms=batch_atoms,
                                     devices=devices, n_threads=4)
    for f in ("pair_offsets", "pair_groups", "pair_atoms", "pair_chain_raw", "pair_areas", "pair_class_buried"):
        assert getattr(bare[7], f).tobytes() == getattr(got[7], f).tobytes(), f
    assert bare[7].n_res_rows == 0 and np.array_equal(bare[5], got[5])


@pytest.mark.parametrize("parser", ["host", "device"])
def test_a_spec_of_two_groups(paths, parser):
    kw, want = long_way(paths, fa.LEE_RICHARDS, 20, "A+B", 0.0)
    got = fa.sweep_files_interfaces(paths, "A+B", ingest_options=DEV if parser == "device" else 0, batch_atoms=3000, devices=[0, 0],
                                    n_threads=4, residues=True)
    same_as_the_long_way(got, want, FILES)
    assert (got[5] == ingest.EGROUP).sum() >= 1 and got[7].n_pairs >= 2
    assert set(got[7].pair_chain) == {("A", "B")}


@pytest.mark.parametrize("parser", ["host", "device"])
def test_single_chain_files_give_empty_tables(parser):
    names = ["1ubq.pdb", "3bkr.cif", "empty.pdb"]
    ps = [fixture(n) for n in names]
    opt = DEV if parser == "device" else 0
    got = fa.sweep_files_interfaces(ps, separate_chains=True, ingest_options=opt, residues=True)
    plain = fa.sweep_files(ps, ingest_options=opt)
    for x, y in zip(plain, got[:4]):
        assert np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(x, y)
    t = got[7]
    assert t.n_pairs == 0 and t.n_res_rows == 0 and t.pair_offsets.tolist() == [0, 0, 0, 0] and t.res_offsets.tolist() == [0]
    assert got[5].tolist() == got[3].tolist() and got[3][2] != 0 and got[6].n_groups == 2


def test_more_than_4096_groups(tmp_path):
    """a file of 4097 one-atom chains between two real files: its own code, its group rows, no interface rows; the neighbours as
    they are without it"""
    labels = ["%s%s%s" % (a, b, c) for a in "ABCDEFGHIJKLMNOPQ" for b in "ABCDEFGHIJKLMNOP" for c in "ABCDEFGHIJKLMNOP"][:4097]
    big = os.path.join(str(tmp_path), "chains4097.cif")
    with open(big, "w") as fh:
        fh.write(cif_text(labels, 1))
    ps = [fixture("2jo4.pdb"), big, fixture("1a0q.pdb")]
    for opt in (0, DEV):
        got = fa.sweep_files_interfaces(ps, separate_chains=True, ingest_options=opt, residues=True)
        alone = fa.sweep_files_interfaces([ps[0], ps[2]], separate_chains=True, ingest_options=opt, residues=True)
        groups = fa.sweep_files_groups(ps, separate_chains=True, ingest_options=opt)
        assert got[3].tolist() == [0, 0, 0] and got[4].tolist() == [0, 0, 0] and got[5].tolist() == [0, fa.EIFACE_GROUPS, 0]
        assert fa.EIFACE_GROUPS not in (ingest.EGROUP, 1, 2, 3, 4, 5, 6, 7)
        gt, t = got[6], got[7]
        assert gt.file(1).stop - gt.file(1).start == 4097 and np.all(gt.group_atoms[gt.file(1)] == 1)
        assert got[0][1] > 0 and got[2][1] == 4097
        for f in ("group_offsets", "group_atoms", "chain_raw", "areas"):
            assert getattr(groups[5], f).tobytes() == getattr(gt, f).tobytes(), f
        assert np.array_equal(bits64(groups[0]), bits64(got[0]))
        assert t.file(1).start == t.file(1).stop and t.pair_offsets.tolist() == [0, 6, 6, 7]
        a = alone[7]
        for f in ("pair_groups", "pair_atoms", "pair_chain_raw", "pair_areas", "pair_class_buried", "res_offsets", "res_index", "res_atoms",
                  "res_areas", "res_name_raw", "res_number_raw", "res_chain_raw"):
            assert getattr(a, f).tobytes() == getattr(t, f).tobytes(), f


def test_repeated_sweeps_keep_no_device_memory(paths):
    # (the pool hands its contexts out in turn, each with the buffers of the calls it has seen: emptied first, and with one batch
    # - so one worker - both calls run on the one context the first of them makes, and every buffer the second needs is there)
    fa.lib().freesasa_gpu_release_pool()
    kw = dict(separate_chains=True, ingest_options=DEV, batch_atoms=0, devices=[0], residues=True)
    first = fa.sweep_files_interfaces(paths, **kw)
    free1 = _free_device_memory()
    second = fa.sweep_files_interfaces(paths, **kw)
    free2 = _free_device_memory()
    assert free2 == free1, (free1, free2)
    for f in ("pair_offsets", "pair_areas", "pair_class_buried", "res_offsets", "res_index", "res_areas", "res_name_raw"):
        assert getattr(first[7], f).tobytes() == getattr(second[7], f).tobytes(), f
