"""The device parser (freesasa_amd/csrc/gpu_parse.hip: kp_count_nl .. kp_atom_keys) on GENERATED PDB / mmCIF files
(tests/parse_gen.py), whose edges are the kernels' own: newlines on the bytes where a 16-byte group or a 4096-byte block
ends, label changes on the 64-line chunk edge of kp_resolve, lines cut at every length parse_pdb_line names, coordinates at
the ends of "%8.3f", mmCIF numbers of 15 and 16 digits, residue changes on atoms 63/64 and 255/256 of a batch.

The bars: a file's `takes` (what the header comment of gpu_parse.hip promises: parsed on the device, or refused), the
reference-minted vectors (tests/golden/parse_gen.json) and the host loader's arrays bit for bit - the host loader itself is
held to the same vectors without a device by tests/test_parse_gen.py.  The files are written once per module."""
import numpy as np
import pytest

import parse_gen
from freesasa_amd import ingest

pytestmark = pytest.mark.gpu

DEV = ingest.PARSE_ON_DEVICE
SWEPT = ("residues", "altloc", "cif_rows")        # the families that go through whole sweeps


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0
    return freesasa_amd


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """{family: {name: path}}"""
    root = tmp_path_factory.mktemp("parse_gen")
    out = {}
    for fam in parse_gen.FAMILIES:
        d = root / fam
        d.mkdir()
        out[fam] = {}
        for name, data, _ in parse_gen.family(fam):
            (d / name).write_bytes(data)
            out[fam][name] = str(d / name)
    return out


def options_of(fam):
    return sorted({o for n, _, _ in parse_gen.family(fam) for o in parse_gen.options_of(fam, n)} - {parse_gen.OCC})


def check_batch(fa, fam, files, written, opt, what):
    """one batch through parse_files_dev: takes, the vectors, the host loader's arrays.  -> files parsed on the device"""
    exp = parse_gen.expected(fam, opt)
    files = [f for f in files if exp[f[0]] != "-"]
    paths = [written[fam][n] for n, _, _ in files]
    want = ingest.load_texts([t for _, t, _ in files], options=opt, n_threads=4)
    xyz, r, cls, offs, status, host = fa.parse_files_dev(paths, ingest_options=opt, n_threads=4)
    wrong = []
    for k, (n, _, takes) in enumerate(files):
        a, b = int(offs[k]), int(offs[k + 1])
        if host[k]:
            if takes is True:
                wrong.append((n, "refused"))
            if b != a:
                wrong.append((n, "a refused file with atoms"))
            continue
        if takes is False:
            wrong.append((n, "not refused"))
        lo, hi = int(want.offsets[k]), int(want.offsets[k + 1])
        if exp[n] != "crash":
            if (status[k] == ingest.OK) != (exp[n] != "fail"):
                wrong.append((n, "status", int(status[k]), exp[n]))
            if parse_gen.view_of(want, k) != exp[n]:
                wrong.append((n, "the host loader misses the vector"))
        if status[k] != want.status[k] or b - a != hi - lo:
            wrong.append((n, "status / atoms", int(status[k]), int(want.status[k]), b - a, hi - lo))
        elif not (xyz[a:b].tobytes() == want.xyz[lo:hi].tobytes() and r[a:b].tobytes() == want.radii[lo:hi].tobytes() and
                  cls[a:b].tobytes() == want.atom_class[lo:hi].tobytes()):
            wrong.append((n, "arrays"))
    assert not wrong, (what, opt, len(wrong), wrong[:12])
    assert offs[-1] == len(r) == len(cls) == len(xyz)
    return int((host == 0).sum())


@pytest.mark.parametrize("fam", sorted(set(parse_gen.FAMILIES) - {"lines"}))
def test_takes_vectors_and_the_host_loaders_arrays(fa, written, fam):
    files = parse_gen.family(fam)
    for opt in options_of(fam):
        exp = parse_gen.expected(fam, opt)
        on_device = check_batch(fa, fam, files, written, opt, fam)
        assert on_device >= sum(1 for n, _, t in files if t is True and exp[n] != "-")


def test_line_batches(fa, written):
    """the batches whose layout is the case: each one parsed as ONE batch, in the builder's order"""
    for name, files in parse_gen.lines_batches().items():
        for opt in options_of("lines"):
            assert check_batch(fa, "lines", files, written, opt, name) == len(files)


def per_file(fa, paths, opt):
    xyz, r, cls, offs, status, host = fa.parse_files_dev(paths, ingest_options=opt, n_threads=4)
    return [(int(host[k]), int(status[k]), xyz[offs[k]:offs[k + 1]].tobytes(), r[offs[k]:offs[k + 1]].tobytes(), cls[offs[k]:offs[k + 1]].tobytes())
            for k in range(len(paths))]


@pytest.mark.parametrize("fam", sorted(set(parse_gen.FAMILIES) - {"lines"}))
def test_a_files_result_does_not_depend_on_its_neighbours(fa, written, fam):
    """alone in the builder's order, reversed, and with the files of `lines` in between"""
    names = [n for n, _, _ in parse_gen.family(fam)]
    paths = [written[fam][n] for n in names]
    between = [written["lines"][n] for n, _, _ in parse_gen.family("lines") if not n.startswith("thousand_")]
    mixed, where = [], []
    for k, p in enumerate(paths):
        where.append(len(mixed))
        mixed += [p, between[k % len(between)]]
    for opt in (0, parse_gen.HETATM | parse_gen.HYDROGEN | parse_gen.JOIN):
        alone = per_file(fa, paths, opt)
        back = per_file(fa, paths[::-1], opt)[::-1]
        among = per_file(fa, mixed, opt)
        for k, n in enumerate(names):
            assert alone[k] == back[k], (fam, opt, n, "reversed")
            assert alone[k] == among[where[k]], (fam, opt, n, "among the files of lines")


def swept_files():
    return [(fam, n, t) for fam in SWEPT for n, _, t in parse_gen.family(fam)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("opt", [0, parse_gen.HETATM | parse_gen.HYDROGEN, parse_gen.JOIN, parse_gen.SKIP, parse_gen.HALT])
def test_residue_tables_of_a_device_parsed_sweep(fa, written, opt):
    """Boundaries, atoms, reference rows and labels: the host loader's.  Areas: the host-parsed sweep's bit for bit - its main /
    side chain split is the host's backbone flags' doing (tests/test_residue_sweep.py holds it to the long way round), and no two
    atoms of these files share a place, so an area does not depend on the batch it was computed in."""
    files = swept_files()
    paths = [written[fam][n] for fam, n, _ in files]
    b = ingest.load_files(paths, options=opt, n_threads=4)
    # (tests/test_residue_sweep.py: the engine shapes a launch by what the context's previous batch taught it, so the two sweeps
    # that are compared bit for bit each run behind a plain sweep of the same list)
    fa.sweep_files(paths, ingest_options=opt | DEV, n_threads=4)
    fa.sweep_parse_stats()
    totals, cls, atoms, status, t = fa.sweep_files_residues(paths, ingest_options=opt | DEV, n_threads=4)
    on_device, by_host = fa.sweep_parse_stats()
    assert on_device + by_host == len(paths) and on_device >= sum(1 for _, _, takes in files if takes is True), (on_device, by_host)
    assert np.array_equal(status, b.status) and np.array_equal(atoms, np.diff(b.offsets))
    assert t.n_residues == b.n_residues > 100 and t.n_files == b.n_structs
    assert np.array_equal(t.res_offsets, b.res_offsets)
    assert np.array_equal(t.res_atoms, np.diff(b.res_first))
    assert np.array_equal(t.res_ref, b.res_ref)
    for f in ("res_name_raw", "res_number_raw", "res_chain_raw"):
        assert getattr(t, f).tobytes() == getattr(b, f).tobytes(), f
    fa.sweep_files(paths, ingest_options=opt, n_threads=4)
    want = fa.sweep_files_residues(paths, ingest_options=opt, n_threads=4)
    for x, y, what in zip(want[:4], (totals, cls, atoms, status), ("totals", "class sums", "atoms", "status")):
        assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y), (opt, what)
    h = want[4]
    assert np.array_equal(bits(t.abs), bits(h.abs))        # total, main chain, side chain, polar, apolar, unknown
    assert np.array_equal(bits(t.abs[:, 1] + t.abs[:, 2]), bits(h.abs[:, 1] + h.abs[:, 2]))
    nan_t, nan_h = np.isnan(t.rel), np.isnan(h.rel)
    assert np.array_equal(nan_t, nan_h) and np.array_equal(bits(t.rel)[~nan_t], bits(h.rel)[~nan_h])
    assert (t.abs[:, 1] > 0).any() and (t.abs[:, 2] > 0).any() and (~nan_t).any()


@pytest.mark.parametrize("opt", [0, parse_gen.HETATM | parse_gen.HYDROGEN])
def test_selections_by_name_and_symbol_of_a_device_parsed_sweep(fa, written, opt):
    """One selection per atom name and per element symbol the host loader stores for these files (those the selection language
    can spell: a letter, then letters and digits - it upper-cases its values, so a stored 'h' matches nothing)."""
    files = swept_files()
    paths = [written[fam][n] for fam, n, _ in files]
    b = ingest.load_files(paths, options=opt, n_threads=4)
    spell = lambda v: v.isalnum() and v[0].isalpha() and v == v.upper()
    names = sorted({v.decode("latin-1") for v in b.atom_name_raw.tolist()})
    symbols = sorted({v.decode("latin-1") for v in b.atom_symbol_raw.tolist()})
    cmds = [(f"n{k}, name {v}", b.atom_name_raw, v) for k, v in enumerate(names) if spell(v)]
    cmds += [(f"s{k}, symbol {v}", b.atom_symbol_raw, v) for k, v in enumerate(symbols) if spell(v)]
    assert len(cmds) >= 20 and {"CA", "OXT", "HG21", "P"} <= set(names) and {"C", "N", "O", "P"} <= set(symbols)
    for lo in range(0, len(cmds), 64):
        part = cmds[lo:lo + 64]
        s = ingest.Selection([c for c, _, _ in part])
        fa.sweep_files(paths, ingest_options=opt | DEV, n_threads=4)      # (both sweeps behind a plain sweep of the same list, as above)
        fa.sweep_parse_stats()
        got = fa.sweep_files_select(paths, s, ingest_options=opt | DEV, n_threads=4)
        on_device, by_host = fa.sweep_parse_stats()
        assert on_device >= sum(1 for _, _, takes in files if takes is True)
        fa.sweep_files(paths, ingest_options=opt, n_threads=4)
        want = fa.sweep_files_select(paths, s, ingest_options=opt, n_threads=4)
        for x, y, what in zip(want, got, ("totals", "class sums", "atoms", "status", "areas", "counts")):
            assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y), (opt, what)
        for q, (_, stored, v) in enumerate(part):
            hit = (stored == v.encode("latin-1")).astype(np.int64)
            per = np.add.reduceat(np.append(hit, 0), b.offsets[:-1]) * (np.diff(b.offsets) > 0)
            assert np.array_equal(got[5][:, q], per), (opt, part[q][0])
        s.close()
