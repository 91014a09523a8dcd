"""User classifiers on the GPU paths: the device-side parser with a classifier's table uploaded per batch
(freesasa_gpu_parse_files_classified, kp_parse_lines<true> in csrc/gpu_parse.hip) and the file sweep with one
(freesasa_gpu_sweep_files_classified) on the host and the device parser, resumable and over a list of devices.

The bars: the host loader under the same classifier (itself pinned to the reference by tests/test_classifier.py), bit for
bit; the reference's own L&R / S&R totals under the NACCESS radii (tests/golden/ingest_classifiers.json); and the done-list
rule that a sweep under one classifier never resumes from another's."""
import json
import os

import numpy as np
import pytest

from freesasa_amd import ingest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(GOLD, "classifiers")
LOADABLE = ["protor", "naccess", "oons", "synthetic"]
EVERYDAY = ["1ubq.pdb", "1a0q.pdb", "3bkr.pdb", "5dx9.pdb", "1ubq.cif", "3bkr.cif"]
with open(os.path.join(GOLD, "ingest_classifiers.json")) as fh:
    VECTORS = json.load(fh)
NAMES = sorted(VECTORS["vectors"]["naccess"])
OPTION_SETS = [0, 1, 4, 5, 32, 128, 64, 129, 37]   # (RADIUS_FROM_OCCUPANCY: the device refuses it outright)


def fixture(name):
    if name.startswith("syn_any"):
        return os.path.join(CFG, name)
    return os.path.join(GOLD, "cif" if name.endswith(".cif") else "pdb", name)


def classifier(name):
    return ingest.Classifier(path=os.path.join(CFG, name + ".config"))


@pytest.fixture(scope="module")
def fa():
    import freesasa_amd
    assert freesasa_amd.device_count() > 0
    return freesasa_amd


@pytest.mark.parametrize("cfg", LOADABLE)
def test_device_parser_equals_the_host_loader_under_every_classifier(fa, cfg):
    c = classifier(cfg)
    paths = [fixture(n) for n in NAMES]
    for opt in OPTION_SETS:
        xyz, r, cls, offs, status, host = fa.parse_files_dev(paths, ingest_options=opt, n_threads=3, classifier=c)
        b = ingest.load_pdb_files(paths, options=opt, classifier=c)
        for k, n in enumerate(NAMES):
            if host[k]:
                assert n not in EVERYDAY, (cfg, n, opt)
                continue
            assert status[k] == b.status[k], (cfg, n, opt)
            a0, a1, h0, h1 = offs[k], offs[k + 1], b.offsets[k], b.offsets[k + 1]
            assert a1 - a0 == h1 - h0, (cfg, n, opt)
            assert xyz[a0:a1].tobytes() == b.xyz[h0:h1].tobytes(), (cfg, n, opt)
            assert r[a0:a1].tobytes() == b.radii[h0:h1].tobytes(), (cfg, n, opt)
            assert cls[a0:a1].tobytes() == b.atom_class[h0:h1].tobytes(), (cfg, n, opt)
        assert host.sum() < len(NAMES) // 2


def test_sweep_under_naccess_matches_the_host_batch_and_the_reference(fa):
    nac = classifier("naccess")
    names = sorted(set(NAMES) - {"1ubq.occ.pdb"})
    paths = [fixture(n) for n in names]
    b = ingest.load_pdb_files(paths, classifier=nac)
    for alg, res, key in ((fa.LEE_RICHARDS, 20, "lr20"), (fa.SHRAKE_RUPLEY, 100, "sr100")):
        sasa, _, want = fa.calc_batch(b.xyz, b.radii, b.offsets, alg=alg, resolution=res)
        runs = [fa.sweep_files(paths, alg=alg, resolution=res, n_threads=4, batch_atoms=3000, classifier=nac, ingest_options=o)
                for o in (0, ingest.PARSE_ON_DEVICE)]
        for totals, cls, atoms, status in runs:
            assert totals.tobytes() == want.tobytes()
            assert np.array_equal(atoms, np.diff(b.offsets)) and np.array_equal(status, b.status)
            for k in range(len(names)):
                s = sasa[b.offsets[k]:b.offsets[k + 1]]
                c = b.atom_class[b.offsets[k]:b.offsets[k + 1]]
                for q in range(3):
                    assert abs(cls[k, q] - s[c == q].sum()) <= 1e-9 * max(1.0, totals[k])
        for x, y in zip(runs[0], runs[1]):
            assert np.array_equal(x, y)                           # host parser and device parser: the same bits
        for n, tot in VECTORS["totals"].items():
            k = names.index(n)
            assert abs(want[k] - tot[key]) < 1e-8, n
            if key == "sr100":
                # S&R is exact per atom: the reference's total is the atoms' areas summed in order (src/sasa_sr.c), bit for bit
                assert sum(sasa[b.offsets[k]:b.offsets[k + 1]].tolist()) == tot[key], n
        if alg == fa.LEE_RICHARDS:
            pro = fa.sweep_files(paths, n_threads=4, batch_atoms=3000)
            ok = [k for k in range(len(names)) if b.status[k] == 0]
            assert not np.array_equal(pro[1][ok], runs[0][1][ok])    # the classifier was applied: NACCESS counts S and P apolar


def test_resumable_sweep_with_a_classifier(fa, tmp_path):
    nac, oons = classifier("naccess"), classifier("oons")
    paths = [fixture(n) for n in sorted(set(NAMES) - {"1ubq.occ.pdb"})] * 2
    _, want_t, want_c, want_a, want_s = fa.sweep_files_resumable(paths, tmp_path / "full.txt", batch_atoms=4000, classifier=nac)
    done = tmp_path / "d.txt"
    ok, *_ = fa.sweep_files_resumable(paths, done, batch_atoms=4000, max_new_batches=1, classifier=nac,
                                      ingest_options=ingest.PARSE_ON_DEVICE)
    assert not ok
    head = done.read_text().splitlines()[0]
    assert head.endswith(" classifier=%016x" % nac.digest)
    for other in (dict(classifier=oons), {}):
        with pytest.raises(RuntimeError, match="other parameters"):
            fa.sweep_files_resumable(paths, done, batch_atoms=4000, **other)
    ok, t, c, a, s = fa.sweep_files_resumable(paths, done, batch_atoms=4000, classifier=nac)
    assert ok
    for x, y in ((t, want_t), (c, want_c), (a, want_a), (s, want_s)):
        assert x.tobytes() == y.tobytes()
    # a done-list written without a classifier keeps its first line and still resumes through the old entry
    plain = tmp_path / "p.txt"
    ok, *_ = fa.sweep_files_resumable(paths, plain, batch_atoms=4000, max_new_batches=1)
    assert not ok and "classifier=" not in plain.read_text()
    with pytest.raises(RuntimeError, match="other parameters"):
        fa.sweep_files_resumable(paths, plain, batch_atoms=4000, classifier=nac)
    ok, t, *_ = fa.sweep_files_resumable(paths, plain, batch_atoms=4000)
    assert ok and t.tobytes() == fa.sweep_files(paths, batch_atoms=4000)[0].tobytes()


def test_two_workers_on_one_device_and_an_oversized_table(fa):
    nac = classifier("naccess")
    paths = [fixture(n) for n in sorted(set(NAMES) - {"1ubq.occ.pdb"})] * 3
    one = fa.sweep_files(paths, batch_atoms=5000, classifier=nac, ingest_options=ingest.PARSE_ON_DEVICE)
    two = fa.sweep_files(paths, batch_atoms=5000, classifier=nac, ingest_options=ingest.PARSE_ON_DEVICE, devices=[0, 0])
    for x, y in zip(one, two):
        assert np.array_equal(x, y)
    # a table beyond the device parser's 16384 rows: every file goes to the host parser, counted, and the sweep still runs
    rows = [f"R{i // 1000:02d} A{i % 1000:03d} C" for i in range(17000)]
    big = ingest.Classifier(text="name: big\ntypes:\nC 1.7 apolar\nO 1.4 polar\natoms:\n" + "\n".join(rows) +
                            "\nANY N O\nANY CA C\nANY C C\nANY O O\nANY CB C\n")
    fa.sweep_parse_stats()
    got = fa.sweep_files(paths, batch_atoms=5000, classifier=big, ingest_options=ingest.PARSE_ON_DEVICE)
    dev, host = fa.sweep_parse_stats()
    assert dev == 0 and host == len(paths)
    want = fa.sweep_files(paths, batch_atoms=5000, classifier=big)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
