"""The host loader (freesasa_amd/csrc/ingest.c) on GENERATED PDB / mmCIF files (tests/parse_gen.py) against vectors minted
from the reference library (tests/golden/make_parse_gen_golden.py -> tests/golden/parse_gen.json): for every family, file
and option set the loader fails where the reference fails, and holds what it holds - atom count, coordinates and radii
bit for bit, classes, residue boundaries and labels, as one 64-bit digest.  A case where the reference itself aborted
("crash") binds nobody.  The generators assert their own edges while they build; the cap on `takes is None` is checked here."""
import os

import numpy as np
import pytest

import parse_gen
from freesasa_amd import ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


host_view, expected = parse_gen.view_of, parse_gen.expected


@pytest.mark.parametrize("fam", sorted(parse_gen.FAMILIES))
def test_generators_hold_their_edges_and_the_cap_on_undecided_cases(fam):
    files = parse_gen.family(fam)                 # (the builders assert their edges while they build)
    names = [n for n, _, _ in files]
    assert len(set(names)) == len(names)
    undecided = [n for n, _, t in files if t is None]
    assert len(undecided) <= 0.05 * len(files), (fam, undecided)
    for n in undecided:
        assert parse_gen.NONE_REASON.get((fam, n)), (fam, n)
    assert all(t in (True, False, None) for _, _, t in files)
    assert list(expected(fam, 0)) == names        # (expected() checks that the vectors are of these generators)
    again = parse_gen.FAMILIES[fam]()             # fixed seeds: the same bytes every time
    assert [(n, t) for n, t, _ in again] == [(n, t) for n, t, _ in files]


def test_the_lines_batches_are_the_lines_family():
    B = parse_gen.lines_batches()
    assert [n for fs in B.values() for n, _, _ in fs] == [n for n, _, _ in parse_gen.family("lines")]
    T = {k: len(parse_gen.batch_text(fs)) for k, fs in B.items()}
    assert (T["len_mod16_0"] % 16, T["len_mod16_1"] % 16, T["len_mod16_15"] % 16) == (0, 1, 15)
    assert T["len_4096"] == 4096 and T["len_8192"] == 8192
    assert (len(B["one_file"]), len(B["two_files"]), len(B["thousand_files"])) == (1, 2, 1000)


@pytest.mark.parametrize("fam", sorted(parse_gen.FAMILIES))
def test_host_loader_against_the_reference_minted_vectors(fam):
    files = parse_gen.family(fam)
    checked, bound = 0, 0
    for opt in sorted({o for n, _, _ in files for o in parse_gen.options_of(fam, n)}):
        exp = expected(fam, opt)
        use = [(n, t) for n, t, _ in files if exp[n] != "-"]
        b = ingest.load_texts([t for _, t in use], options=opt, n_threads=4)
        wrong = []
        for k, (n, _) in enumerate(use):
            checked += 1
            if exp[n] == "crash":
                continue
            bound += 1
            got = host_view(b, k)
            if got != exp[n]:
                wrong.append((n, int(b.status[k]), got, exp[n]))
        assert not wrong, (fam, opt, len(wrong), wrong[:12])
    assert bound >= 0.9 * checked > 0


def test_the_16_byte_line_has_no_label_whatever_stands_behind_it():
    """A line of 15 characters and its newline: the reference reads its buffer's terminator where the label would be, so the line
    is skipped under a label in force - whatever the NEXT line, or the next file, begins with.  Known by construction: status and
    atom counts; the minted vectors hold the rest."""
    fs = {n: t for n, t, _ in parse_gen.family("pdb_lengths")}
    names = ["line16_then_atom.pdb", "line16_then_hetatm.pdb", "line16_then_remark.pdb", "line16_last_nl.pdb", "line16_last.pdb"]
    for opt, want in ((0, [4, 3, 3, 2, 2]), (ingest.INCLUDE_HETATM, [4, 4, 3, 2, 2])):
        for order in (names, names[::-1]):
            b = ingest.load_texts([fs[n] for n in order], options=opt, n_threads=1)
            assert (b.status == ingest.OK).all(), (opt, order, b.status)
            assert np.diff(b.offsets).tolist() == (want if order is names else want[::-1]), (opt, order)
            exp = expected("pdb_lengths", opt)
            assert [host_view(b, k) for k in range(len(order))] == [exp[n] for n in order]


@pytest.mark.parametrize("fam", sorted(parse_gen.FAMILIES))
def test_host_parsers_under_sanitizers_stand_alone(fam, tmp_path):
    """csrc/ingest.c compiled with -fsanitize=address,undefined into a program of its own (tests/emu/ingest_check), run as a child
    process over the family's files, every text in a block of exactly its size: no sanitizer report - a parser that looks at
    the byte behind a text, as the 16-byte line's label once did, ends the program -, and the library's status and counts."""
    import subprocess
    subprocess.run(["make", "-C", ROOT, "tests/emu/ingest_check"], check=True, stdout=subprocess.DEVNULL)
    files = parse_gen.family(fam)
    for name, data, _ in files:
        (tmp_path / name).write_bytes(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")        # (the loader keeps its arenas for the next call)
    for opt in (0, parse_gen.HETATM | parse_gen.HYDROGEN | parse_gen.JOIN):
        res = subprocess.run([os.path.join(ROOT, "tests", "emu", "ingest_check"), str(opt)] + [str(tmp_path / n) for n, _, _ in files],
                             capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 0, res.stderr[-3000:]
        assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
        b = ingest.load_texts([t for _, t, _ in files], options=opt, n_threads=2)
        want = [f"{int(b.status[k])} {int(b.offsets[k + 1] - b.offsets[k])} {int(b.res_offsets[k + 1] - b.res_offsets[k])}" for k in range(len(files))]
        assert res.stdout.splitlines() == want
