"""Generated PDB / mmCIF inputs for the parsers: the host loader (freesasa_amd/csrc/ingest.c) and the device parser
(freesasa_amd/csrc/gpu_parse.hip).  Pure Python, fixed seeds, no product code.

Every family is a function that returns a list of (name, bytes, takes).  `takes` is what the header comment of
gpu_parse.hip promises for the file, known from how the file was built:
    True   an everyday form: the device parses it itself under every option set but RADIUS_FROM_OCCUPANCY
    False  the device refuses it (the file goes to the host parser)
    None   either is acceptable; only for single cases, each with a one-line reason in NONE_REASON, at most 5 % of a family
The builders assert their own edges ("this batch has a newline at byte 4095") so that a change to a builder cannot
quietly move a case off the edge it was made for.  What the files must parse TO is not decided here: the reference
library decides (tests/golden/make_parse_gen_golden.py -> tests/golden/parse_gen.json).

A batch of files lies in the device's text buffer one file after the other, every file followed by one '\\n' of the
driver's (batch_text() below); positions "of the batch" are positions in that text."""
import hashlib
import json
import os
import random

import numpy as np

HETATM, HYDROGEN, JOIN, HALT, SKIP, OCC = 1, 1 << 2, 1 << 5, 1 << 6, 1 << 7, 1 << 8
ALL_OPTIONS = [0, HETATM, HYDROGEN, HETATM | HYDROGEN, JOIN, SKIP, HALT, HETATM | SKIP, OCC, HETATM | HYDROGEN | JOIN]
THIN_OPTIONS = [0, HETATM | HYDROGEN, JOIN, HALT]          # the two largest families
NONE_REASON = {}                                           # (family, name) -> why takes is None

CHUNK = 64        # lines per step of kp_resolve
GROUP = 16        # bytes per thread of the line kernels
BLOCK = 4096      # bytes per workgroup of the line kernels


def options_of(family, name=""):
    """the option sets a file of a family is minted and tested under"""
    opts = {"lines": THIN_OPTIONS, "pdb_truncated": THIN_OPTIONS, "altloc": ALL_OPTIONS + [SKIP | HALT]}.get(family, ALL_OPTIONS)
    if name.endswith(".cif"):
        opts = [o for o in opts if o != OCC]       # (the reference's mmCIF reader has no such option)
    return opts


def digest(n_atoms, xyz, radii, classes, res_first, labels):
    """64 bits over what a reader holds for one file: atom count, coordinates and radii (their bits), classes, residue
    boundaries (first atom of every residue, then the atom count) and the residues' labels "name|number|chain"."""
    h = hashlib.blake2b(digest_size=8)
    h.update(np.int64(n_atoms).tobytes())
    h.update(np.ascontiguousarray(xyz, dtype=np.float64).tobytes())
    h.update(np.ascontiguousarray(radii, dtype=np.float64).tobytes())
    h.update(np.ascontiguousarray(classes, dtype=np.uint8).tobytes())
    h.update(np.ascontiguousarray(res_first, dtype=np.int64).tobytes())
    h.update("\n".join(labels).encode())
    return h.hexdigest()


def view_of(b, k):
    """what the digest covers, for input k of a loaded batch (anything with the fields of freesasa_amd.ingest.Batch): "fail", or
    the digest of what the loader holds for it"""
    if b.status[k] != 0:
        assert b.offsets[k + 1] == b.offsets[k]
        return "fail"
    lo, hi = int(b.offsets[k]), int(b.offsets[k + 1])
    rl, rh = int(b.res_offsets[k]), int(b.res_offsets[k + 1])
    labels = [f"{b.res_name_raw[r].decode('latin-1')}|{b.res_number_raw[r].decode('latin-1')}|{b.res_chain_raw[r].decode('latin-1')}" for r in range(rl, rh)]
    return digest(hi - lo, b.xyz[lo:hi], b.radii[lo:hi], b.atom_class[lo:hi], np.append(b.res_first[rl:rh] - lo, hi - lo), labels)


_gold = None


def names_digest(fam):
    return hashlib.blake2b("\n".join(n for n, _, _ in family(fam)).encode(), digest_size=8).hexdigest()


def expected(fam, opt):
    """{name: entry} of a family under an option set, from tests/golden/parse_gen.json: a digest, "fail", "crash" (the reference
    aborted: nobody is bound) or "-" (not an option set of that file).  The file keeps every distinct entry once ("entries"),
    every distinct row of entries over the option sets once ("rows", indices into the entries), and per file its row ("files")."""
    global _gold
    if _gold is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parse_gen.json")) as fh:
            _gold = json.load(fh)
    g = _gold[fam]
    assert g["names"] == names_digest(fam) and len(g["files"]) == len(family(fam)), \
        "tests/golden/parse_gen.json is not of these generators: run its recipe again"
    col = g["options"].index(opt)
    return {n: g["entries"][g["rows"][r][col]] for (n, _, _), r in zip(family(fam), g["files"])}


def batch_text(files):
    """the text of a batch as the device sees it"""
    return b"".join(t + b"\n" for _, t, _ in files)


# ------------------------------------------------------------------ PDB lines
def c83(m):
    """thousandths -> the "%8.3f" field, made from integers (no float formatting in between)"""
    if isinstance(m, str):
        assert len(m) == 8
        return m
    s = ("-" if m < 0 else "") + f"{abs(m) // 1000}.{abs(m) % 1000:03d}"
    assert len(s) <= 8, s
    return s.rjust(8)


def place(i):
    """thousandths: a lattice of 3.8 A, no two atoms of a file at one place"""
    return ((i % 40) * 3800, ((i // 40) % 40) * 3800 - 20000, (i // 1600) * 3800 + 1500)


ALA = [(" N  ", " N"), (" CA ", " C"), (" C  ", " C"), (" O  ", " O"), (" CB ", " C")]


def atom(serial, name=" CA ", res="ALA", chain="A", num=1, xyz=None, alt=" ", rec="ATOM  ", icode=" ", elem=" C", coords=None):
    c = coords if coords is not None else "".join(c83(v) for v in (xyz if xyz is not None else place(serial)))
    assert len(c) == 24 and len(name) == 4 and len(res) == 3 and len(rec) == 6 and len(elem) == 2 and len(chain) == 1
    line = f"{rec}{serial % 100000:5d} {name}{alt}{res} {chain}{num % 10000:4d}{icode}   {c}  1.00 10.00          {elem}  "
    assert len(line) == 80
    return line


def ala(i, **kw):
    """atom i of a chain of alanines, five atoms per residue"""
    name, elem = ALA[i % 5]
    kw.setdefault("num", i // 5 + 1)
    return atom(i, name=name, elem=elem, **kw)


def text(lines, final_newline=True):
    t = "\n".join(lines) + ("\n" if final_newline and lines else "")
    return t.encode("latin-1")


def filler(nbytes):
    """a file of exactly nbytes bytes that keeps no atom: REMARK lines of at most 100 bytes, the last byte a newline"""
    assert nbytes >= 7, nbytes
    parts, left = [], nbytes
    while left > 160:
        parts.append(80)
        left -= 80
    parts += [left] if left < 16 else [left // 2, left - left // 2]
    out = b"".join(b"REMARK" + b"x" * (p - 7) + b"\n" for p in parts)
    assert len(out) == nbytes and max(parts) <= 100 and min(parts) >= 7
    return out


# ------------------------------------------------------------------ family: lines
def lines_batches():
    """{batch name: [(name, bytes, takes)]}: the batches whose LAYOUT is the case (kp_count_nl, kp_scan_blocks, kp_line_starts)."""
    B = {}
    # --- edges: newlines on chosen bytes of the batch
    files, pos = [], 0

    def add(name, t):
        nonlocal pos
        files.append((f"edges_{name}.pdb", t, True))
        pos += len(t) + 1
        return pos - len(t) - 1

    def align(name, target):
        if target - pos - 1 < 7:
            raise AssertionError((name, target, pos))
        add(name, filler(target - pos - 1))
        assert pos == target

    p = add("mod16", text([ala(i) for i in range(16)]))
    marks = {"mod16": (p, 16 * 81)}
    align("fill_a", 4095 - 80)
    marks["nl4095"] = add("nl4095", text([ala(100)]))
    marks["nl4097"] = add("nl4097", b"\n" + text([ala(101)]))
    align("fill_b", (pos + 7 + 15 + 16) // 16 * 16)
    marks["nl16"] = add("nl16", b"\n" * 20 + text([ala(102)]))
    align("fill_c", (pos + 7 + 15 + 16) // 16 * 16)
    marks["al16"] = add("al16", text([ala(110 + i) for i in range(15)]))
    marks["al16_end"] = pos
    align("fill_d", (pos + 7 + BLOCK) // BLOCK * BLOCK)
    marks["al4096"] = add("al4096", text([ala(130 + i) for i in range(50)]) + filler(45))
    marks["al4096_end"] = pos
    pad = []
    for k, length in enumerate(range(54, 119)):
        pad.append(ala(200 + k)[:54].ljust(length))
        if k % 5 == 0:
            pad.append("")
    add("padded", text(pad))
    T = batch_text(files)
    nl = {i for i, b in enumerate(T) if b == 10}
    p, n = marks["mod16"]
    assert {i % GROUP for i in nl if p <= i < p + n} == set(range(GROUP))                 # a newline on every residue mod 16
    assert {4095, 4096, 4097} <= nl and marks["nl4095"] == 4095 - 80 and marks["nl4097"] == 4097
    assert marks["nl16"] % GROUP == 0 and all(marks["nl16"] + k in nl for k in range(GROUP))  # 16 newlines in one group
    assert marks["al16"] % GROUP == 0 and marks["al16_end"] % GROUP == 0
    assert marks["al4096"] % BLOCK == 0 and marks["al4096_end"] % BLOCK == 0 and marks["al4096_end"] - marks["al4096"] == BLOCK
    assert sorted({len(l) for l in pad if l}) == list(range(54, 119)) and "" in pad
    B["edges"] = files

    # --- the batch text's length: mod 16 = 0, 1, 15; exactly one block, exactly two
    def sized(name, n_lines, T_want=None, mod=None):
        a = text([ala(i) for i in range(n_lines)])
        f = (T_want - len(a) - 2) if T_want is not None else next(f for f in range(7, 23) if (len(a) + f + 2) % GROUP == mod)
        fs = [(f"{name}_a.pdb", a, True), (f"{name}_b.pdb", filler(f), True)]
        Tn = len(batch_text(fs))
        assert (Tn == T_want) if T_want is not None else (Tn % GROUP == mod)
        B[name] = fs
    sized("len_mod16_0", 1, mod=0)
    sized("len_mod16_1", 1, mod=1)
    sized("len_mod16_15", 1, mod=15)
    sized("len_4096", 40, T_want=BLOCK)
    sized("len_8192", 90, T_want=2 * BLOCK)

    # --- 1, 2 and 1000 one-line files; zero-byte files next to each other
    def one_line(k):
        return text([ala(k, num=k % 9999 + 1)], final_newline=k % 2 == 0)
    B["one_file"] = [("one_0.pdb", one_line(0), True)]
    B["two_files"] = [(f"two_{k}.pdb", one_line(k + 1), True) for k in range(2)]
    B["thousand_files"] = [(f"thousand_{k:04d}.pdb", one_line(k), True) for k in range(1000)]
    B["empty_files"] = [("empty_a.pdb", one_line(3), True), ("empty_b.pdb", b"", True), ("empty_c.pdb", b"", True),
                        ("empty_d.pdb", b"", True), ("empty_e.pdb", one_line(4), True), ("empty_f.pdb", b"", True)]
    assert [len(t) for _, t, _ in B["empty_files"]].count(0) == 4
    return B


def lines():
    return [f for fs in lines_batches().values() for f in fs]


# ------------------------------------------------------------------ family: pdb_lengths
LENGTHS = [3, 4, 6, 12, 13, 15, 16, 17, 19, 20, 21, 26, 27, 53, 54, 55, 76, 77, 78, 79, 80, 81, 118, 119, 120]   # every n parse_pdb_line names


def label_context(kind):
    """(lines before the line under test, its label)"""
    if kind == "nolabel":
        return [ala(0), ala(1)], " "
    first = [ala(0, alt="A"), ala(1, alt="A")]
    return (first, "A") if kind == "inforce" else (first, "B")


def short_line_takes(chars, newline):
    """a candidate atom line of `chars` characters: n = chars (+ 1 with its newline) as parse_pdb_line counts it"""
    n = chars + (1 if newline else 0)
    if n > 119:
        return False                 # over the reference's 119-byte chunk
    if n >= 54 and chars < 54:
        return False                 # the newline stands inside the z field: not "%8.3f"
    return True                      # complete coordinates, or too short for them (an error the device reports itself)


def pdb_lengths():
    out = []
    for kind in ("nolabel", "inforce", "other"):
        before, lab = label_context(kind)
        full = ala(2, alt=lab).ljust(121)
        for n in LENGTHS:
            for where in ("inner", "last_nl", "last"):
                chars = n if where == "last" else n - 1       # n counts the newline where there is one
                cutl = full[:chars]
                assert len(cutl) == chars
                if where == "inner":
                    t = text(before + [cutl, ala(3)])
                else:
                    t = text(before + [cutl], final_newline=where == "last_nl")
                out.append((f"len_{kind}_{n:03d}_{where}.pdb", t, short_line_takes(chars, where != "last")))
        # an embedded NUL at each of those positions of a 118-character line
        for k in [n for n in LENGTHS if n < 118]:
            l = ala(2, alt=lab).ljust(118)
            l = l[:k] + "\0" + l[k + 1:]
            assert len(l) == 118 and l[k] == "\0"
            out.append((f"nul_{kind}_{k:03d}.pdb", text(before + [l, ala(3)]), True))
    # the 16-byte line: 15 characters and the newline, under a label, then a line whose first byte used to be taken for the label
    short = ala(2, alt="A")[:15]
    assert len(short) + 1 == 16
    for nxt_name, nxt in (("atom", ala(3)), ("hetatm", atom(3, " O  ", "HOH", "A", 9, rec="HETATM", elem=" O")), ("remark", "REMARK   1")):
        out.append((f"line16_then_{nxt_name}.pdb", text([ala(0, alt="A"), ala(1, alt="A"), short, nxt, ala(4)]), True))
    out.append(("line16_last_nl.pdb", text([ala(0, alt="A"), ala(1, alt="A"), short]), True))
    out.append(("line16_last.pdb", text([ala(0, alt="A"), ala(1, alt="A"), short + " "], final_newline=False), True))   # 16 characters, no newline: n = 16
    out.append(("line16_nolabel.pdb", text([ala(0), ala(1), short, ala(3, alt="A"), ala(4)]), True))
    out.append(("line21_chain.pdb", text([ala(0), ala(2)[:20], ala(3)]), True))                # n == 21: the chain column's twin of the case
    # CRLF
    out.append(("crlf_full.pdb", text([ala(i) for i in range(5)]).replace(b"\n", b"\r\n"), True))
    out.append(("crlf_cut54.pdb", text([ala(0), ala(1)[:54], ala(2)]).replace(b"\n", b"\r\n"), True))
    # record names
    for v in ("ATOMX ", "atom  ", "HETATM", "ENDMDL", "ENDMDLX", "END   ", "ENDMD ", "HETAT "):
        l = v + ala(2)[len(v):]
        assert len(l) == 80
        out.append((f"record_{v.strip()}.pdb", text([ala(0), ala(1), l, ala(3)]), True))
    # the hydrogen rule: element columns x the name's first two columns
    for ename, elem in (("H", " H"), ("D", " D"), ("blank", "  "), ("absent", None)):
        for c0 in " 1590HD":
            for c1 in "HDC":
                l = atom(1, name=c0 + c1 + "1 ", elem=elem or "  ")
                if elem is None:
                    l = l[:76]
                out.append((f"hyd_{ename}_{c0.replace(' ', '_')}{c1}.pdb", text([ala(0), l, ala(2)]), True))
    assert len({n for n, _, _ in out}) == len(out)
    return out


# ------------------------------------------------------------------ family: pdb_truncated
def pdb_truncated():
    base_lines = [ala(0), ala(1), ala(2), ala(3, alt="A"), ala(3, alt="B"),
                  atom(5, " O  ", "HOH", "A", 50, rec="HETATM", elem=" O"), "REMARK 465 nothing to see", ala(4), "ENDMDL",
                  ala(5), ala(6)]
    base = text(base_lines)
    atom_like = {0: "atom", 1: "atom", 2: "atom", 3: "atom", 4: "atom", 5: "hetatm", 7: "atom", 9: "later", 10: "later"}
    prefixes = [b"", text([atom(90, " O  ", "HOH", "B", 90, rec="HETATM", elem=" O")]), b"REMARK   2 first line\n"]
    starts = [0]
    for l in base_lines:
        starts.append(starts[-1] + len(l) + 1)
    out, k = [], 0
    for c in range(len(base) + 1):
        li = base[:c].count(b"\n")
        chars = c - starts[li]
        for newline in (False, True):
            takes, kind = True, atom_like.get(li)
            if newline and chars == 53 and kind:            # the appended newline stands inside the z field
                takes = False if kind == "atom" else None
            name = f"cut_{c:04d}{'_nl' if newline else ''}.pdb"
            if takes is None:
                NONE_REASON[("pdb_truncated", name)] = ("a HETATM line: a candidate only with INCLUDE_HETATM" if kind == "hetatm"
                                                        else "behind ENDMDL: looked at only with JOIN_MODELS")
            out.append((name, prefixes[k % 3] + base[:c] + (b"\n" if newline else b""), takes))
            k += 1
            if k % 12 == 0:
                out.append((f"data_{k:04d}.cif", b"data_x\n", False))    # mmCIF without an _atom_site loop: the host's
    firsts = [t[:6] for _, t, _ in out]
    for a, b in ((b"ATOM  ", b"HETATM"), (b"HETATM", b"REMARK"), (b"REMARK", b"ATOM  "), (b"REMARK", b"data_x"), (b"data_x", b"ATOM  ")):
        assert any(firsts[i] == a and firsts[i + 1] == b for i in range(len(firsts) - 1)), (a, b)   # each kind of file stands behind another
    assert sum(1 for _, t, _ in out if len(t) == 0) == 1
    return out


# ------------------------------------------------------------------ mmCIF
NEEDED = ["group_PDB", "auth_asym_id", "auth_seq_id", "pdbx_PDB_ins_code", "auth_comp_id", "auth_atom_id", "label_alt_id",
          "type_symbol", "Cartn_x", "Cartn_y", "Cartn_z", "pdbx_PDB_model_num"]


def cif_atom(i, name=None, comp="ALA", asym="A", seq=None, ins="?", alt=".", sym=None, xyz=None, model="1", group="ATOM"):
    n, e = ALA[i % 5]
    x, y, z = xyz if xyz is not None else place(i)
    num = lambda v: v if isinstance(v, str) else c83(v).strip()
    return {"group_PDB": group, "auth_asym_id": asym, "auth_seq_id": str(i // 5 + 1 if seq is None else seq), "pdbx_PDB_ins_code": ins,
            "auth_comp_id": comp, "auth_atom_id": n.strip() if name is None else name, "label_alt_id": alt,
            "type_symbol": e.strip() if sym is None else sym, "Cartn_x": num(x), "Cartn_y": num(y), "Cartn_z": num(z),
            "pdbx_PDB_model_num": str(model)}


def cif_text(rows, cols=NEEDED, sep=" ", eol="\n", head="data_GEN\n#\nloop_\n", tail="#\n", between=""):
    """rows: dicts (a row of the loop) or strings (a line as it is)"""
    body = ""
    for r in rows:
        body += (r if isinstance(r, str) else sep.join(r.get(c, "x") for c in cols)) + "\n" + between
    t = head + "".join(f"_atom_site.{c}\n" for c in cols) + body + tail
    return t.replace("\n", eol).encode("latin-1")


# ------------------------------------------------------------------ family: coords
def coords():
    out = []

    def pdb_of(name, triples, takes=True):
        out.append((name, text([ala(i, xyz=t) for i, t in enumerate(triples)]), takes))
    # a field whose eight columns are all taken (1000.000 and above) is the host's: nothing separates it from its neighbour
    wide = lambda triples: any(len(c83(v).strip()) == 8 and not c83(v).startswith("-") for t in triples for v in t)
    digit_counts = [1000, 12000, 123000, -1000, -12000, -123000, 123456, -123456, 1, 12, 123, -999999]
    tr = [(v, digit_counts[(k + 1) % len(digit_counts)], digit_counts[(k + 5) % len(digit_counts)]) for k, v in enumerate(digit_counts)]
    assert {len(c83(v).strip()) for v in digit_counts} == {5, 6, 7, 8} and not wide(tr)      # every digit count the device takes
    pdb_of("digits.pdb", tr)
    tr = [(1234000, 1000, 2000), (1000, 1234567, 2000), (1000, 2000, 1000000), (9999999, 9999999, 9999999), (1000, 9999999, -1000)]
    assert wide(tr)
    pdb_of("digits_wide.pdb", tr, False)
    ends = [0, "  -0.000", 1, -1, 999999, -999999, 999000, -999000, 999, -999]
    assert c83(9999999) == "9999.999" and c83(-999999) == "-999.999" and c83(1) == "   0.001" and c83(-1) == "  -0.001" and c83(0) == "   0.000"
    pdb_of("ends.pdb", [(ends[k], ends[(k + 3) % len(ends)], ends[(k + 7) % len(ends)]) for k in range(len(ends))])
    pdb_of("ends_wide.pdb", [(9999999, 0, 0), (0, -999999, 9999999), (9999000, 1000000, 1)], False)
    rng = random.Random(20240601)
    per = 510
    vals = [rng.randint(-999999, 999999) for _ in range(3000)] + [rng.randint(-999, 999) for _ in range(60)]
    assert min(vals) < -990000 and max(vals) > 990000 and len(vals) == 6 * per
    for k in range(0, len(vals), per):
        tr = [tuple(vals[j:j + 3]) for j in range(k, k + per, 3)]
        assert not wide(tr)
        pdb_of(f"seeded_{k // per:02d}.pdb", tr)
    vals = [rng.randint(-999999, 9999999) for _ in range(4 * per)]                    # 5100 seeded values in all, these over the whole range
    assert max(vals) > 9900000
    for k in range(0, len(vals), per):
        tr = [tuple(vals[j:j + 3]) for j in range(k, k + per, 3)]
        assert wide(tr)
        pdb_of(f"seeded_wide_{k // per:02d}.pdb", tr, False)
    # not "%8.3f": the host's strtod path
    good = c83(1500) + c83(2500)
    for name, sec in (("exponent", "   1e1  " + good), ("shifted", (" " + c83(1000) + good)[:24]),
                      ("plus", "  +1.000" + good), ("four_decimals", "  1.0000" + good), ("no_integer", "    .123" + good),
                      ("no_fraction", "     12." + good), ("lone_minus", "       -" + good), ("tab", " \t 1.000" + good),
                      ("exponent_z", good + " 2.5E-01"), ("shifted_left", (c83(1000) + good)[1:] + " ")):
        assert len(sec) == 24
        out.append((f"nonform_{name}.pdb", text([ala(0), ala(1, coords=sec), ala(2)]), False))
    # three fields filled by their '-': run together for the eye, three numbers for sscanf and for the device
    out.append(("minus_fills_fields.pdb", text([ala(0), ala(1, coords="-100.123-200.456-300.789"), ala(2)]), True))
    # mmCIF numbers: 1..15 digits, every split between integer and fraction, bare, with '-' and with '+'
    D = "123456789012345"
    toks = []
    for d in range(1, 16):
        for frac in range(0, d + 1):
            toks.append(D[:d - frac] + ("." + D[d - frac:d] if frac else ""))
    assert len(toks) == 135 and max(len(t.replace(".", "")) for t in toks) == 15 and ".1" in toks and "123456789012345" in toks
    out.append(("digits.cif", cif_text([cif_atom(i, xyz=(t, "-" + t, "+" + t)) for i, t in enumerate(toks)]), True))
    out.append(("forms.cif", cif_text([cif_atom(0, xyz=("-.5", "5.", "+1.5")), cif_atom(1, xyz=("0", "-0", "-0.000")), cif_atom(2)]), True))
    for name, tok in (("16_digits", "1234567890.123456"), ("16_digits_int", "1234567890123456"), ("dot", "."), ("minus", "-"), ("exponent", "1e3"), ("question", "?")):
        out.append((f"nonform_{name}.cif", cif_text([cif_atom(0), cif_atom(1, xyz=(1000, tok, 2000)), cif_atom(2)]), False))
    return out


# ------------------------------------------------------------------ family: altloc
UNKNOWN = dict(name=" XX ", elem=" C")


def alt_lines(spec):
    """spec: one item per line - ' ', 'A', 'B', 'C': an atom line with that label; 'R' a REMARK; 'H', 'h': a hydrogen (filtered
    without INCLUDE_HYDROGEN), blank or labelled B; 'T': a HETATM water; 'S' + label: a line too short for coordinates; 'U' + label:
    an atom the classifier does not know; 'E': ENDMDL"""
    out = []
    for i, s in enumerate(spec):
        if s in (" ", "A", "B", "C"):
            out.append(ala(i, alt=s))
        elif s == "R":
            out.append(f"REMARK {i:4d}")
        elif s in ("H", "h"):
            out.append(atom(i, " H  ", num=i // 5 + 1, elem=" H", alt=" " if s == "H" else "B"))
        elif s == "T":
            out.append(atom(i, " O  ", "HOH", "W", i, rec="HETATM", elem=" O"))
        elif s[0] == "S":
            out.append(ala(i, alt=s[1])[:40])
        elif s[0] == "U":
            out.append(atom(i, num=i // 5 + 1, alt=s[1], **UNKNOWN))
        elif s == "E":
            out.append("ENDMDL")
        else:
            raise AssertionError(s)
    return out


def is_candidate(s):
    """under the default options"""
    return s in (" ", "A", "B", "C") or s[0] in "SU"


def altloc():
    out = []
    rng = random.Random(7)
    for n in (1, 63, 64, 65, 127, 128, 129, 200):
        for k in range(4):
            spec = [rng.choices([" ", "A", "B", "C", "R", "H", "h", "T"], weights=[28, 20, 14, 8, 10, 6, 4, 10])[0] for _ in range(n)]
            out.append((f"seeded_{n:03d}_{k}.pdb", text(alt_lines(spec), final_newline=k != 3), True))
    built = {}

    def case(name, spec, check):
        assert check(spec), name
        built[name] = spec
        out.append((f"{name}.pdb", text(alt_lines(spec)), True))
    cands = lambda spec, lo, hi: [i for i in range(lo, min(hi, len(spec))) if is_candidate(spec[i])]
    # a label set in chunk 0, a chunk of 64 non-candidates, the label still in force in chunk 2
    case("carry_two_chunks", [" "] * 10 + ["A"] + ["R"] * 53 + ["R"] * 32 + ["H"] * 16 + ["T"] * 16 + ["B", "A", "B", " ", "B", "A"],
         lambda s: cands(s, 0, 64) == list(range(11)) and s[10] == "A" and not cands(s, 64, 128) and s[128:131] == ["B", "A", "B"])
    # the last candidate of a chunk blank / labelled, the next chunk begins with labels
    case("chunk_ends_blank", ["A"] * 20 + ["R"] * 43 + [" "] + ["B", "A", "B", " "], lambda s: s[63] == " " and cands(s, 0, 64)[-1] == 63 and s[64] == "B")
    case("chunk_ends_labelled", [" "] * 20 + ["R"] * 43 + ["A"] + ["B", "A", "B", " "], lambda s: s[63] == "A" and cands(s, 0, 64)[-1] == 63 and s[64] == "B")
    case("chunk_ends_labelled_inner", [" "] * 20 + ["A"] + ["R"] * 43 + ["B", "A", "B", " "], lambda s: cands(s, 0, 64)[-1] == 20 and s[20] == "A" and s[64] == "B")
    # the first candidate at lane 0 / lane 63
    case("first_at_lane_0", ["B"] + ["R"] * 63 + ["A", "B", " ", "A"], lambda s: cands(s, 0, 64) == [0])
    case("first_at_lane_63", ["R"] * 63 + ["B"] + ["A", "B", " ", "A"], lambda s: cands(s, 0, 64) == [63])
    # a short line under a label not in force (skipped) and in force (error), on both sides of a chunk edge
    for at in (63, 64):
        for lab, what in (("B", "skipped"), ("A", "error")):
            spec = [" ", "A"] + ["A"] * (at - 2) + ["S" + lab] + ["A", " ", " "]
            case(f"short_{what}_at_{at}", spec, lambda s, at=at: s[at][0] == "S" and len(s) == at + 4)
    # an unknown atom in chunk 1 and a short line in chunk 2, and the reverse
    case("unknown_then_short", [" "] * 70 + ["U "] + [" "] * 70 + ["S "] + [" "] * 3, lambda s: s[70] == "U " and s[141] == "S " and 64 <= 70 < 128 <= 141)
    case("short_then_unknown", [" "] * 70 + ["S "] + [" "] * 70 + ["U "] + [" "] * 3, lambda s: s[70] == "S " and s[141] == "U ")
    case("unknown_then_unknown_labelled", ["A"] * 70 + ["UB"] + ["A"] * 70 + ["UA"] + [" "] * 3, lambda s: s[70] == "UB" and s[141] == "UA")
    # ENDMDL as line 0, 63 and 64
    for at in (0, 63, 64):
        case(f"endmdl_at_{at}", [" "] * at + ["E"] + [" ", "A", "B"] + [" "] * 70 + ["E", " "], lambda s, at=at: s[at] == "E" and "E" not in s[:at])
    # files that keep no atom
    case("none_remarks", ["R"] * 70, lambda s: not cands(s, 0, len(s)))
    case("none_hydrogens", ["H"] * 70, lambda s: not cands(s, 0, len(s)))
    case("none_hetatm", ["T"] * 130, lambda s: not cands(s, 0, len(s)))
    case("none_behind_endmdl", ["E"] + [" "] * 5, lambda s: s[0] == "E")
    # mmCIF: the same rule over rows ('.' is the blank label, '?' is a label like any other)
    rng = random.Random(11)
    for n in (1, 63, 64, 65, 129, 200):
        rows = []
        for i in range(n):
            kind = rng.choices(["atom", "het", "h", "comment", "model2"], weights=[70, 8, 8, 7, 7])[0]
            alt = rng.choices([".", "A", "B", "C", "?"], weights=[35, 25, 20, 10, 10])[0]
            if kind == "comment":
                rows.append(f"# {i}")
            elif kind == "het":
                rows.append(cif_atom(i, name="O", comp="HOH", sym="O", group="HETATM", alt=alt))
            elif kind == "h":
                rows.append(cif_atom(i, name="H", sym="H", alt=alt))
            else:
                rows.append(cif_atom(i, alt=alt, model="2" if kind == "model2" and i > 0 else "1"))
        out.append((f"seeded_{n:03d}.cif", cif_text(rows), True))
    carry = [cif_atom(i) for i in range(10)] + [cif_atom(10, alt="A")] + [f"# {i}" for i in range(11, 128)] + [cif_atom(128 + k, alt=a) for k, a in enumerate("BAB.BA")]
    assert len(carry) == 134 and all(isinstance(r, str) for r in carry[64:128])
    out.append(("carry_two_chunks.cif", cif_text(carry), True))
    assert len({n for n, _, _ in out}) == len(out)
    return out


# ------------------------------------------------------------------ family: cif_rows
def cif_rows():
    out = []
    rows = lambda n=7, **kw: [cif_atom(i, **kw) for i in range(n)]

    def add(name, t, takes=True, why=None):
        if takes is None:
            NONE_REASON[("cif_rows", name + ".cif")] = why
        out.append((name + ".cif", t, takes))
    rng = random.Random(3)
    for k in range(3):
        cols = NEEDED[:]
        rng.shuffle(cols)
        add(f"permuted_12_{k}", cif_text(rows(), cols=cols))

    def widened(ncol, at=None):
        """the twelve among ncol columns, shuffled; at: a needed column at that index"""
        extra = [f"extra_{j}" for j in range(ncol - 12)]
        cols = NEEDED + extra
        rng.shuffle(cols)
        if at is not None:
            j = cols.index("Cartn_y")
            cols[j], cols[at] = cols[at], cols[j]
            assert cols[at] == "Cartn_y"
        assert len(cols) == ncol and set(NEEDED) <= set(cols)
        return cols
    add("cols_20", cif_text(rows(), cols=widened(20)))
    add("cols_64", cif_text(rows(), cols=widened(64)))
    add("cols_64_needed_at_63", cif_text(rows(), cols=widened(64, at=63)))
    add("cols_65_needed_at_64", cif_text(rows(), cols=widened(65, at=64)), False)     # wider than the device's table of 64 columns
    add("cols_70", cif_text(rows(), cols=widened(70)), False)
    # quoted tokens
    add("quoted", cif_text([cif_atom(0, name="'N'"), cif_atom(1, name='"CA"'), cif_atom(2, name='"O5\'"', comp="A", sym="O"), cif_atom(3, name="O"),
                            cif_atom(4, comp="'ALA'"), cif_atom(5, name="'CA'", sym='"C"')]))
    add("quoted_blank", cif_text([cif_atom(0), cif_atom(1, name="'a b'"), cif_atom(2)]), False)
    add("quoted_blank_comp", cif_text([cif_atom(0), cif_atom(1, comp='"A B"'), cif_atom(2)]), False)
    # comments, tabs, CRLF, empty lines
    add("comments", cif_text([cif_atom(0), "# alone on a line", cif_atom(1), " ".join(cif_atom(2)[c] for c in NEEDED) + " # behind a row", cif_atom(3)]))
    add("tabs", cif_text(rows(), sep="\t"))
    add("tabs_and_blanks", cif_text(rows(), sep=" \t  "))
    add("crlf", cif_text(rows(), eol="\r\n"))
    add("empty_lines", cif_text(rows(), between="\n"))
    add("leading_blanks", cif_text(["   " + " ".join(cif_atom(i)[c] for c in NEEDED) + "  " for i in range(5)]))
    # model numbers
    add("models_out_of_order", cif_text([cif_atom(i, model=m) for i, m in enumerate([3, 2, 3, 2, 5, 2, 3])]))
    add("models_negative", cif_text([cif_atom(i, model=m) for i, m in enumerate([1, -1, 1, -1, 0, -2, -2])]))
    add("models_9_digits", cif_text([cif_atom(i, model=m) for i, m in enumerate([123456789, 123456788, 123456789, 123456788])]))
    add("models_12_digits", cif_text([cif_atom(i, model=m) for i, m in enumerate([123456789012, 123456789011, 123456789012])]), None,
        "model numbers beyond an int: gpu_parse.hip's header is silent about them")
    # '.' and '?' as alt id and as insertion code
    add("alt_and_icode", cif_text([cif_atom(0, alt="."), cif_atom(1, alt="?"), cif_atom(2, alt="."), cif_atom(3, alt="A"), cif_atom(4, alt="?"),
                                   cif_atom(5, ins="."), cif_atom(6, ins="?"), cif_atom(7, ins="A"), cif_atom(8, ins="."), cif_atom(9, alt="B", ins="B")]))
    # H, h and D as symbol
    add("symbols", cif_text([cif_atom(0), cif_atom(1, name="H", sym="H"), cif_atom(2, name="H", sym="h"), cif_atom(3, name="D", sym="D"),
                             cif_atom(4, name="HA", sym="H"), cif_atom(5, name="QQ", sym="Q"), cif_atom(6, name="XX", sym="FE")]))
    # what ends the rows
    add("end_tag", cif_text(rows(), tail="_cell.length_a 10.0\n"))
    add("end_loop", cif_text(rows(), tail="loop_\n_other.id\n_other.value\n1 2\n3 4\n"))
    add("end_LOOP", cif_text(rows(), tail="LOOP_\n_other.id\n1\n2\n"))
    add("end_save", cif_text(rows(), tail="save_x\n_other.id 1\nsave_\n"))
    add("end_data", cif_text(rows(), tail="data_x\n_cell.length_a 10.0\n"), False)           # a second data block
    add("end_data_atoms", cif_text(rows(), tail="") + cif_text([cif_atom(i) for i in range(10, 13)], head="data_TWO\nloop_\n"), False)
    add("end_nothing", cif_text(rows(), tail="")[:-1])                                       # the last row without its newline
    # not one row per line
    add("keyword_behind_values", cif_text([cif_atom(0), " ".join(cif_atom(1)[c] for c in NEEDED) + " loop_", "_other.id", "1"]), False)
    r = [cif_atom(1)[c] for c in NEEDED]
    add("row_over_lines", cif_text([cif_atom(0), " ".join(r[:5]), " ".join(r[5:]), cif_atom(2)]), False)
    add("text_field", cif_text([cif_atom(0), " ".join(r[:5]), ";" + r[5], ";", " ".join(r[6:]), cif_atom(2)]), False)
    add("pair_form", ("data_PAIR\n" + "".join(f"_atom_site.{c} {cif_atom(0)[c]}\n" for c in NEEDED)).encode(), False)
    add("two_blocks_first_without", b"data_ONE\n_cell.length_a 10.0\n" + cif_text(rows(), head="data_TWO\nloop_\n"), False)
    return out


# ------------------------------------------------------------------ family: residues
def residues():
    """ORDER matters: the builder counts the atoms kept under the default options so that residue changes fall on atoms 63/64 and
    255/256 of the batch (kp_res_count / kp_res_build: a wave's edge, a workgroup's edge)."""
    out, total, edges = [], 0, []

    def add(name, lines, kept, takes=True, cif=None):
        nonlocal total
        out.append((name, cif if cif is not None else text(lines), takes))
        total += kept
    # 512 atoms per file: changes at the file's atoms 64 and 256 by number only, by chain only, by insertion code only
    for what in ("number", "chain", "icode"):
        ls = []
        for i in range(512):
            seg = (i >= 64) + (i >= 256)
            kw = dict(num=1, chain="A", icode=" ")
            if what == "number":
                kw["num"] = 1 + seg
            elif what == "chain":
                kw["chain"] = "ABC"[seg]
            else:
                kw["icode"] = " AB"[seg]
            name, elem = ALA[i % 5]
            ls.append(atom(i, name=name, elem=elem, xyz=place(i), **kw))
        edges += [(what, total + 64), (what, total + 256)]
        add(f"change_by_{what}.pdb", ls, 512)
    assert all(e % 64 == 0 for _, e in edges) and {e % 256 for _, e in edges} == {0, 64} and total == 1536
    # a file whose first kept atom has the number and chain of the last atom of the file before it
    add("same_key_a.pdb", [ala(i, num=7) for i in range(3)], 3)
    add("same_key_b.pdb", [atom(0, " H  ", num=7, elem=" H")] + [ala(i, num=7) for i in range(3, 6)], 3)   # (its first LINE is a filtered hydrogen)
    assert out[-2][1].split(b"\n")[-2][21:27] == out[-1][1].split(b"\n")[1][21:27] == b"A   7 "
    # residue names with blanks, in and out of the reference-area table
    names = ["ALA", "  A", " DA", "XYZ", "A  ", " A ", "GLY", "HOH", "UNK", "ASX", "  U", " DT", "CYS", "MSE"]
    add("residue_names.pdb", [atom(i, " P  " if r.strip() in ("A", "DA", "U", "DT") else " CA ", r, "A", i + 1, elem=" P" if r.strip() in ("A", "DA", "U", "DT") else " C")
                              for i, r in enumerate(names)], len(names))
    # atom names of 1 to 4 characters, in and out of the backbone list
    anames = [" N  ", " CA ", " C  ", " O  ", " OXT", " CB ", "C   ", "  N ", "   O", " C1'", " O5'", " P  ", " OP1", "HG21", " CG1", "CA  ", "N   "]
    add("atom_names.pdb", [atom(i, n, "ILE" if "G" in n else "ALA", "A", 1 + i // 6, elem="  ") for i, n in enumerate(anames)], len(anames))
    # element columns present, blank or absent
    ls = []
    for i in range(12):
        name, elem = ALA[i % 5]
        l = atom(i, name=name, elem=elem if i % 3 == 0 else "  ", num=1 + i // 5)
        ls.append(l[:60] if i % 3 == 2 else l)
    add("element_columns.pdb", ls, 12)
    # mmCIF: number + insertion code, chains cut to three characters, names cut to their widths
    rows = [cif_atom(0, seq=1), cif_atom(1, seq=1), cif_atom(2, seq=1, ins="A"), cif_atom(3, seq=1, ins="A"), cif_atom(4, seq=1, ins="B"),
            cif_atom(5, seq=2, asym="A"), cif_atom(6, seq=2, asym="B"), cif_atom(7, seq=2, asym="AAAA"), cif_atom(8, seq=2, asym="AAAB"),
            cif_atom(9, seq=123456), cif_atom(10, seq=123457), cif_atom(11, seq=12345, ins="A"), cif_atom(12, seq=-5), cif_atom(13, seq=-5, ins="."),
            cif_atom(14, comp="ALANINE", seq=9), cif_atom(15, comp="A", name="P", sym="P", seq=10), cif_atom(16, comp="DA", name='"C1\'"', seq=11),
            cif_atom(17, name="CG1X5", comp="ILE", seq=12), cif_atom(18, comp="XYZ", seq=13)]
    add("residues.cif", None, len(rows), cif=cif_text(rows))
    return out


FAMILIES = {"lines": lines, "pdb_lengths": pdb_lengths, "pdb_truncated": pdb_truncated, "coords": coords, "altloc": altloc,
            "cif_rows": cif_rows, "residues": residues}
_cache = {}


def family(name):
    """the family's files, built once"""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]
