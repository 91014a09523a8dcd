"""Contained caps (lr2_prune_contained): the kept hits closed up before the pair records, the saturated list election, and
what the headline's build of the tile kernel costs in registers.  CPU only: the emulation of the kernel phases, a host build
of the election, and the compiler's resource report."""
import os
import re
import subprocess

import numpy as np
import pytest

import emu
import tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LK = 4  # LR2_PRUNE_LIST


def _with_prune(want, fn):
    old = os.environ.get("EMU_LR2_PRUNE")
    os.environ["EMU_LR2_PRUNE"] = str(want)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["EMU_LR2_PRUNE"]
        else:
            os.environ["EMU_LR2_PRUNE"] = old


def _hostile_geometry():
    """Neighbors either side of beta's cut, spheres that hold the atom, twins at 1e-9 A, a ring of equal caps."""
    rng = np.random.default_rng(11)
    pts = [(0.0, 0.0, 0.0, 1.8)]
    for k in range(40):
        d = 2.0 + 2.5 * rng.random()
        e = (1 if k % 2 else -1) * 10.0 ** rng.uniform(-12, -1)
        pts.append((-d, e * d, rng.uniform(-1.5, 1.5), rng.choice([1.2, 1.6, 1.9])))
    pts += [(0.3, 0.1, 0.2, 3.5), (0.31, 0.1, 0.2, 3.5 + 1e-9), (0.3 + 1e-9, 0.1, 0.2, 3.5)]
    for k in range(12):
        pts.append((3.0 * np.cos(k * np.pi / 6), 3.0 * np.sin(k * np.pi / 6), 0.0, 1.7))
    pts += [(6.0 + 3 * rng.random(), 4 * rng.random() - 2, 4 * rng.random() - 2, 1.5 + 0.5 * rng.random()) for _ in range(60)]
    p = np.array(pts)
    return p[:, :3].copy(), p[:, 3].copy()


def test_closed_up_hits_keep_every_bit_at_the_headline_shape():
    """The headline's tile shape (six atoms at 20 slices: two or three rounds of hits, most of them one round fewer once the
    contained caps are gone) and the 100-slice shape, with the kept hits closed up into the lowest places before P3: every area
    equals the unpruned build's bit for bit, on random coils and on hostile geometry."""
    L = emu._load()
    emu.set_lr2_opts(True, False)
    L.emu_set_lr2(1, 0, 0)  # the tile shape the host would choose
    xyz, r = tools.coil(3000, 91)[:2]
    hx, hr = _hostile_geometry()
    outs = {}
    try:
        for want in (0, 3, 4):
            res = []
            for ns in (20, 100):
                s, _, _, st = _with_prune(want, lambda: emu.run_batch(True, xyz, r, resolution=ns))
                if ns == 20:
                    assert st["TA"] == 6
                res.append(s)
                res.append(_with_prune(want, lambda: emu.run_batch(True, hx, hr, resolution=ns))[0])
            outs[want] = np.concatenate(res)
    finally:
        emu.set_lr2_opts(False, False)  # (the emulation's defaults, for the tests that follow in this process)
    assert np.all(np.isfinite(outs[0][:3000]))
    for want in (3, 4):
        assert np.array_equal(outs[0], outs[want], equal_nan=True), (want, float(np.nanmax(np.abs(outs[0] - outs[want]))))


@pytest.fixture(scope="module")
def last_bin(tmp_path_factory):
    """lr2_prune_last_bin, built for the host from the kernel's own header."""
    d = tmp_path_factory.mktemp("lastbin")
    src = d / "lastbin.cpp"
    src.write_text('#include <cstring>\n#include <cmath>\n#include "%s"\nextern "C" int last_bin(unsigned long long h) { return sasa::lr2_prune_last_bin(h); }\n'
                   % os.path.join(ROOT, "freesasa_amd", "csrc", "lr2_kernels.h"))
    so = str(d / "liblastbin.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DSASA_EMU", "-shared", "-o", so, str(src), "-lm"],
                   check=True)
    import ctypes as C
    lib = C.CDLL(so)
    lib.last_bin.argtypes = [C.c_ulonglong]
    lib.last_bin.restype = C.c_int
    return lambda counts: lib.last_bin(sum(int(c) << (8 * b) for b, c in enumerate(counts)))


def _want(counts):
    """The leading bins that together hold at most LK hits: the last one's index (-1: the first alone is too many)."""
    cum = 0
    for b, c in enumerate(counts):
        cum += c
        if cum > LK:
            return b - 1
    return 7


def test_list_election_saturates_for_crowded_sides(last_bin):
    """The byte-parallel election of a list's bins.  Running sums of raw counts wrapped once a side held 133 hits or more, and
    then more caps qualified than a list holds - which of them were listed followed their order of arrival.  With every bin
    saturated first, the listed bins hold at most LK hits for any histogram a tile can have (<= 192 hits), so the list is
    every qualifying hit, whatever the order."""
    rng = np.random.default_rng(3)
    cases = [[0] * 8, [LK] + [0] * 7, [LK + 1] + [0] * 7, [1] * 8, [0] * 7 + [192], [133] + [0] * 7, [0, 0, 2, 2, 129, 0, 0, 0],
             [1, 1, 1, 1, 60, 60, 60, 8], [0, 0, 0, 0, 0, 0, 4, 188]]
    for _ in range(4000):
        total = int(rng.integers(0, 193))
        cases.append(list(rng.multinomial(total, rng.dirichlet(np.full(8, 0.4)))))
    for counts in cases:
        tb = last_bin(counts)
        assert tb == _want(counts), (counts, tb)
        assert sum(counts[:tb + 1]) <= LK


def test_headline_build_keeps_its_registers():
    """The build the headline runs (k_lr2_tile<4, 0, 4, false, true, 1>, coils at 20 slices) closes the kept hits up with no
    scratch and no more VGPRs than before it did (125)."""
    path = os.path.join(ROOT, "freesasa_amd", "lib", "kernel_resources.txt")
    if not os.path.exists(path):
        pytest.skip("library was built without the resource report")
    txt = open(path).read()
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", txt, flags=re.S)
    seen = {name: (int(v), int(sc)) for name, v, sc in blocks}
    head = "_Z10k_lr2_tileILi4ELi0ELi4ELb0ELb1ELi1EEvN4sasa7Lr2ArgsE"
    assert head in seen
    assert seen[head][0] <= 125 and seen[head][1] == 0, seen[head]
    for n, (v, sc) in seen.items():
        if "k_lr2_tile" in n:
            assert sc == 0, (n, v, sc)
