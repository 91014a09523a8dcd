"""Records traj_entry_refusals.json: what every trajectory entry with a topology (include/freesasa_gpu.h: the memory form and
the file form of the topology, groups, statistics, interfaces, interface-residue, volume and mask entries, the periodic siblings
and the segments entry) answers for a list of single defects of its arguments AND for every pair of them - the return code and
the whole message.  Which refusal speaks first when two things are wrong is part of the interface; the table was recorded with the
library as it was BEFORE the entries were rewritten over one call description (gpu_drivers.hip, TrajCall), and
tests/test_traj_entry_refusals.py replays it.  No device and no frame file: the baseline of every entry is valid up to the device
check.  The argument lists are spelled here from named pieces, on their own: the prototypes of freesasa_amd must have their length.
Run from the repository root with a built library:  python tests/golden/make_traj_entry_refusals_golden.py"""
import ctypes as C
import itertools
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import freesasa_amd as fa  # noqa: E402
from freesasa_amd import ingest  # noqa: E402

NOWHERE = "/nonexistent/freesasa_amd/"
F, G, FA_MAX = 2, 2, 4          # frames of the memory form; groups; the frames hold room for up to FA_MAX atoms more than the structure's
PBC = fa.FRAMES_DCD | fa.FRAMES_PBC
# answers at or past the device check are the machine's: without a device the device list is refused, with one a frame file
# that does not exist is, and a memory-form run just runs (rc 0, no message); with them every entry's own baseline answer
PAST = ("no HIP device available: libfreesasa_amd has no CPU path", "cannot open the frame file", "")


def dimer_pdb():
    """two chains, 13 atoms: A = GLY 1, ALA 2; B = GLY 1"""
    atoms = [("N", "GLY", "A", 1), ("CA", "GLY", "A", 1), ("C", "GLY", "A", 1), ("O", "GLY", "A", 1),
             ("N", "ALA", "A", 2), ("CA", "ALA", "A", 2), ("C", "ALA", "A", 2), ("O", "ALA", "A", 2), ("CB", "ALA", "A", 2),
             ("N", "GLY", "B", 1), ("CA", "GLY", "B", 1), ("C", "GLY", "B", 1), ("O", "GLY", "B", 1)]
    lines = []
    for i, (name, res, chain, num) in enumerate(atoms):
        x, y, z = 1.4 * (i % 9), 3.5 * (chain == "B") + 0.6 * (i % 3), 0.9 * (i % 2) + 0.3 * (i % 5)
        lines.append("ATOM  %5d  %-3s %s %s%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s" % (i + 1, name, res, chain, num, x, y, z, name[0]))
    return "\n".join(lines) + "\nEND\n"


def dimer(tmp):
    """(batch, group ids [n]: chain A 0, chain B 1) of the dimer, loaded from a file written into tmp"""
    path = os.path.join(str(tmp), "dimer.pdb")
    with open(path, "w") as fh:
        fh.write(dimer_pdb())
    b = ingest.load_pdb_files([path])
    assert b.n_structs == 1 and b.status[0] == 0 and b.n_atoms == 13 and b.n_residues == 3
    return b, (np.arange(13) >= 9).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the argument lists, from pieces
MEM, FILE = ("xyz", "n_frames"), ("frames_path", "frames_f32", "header_bytes", "n_frames")
TOPO, GROUPS, PARAMS = ("batch", "structure", "frame_atoms", "atom_index", "sel"), ("group", "n_groups"), ("alg", "probe", "resolution", "frames_per_batch")
OUT5, GOUT = ("totals", "sasa", "class_sums", "residues", "sel_area", "sel_atoms"), ("group_areas", "iso")
DEVS, FTAIL = ("devices", "n_devices"), ("done_path", "max_new_shards", "devices", "n_devices", "frames_total")
STATS, PAIRS, PRES, ERR = ("stats", "stats_to", "partials_to"), ("pairs", "n_pairs", "pair_areas"), ("min_buried", "pair_res"), ("err", "err_len")
P = "freesasa_gpu_trajectory_"
ENTRIES = {
    P + "topology": MEM + TOPO + PARAMS + OUT5 + DEVS + ERR,
    P + "groups": MEM + TOPO + GROUPS + PARAMS + OUT5 + GOUT + DEVS + ERR,
    P + "groups_stats": MEM + TOPO + GROUPS + PARAMS + OUT5 + GOUT + DEVS + STATS + ERR,
    P + "interfaces": MEM + TOPO + GROUPS + PARAMS + OUT5 + GOUT + DEVS + STATS + PAIRS + ERR,
    P + "interface_residues": MEM + TOPO + GROUPS + PARAMS + OUT5 + GOUT + DEVS + STATS + PAIRS + PRES + ERR,
    P + "volume": MEM + TOPO + PARAMS + OUT5 + ("volumes",) + DEVS + ERR,
    P + "masks": MEM + TOPO + PARAMS + OUT5 + ("masks",) + DEVS + ERR,
    P + "interface_segments": ("batch", "structure") + GROUPS + ("pairs", "n_pairs", "seg_capacity", "n_segments", "seg_offsets", "seg_res", "seg_atoms") + ERR,
    P + "file_topology": FILE + TOPO + PARAMS + OUT5 + FTAIL + ERR,
    P + "file_groups": FILE + TOPO + GROUPS + PARAMS + OUT5 + GOUT + FTAIL + ERR,
    P + "file_groups_stats": FILE + TOPO + GROUPS + PARAMS + OUT5 + GOUT + FTAIL + STATS + ERR,
    P + "file_groups_periodic": FILE + TOPO + GROUPS + PARAMS + OUT5 + GOUT + FTAIL + STATS + ERR,
    P + "file_interfaces": FILE + TOPO + GROUPS + PARAMS + OUT5 + GOUT + FTAIL + STATS + PAIRS + ERR,
    P + "file_interfaces_periodic": FILE + TOPO + GROUPS + PARAMS + OUT5 + GOUT + FTAIL + STATS + PAIRS + ERR,
    P + "file_interface_residues": FILE + TOPO + GROUPS + PARAMS + OUT5 + GOUT + FTAIL + STATS + PAIRS + PRES + ERR,
    P + "file_interface_residues_periodic": FILE + TOPO + GROUPS + PARAMS + OUT5 + GOUT + FTAIL + STATS + PAIRS + PRES + ERR,
    P + "file_volume": FILE + TOPO + PARAMS + OUT5 + ("volumes",) + FTAIL + ERR,
    P + "file_masks": FILE + TOPO + PARAMS + OUT5 + ("masks",) + FTAIL + ERR,
}
PERIODIC = tuple(e for e in ENTRIES if e.endswith("_periodic"))
SR_ONLY = tuple(e for e in ENTRIES if e.endswith("volume") or e.endswith("masks"))


class System:
    """the dimer, one selection set and every array a valid call of any entry writes to (a machine with a device runs the memory form)"""

    def __init__(self, tmp):
        self.batch, self.ids = dimer(tmp)
        self.cb = self.batch._as_c()
        self.sel = ingest.Selection(["a, chain A"])
        n, R = self.batch.n_atoms, self.batch.n_residues
        self.n = n
        rng = np.random.default_rng(7)
        self.xyz = np.zeros((F, n + FA_MAX, 3))
        self.xyz[:, :n] = np.asarray(self.batch.xyz, dtype=np.float64).reshape(1, n, 3) + rng.uniform(-0.1, 0.1, (F, n, 3))
        self.xyz[:, n:] = 100.0 + 5.0 * np.arange(FA_MAX)[None, :, None]
        self.devices = np.zeros(1, dtype=np.int32)
        z = np.zeros
        self.mem = dict(totals=z(F), sasa=None, class_sums=z((F, 3)), residues=z((F, R, 6)), sel_area=z((F, 1)), sel_atoms=z(1, np.int64),
                        group_areas=z((F, G, 3)), iso=None, volumes=z(F), masks=z((F, n, 4), np.uint32), pair_areas=z((F, 4, 6)),
                        pair_res=z((F, 64, 4)), stats_to=z((4, 4096)), partials_to=None)
        self.n_segments, self.seg_offsets, self.seg_res, self.seg_atoms = C.c_longlong(0), z(9, np.int64), z(64, np.int32), z(64, np.int32)

    def baseline(self, entry):
        names = ENTRIES[entry]
        is_file = "frames_path" in names
        v = dict(xyz=self.xyz, n_frames=0 if is_file else F, frames_path=(NOWHERE + "frames").encode(), frames_f32=PBC if entry in PERIODIC else 0,
                 header_bytes=0, batch=C.byref(self.cb), structure=0, frame_atoms=self.n, atom_index=None, sel=self.sel.handle, group=self.ids,
                 n_groups=G, alg=fa.SHRAKE_RUPLEY if entry in SR_ONLY else fa.LEE_RICHARDS, probe=1.4, resolution=20, frames_per_batch=0,
                 devices=self.devices, n_devices=1, done_path=None, max_new_shards=0, frames_total=None, stats=0, stats_to=None, partials_to=None,
                 pairs=np.array([[0, 1]], np.int32), n_pairs=1, min_buried=0.0, seg_capacity=64, n_segments=C.byref(self.n_segments),
                 seg_offsets=self.seg_offsets, seg_res=self.seg_res, seg_atoms=self.seg_atoms)
        for k, a in self.mem.items():
            if k not in ("stats_to", "partials_to"):
                v[k] = (NOWHERE + k).encode() if is_file and k != "sel_atoms" and a is not None else a
        return {k: v[k] for k in names if k not in ERR}

    def stats_dest(self, entry):
        if "frames_path" in ENTRIES[entry]:
            return dict(stats_to=(NOWHERE + "stats").encode(), partials_to=(NOWHERE + "partials").encode())
        return dict(stats_to=self.mem["stats_to"])


def defects(sys_):
    """name -> f(entry, values) -> the arguments the defect sets ("stats|": bits or-ed into the word; "with|": arguments that go
    with it and are no defect), or None where the entry has no such argument or the defect is none there"""
    n, ids = sys_.n, sys_.ids
    has = lambda e, *ks: all(k in ENTRIES[e] for k in ks)
    run = lambda e: "totals" in ENTRIES[e]
    is_file = lambda e: has(e, "frames_path")
    dup = np.arange(n, dtype=np.int32)
    dup[1] = 0
    bad_id = ids.copy()
    bad_id[3] = G
    # (a statistics bit comes with somewhere for the statistics to go, "with|": the missing destination is a defect of its own)
    with_stats = lambda e, bits, **more: dict({"stats|": bits, "with|": sys_.stats_dest(e)}, **more) if has(e, "stats") else None
    refuses_bit3 = tuple(P + k for k in ("file_groups", "file_groups_stats", "file_interfaces", "file_interface_residues", "file_volume", "file_masks"))
    return {
        "batch NULL": lambda e, v: dict(batch=None),
        "structure out of range": lambda e, v: dict(structure=5),
        "frame_atoms too small": lambda e, v: dict(frame_atoms=n - 1) if run(e) else None,
        "frame_atoms != n without an index": lambda e, v: dict(frame_atoms=n + 2) if run(e) else None,
        "a duplicate index entry": lambda e, v: dict(atom_index=dup) if run(e) else None,
        "an unknown statistics bit": lambda e, v: with_stats(e, 1 << 20),
        "a statistics bit that needs groups": lambda e, v: with_stats(e, fa.STATS_BITS["groups"], group=None),
        "a statistics bit that needs a selection": lambda e, v: with_stats(e, fa.STATS_BITS["selections"], sel=None),
        "a statistics word with nowhere to go": lambda e, v: {"stats|": fa.STATS_BITS["totals"], "stats_to": None, "partials_to": None} if has(e, "stats") else None,
        "a group output without ids": lambda e, v: dict(group=None) if has(e, "group_areas") else None,
        "ids without a group output": lambda e, v: dict(group_areas=None, iso=None) if has(e, "group_areas") else None,
        "n_groups 0": lambda e, v: dict(n_groups=0) if has(e, "n_groups") else None,
        "an id >= n_groups": lambda e, v: dict(group=bad_id) if has(e, "group") else None,
        "pairs NULL": lambda e, v: dict(pairs=None) if has(e, "pairs") else None,
        "n_pairs 0": lambda e, v: dict(n_pairs=0) if has(e, "pairs") else None,
        "a pair with g >= h": lambda e, v: dict(pairs=np.array([[1, 0]], np.int32)) if has(e, "pairs") else None,
        "a duplicate pair": lambda e, v: dict(pairs=np.array([[0, 1], [0, 1]], np.int32), n_pairs=2) if has(e, "pairs") else None,
        "no pair destination and no pair bit": lambda e, v: dict({"pair_areas": None}, **({"pair_res": None} if has(e, "pair_res") else {})) if has(e, "pair_areas") else None,
        "min_buried NaN": lambda e, v: dict(min_buried=float("nan")) if has(e, "min_buried") else None,
        "selection outputs without a selection": lambda e, v: dict(sel=None) if run(e) else None,
        "frames NULL": lambda e, v: (dict(frames_path=None) if is_file(e) else dict(xyz=None)) if run(e) else None,
        "totals NULL": lambda e, v: dict(totals=None) if run(e) else None,
        "header_bytes -1": lambda e, v: dict(header_bytes=-1) if is_file(e) else None,
        "alg 2": lambda e, v: dict(alg=2) if run(e) else None,
        "alg 0 for volume and masks": lambda e, v: dict(alg=0) if e in SR_ONLY else None,
        "resolution 0": lambda e, v: dict(resolution=0) if run(e) else None,
        "resolution 129 for volume and masks": lambda e, v: dict(resolution=129) if e in SR_ONLY else None,
        "bit 3 set where it is refused": lambda e, v: dict(frames_f32=PBC) if e in refuses_bit3 else None,
        "bit 3 clear where it is required": lambda e, v: dict(frames_f32=fa.FRAMES_DCD) if e in PERIODIC else None,
        "bit 4 set with groups": lambda e, v: dict(frames_f32=PBC | fa.FRAMES_TRICLINIC) if is_file(e) and has(e, "group") and e not in PERIODIC else None,
        "n_frames 0 in the memory form": lambda e, v: dict(n_frames=0) if run(e) and not is_file(e) else None,
    }


def _same(a, b):
    return a is b or (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)) or \
        (not isinstance(a, np.ndarray) and not isinstance(b, np.ndarray) and a == b)


def call(L, entry, values):
    fn = getattr(L, entry)
    names = ENTRIES[entry]
    assert len(fn.argtypes) == len(names), (entry, len(fn.argtypes), len(names))
    err = C.create_string_buffer(512)
    args = []
    for name, ctype in zip(names[:-2], fn.argtypes):
        a = values[name]
        args.append(a.ctypes.data_as(ctype) if isinstance(a, np.ndarray) else a)
    rc = fn(*args, err, 512)
    return int(rc), err.value.decode()


def table(L, tmp):
    """(entries, defect names, rows of (entry, defects (), (d,) or (d, e), rc, message))"""
    sys_ = System(tmp)
    ds = defects(sys_)
    names = list(ds)
    rows = []
    for ei, entry in enumerate(ENTRIES):
        base = sys_.baseline(entry)
        rows.append((ei, (), ) + call(L, entry, base))
        sets = [ds[d](entry, base) for d in names]
        for combo in itertools.chain(((k,) for k in range(len(names))), itertools.combinations(range(len(names)), 2)):
            if any(sets[k] is None for k in combo):
                continue
            first, second = sets[combo[0]], sets[combo[-1]]
            if any(k[-1] != "|" and k in second and not _same(first[k], second[k]) for k in first):
                continue    # (two defects that set one argument to different things are no pair)
            v = dict(base, **first.get("with|", {}))
            v.update(second.get("with|", {}))
            v.update(first)
            v.update(second)
            v.pop("with|", None)
            if v.pop("stats|", 0):
                v["stats"] = first.get("stats|", 0) | second.get("stats|", 0)
            rows.append((ei, combo) + call(L, entry, v))
    sys_.sel.close()
    return list(ENTRIES), names, rows


def past(entries_rows):
    """the class of answers at or past the device check: PAST and what the baselines alone yield"""
    return set(PAST) | {msg for _, combo, _, msg in entries_rows if not combo}


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        entries, names, rows = table(fa._stats_proto(fa._topology_proto(fa.lib())), tmp)
    messages = sorted({r[3] for r in rows})
    at = {m: k for k, m in enumerate(messages)}
    with open(os.path.join(ROOT, "tests", "golden", "traj_entry_refusals.json"), "w") as f:
        json.dump({"entries": entries, "defects": names, "messages": messages,
                   "rows": [[e, list(c), rc, at[m]] for e, c, rc, m in rows]}, f, separators=(",", ":"))
        f.write("\n")
    print(len(rows), "rows,", len(messages), "distinct messages,", len(set(messages) - past(rows)), "of them before the device check")
