"""Records traj_done_heads.json: the first line of the done-list that every file entry of the trajectory drivers writes - the
plain ones and each entry with a topology - for a three-frame file of the 13-atom dimer of make_traj_entry_refusals_golden.py
(raw fp64; for the periodic entries a DCD file with a unit cell), its modification time set to a fixed value, run with
frames_per_batch = 2.  The line names the run (its parameters, the frame file, digests of the topology, the outputs) and decides
whether a later call resumes it: it is interface.  Recorded with the library as it was BEFORE the entries were rewritten over
one call description (gpu_drivers.hip, TrajCall); tests/test_traj_done_head_gpu.py replays it.  Needs a device.
Run from the repository root with a built library:  python tests/golden/make_traj_done_heads_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import freesasa_amd as fa  # noqa: E402
from freesasa_amd import ingest  # noqa: E402
from make_traj_entry_refusals_golden import dimer  # noqa: E402

F, FPB = 3, 2
MTIME_NS = 1_600_000_000_123_456_789
CELL = (31.0, 29.5, 33.25)
SR = dict(alg=fa.SHRAKE_RUPLEY, resolution=20)
GRP = dict(n_groups=2, group_areas_path="groups", isolated_path="iso")
PAIR = dict(GRP, interface_pairs="all", pair_areas_path="pairs")
PRES = dict(PAIR, pair_residues_path="pres", min_buried=0.5, stats=("pairs", "pair_residues"), stats_path="stats", partials_path="partials")
TOPO = dict(selection=True, sasa_path="sasa", class_sums_path="cls", residues_path="res", selections_path="sel")
# case -> (the Python call, its keywords: a string is a result file's name in the case's directory)
CASES = {
    "freesasa_gpu_trajectory_file": ("plain", dict(sasa_path="sasa")),
    "freesasa_gpu_trajectory_file_devices": ("plain", dict(devices=[0], out_f32=True, sasa_path="sasa")),
    "freesasa_gpu_trajectory_file_stats": ("plain", dict(stats=("totals", "atoms"), stats_path="stats", partials_path="partials")),
    "freesasa_gpu_trajectory_file_topology": ("topology", dict(TOPO)),
    "freesasa_gpu_trajectory_file_groups": ("topology", dict(TOPO, **GRP)),
    "freesasa_gpu_trajectory_file_groups_stats": ("topology", dict(TOPO, **GRP, stats=("residues", "groups"), stats_path="stats", partials_path="partials")),
    "freesasa_gpu_trajectory_file_interfaces": ("topology", dict(TOPO, **PAIR)),
    "freesasa_gpu_trajectory_file_interface_residues": ("topology", dict(TOPO, **PRES)),
    "freesasa_gpu_trajectory_file_volume": ("topology", dict(TOPO, volumes_path="volumes", **SR)),
    "freesasa_gpu_trajectory_file_masks": ("topology", dict(TOPO, masks_path="masks", **SR)),
    "freesasa_gpu_trajectory_file_groups_periodic": ("periodic", dict(TOPO, **GRP)),
    "freesasa_gpu_trajectory_file_interfaces_periodic": ("periodic", dict(TOPO, **PAIR)),
    "freesasa_gpu_trajectory_file_interface_residues_periodic": ("periodic", dict(TOPO, **PRES)),
}


def frames_of(b):
    rng = np.random.default_rng(3)
    x0 = np.asarray(b.xyz, dtype=np.float64).reshape(-1, 3) + 8.0
    return (x0[None] + rng.uniform(-0.2, 0.2, (F,) + x0.shape)).astype(np.float32)


def run_case(tmp, case, b, ids, sel):
    """one call of the case in the directory tmp (the frame file is written where it is not there yet) -> (complete, n_frames,
    the done-list's path)"""
    from test_dcd import write_dcd
    from test_pbc_gpu import patch_cells
    how, kw = CASES[case]
    tmp = str(tmp)
    path = lambda k: os.path.join(tmp, k)
    kw = {k: path(v) if isinstance(v, str) and k.endswith("_path") else v for k, v in kw.items()}
    if kw.get("selection"):
        kw["selection"] = sel
    if "n_groups" in kw:
        kw["group"] = ids
    frames = path("frames.dcd" if how == "periodic" else "frames.f64")
    if not os.path.exists(frames):
        if how == "periodic":
            write_dcd(frames, frames_of(b), cell=True)
            patch_cells(frames, [CELL] * F)
        else:
            frames_of(b).astype(np.float64).tofile(frames)
        os.utime(frames, ns=(MTIME_NS, MTIME_NS))
    kw.update(done_path=path("done"), frames_per_batch=FPB)
    if how == "plain":
        res = fa.trajectory_file(frames, b.radii, path("totals"), **kw)
    elif how == "topology":
        res = fa.trajectory_file_topology(frames, b, path("totals"), **kw)
    else:
        res = fa.trajectory_file_groups_periodic(frames, b, path("totals"), dcd=True, **kw)
    return res[0], res[1], path("done")


def heads(tmp):
    b, ids = dimer(tmp)
    sel = ingest.Selection(["a, chain A"])
    out = {}
    for case in CASES:
        d = os.path.join(str(tmp), case)
        os.mkdir(d)
        complete, n_frames, done = run_case(d, case, b, ids, sel)
        assert complete and n_frames == F
        with open(done, "rb") as fh:
            out[case] = fh.readline().decode()
    sel.close()
    return out


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        out = heads(tmp)
    with open(os.path.join(HERE, "traj_done_heads.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(len(out), "done-list heads")
