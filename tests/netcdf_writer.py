"""TESTS ONLY: a writer of NetCDF classic files (versions 1 and 2) from struct and numpy alone, and the AMBER trajectory
convention 1.0 on top of it.  tests/test_netcdf.py holds it to scipy.io.netcdf_file byte for byte; the GPU tests use it because
a GPU box may have no scipy.  The layout is scipy's: variables without the record dimension first (by shape, descending), then
the record variables in the order given, their records interleaved."""
import struct

import numpy as np

NC_TYPE = {"S1": 2, "i4": 4, "f4": 5, "f8": 6}


def _name(s):
    b = s.encode("latin1")
    return struct.pack(">i", len(b)) + b + b"\0" * (-len(b) % 4)


def _atts(atts):
    """an attribute list: str -> NC_CHAR, float -> NC_FLOAT, int -> NC_INT (as scipy chooses), arrays by their dtype"""
    if not atts:
        return b"\0" * 8
    out = [struct.pack(">ii", 0x0C, len(atts))]
    for k, v in atts.items():
        if isinstance(v, str):
            t, body, n = 2, v.encode("latin1"), len(v)
        elif isinstance(v, (float, int)):
            t, body, n = (5, struct.pack(">f", v), 1) if isinstance(v, float) else (4, struct.pack(">i", v), 1)
        else:
            v = np.asarray(v)
            t, body, n = NC_TYPE[v.dtype.str[1:]], v.astype(v.dtype.newbyteorder(">")).tobytes(), v.size
        out.append(_name(k) + struct.pack(">ii", t, n) + body + b"\0" * (-len(body) % 4))
    return b"".join(out)


def write_nc(path, dims, gatts, variables, version=2, numrecs=None):
    """dims: [(name, length or None for the record dimension)]; variables: [(name, dimension names, attributes, data)], a record
    variable's data [records, ...]; numrecs: what the header claims (None: the truth, -1: streaming).  Returns the bytes."""
    names, length = [d for d, _ in dims], dict(dims)
    isrec = lambda v: bool(v[1]) and length[v[1][0]] is None
    variables = [(n, d, a, np.asarray(x).astype(np.asarray(x).dtype.newbyteorder(">"))) for n, d, a, x in variables]
    variables = sorted(variables, key=lambda v: (-1,) if isrec(v) else tuple(v[3].shape), reverse=True)
    recs = [v for v in variables if isrec(v)]
    nrec = max([len(v[3]) for v in recs], default=0)
    assert all(len(v[3]) == nrec for v in recs)

    def vsize(v):
        s = (v[3][0].size if isrec(v) else v[3].size) * v[3].itemsize
        return s if isrec(v) and len(recs) == 1 else s + -s % 4
    head = b"CDF" + bytes([version]) + struct.pack(">I", (nrec if numrecs is None else numrecs) & 0xffffffff)
    head += (struct.pack(">ii", 0x0A, len(dims)) + b"".join(_name(n) + struct.pack(">i", l or 0) for n, l in dims)) if dims else b"\0" * 8
    head += _atts(gatts)
    metas = [_name(v[0]) + struct.pack(">i", len(v[1])) + b"".join(struct.pack(">i", names.index(d)) for d in v[1]) + _atts(v[2]) +
             struct.pack(">ii", NC_TYPE[v[3].dtype.str[1:]], vsize(v)) for v in variables]
    pos = len(head) + 8 + sum(len(m) + (4 if version == 1 else 8) for m in metas)
    out = [head, struct.pack(">ii", 0x0B, len(variables)) if variables else b"\0" * 8]
    for m, v in zip(metas, variables):
        out.append(m + struct.pack(">i" if version == 1 else ">q", pos))
        pos += vsize(v)
    pad = lambda b, v: b + b"\0" * (vsize(v) - len(b))
    out += [pad(v[3].tobytes(), v) for v in variables if not isrec(v)]
    out += [pad(v[3][r:r + 1].tobytes(), v) for r in range(nrec) for v in recs]    # (a slice: a numpy scalar forgets its byte order)
    data = b"".join(out)
    with open(path, "wb") as fh:
        fh.write(data)
    return data


def amber(frames, cells=None, time=True, velocities=False, conventions="AMBER", coord_atts=None):
    """(dims, global attributes, variables) of an AMBER NetCDF trajectory of frames [F, N, 3]; cells [F, 6]: a, b, c, alpha, beta,
    gamma per frame.  A record holds, in this order, time (fp32), coordinates (fp32), cell_lengths and cell_angles (fp64),
    velocities (fp32)."""
    frames = np.asarray(frames, dtype=">f4")
    F, N = frames.shape[:2]
    dims = [("frame", None), ("spatial", 3), ("atom", N)]
    gatts = {"title": "test", "application": "freesasa_amd", "program": "tests", "programVersion": "1.0", "Conventions": conventions,
             "ConventionVersion": "1.0"}
    if conventions is None:
        del gatts["Conventions"]
    variables = [("spatial", ("spatial",), {}, np.array(list("xyz"), dtype="S1"))]
    if cells is not None:
        cells = np.asarray(cells, dtype=">f8").reshape(F, 6)
        dims += [("cell_spatial", 3), ("label", 5), ("cell_angular", 3)]
        variables += [("cell_spatial", ("cell_spatial",), {}, np.array(list("abc"), dtype="S1")),
                      ("cell_angular", ("cell_angular", "label"), {}, np.array([list("alpha"), list("beta "), list("gamma")], dtype="S1"))]
    if time:
        variables.append(("time", ("frame",), {"units": "picosecond"}, np.arange(F, dtype=">f4")))
    variables.append(("coordinates", ("frame", "atom", "spatial"), dict({"units": "angstrom"}, **(coord_atts or {})), frames))
    if cells is not None:
        variables += [("cell_lengths", ("frame", "cell_spatial"), {"units": "angstrom"}, cells[:, :3]),
                      ("cell_angles", ("frame", "cell_angular"), {"units": "degree"}, cells[:, 3:])]
    if velocities:
        variables.append(("velocities", ("frame", "atom", "spatial"), {"units": "angstrom/picosecond", "scale_factor": 20.455}, frames[::-1] * np.float32(0.01)))
    return dims, gatts, variables


def write_amber(path, frames, cells=None, version=2, numrecs=None, **kw):
    return write_nc(path, *amber(frames, cells, **kw), version=version, numrecs=numrecs)
