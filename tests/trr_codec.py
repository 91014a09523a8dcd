"""TESTS ONLY: a pure-Python writer and reader of GROMACS TRR trajectories, written from the format's description (no GROMACS
source, no TRR library): the yardstick of freesasa_amd/csrc/trr.c and of traj_gather_trr (traj_kernels.h).

Every value is XDR: big-endian, 4-byte units.  A record:
    int magic = 1993 | int 13 | int 12 | 12 bytes "GMX_trn_file" |
    int ir_size, e_size, box_size, vir_size, pres_size, top_size, sym_size, x_size, v_size, f_size, natoms, step, nre |
    real t | real lambda | box[9] | vir[9] | pres[9] | x[3 natoms] | v[3 natoms] | f[3 natoms]
each part of the body present only when its size is not 0.  real is 4 or 8 bytes for the whole record: box_size / 9 when
box_size != 0, else the first non-zero of x_size, v_size, f_size divided by 3 natoms.  Units are nm; the box rows are a, b, c."""
import struct

import numpy as np

MAGIC = 1993
VERSION = b"GMX_trn_file"
SIZES = ("ir_size", "e_size", "box_size", "vir_size", "pres_size", "top_size", "sym_size", "x_size", "v_size", "f_size", "natoms", "step", "nre")
WORD_OF = {name: 24 + 4 * k for k, name in enumerate(SIZES)}       # byte of every header integer within a record


def header_bytes(double):
    return 76 + (16 if double else 8)


class Record:
    """one record as the reader found it: offset and size in the file, the 13 integers (sizes), double, t, lam, and box [3, 3],
    vir, pres, x [n, 3], v, f as arrays of the file's precision, or None; x_off, box_off: their bytes in the file, or None"""


def record_bytes(natoms, double=False, x=None, v=None, f=None, box=None, vir=None, pres=None, step=0, t=0.0, lam=0.0, **override):
    """one record; x, v, f [natoms, 3] and box, vir, pres [3, 3] in nm (None: the record has no such part).  override: header
    integers by name (a key of WORD_OF; natoms_word for natoms), or magic, slen1, slen2, version - written as given, whatever the body holds"""
    w = 8 if double else 4
    dt = ">f8" if double else ">f4"
    parts = dict(box=box, vir=vir, pres=pres, x=x, v=v, f=f)
    body = {}
    for name, a in parts.items():
        if a is None:
            body[name] = b""
            continue
        a = np.asarray(a, dtype=np.float64).astype(dt)
        assert a.shape == ((3, 3) if name in ("box", "vir", "pres") else (natoms, 3)), name
        body[name] = a.tobytes()
    ints = dict(ir_size=0, e_size=0, top_size=0, sym_size=0, natoms=natoms, step=step, nre=0)
    for name in ("box", "vir", "pres", "x", "v", "f"):
        ints[name + "_size"] = len(body[name])
    head = dict(magic=MAGIC, slen1=13, slen2=12, version=VERSION)
    for k, val in override.items():
        if k in head:
            head[k] = val
        elif k == "natoms_word":                                     # (the header's atom count, whatever the arrays hold)
            ints["natoms"] = val
        else:
            assert k in WORD_OF, k
            ints[k] = val
    out = struct.pack(">iii", head["magic"], head["slen1"], head["slen2"]) + bytes(head["version"])[:12].ljust(12, b"\0")
    out += b"".join(struct.pack(">i", int(ints[name])) for name in SIZES)
    out += struct.pack(">dd" if double else ">ff", t, lam)
    assert len(out) == header_bytes(double) and w in (4, 8)
    return out + b"".join(body[name] for name in ("box", "vir", "pres", "x", "v", "f"))


def write_trr(path, records):
    """records: dicts of record_bytes' keywords -> the file's bytes (also written to path, unless None)"""
    data = b"".join(record_bytes(**r) for r in records)
    if path is not None:
        with open(path, "wb") as fp:
            fp.write(data)
    return data


def decode(data):
    """every record of the bytes -> [Record]; ValueError for what is no whole TRR record"""
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 76:
            raise ValueError(f"record {len(out)}: the bytes end inside its header")
        magic, s1, s2 = struct.unpack_from(">iii", data, at)
        if magic != MAGIC or s1 != 13 or s2 != 12 or data[at + 12:at + 24] != VERSION:
            raise ValueError(f"record {len(out)}: not a TRR header")
        r = Record()
        r.offset = at
        r.sizes = dict(zip(SIZES, struct.unpack_from(">13i", data, at + 24)))
        s = r.sizes
        n = s["natoms"]
        if n <= 0:
            raise ValueError(f"record {len(out)}: natoms {n}")
        w = s["box_size"] // 9 if s["box_size"] else next((s[k] // (3 * n) for k in ("x_size", "v_size", "f_size") if s[k]), 0)
        if w not in (4, 8):
            raise ValueError(f"record {len(out)}: reals of {w} bytes")
        for k in ("ir_size", "e_size", "top_size", "sym_size"):
            if s[k]:
                raise ValueError(f"record {len(out)}: {k} {s[k]}")
        for k in ("box_size", "vir_size", "pres_size"):
            if s[k] not in (0, 9 * w):
                raise ValueError(f"record {len(out)}: {k} {s[k]}")
        for k in ("x_size", "v_size", "f_size"):
            if s[k] not in (0, 3 * n * w):
                raise ValueError(f"record {len(out)}: {k} {s[k]}")
        r.double, r.natoms, r.step = w == 8, n, s["step"]
        hb = header_bytes(r.double)
        if len(data) - at < hb:
            raise ValueError(f"record {len(out)}: the bytes end inside its header")
        r.t, r.lam = struct.unpack_from(">dd" if r.double else ">ff", data, at + 76)
        p = at + hb
        dt = ">f8" if r.double else ">f4"
        r.box_off = r.x_off = None
        for name in ("box", "vir", "pres", "x", "v", "f"):
            size = s[name + "_size"]
            if p + size > len(data):
                raise ValueError(f"record {len(out)}: the bytes end inside its body")
            if name == "box" and size:
                r.box_off = p
            if name == "x" and size:
                r.x_off = p
            a = np.frombuffer(data, dtype=dt, count=size // w, offset=p).reshape(-1, 3) if size else None
            setattr(r, name, None if a is None else a.astype(a.dtype.newbyteorder("=")))
            p += size
        r.size = p - at
        out.append(r)
        at = p
    return out


def frames_angstrom(records):
    """what a run reads of the records: float64(x_nm) * 10.0 of every record WITH coordinates, [F, n, 3]"""
    return np.array([r.x.astype(np.float64) * 10.0 for r in records if r.x is not None])
