"""TESTS ONLY: a pure-Python codec of GROMACS XTC frames (compressed coordinates, magic 1995, more than 9 atoms), written
from the format's description and independent of freesasa_amd/csrc/xtc.c and xtc_kernels.h - the yardstick of both.

A frame (all values XDR, big-endian): int magic = 1995, int natoms, int step, float time, float box[3][3] (nm), int natoms,
float precision, int minint[3], int maxint[3], int smallidx, int bytecount, then bytecount bytes padded to a multiple of 4.
The stream is read MSB first.  A GROUP is one "big" triple (all three integers in `bitsize` bits, or - bitsize 0 - one field per
dimension), a flag bit, with the flag a 5-bit field r (is_smaller = r % 3 - 1, run = r - r % 3; without the flag the run keeps
its value), and run / 3 "small" triples of smallidx bits each, offsets from the atom before; the first small atom of a group is
output IN FRONT of the big one.

decode(bytes) -> a list of Frame; encode(int_coords, precision, box, plan) -> the bytes of one frame.  A plan is a list of
(small atoms of the group, smallidx step) - the tests force every path with it; default_plan picks the runs greedily."""
import struct

import numpy as np

MAGIC = 1995
FIRSTIDX, LASTIDX = 9, 72
MAGICINTS = [0] * 9 + [
    8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512, 645, 812, 1024, 1290, 1625, 2048, 2580, 3250,
    4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768, 41285, 52015, 65536, 82570, 104031, 131072, 165140, 208063,
    262144, 330280, 416127, 524287, 660561, 832255, 1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304, 5284491, 6658042,
    8388607, 10568983, 13316085, 16777216]
assert len(MAGICINTS) == 73
HEADER = 92


def sizeofint(s):
    """the smallest b <= 32 with 2^b > s"""
    b = 0
    while b < 32 and (1 << b) <= s:
        b += 1
    return b


def bit_sizes(sizeint):
    """(bitsize, bitsizeint[3]): bitsize 0 when a dimension spans more than 0xffffff, then one field per dimension"""
    if (sizeint[0] | sizeint[1] | sizeint[2]) > 0xffffff:
        return 0, [sizeofint(s) for s in sizeint]
    return (sizeint[0] * sizeint[1] * sizeint[2]).bit_length(), [0, 0, 0]


def wrap32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


class BitReader:
    def __init__(self, data):
        self.data, self.pos, self.total = data, 0, 8 * len(data)

    def bits(self, n):
        if self.pos + n > self.total:
            raise ValueError("the stream ends inside a field")
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.data[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def ints(self, nbits, sizes):
        """receiveints: nbits as bytes, the first byte read the lowest; then two divisions"""
        v, j = 0, 0
        while nbits > 8:
            v |= self.bits(8) << (8 * j)
            j += 1
            nbits -= 8
        if nbits > 0:
            v |= self.bits(nbits) << (8 * j)
        n2 = v % sizes[2]
        v //= sizes[2]
        n1 = v % sizes[1]
        n0 = v // sizes[1]
        if n0 >= sizes[0]:
            raise ValueError("an unpacked value is out of its range")
        return [n0, n1, n2]


class BitWriter:
    def __init__(self):
        self.parts, self.n = [], 0                  # the fields as strings of 0 / 1; bits so far

    def bits(self, v, n):
        assert n == 0 or 0 <= v < (1 << n)
        if n:
            self.parts.append(format(v, "0%db" % n))
            self.n += n

    def ints(self, nbits, sizes, vals):
        v = (vals[0] * sizes[1] + vals[1]) * sizes[2] + vals[2]
        assert v < (1 << nbits)
        j = 0
        while nbits > 8:
            self.bits((v >> (8 * j)) & 0xff, 8)
            j += 1
            nbits -= 8
        if nbits > 0:
            self.bits(v >> (8 * j), nbits)

    def bytes(self):
        text = "".join(self.parts) + "0" * (-self.n % 8)
        return int(text, 2).to_bytes(len(text) // 8, "big") if text else b""


class Frame:
    """natoms, step, time, box [3, 3] float32 (nm), precision (float32), minint, maxint, smallidx, bytecount, ints [natoms, 3]
    int32, xyz [natoms, 3] float32 in Angstrom, trace: per group (bit offset, first atom, run, smallidx), offset and size: the
    frame's bytes within the file, stream: its bytes"""


def decode_stream(stream, natoms, minint, maxint, smallidx):
    """the integer coordinates [natoms, 3] and the per-group trace of one frame's stream; ValueError for a stream that does not
    hold natoms atoms in range"""
    sizeint = [maxint[k] - minint[k] + 1 for k in range(3)]
    bitsize, bitsizeint = bit_sizes(sizeint)
    rd = BitReader(stream)
    smallnum = MAGICINTS[smallidx] // 2
    smaller = MAGICINTS[max(FIRSTIDX, smallidx - 1)] // 2
    sizesmall = [MAGICINTS[smallidx]] * 3
    out, trace, run, i = [], [], 0, 0
    while i < natoms:
        start = rd.pos
        if bitsize:
            big = rd.ints(bitsize, sizeint)
        else:
            big = [rd.bits(bitsizeint[k]) for k in range(3)]
            if any(big[k] >= sizeint[k] for k in range(3)):
                raise ValueError("an unpacked value is out of its range")
        prev = [wrap32(big[k] + minint[k]) for k in range(3)]
        flag, is_smaller = rd.bits(1), 0
        if flag:
            r = rd.bits(5)
            is_smaller, run = r % 3 - 1, r - r % 3
        if i + 1 + run // 3 > natoms:
            raise ValueError("a group runs past the frame's atoms")
        trace.append((start, i, run, smallidx))
        if run > 0:
            big_atom = prev
            for k in range(run // 3):
                n = rd.ints(smallidx, sizesmall)
                this = [wrap32(n[d] + prev[d] - smallnum) for d in range(3)]
                out.append(this)
                if k == 0:
                    out.append(big_atom)
                prev = this
        else:
            out.append(prev)
        i += 1 + run // 3
        smallidx += is_smaller
        if not FIRSTIDX <= smallidx <= LASTIDX:
            raise ValueError("smallidx leaves its range")
        if is_smaller < 0:
            smallnum = smaller
            smaller = MAGICINTS[smallidx - 1] // 2 if smallidx > FIRSTIDX else 0
        elif is_smaller > 0:
            smaller = smallnum
            smallnum = MAGICINTS[smallidx] // 2
        sizesmall = [MAGICINTS[smallidx]] * 3
    return np.array(out, dtype=np.int64).astype(np.int32).reshape(natoms, 3), trace


def to_angstrom(ints, precision):
    """two fp32 products: the integer times (float)(1 / (double) precision), then times 10"""
    inv = np.float32(1.0 / float(np.float32(precision)))
    return (ints.astype(np.float32) * inv) * np.float32(10.0)


def parse_header(data, offset=0):
    """the header of the frame at `offset` -> a Frame without its coordinates"""
    if len(data) - offset < HEADER:
        raise ValueError("the file ends inside a header")
    f = Frame()
    magic, f.natoms, f.step = struct.unpack_from(">iii", data, offset)
    if magic != MAGIC:
        raise ValueError(f"magic {magic}")
    f.time = struct.unpack_from(">f", data, offset + 12)[0]
    f.box = np.array(struct.unpack_from(">9f", data, offset + 16), dtype=np.float32).reshape(3, 3)
    natoms2, f.precision = struct.unpack_from(">if", data, offset + 52)
    if natoms2 != f.natoms or f.natoms <= 9:
        raise ValueError("atom counts")
    f.precision = np.float32(f.precision)
    v = struct.unpack_from(">8i", data, offset + 60)
    f.minint, f.maxint, f.smallidx, f.bytecount = list(v[0:3]), list(v[3:6]), v[6], v[7]
    f.offset, f.size = offset, HEADER + (f.bytecount + 3) // 4 * 4
    if f.bytecount < 0 or offset + f.size > len(data):
        raise ValueError("bytecount")
    f.stream = bytes(data[offset + HEADER:offset + HEADER + f.bytecount])
    return f


def decode(data):
    """every frame of an XTC file's bytes"""
    frames, at = [], 0
    while at < len(data):
        f = parse_header(data, at)
        f.ints, f.trace = decode_stream(f.stream, f.natoms, f.minint, f.maxint, f.smallidx)
        f.xyz = to_angstrom(f.ints, f.precision)
        frames.append(f)
        at += f.size
    return frames


def default_plan(ints, smallidx):
    """greedy: a group takes the atoms that follow while each is within the small range of the one before (8 at the most, as
    GROMACS does); smallidx stays where it is"""
    ints = np.asarray(ints, dtype=np.int64)
    half = MAGICINTS[smallidx] // 2
    plan, i, n = [], 0, len(ints)
    while i < n:
        k = 0
        # in output order the group is small 0, big, small 1, small 2, ...: small 0 is coded against the big atom, small 1
        # against small 0, every later one against the small one before it
        while k < 8 and i + 1 + k < n:
            this, ref = ((i, i + 1), (i + 2, i))[k] if k < 2 else (i + 1 + k, i + k)
            d = ints[this] - ints[ref] + half
            if np.any(d < 0) or np.any(d >= MAGICINTS[smallidx]):
                break
            k += 1
        plan.append((k, 0))
        i += 1 + k
    return plan


def encode_stream(ints, minint, maxint, smallidx, plan, force_flag=False):
    """ints [natoms, 3] in OUTPUT order -> (stream bytes, trace).  plan: per group (small atoms k, step of smallidx in -1, 0, 1);
    a group with the run of the group before and step 0 is written with flag 0 (it inherits the run) unless force_flag."""
    ints = [[int(v) for v in row] for row in np.asarray(ints).reshape(-1, 3)]
    sizeint = [maxint[k] - minint[k] + 1 for k in range(3)]
    bitsize, bitsizeint = bit_sizes(sizeint)
    wr = BitWriter()
    smallnum = MAGICINTS[smallidx] // 2
    sizesmall = [MAGICINTS[smallidx]] * 3
    i, run_before, trace = 0, 0, []
    assert sum(1 + k for k, _ in plan) == len(ints), "the plan does not cover the atoms"
    for k, step in plan:
        # output order: the first small atom in front of the big one
        big = ints[i + 1] if k else ints[i]
        smalls = ([ints[i]] + ints[i + 2:i + 1 + k]) if k else []
        trace.append((wr.n, i, 3 * k, smallidx))
        rel = [big[d] - minint[d] for d in range(3)]
        assert all(0 <= rel[d] < sizeint[d] for d in range(3))
        if bitsize:
            wr.ints(bitsize, sizeint, rel)
        else:
            for d in range(3):
                wr.bits(rel[d], bitsizeint[d])
        run = 3 * k
        if run == run_before and step == 0 and not force_flag:
            wr.bits(0, 1)
        else:
            wr.bits(1, 1)
            wr.bits(run + step + 1, 5)
        prev = big
        for s in smalls:
            d = [s[q] - prev[q] + smallnum for q in range(3)]
            assert all(0 <= v < sizesmall[0] for v in d), "a small atom is out of the small range: the plan does not fit"
            wr.ints(smallidx, sizesmall, d)
            prev = s
        run_before = run
        i += 1 + k
        smallidx += step
        assert FIRSTIDX <= smallidx <= LASTIDX
        smallnum = MAGICINTS[smallidx] // 2
        sizesmall = [MAGICINTS[smallidx]] * 3
    return wr.bytes(), trace


def frame_bytes(natoms, step, time, box, precision, minint, maxint, smallidx, stream, magic=MAGIC, natoms2=None):
    head = struct.pack(">iiif", magic, natoms, step, time) + struct.pack(">9f", *np.asarray(box, dtype=np.float32).reshape(9)) + \
        struct.pack(">if", natoms if natoms2 is None else natoms2, precision) + struct.pack(">3i3i", *minint, *maxint) + \
        struct.pack(">ii", smallidx, len(stream))
    assert len(head) == HEADER
    return head + stream + b"\0" * (-len(stream) % 4)


def encode(int_coords, precision=1000.0, box=None, plan=None, smallidx=None, step=0, time=0.0, force_flag=False, minint=None, maxint=None):
    """one frame of integer coordinates [natoms, 3] (nm * precision, rounded) -> its bytes.  smallidx: the frame's first (default:
    the smallest index whose range holds the median step between atoms, as a writer would choose); plan: see encode_stream."""
    ints = np.asarray(int_coords, dtype=np.int64).reshape(-1, 3)
    assert len(ints) > 9
    minint = [int(v) for v in ints.min(0)] if minint is None else list(minint)
    maxint = [int(v) for v in ints.max(0)] if maxint is None else list(maxint)
    if smallidx is None:
        d = int(np.median(np.abs(np.diff(ints, axis=0)).max(1))) if len(ints) > 1 else 0
        smallidx = FIRSTIDX
        while smallidx < LASTIDX and MAGICINTS[smallidx] // 2 <= d:
            smallidx += 1
    if plan is None:
        plan = default_plan(ints, smallidx)
    stream, _ = encode_stream(ints, minint, maxint, smallidx, plan, force_flag)
    return frame_bytes(len(ints), step, time, np.zeros((3, 3)) if box is None else box, precision, minint, maxint, smallidx, stream)


def quantize(xyz_angstrom, precision=1000.0):
    """Angstrom -> the integers a writer stores: nm * precision, rounded"""
    return np.rint(np.asarray(xyz_angstrom, dtype=np.float64) * 0.1 * precision).astype(np.int64)


def write_xtc(path, frames_angstrom, precision=1000.0, boxes=None, plans=None, **kw):
    """frames [F, natoms, 3] in Angstrom -> an XTC file; returns its bytes (what decode() reads back is what the file holds)"""
    data = b""
    for f, xyz in enumerate(frames_angstrom):
        data += encode(quantize(xyz, precision), precision, None if boxes is None else boxes[f], None if plans is None else plans[f],
                       step=f, time=float(f), **kw)
    with open(path, "wb") as fp:
        fp.write(data)
    return data
