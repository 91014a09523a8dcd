/*
 * xtc_kernels.h — phase functions of the XTC decoder of the trajectory file drivers (FREESASA_GPU_FRAMES_XTC,
 * include/freesasa_gpu.h; xtc.c has the frame layout and makes the per-frame descriptors).  A shard's bytes lie on the device
 * as they lie in the file; behind them one freesasa_gpu_xtc_frame per frame.  Two kernels make of them raw interleaved fp32
 * frames in Angstrom, [n_frames][n_atoms][3] - what a raw fp32 frame file holds - and from there the raw fp32 path goes on
 * (traj_gather<float> or the widening): there is no third gather.
 *
 * The stream of a frame, bits MSB first, is a sequence of GROUPS: one "big" triple - three integers below sizeint[], packed
 * into ONE field of `bitsize` bits, or, bitsize 0, three fields of bitsizeint[k] bits -, a flag bit, with the flag a 5-bit
 * field r (is_smaller = r % 3 - 1, run = r - r % 3; without it the run KEEPS its value and is_smaller is 0), and run / 3 "small"
 * triples of smallidx bits each, packed against sizesmall = magicints[smallidx].  A packed field of nbits is read as bytes, the
 * first byte the lowest (the last takes the 1 .. 8 bits that remain): V = sum b_j 256^j, up to 72 bits wide; then n2 = V mod
 * sizes[2], V /= sizes[2], n1 = V mod sizes[1], n0 = V / sizes[1].  A big atom is its triple + minint; a small atom is its
 * triple + the atom before - magicints[smallidx] / 2; the FIRST small atom of a group is output in front of the big one.  After
 * the group smallidx += is_smaller.
 *
 * Only the POSITIONS depend on what came before, so the decode has two phases:
 *   xtc_scan    one wavefront per frame (a workgroup of XTC_SCAN_B = 64 threads): the lanes stage a window of the stream
 *               through LDS in coalesced 4-byte words, lane 0 walks the groups - it reads the flag and the 5-bit field only
 *               and advances by known widths - and writes per group a 16-byte record (bit offset, first atom, run, smallidx)
 *               and per frame the group count and a status.  A frame's walk is serial and latency-bound (one LDS read per
 *               group); a shard has a few hundred frames at the most, fewer than the device has CUs, so every frame gets a
 *               workgroup and with it a CU of its own rather than sharing one with other frames.
 *   xtc_unpack  one thread per group record (the grid is sized by n_atoms, a frame has at most that many groups): the wide
 *               divisions - byte by byte with 32-bit integers: every divisor is below 2^24 + 1 - and the chain of the group's
 *               atoms; writes the fp32 coordinates of its atoms.
 * The status is non-zero when the bit position would pass 8 bytecount, the atoms would pass n_atoms, smallidx would leave
 * 9 .. 72 (scan), or an unpacked value is not below its size (unpack).  The scan stops there; it reads nothing outside the
 * frame's padded bytes and writes no record past n_atoms records; a group of a frame with a non-zero status writes nothing.
 *
 * An output value is (float) integer * inv_precision, one fp32 product, times 10.0f, a second one (nm -> Angstrom): two
 * roundings, never one (a product and a product cannot be contracted; the tree is built with -ffp-contract=off all the same).
 *
 * Written like traj_kernels.h: a -DSASA_EMU build drives the phase functions on the CPU (tests/emu/emu_xtc.cpp); the
 * __global__ wrappers and kl_xtc_* launchers are in gpu_kernels.hip.
 */
#ifndef FREESASA_AMD_XTC_KERNELS_H
#define FREESASA_AMD_XTC_KERNELS_H

#include "sasa_kernels.h"
#include "../../include/freesasa_gpu.h"

namespace sasa {

#define XTC_SCAN_B 64   /* threads of xtc_scan's workgroup: one wavefront */
#define XTC_WIN 512     /* 32-bit words of the stream in LDS at a time */
#define XTC_UNPACK_B 256
#define XTC_FIRSTIDX 9
#define XTC_LASTIDX 72

enum { XTC_OK = 0, XTC_ST_BITS = 1, XTC_ST_ATOMS = 2, XTC_ST_SMALLIDX = 4, XTC_ST_VALUE = 8 }; /* a frame's status: bits */

#ifdef SASA_EMU
#define XTC_TABLE static const
#define XTC_STATUS_OR(p, v) (*(p) |= (v))
#else
#define XTC_TABLE static __device__ const
#define XTC_STATUS_OR(p, v) atomicOr((p), (v))
#endif
/* (5060, 524287 and 8388607 are the format's own irregularities) */
XTC_TABLE int32_t xtc_magicints[73] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512, 645, 812, 1024, 1290, 1625,
    2048, 2580, 3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768, 41285, 52015, 65536, 82570, 104031, 131072,
    165140, 208063, 262144, 330280, 416127, 524287, 660561, 832255, 1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304,
    5284491, 6658042, 8388607, 10568983, 13316085, 16777216};

struct XtcRec { int32_t bit, atom, run, smallidx; }; /* a group: its first bit within the stream, its first atom, its run, smallidx while it is read */

struct XtcArgs {
    int n_atoms, n_frames;                  /* atoms of every frame, frames of this shard */
    const uint32_t *in;                     /* the shard's bytes as 32-bit words */
    const freesasa_gpu_xtc_frame *desc;     /* [n_frames] */
    XtcRec *rec;                            /* [n_frames * n_atoms] */
    int32_t *count;                         /* [n_frames * 2] groups, status */
    float *out;                             /* [n_frames * n_atoms * 3] */
};

/* what lane 0 carries from one window of the stream to the next (in LDS: every lane reads w0 and done) */
struct XtcScanState {
    uint32_t pos, w0;   /* the next group's first bit; the window's first word within the stream */
    int32_t atom, run, smallidx, groups, status, done;
};

SASA_D uint32_t xtc_be32(uint32_t w) { return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24); }

/* n = 1 .. 32 bits from bit `pos` of the stream at `w`, MSB first; the caller has checked pos + n <= 8 bytecount: the second
   word is read only when the field reaches into it */
SASA_D uint32_t xtc_bits(const uint32_t *w, uint32_t pos, int n)
{
    const uint32_t wi = pos >> 5, off = pos & 31u;
    uint64_t v = (uint64_t)xtc_be32(w[wi]) << 32;
    if (off + (uint32_t)n > 32u) v |= xtc_be32(w[wi + 1]);
    return (uint32_t)((v << off) >> (64 - n));
}

/* receiveints: the packed field of nbits <= 72 at `pos` against sizes s0, s1, s2 (s1, s2 <= 2^24) -> n[3]; false when n0 is
   not below s0.  Nine bytes at the most, the loops unrolled so that they stay in registers. */
SASA_D bool xtc_receiveints(const uint32_t *w, uint32_t pos, int nbits, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t n[3])
{
    uint32_t b[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int left = nbits - 8 * j;
        b[j] = left > 0 ? xtc_bits(w, pos + 8u * (uint32_t)j, left > 8 ? 8 : left) : 0u;
    }
    uint32_t rem = 0;
#pragma unroll
    for (int j = 8; j >= 0; --j) {
        const uint32_t num = (rem << 8) | b[j], q = num / s2;
        b[j] = q;
        rem = num - q * s2;
    }
    n[2] = rem;
    rem = 0;
#pragma unroll
    for (int j = 8; j >= 0; --j) {
        const uint32_t num = (rem << 8) | b[j], q = num / s1;
        b[j] = q;
        rem = num - q * s1;
    }
    n[1] = rem;
    n[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    return (b[4] | b[5] | b[6] | b[7] | b[8]) == 0u && n[0] < s0;
}

SASA_D int xtc_bigbits(const freesasa_gpu_xtc_frame &d) { return d.bitsize ? d.bitsize : d.bitsizeint[0] + d.bitsizeint[1] + d.bitsizeint[2]; }

/* ------------------------------------------------------------------ xtc_scan */

SASA_D void xtc_scan_init(const XtcArgs &a, int f, XtcScanState &st)
{
    st.pos = 0; st.w0 = 0; st.atom = 0; st.run = 0; st.smallidx = a.desc[f].smallidx; st.groups = 0; st.status = XTC_OK; st.done = 0;
}

/* one lane's share of a window: words w0 + lane, w0 + lane + 64, ... of the stream, as far as the stream's padded bytes go */
SASA_D void xtc_scan_stage(const XtcArgs &a, int f, const XtcScanState &st, uint32_t *lds, int lane)
{
    const freesasa_gpu_xtc_frame &d = a.desc[f];
    const uint32_t nwords = ((uint32_t)d.bytecount + 3u) >> 2;
    const uint32_t *src = a.in + (d.stream_off >> 2);
    for (uint32_t k = (uint32_t)lane; k < XTC_WIN; k += XTC_SCAN_B)
        if (st.w0 + k < nwords) lds[k] = src[st.w0 + k];
}

/* lane 0: the groups whose flag and run field lie in the window (lds: XTC_WIN + 1 words, the last one 0).  Returns with
   st.done set - the frame is walked or has a status: count[] is written - or with st.w0 moved on: stage again. */
SASA_D void xtc_scan_walk(const XtcArgs &a, int f, XtcScanState &st, const uint32_t *lds)
{
    const freesasa_gpu_xtc_frame &d = a.desc[f];
    const uint32_t total = 8u * (uint32_t)d.bytecount, w0 = st.w0;
    const int bigbits = xtc_bigbits(d);
    XtcRec *rec = a.rec + (int64_t)f * a.n_atoms;
    uint32_t pos = st.pos;
    int atom = st.atom, run = st.run, smallidx = st.smallidx, groups = st.groups, status = XTC_OK;
    bool done = true;
    while (atom < a.n_atoms) {
        const uint32_t fpos = pos + (uint32_t)bigbits; /* the flag's bit */
        if (fpos + 1u > total) { status = XTC_ST_BITS; break; }
        const uint32_t end = fpos + 6u < total ? fpos + 6u : total;
        if (end > 32u * (w0 + XTC_WIN)) { st.w0 = fpos >> 5; done = false; break; }
        const uint32_t wi = (fpos >> 5) - w0;
        const uint64_t v = ((uint64_t)xtc_be32(lds[wi]) << 32) | xtc_be32(lds[wi + 1]);
        const uint32_t six = (uint32_t)((v << (fpos & 31u)) >> 58); /* the flag and, behind it, the run field */
        uint32_t q = fpos + 1u;
        int is_smaller = 0;
        if (six >> 5) {
            if (q + 5u > total) { status = XTC_ST_BITS; break; }
            const int r = (int)(six & 31u);
            is_smaller = r % 3 - 1;
            run = r - r % 3;
            q += 5u;
        }
        const int k = run / 3;
        if (atom + 1 + k > a.n_atoms) { status = XTC_ST_ATOMS; break; }
        const uint32_t small_bits = (uint32_t)(k * smallidx);
        if (q + small_bits > total) { status = XTC_ST_BITS; break; }
        const XtcRec r4 = {(int32_t)pos, atom, run, smallidx};
        rec[groups++] = r4;
        pos = q + small_bits;
        atom += 1 + k;
        smallidx += is_smaller;
        if (smallidx < XTC_FIRSTIDX || smallidx > XTC_LASTIDX) { status = XTC_ST_SMALLIDX; break; }
    }
    st.pos = pos; st.atom = atom; st.run = run; st.smallidx = smallidx; st.groups = groups; st.status = status;
    st.done = done ? 1 : 0;
    if (done) { a.count[2 * f] = groups; a.count[2 * f + 1] = status; }
}

/* ------------------------------------------------------------------ xtc_unpack */

SASA_D void xtc_put(float *o, const int32_t c[3], float inv_precision)
{
    for (int k = 0; k < 3; ++k) {
        const float nm = (float)c[k] * inv_precision;
        o[k] = nm * 10.0f;
    }
}

/* one thread per slot t = f n_atoms + g: group g of frame f, if the frame has that many */
SASA_D void xtc_unpack(const XtcArgs &a, int64_t t)
{
    if (t >= (int64_t)a.n_frames * a.n_atoms) return;
    const int f = (int)(t / a.n_atoms), g = (int)(t - (int64_t)f * a.n_atoms);
    if (g >= a.count[2 * f] || a.count[2 * f + 1] != XTC_OK) return;
    const freesasa_gpu_xtc_frame &d = a.desc[f];
    const XtcRec r = a.rec[t];
    const uint32_t *w = a.in + (d.stream_off >> 2);
    uint32_t pos = (uint32_t)r.bit, n[3];
    bool ok;
    if (d.bitsize) {
        ok = xtc_receiveints(w, pos, d.bitsize, d.sizeint[0], d.sizeint[1], d.sizeint[2], n);
    } else {
        uint32_t p = pos;
        ok = true;
        for (int k = 0; k < 3; ++k) {
            n[k] = xtc_bits(w, p, d.bitsizeint[k]);
            p += (uint32_t)d.bitsizeint[k];
            ok = ok && n[k] < d.sizeint[k];
        }
    }
    if (!ok) { XTC_STATUS_OR(&a.count[2 * f + 1], XTC_ST_VALUE); return; }
    pos += (uint32_t)xtc_bigbits(d);
    pos += xtc_bits(w, pos, 1) ? 6u : 1u;
    int32_t big[3], prev[3];
    for (int k = 0; k < 3; ++k) big[k] = prev[k] = (int32_t)(n[k] + (uint32_t)d.minint[k]);
    float *o = a.out + 3 * ((int64_t)f * a.n_atoms + r.atom);
    if (r.run == 0) { xtc_put(o, big, d.inv_precision); return; }
    const uint32_t sizesmall = (uint32_t)xtc_magicints[r.smallidx], smallnum = sizesmall / 2u;
    for (int k = 0; k < r.run / 3; ++k, pos += (uint32_t)r.smallidx) {
        if (!xtc_receiveints(w, pos, r.smallidx, sizesmall, sizesmall, sizesmall, n)) { XTC_STATUS_OR(&a.count[2 * f + 1], XTC_ST_VALUE); return; }
        for (int c = 0; c < 3; ++c) prev[c] = (int32_t)(n[c] + (uint32_t)prev[c] - smallnum);
        /* the first small atom goes in front of the big one */
        xtc_put(o + (k == 0 ? 0 : 3 * (k + 1)), prev, d.inv_precision);
        if (k == 0) xtc_put(o + 3, big, d.inv_precision);
    }
}

} /* namespace sasa */

#endif
