/*
 * kat_kernels.h — TEST HOOKS: known-answer kernels over the arithmetic and the lane primitives whose device definition is
 * not the one the CPU emulation compiles (sasa_kernels.h: the hardware seeds and the inline assembly behind SASA_*;
 * lr2_kernels.h: the data-parallel scans, mbcnt, ballot, readlane, the 24-bit products, the fp32 seeds) and over
 * everything built on the seeds.  Every function is one thread's share and calls the product's macros and functions:
 * nothing is restated here.  Wrapped in __global__ kernels by gpu_kernels.hip (freesasa_gpu_kat_elementwise_dev,
 * freesasa_gpu_kat_wave_dev) and driven on the CPU by tests/emu/emu.cpp (-DSASA_EMU), so that one set of cases runs
 * through both definitions against plain references (tests/device_arith_ref.py).  No product kernel calls into this file.
 */
#ifndef KAT_KERNELS_H
#define KAT_KERNELS_H

#include <string.h>

#include "lr2_kernels.h"

namespace sasa {

/* Elementwise ops: thread i reads a[i], b[i], c[i] (those the op takes) and the scalar k, writes o0[i] and o1[i] (those
   it gives).  32-bit words travel in the low half of a double's bit pattern (KAT_SHIFT_IN), floats as the doubles that
   hold them exactly (KAT_F32, KAT_F32_SQRT). */
enum {
    KAT_RSQ = 0,     /* o0 = SASA_RSQ(a) */
    KAT_RCP,         /* o0 = SASA_RCP(a) */
    KAT_SQRT_G,      /* o0 = sqrt_g(a) */
    KAT_SQRT_RH,     /* sqrt_rh(a, o0, o1) */
    KAT_H2_LIMIT,    /* LR2_H2(a, o0); o1 = lr2_arc_limit(a, o0) */
    KAT_ACOS,        /* o0 = acos_fast(a) */
    KAT_ACOS2,       /* o0 = acos_fast2(a) */
    KAT_ACOS_LOWER,  /* o0 = lr2_acos_lower(a) */
    KAT_ATAN2,       /* o0 = atan2_fast(a, b) */
    KAT_ATAN2_INV,   /* o0 = atan2_inv(a, b, c) */
    KAT_DIV_NS,      /* o0 = lr2_div_ns(a, b, c) */
    KAT_FMA_K,       /* o0 = SASA_FMA_K(a, b, k): k the kernel's argument, in scalar registers as the polynomials' coefficients */
    KAT_MIN,         /* o0 = SASA_MIN(a, b); o1 = a after SASA_MIN_INTO(a, b) */
    KAT_MAX,         /* o0 = SASA_MAX(a, b); o1 = a after SASA_MAX_INTO(a, b) */
    KAT_SHIFT_IN,    /* w = low word of a: o0 = SASA_SHIFT_IN_LT1(w, b), o1 = LR2_SHIFT_IN_LT(w, b, c), both as low words */
    KAT_F32,         /* o0 = LR2_RCPF((float)a), o1 = LR2_RSQF((float)a) */
    KAT_F32_SQRT,    /* o0 = LR2_SQRTF((float)a) */
    KAT_EW_OPS
};
/* the arrays an elementwise op takes and gives: bits 0-2 a, b, c; bits 4-5 o0, o1; 0: no such op */
SASA_HD int kat_ew_arrays(int op)
{
    switch (op) {
    case KAT_RSQ: case KAT_RCP: case KAT_SQRT_G: case KAT_ACOS: case KAT_ACOS2: case KAT_ACOS_LOWER: case KAT_F32_SQRT: return 0x11;
    case KAT_SQRT_RH: case KAT_H2_LIMIT: case KAT_F32: return 0x31;
    case KAT_ATAN2: case KAT_FMA_K: return 0x13;
    case KAT_ATAN2_INV: case KAT_DIV_NS: return 0x17;
    case KAT_MIN: case KAT_MAX: return 0x33;
    case KAT_SHIFT_IN: return 0x37;
    }
    return 0;
}
#define KAT_EW_MAX (1 << 20) /* operands of one elementwise call */

SASA_D double kat_word(unsigned w) /* a 32-bit word as the low half of a double's bit pattern */
{
    const unsigned long long b = w;
    double v;
    memcpy(&v, &b, 8);
    return v;
}
SASA_D unsigned kat_low(double v)
{
    unsigned long long b;
    memcpy(&b, &v, 8);
    return (unsigned)b;
}

SASA_D void kat_elementwise(int op, const double *a, const double *b, const double *c, double k, double *o0, double *o1, int i)
{
    switch (op) {
    case KAT_RSQ: o0[i] = SASA_RSQ(a[i]); break;
    case KAT_RCP: o0[i] = SASA_RCP(a[i]); break;
    case KAT_SQRT_G: o0[i] = sqrt_g(a[i]); break;
    case KAT_SQRT_RH: { double g, h; sqrt_rh(a[i], g, h); o0[i] = g; o1[i] = h; } break;
    case KAT_H2_LIMIT: { double h; LR2_H2(a[i], h); o0[i] = h; o1[i] = lr2_arc_limit(a[i], h); } break;
    case KAT_ACOS: o0[i] = acos_fast(a[i]); break;
    case KAT_ACOS2: o0[i] = acos_fast2(a[i]); break;
    case KAT_ACOS_LOWER: o0[i] = lr2_acos_lower(a[i]); break;
    case KAT_ATAN2: o0[i] = atan2_fast(a[i], b[i]); break;
    case KAT_ATAN2_INV: o0[i] = atan2_inv(a[i], b[i], c[i]); break;
    case KAT_DIV_NS: o0[i] = lr2_div_ns(a[i], b[i], c[i]); break;
    case KAT_FMA_K: o0[i] = SASA_FMA_K(a[i], b[i], k); break;
    case KAT_MIN: { double x = a[i]; const double y = b[i]; o0[i] = SASA_MIN(x, y); SASA_MIN_INTO(x, y); o1[i] = x; } break;
    case KAT_MAX: { double x = a[i]; const double y = b[i]; o0[i] = SASA_MAX(x, y); SASA_MAX_INTO(x, y); o1[i] = x; } break;
    case KAT_SHIFT_IN: {
        const unsigned w = kat_low(a[i]);
        const double v = b[i], lim = c[i];
        o0[i] = kat_word(SASA_SHIFT_IN_LT1(w, v));
        o1[i] = kat_word(LR2_SHIFT_IN_LT(w, v, lim));
    } break;
    case KAT_F32: { const float x = (float)a[i]; o0[i] = (double)LR2_RCPF(x); o1[i] = (double)LR2_RSQF(x); } break;
    case KAT_F32_SQRT: o0[i] = (double)LR2_SQRTF((float)a[i]); break;
    }
}

/* Wave ops: ONE full wave walks `rows` rows of 64 words; lane l reads in[64 r + l] and writes out[64 r + l].  The op and
   the row are the same in every lane, and no lane leaves or branches around a cross-lane operation: as in the product,
   they run with every lane active.  lo / hi: the word's low and high 32 bits. */
enum {
    KAT_SCAN_ADD = 0, /* lr2_scan_add(lo, lane) */
    KAT_SCAN_ADD16,   /* lr2_scan_add16(lo, lane) */
    KAT_SCAN_MAX16,   /* lr2_scan_max16(lo, lane) */
    KAT_RANK,         /* every lane holds the row's mask: LR2_RANK(mask, lane) | LR2_RANK(the mask as LR2_BALLOT returns it, lane) << 32 */
    KAT_BALLOT,       /* every lane holds the row's mask: LR2_BALLOT(bit `lane` of it) */
    KAT_READLANE,     /* LR2_READLANE(lo, r % 64) */
    KAT_UNIFORM,      /* LR2_UNIFORM(lo): every lane of a row holds the same word, as the macro's users promise */
    KAT_SHFL,         /* LR2_SHFL(lo, hi), hi = the source lane, 0 .. 63 */
    KAT_SHFL_F64,     /* rows in pairs: lr2_shfl_f64(word of row 2 q, source lane = lo of row 2 q + 1) into row 2 q; row 2 q + 1 gets 0 */
    KAT_POPC,         /* LR2_POPC64(word) | LR2_POPC32(lo) << 32 */
    KAT_CELL_RANK,    /* cell_rank(word, lane) */
    KAT_MUL24,        /* LR2_MUL24(lo, hi), an int: sign-extended to 64 bits */
    KAT_UMUL24,       /* LR2_UMUL24(lo, hi), unsigned: zero-extended */
    KAT_DIV,          /* lr2_div9(lo) | lr2_div3(hi) << 32; lo < 69, hi < 44 */
    KAT_WAVE_OPS
};
#define KAT_WAVE_ROWS_MAX 4096

/* what a wave call's arguments must hold beyond their sizes (host side: the hook and the emulation ask before they run);
   null: fine */
inline const char *kat_wave_refusal(int op, const unsigned long long *in, int rows)
{
    if (op == KAT_SHFL_F64 && (rows & 1)) return "the 64-bit shuffle takes its rows in pairs";
    for (long long j = 0; j < (long long)rows * LR2_LANES; ++j) {
        const unsigned lo = (unsigned)in[j], hi = (unsigned)(in[j] >> 32);
        if (op == KAT_SHFL && hi >= LR2_LANES) return "source lane out of range";
        if (op == KAT_SHFL_F64 && ((j / LR2_LANES) & 1) && lo >= LR2_LANES) return "source lane out of range";
        if (op == KAT_DIV && (lo >= 69 || hi >= 44)) return "operand beyond the range of lr2_div9 / lr2_div3";
    }
    return nullptr;
}

SASA_D void kat_wave(int op, const unsigned long long *in, unsigned long long *out, int rows, int lane)
{
    for (int r = 0; r < rows; ++r) {
        const unsigned long long w = in[(size_t)r * LR2_LANES + lane];
        const int lo = (int)(unsigned)w, hi = (int)(unsigned)(w >> 32);
        unsigned long long res = 0;
        switch (op) {
        case KAT_SCAN_ADD: res = (unsigned)lr2_scan_add(lo, lane); break;
        case KAT_SCAN_ADD16: res = (unsigned)lr2_scan_add16(lo, lane); break;
        case KAT_SCAN_MAX16: res = (unsigned)lr2_scan_max16(lo, lane); break;
        case KAT_RANK: {
            const unsigned long long m = LR2_BALLOT(((w >> lane) & 1ull) != 0);
            res = (unsigned)LR2_RANK(w, lane) | ((unsigned long long)(unsigned)LR2_RANK(m, lane) << 32);
        } break;
        case KAT_BALLOT: res = LR2_BALLOT(((w >> lane) & 1ull) != 0); break;
        case KAT_READLANE: res = (unsigned)LR2_READLANE(lo, r & (LR2_LANES - 1)); break;
        case KAT_UNIFORM: res = (unsigned)LR2_UNIFORM(lo); break;
        case KAT_SHFL: res = (unsigned)LR2_SHFL(lo, hi); break;
        case KAT_SHFL_F64:
            if (!(r & 1)) { /* (the row is the same in every lane) */
                const int src = (int)(unsigned)in[(size_t)(r + 1) * LR2_LANES + lane];
                double v;
                memcpy(&v, &w, 8);
                v = lr2_shfl_f64(v, src);
                memcpy(&res, &v, 8);
            }
            break;
        case KAT_POPC: res = (unsigned)LR2_POPC64(w) | ((unsigned long long)(unsigned)LR2_POPC32((unsigned)lo) << 32); break;
        case KAT_CELL_RANK: res = (unsigned)cell_rank(w, lane); break;
        case KAT_MUL24: res = (unsigned long long)(long long)LR2_MUL24(lo, hi); break;
        case KAT_UMUL24: res = (unsigned long long)LR2_UMUL24(lo, hi); break;
        case KAT_DIV: res = (unsigned)lr2_div9(lo) | ((unsigned long long)(unsigned)lr2_div3(hi) << 32); break;
        }
        out[(size_t)r * LR2_LANES + lane] = res;
    }
}

} /* namespace sasa */

#endif
