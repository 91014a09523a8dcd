/*
 * contact_kernels.h — phase functions of the ATOM-ATOM CONTACT TABLES of the interfaces between chain groups
 * (freesasa_gpu_interface_contacts_dev; include/freesasa_gpu.h has the definitions, tests/interface_contacts_ref.py restates them
 * in numpy): which atom of the partner buries which atom, and how much.  Shrake-Rupley only.  The stage runs behind the
 * interface pipeline (iface_kernels.h) on the pair batch it leaves on the device - pxyz, pradii, side_off - and on two sets of
 * exposure masks of the same M atoms (sr_caps.h's store phase): taken as the 2 P sides (side_mask) and as the P pair structures
 * (pair_mask).
 *
 *   contact_masks        one thread per pair-structure atom: buried = side & ~pair over the N bits that exist
 *   scan, expansion      dots_kernels.h on the buried masks, unchanged: dot_first [M + 1], the buried points in space (the
 *                        engine's own test point, t = u_k * R_i; t += x_i), their atom and their point number; D_b = dot_first[M]
 *   contact_attribute    one lane per buried dot, CT_B consecutive dots to a workgroup: the PARTNER of the dot - of the atoms j
 *                        of the other side of the same pair that cover it,
 *                            dx * dx + dy * dy + dz * dz <= R_j * R_j,   dx = t_x - x_j ...          (ref: src/sasa_sr.c:321-324)
 *                        the one with the smallest w = (dx * dx + dy * dy + dz * dz) - R_j * R_j, the lowest j among equals.
 *                        A dot without a cover gets -1 and raises a.flag (an integer maximum: the atom + 1).
 *   contact_rows_count   one thread per dot over its atom's run of at most 128 dots: is it the first of its partner, and how many
 *                        dots of the run share the partner - cnt[d], 0 where it is not the first
 *   contact_rows_rank    one thread per dot: a first dot's rank among the run's distinct partners by j; the run's first dot also
 *                        writes the atom's number of distinct partners to nd[i] (zeroed by the host: an atom without dots has 0)
 *   scan                 kl_iface_res_scan (iface_kernels.h) over nd [M + 1] in place: the rows before every atom, nd[M] = C
 *   contact_rows_write   one thread per dot and per atom: a first dot writes its row at nd[i] + rank - partner, points and
 *                        area = (4.0 * PI * R_i * R_i * n) / N (ref: src/sasa_sr.c:337) - and thread m <= M contact_first[m] = nd[m]
 *
 * Dots are in atom order and a side's atoms are consecutive, so a workgroup of contact_attribute holds one or more whole or
 * partial (pair, side) runs; it walks the distinct sides it holds (their first lanes are compacted by ballot).  For each: the
 * bounding box of the workgroup's dots on that side (wave shuffles, then LDS across the waves); the other side's atoms streamed
 * through LDS in tiles of CT_B (x, y, z, R * R), kept only if their sphere reaches the box, compacted by ballot so that ascending j
 * is preserved; every lane of the side tests the survivors and carries (w, j) across the tiles, replacing on a strict < only.
 * No workgroup waits for another; no floating-point atomics; every lane's result depends on its own dot and the atoms alone,
 * whatever the launch shape.
 *
 * Why the box filter cannot drop a cover.  Rounding is monotone (iface_kernels.h).  Atom j is dropped iff s_box > R_j * R_j,
 *     s_box = gx * gx + gy * gy + gz * gz,   g_c = max(lo_c - x_j, x_j - hi_c, 0)   (every operation rounded, left to right)
 * with lo, hi the box of the workgroup's dots of the side.  For a dot t in the box and an axis with g_c > 0, say x_j < lo_c <= t_c:
 * fl(t_c - x_j) >= fl(lo_c - x_j) = g_c > 0, and x -> fl(x * x) does not decrease on x >= 0, so fl(d_c * d_c) >= fl(g_c * g_c); the
 * other case is its mirror image (fl(a - b) = -fl(b - a)), and where g_c = 0, fl(d_c * d_c) >= 0 = fl(g_c * g_c).  The three
 * squares are added in the same order on both sides, so the dot's sum is >= s_box > fl(R_j * R_j): j does not cover the dot.
 * Both sides of the comparison are computed the same way, with one operand replaced by a bound of it.
 *
 * Sizes.  D_b comes back to the host behind the scan, so the arrays of the dots and of the rows hold exactly D_b (C <= D_b) and
 * the grids are made for it; D_b and C are below 2^31 (the host refuses more).  No phase writes at or beyond D_b.
 *
 * Written like dots_kernels.h: every function is one thread's share of a phase (contact_attribute: one thread of a workgroup's,
 * with the barriers in uniform control flow), so that a -DSASA_EMU build can drive them on the CPU (tests/emu/emu_contacts.cpp);
 * the __global__ wrappers and kl_contact_* launchers are in gpu_kernels.hip, the host side in gpu_interfaces.hip.
 */
#ifndef FREESASA_AMD_CONTACT_KERNELS_H
#define FREESASA_AMD_CONTACT_KERNELS_H

#include "dots_kernels.h"
#include "iface_kernels.h"

namespace sasa {

#define CT_B 256 /* threads per workgroup of every phase; dots per workgroup and atoms per tile of contact_attribute */

struct ContactArgs {
    int64_t n_pair_atoms, n_sides; /* M, 2 P */
    int n_points;
    double probe;
    const int64_t *side_off;       /* [2 P + 1] */
    const double *pxyz, *pradii;   /* [3 M], [M] the pair batch */
    const unsigned *side_masks;    /* [M][SR_CAP_WORDS] the atoms' masks with their side a structure of its own */
    const unsigned *pair_masks;    /* [M][SR_CAP_WORDS] ... in the pair structure */
    unsigned *buried;              /* [M][SR_CAP_WORDS] */
    /* the buried dots (DotsArgs over `buried`) */
    int64_t n_dots;                /* D_b: the dots, and the rows the arrays below hold */
    const int64_t *dot_first;      /* [M + 1] */
    const double *dot_xyz;         /* [3 D_b] */
    const int *dot_atom;           /* [D_b] */
    int *dot_partner;              /* [D_b] */
    int *flag;                     /* [1] zeroed by the host; the largest atom + 1 with a dot no atom covers */
    /* the rows */
    int *cnt, *rank;               /* [D_b] */
    int *nd;                       /* [M + 1] distinct partners per atom, then their exclusive scan; nd[M] = C */
    int64_t *contact_first;        /* [M + 1] */
    int *contact_partner, *contact_points; /* [D_b] (C used) */
    double *contact_area;          /* [D_b] */
};

struct ContactLds {
    double at[4 * CT_B];        /* the tile's survivors: x, y, z, R * R */
    int aj[CT_B];               /* their pair-structure atoms, ascending */
    int q[CT_B];                /* the lanes' sides */
    int hq[CT_B];               /* the distinct sides of the workgroup, ascending */
    double wbox[6 * (CT_B / 64)]; /* the waves' boxes */
    int wcnt[CT_B / 64];        /* the waves' counts of a compaction */
};

/* one thread per pair-structure atom m */
SASA_D void contact_masks(const ContactArgs &a, int64_t m)
{
    if (m >= a.n_pair_atoms) return;
    const SrMaskWords s = *(const SrMaskWords *)(a.side_masks + SR_CAP_WORDS * m), p = *(const SrMaskWords *)(a.pair_masks + SR_CAP_WORDS * m);
    SrMaskWords b;
    for (int w = 0; w < SR_CAP_WORDS; ++w) b.w[w] = s.w[w] & ~p.w[w] & sr_cap_full_word(a.n_points, w);
    *(SrMaskWords *)(a.buried + SR_CAP_WORDS * m) = b;
}

/* the side of pair-structure atom m: the last side that begins at or before m (no side of a pair is empty) */
SASA_D int contact_side(const ContactArgs &a, int64_t m)
{
    int64_t lo = 0, hi = a.n_sides - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.side_off[mid] <= m) lo = mid;
        else hi = mid - 1;
    }
    return (int)lo;
}

/* the place of a lane among the workgroup's lanes with pred, in lane order, and their number (two barriers; wcnt is free again
   behind the second) */
SASA_D int contact_compact(ContactLds &m, bool pred, int tid, int &total)
{
    const unsigned long long b = LR2_BALLOT(pred);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) m.wcnt[wave] = LR2_POPC64(b);
    IF_BARRIER();
    int base = 0, sum = 0;
    for (int w = 0; w < CT_B / 64; ++w) {
        const int c = m.wcnt[w];
        base += w < wave ? c : 0;
        sum += c;
    }
    IF_BARRIER();
    total = sum;
    return base + LR2_POPC64(b & ((1ull << lane) - 1ull));
}

/* the squared distance from atom x to the box lo .. hi, as the file's head has it */
SASA_D double contact_box_dist2(const double *lo, const double *hi, double x, double y, double z)
{
    const double p[3] = {x, y, z};
    double g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double below = lo[c] - p[c], above = p[c] - hi[c];
        double v = below > above ? below : above;
        g[c] = v > 0.0 ? v : 0.0;
    }
    return g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
}

/* ONE WORKGROUP OF CT_B THREADS PER BLOCK OF CT_B DOTS (every thread calls this with the same block) */
SASA_D void contact_attribute(const ContactArgs &a, ContactLds &m, int64_t block, int tid)
{
    const int64_t d = block * CT_B + tid;
    const bool valid = d < a.n_dots;
    const int lane = tid & 63, wave = tid >> 6;
    double t[3] = {0.0, 0.0, 0.0};
    int i = -1, q = -1;
    if (valid) {
        i = a.dot_atom[d];
        q = contact_side(a, i);
        t[0] = a.dot_xyz[3 * d]; t[1] = a.dot_xyz[3 * d + 1]; t[2] = a.dot_xyz[3 * d + 2];
    }
    m.q[tid] = q;
    IF_BARRIER();
    const bool head = valid && (tid == 0 || m.q[tid - 1] != q);
    int n_heads;
    const int hslot = contact_compact(m, head, tid, n_heads);
    if (head) m.hq[hslot] = q;
    IF_BARRIER();
    double best_w = 0.0;
    int best_j = -1;
    for (int s = 0; s < n_heads; ++s) {
        const int qs = m.hq[s];
        const bool mine = valid && q == qs;
        /* the box of this side's dots: every wave its own, then across the waves */
        double v[6] = {mine ? t[0] : IF_INF, mine ? t[1] : IF_INF, mine ? t[2] : IF_INF, mine ? t[0] : -IF_INF, mine ? t[1] : -IF_INF, mine ? t[2] : -IF_INF};
#pragma unroll
        for (int e = 32; e > 0; e >>= 1) {
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double o = if_shfl_d(v[c], lane ^ e);
                if (c < 3 ? o < v[c] : o > v[c]) v[c] = o;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) m.wbox[6 * wave + c] = v[c];
        }
        IF_BARRIER();
        double lo[3], hi[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = m.wbox[c]; hi[c] = m.wbox[3 + c];
            for (int w = 1; w < CT_B / 64; ++w) {
                const double l = m.wbox[6 * w + c], h = m.wbox[6 * w + 3 + c];
                if (l < lo[c]) lo[c] = l;
                if (h > hi[c]) hi[c] = h;
            }
        }
        /* the other side of the same pair, a tile at a time */
        const int64_t j0 = a.side_off[qs ^ 1], j1 = a.side_off[(qs ^ 1) + 1];
        for (int64_t jb = j0; jb < j1; jb += CT_B) {
            const int64_t j = jb + tid;
            const bool in = j < j1;
            const int64_t jr = in ? j : j1 - 1;
            const double x = a.pxyz[3 * jr], y = a.pxyz[3 * jr + 1], z = a.pxyz[3 * jr + 2], R = a.pradii[jr] + a.probe;
            const double R2 = R * R;
            const bool keep = in && !(contact_box_dist2(lo, hi, x, y, z) > R2);
            int n_keep;
            const int slot = contact_compact(m, keep, tid, n_keep); /* (its first barrier: the tile before has been read by all) */
            if (keep) { m.at[4 * slot] = x; m.at[4 * slot + 1] = y; m.at[4 * slot + 2] = z; m.at[4 * slot + 3] = R2; m.aj[slot] = (int)j; }
            IF_BARRIER();
            if (mine) {
                for (int k = 0; k < n_keep; ++k) {
                    const double dx = t[0] - m.at[4 * k], dy = t[1] - m.at[4 * k + 1], dz = t[2] - m.at[4 * k + 2], r2 = m.at[4 * k + 3];
                    const double s2 = dx * dx + dy * dy + dz * dz;
                    const double w = s2 - r2;
                    if (s2 <= r2 && (best_j < 0 || w < best_w)) { best_w = w; best_j = m.aj[k]; }
                }
            }
        }
        IF_BARRIER(); /* (wbox and the last tile have been read by all) */
    }
    if (valid) {
        a.dot_partner[d] = best_j;
        if (best_j < 0) SASA_ATOMIC_MAX_GLB(a.flag, i + 1);
    }
}

/* one thread per dot d: cnt[d] */
SASA_D void contact_rows_count(const ContactArgs &a, int64_t d)
{
    if (d >= a.n_dots) return;
    const int i = a.dot_atom[d], p = a.dot_partner[d];
    const int64_t b = a.dot_first[i], e = a.dot_first[i + 1];
    bool first = true;
    int n = 0;
    for (int64_t k = b; k < e; ++k) {
        const bool same = a.dot_partner[k] == p;
        first = first && !(same && k < d);
        n += same ? 1 : 0;
    }
    a.cnt[d] = first ? n : 0;
}
/* one thread per dot d: rank[d] of a first dot; nd[i] by the run's first dot */
SASA_D void contact_rows_rank(const ContactArgs &a, int64_t d)
{
    if (d >= a.n_dots) return;
    const int i = a.dot_atom[d], p = a.dot_partner[d];
    const int64_t b = a.dot_first[i], e = a.dot_first[i + 1];
    int below = 0, distinct = 0;
    for (int64_t k = b; k < e; ++k) {
        const bool f = a.cnt[k] > 0;
        distinct += f ? 1 : 0;
        below += f && a.dot_partner[k] < p ? 1 : 0;
    }
    a.rank[d] = below;
    if (d == b) a.nd[i] = distinct;
}
/* thread t: dot t's row where it is a first dot; contact_first[t] for t <= M */
SASA_D void contact_rows_write(const ContactArgs &a, int64_t t)
{
    if (t <= a.n_pair_atoms) a.contact_first[t] = a.nd[t];
    if (t >= a.n_dots) return;
    const int n = a.cnt[t];
    if (n <= 0) return;
    const int i = a.dot_atom[t];
    const int64_t slot = (int64_t)a.nd[i] + a.rank[t];
    if (slot < 0 || slot >= a.n_dots) return;
    const double R = a.pradii[i] + a.probe;
    a.contact_partner[slot] = a.dot_partner[t];
    a.contact_points[slot] = n;
    a.contact_area[slot] = (4.0 * SASA_PI * R * R * n) / a.n_points; /* ref: src/sasa_sr.c:337 */
}

} /* namespace sasa */

#endif
