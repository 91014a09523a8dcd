/*
 * rescontact_kernels.h — phase functions of the RESIDUE-RESIDUE CONTACT TABLES of the interfaces between chain groups
 * (freesasa_gpu_interface_residue_contacts_dev; include/freesasa_gpu.h has the definitions, tests/interface_residue_contacts_ref.py
 * restates them in numpy): the atom-atom contact rows (contact_kernels.h) folded per pair of residues, and for every folded row
 * the row that runs the other way.  The stage runs behind the contact stage on what it leaves on the device - contact_first,
 * contact_partner, contact_points, contact_area - and on the segments of the per-residue tables (iface_kernels.h: iface_res_head,
 * the block scan, iface_res_first, as they are): atom_res [M], hs [M + 1] (the exclusive scan of the head flags, hs[M] = K) and
 * seg_first [K + 1].  The segment of pair-structure atom j is hs[j + 1] - 1.
 *
 * A side's atoms are in input order and a residue's atoms are contiguous in the input, so along a side residues and segments
 * ascend together: within the other side of a pair the partner RESIDUE and the partner SEGMENT are the same thing, in the same
 * order.  The KEY of contact row t is the segment of contact_partner[t].
 *
 *   rc_fold_count   ONE WAVE PER SEGMENT a AT A TIME (RC_WAVES waves to a workgroup, each striding over the K segments on its own;
 *                   fc is zeroed by the host, so a slot at or beyond K holds 0): the segment's rows contact_first[b] ..
 *                   contact_first[e] - 1 are contiguous.  Their keys are staged in LDS - the first RC_STAGE of them; a row
 *                   behind that is keyed from memory again - and the distinct keys are counted in ascending order: "the
 *                   smallest key greater than the last", a minimum over the lanes' rows and then across the wave, until there
 *                   is none.  fc[a] = the count.
 *   scan            kl_iface_res_scan over fc [M + 1] in place: the folded rows before every segment, fc[M] = Q
 *   rc_fold_write   the same walk, 64 distinct keys at a time: lane l keeps the l-th of them and then runs over ALL rows of the
 *                   segment in row order with one accumulator each for n_rows, n_points and the area - one addition at a time
 *                   from 0, whatever the launch shape - and writes folded row fc[a] + (keys before the chunk) + l: the residues of
 *                   source and partner, the counts, the area and, for rc_reverse, the partner segment
 *   rc_reverse      one thread per folded row k: a binary search for the source residue among the partner segment's folded rows
 *                   (fc[s] .. fc[s + 1] - 1, whose partner residues ascend); thread t <= 2 P also writes
 *                   rescontact_offsets[t] = fc[hs[side_off[t]]], the folded rows before the side's first segment
 *
 * A wave works alone, in LDS of its own, whatever the other waves of its workgroup do: no barrier, no workgroup waits for
 * another, no floating-point atomics, no sum combined across lanes.  Which wave takes which segment shows in no result.
 * Integer minima do not depend on the order they are taken in.  Sizes: Q <= C < 2^31; no phase writes at or beyond row_cap = C.
 *
 * Written like contact_kernels.h: rc_fold_count and rc_fold_write are one lane of a wave's share (every lane of the wave calls
 * them with the same segment; ballots and shuffles in uniform control flow), so that a -DSASA_EMU build can drive them on the
 * CPU (tests/emu/emu_rescontacts.cpp); the __global__ wrappers and kl_rc_* launchers are in gpu_kernels.hip, the host side in
 * gpu_interfaces.hip.
 */
#ifndef FREESASA_AMD_RESCONTACT_KERNELS_H
#define FREESASA_AMD_RESCONTACT_KERNELS_H

#include "iface_kernels.h"

namespace sasa {

#define RC_WAVE 64    /* the lanes that work on one segment: one wave */
#define RC_WAVES 4    /* waves to a workgroup of the two fold kernels: each has its own segments and its own LDS */
#define RC_GRID 2048  /* workgroups of the two fold kernels at most: eight to a CU; the waves stride over the segments */
#define RC_STAGE 256  /* keys of a segment's rows kept in LDS (1 KiB); the rows behind them are keyed from memory */
#define RC_NO_KEY 0x7fffffff

struct ResContactArgs {
    int64_t n_pair_atoms, n_sides; /* M, 2 P */
    int64_t row_cap;               /* C: the rows the folded arrays hold */
    const int64_t *side_off;       /* [2 P + 1] */
    /* the segments (IfaceResArgs) */
    const int *atom_res;           /* [M] */
    const int *hs;                 /* [M + 1]; hs[M] = K */
    const int *seg_first;          /* [K + 1] */
    /* the contact rows (ContactArgs) */
    const int64_t *contact_first;  /* [M + 1] */
    const int *contact_partner, *contact_points; /* [C] */
    const double *contact_area;    /* [C] */
    /* the fold */
    int *fc;                       /* [M + 1] zeroed by the host; distinct partners per segment, then their exclusive scan; fc[M] = Q */
    int *pseg;                     /* [C] (Q used) the partner segment of every folded row */
    int64_t *rc_off;               /* [2 P + 1] */
    int *rc_res, *rc_cnt;          /* [2 C] (2 Q used) source and partner residue; n_rows and n_points */
    double *rc_area;               /* [C] */
    int *rc_rev;                   /* [C] */
};

struct ResContactLds {
    int key[RC_STAGE];
};

/* the key of row r0 + i of a segment whose first RC_STAGE keys are staged */
SASA_D int rc_key(const ResContactArgs &a, const ResContactLds &m, int r0, int i)
{
    return i < RC_STAGE ? m.key[i] : a.hs[a.contact_partner[r0 + i] + 1] - 1;
}
/* the rows of segment s, their keys staged (every lane; the wave's own LDS, ordered by LR2_SYNC): r0 and the number of rows */
SASA_D int rc_stage(const ResContactArgs &a, ResContactLds &m, int s, int lane, int &r0)
{
    const int b = a.seg_first[s], e = a.seg_first[s + 1];
    r0 = (int)a.contact_first[b];
    const int n = (int)a.contact_first[e] - r0;
    LR2_SYNC(); /* (the segment before has been read by all) */
    for (int i = lane; i < n && i < RC_STAGE; i += RC_WAVE) m.key[i] = a.hs[a.contact_partner[r0 + i] + 1] - 1;
    LR2_SYNC();
    return n;
}
/* the smallest key of the segment's n rows that is greater than last, RC_NO_KEY if there is none (every lane; uniform) */
SASA_D int rc_next_key(const ResContactArgs &a, const ResContactLds &m, int r0, int n, int last, int lane)
{
    int best = RC_NO_KEY;
    for (int i = lane; i < n; i += RC_WAVE) {
        const int k = rc_key(a, m, r0, i);
        if (k > last && k < best) best = k;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int o = LR2_SHFL(best, lane ^ d);
        if (o < best) best = o;
    }
    return best;
}

/* ONE WAVE PER SEGMENT s (every lane calls this with the same s; a slot at or beyond K gets its 0 here too) */
SASA_D void rc_fold_count(const ResContactArgs &a, ResContactLds &m, int64_t s, int lane)
{
    if (s >= a.n_pair_atoms) return;
    if (s >= a.hs[a.n_pair_atoms]) { if (lane == 0) a.fc[s] = 0; return; }
    int r0;
    const int n = rc_stage(a, m, (int)s, lane, r0);
    int cnt = 0;
    for (int last = -1;;) {
        last = rc_next_key(a, m, r0, n, last, lane);
        if (last == RC_NO_KEY) break;
        ++cnt;
    }
    if (lane == 0) a.fc[s] = cnt;
}

/* ONE WAVE PER SEGMENT s, behind the scan of fc */
SASA_D void rc_fold_write(const ResContactArgs &a, ResContactLds &m, int64_t s, int lane)
{
    if (s >= a.n_pair_atoms || s >= a.hs[a.n_pair_atoms]) return;
    int r0;
    const int n = rc_stage(a, m, (int)s, lane, r0);
    const int src_res = a.atom_res[a.seg_first[s]];
    int64_t row = a.fc[s];
    for (int last = -1;;) {
        int mine = RC_NO_KEY, taken = 0;
        for (; taken < RC_WAVE; ++taken) {
            const int k = rc_next_key(a, m, r0, n, last, lane);
            if (k == RC_NO_KEY) break;
            if (lane == taken) mine = k;
            last = k;
        }
        if (lane < taken && row + lane < a.row_cap) {
            int n_rows = 0, n_points = 0;
            double area = 0.0;
            for (int i = 0; i < n; ++i) {
                if (rc_key(a, m, r0, i) != mine) continue;
                ++n_rows;
                n_points += a.contact_points[r0 + i];
                area += a.contact_area[r0 + i];
            }
            const int64_t k = row + lane;
            a.rc_res[2 * k] = src_res; a.rc_res[2 * k + 1] = a.atom_res[a.seg_first[mine]];
            a.rc_cnt[2 * k] = n_rows; a.rc_cnt[2 * k + 1] = n_points;
            a.rc_area[k] = area;
            a.pseg[k] = mine;
        }
        row += taken;
        if (taken < RC_WAVE) break;
    }
}

/* one thread per folded row and per side boundary */
SASA_D void rc_reverse(const ResContactArgs &a, int64_t t)
{
    if (t <= a.n_sides) a.rc_off[t] = a.fc[a.hs[a.side_off[t]]];
    if (t >= a.fc[a.n_pair_atoms] || t >= a.row_cap) return;
    const int s = a.pseg[t], want = a.rc_res[2 * t];
    int lo = a.fc[s], hi = a.fc[s + 1]; /* the first row of s .. hi - 1 whose partner residue is >= want */
    const int end = hi;
    while (lo < hi) {
        const int mid = (int)(((int64_t)lo + hi) >> 1);
        if (a.rc_res[2 * (int64_t)mid + 1] < want) lo = mid + 1;
        else hi = mid;
    }
    a.rc_rev[t] = lo < end && a.rc_res[2 * (int64_t)lo + 1] == want ? lo : -1;
}

} /* namespace sasa */

#endif
