/* TESTS ONLY: the phase functions of the file sweep's interface kernels (freesasa_amd/csrc/ifsweep_kernels.h) driven on the CPU as
 * gpu_kernels.hip launches them: every kernel a loop over its grid's workgroups of IFS_B threads, idle threads included (no phase
 * function holds a barrier, so no fibers are needed).  The class sums behind the gather are the class-sum kernel's phases
 * (sasa_kernels.h) over the sides, as gpu_sweep.hip runs them.
 * With -DIFSWEEP_CHECK_MAIN: a stand-alone program (tests/emu/ifsweep_check, built with AddressSanitizer + UBSan) that drives the
 * same phases over generated tables against a plain loop, every array a heap block of its exact size: one line per case.
 * Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../freesasa_amd/csrc/ifsweep_kernels.h"

using namespace sasa;

extern "C" int emu_ifsweep_threads(void) { return IFS_B; }

/* k_ifs_side_class: pcls [M] */
extern "C" int emu_ifs_side_class(const int32_t *pair_atom, long long M, const unsigned char *cls, unsigned char *pcls)
{
    if (!pair_atom || M <= 0 || !cls || !pcls) return -1;
    IfsClassArgs a;
    memset(&a, 0, sizeof a);
    a.n_pair_atoms = M; a.pair_atom = pair_atom; a.cls = cls; a.pcls = pcls;
    const int64_t grid = (M + IFS_B - 1) / IFS_B * IFS_B;
    for (int64_t m = 0; m < grid; ++m) ifs_side_class(a, m);
    return 0;
}

/* ... and the class-sum kernel over the sides behind it: out [3 n_sides] */
extern "C" int emu_ifs_side_class_sums(const int32_t *pair_atom, long long M, const unsigned char *cls, const double *pair_buried,
                                       const int64_t *side_off, int n_sides, double *out)
{
    if (!pair_buried || !side_off || n_sides <= 0 || !out || side_off[n_sides] != M) return -1;
    unsigned char *pcls = new unsigned char[(size_t)M];
    const int rc = emu_ifs_side_class(pair_atom, M, cls, pcls);
    if (!rc) {
        double part[3 * SASA_TOT_B];
        for (int s = 0; s < n_sides; ++s) {
            for (int t = 0; t < SASA_TOT_B; ++t) class_phase0(pair_buried, pcls, side_off, part, s, t);
            for (int t = 0; t < SASA_TOT_B; ++t) class_phase1(part, out, s, t);
        }
    }
    delete[] pcls;
    return rc;
}

/* k_ifs_res_rows: the label planes are names [4] | chains [4] | numbers [6] bytes per residue, the device parser's n_res_dev
   residues in lab_d, the host parser's n_res - n_res_dev in lab_h (either may be null where it has none); out_lab: the same
   planes for the R rows */
extern "C" int emu_ifs_res_rows(long long R, long long n_sides, const int64_t *res_off, const int32_t *pair_struct, const int64_t *offsets,
                                const int64_t *res_first, long long n_res, long long n_res_dev, const int32_t *res_index,
                                const unsigned char *lab_d, const unsigned char *lab_h, int32_t *res_local, unsigned char *out_lab)
{
    if (R <= 0 || n_sides <= 0 || !res_off || !pair_struct || !offsets || !res_first || n_res <= 0 || n_res_dev < 0 || n_res_dev > n_res ||
        !res_index || !res_local || !out_lab || (n_res_dev > 0 && !lab_d) || (n_res_dev < n_res && !lab_h))
        return -1;
    const size_t Rd = (size_t)n_res_dev, Rh = (size_t)(n_res - n_res_dev);
    IfsRowArgs a;
    memset(&a, 0, sizeof a);
    a.n_rows = R; a.n_sides = n_sides; a.res_off = res_off; a.pair_struct = pair_struct; a.offsets = offsets;
    a.res_first = res_first; a.n_res = n_res; a.n_res_dev = n_res_dev; a.res_index = res_index;
    a.name_d = (const uint32_t *)lab_d; a.chain_d = a.name_d + Rd; a.number_d = (const uint16_t *)(a.chain_d + Rd);
    a.name_h = (const uint32_t *)lab_h; a.chain_h = a.name_h + Rh; a.number_h = (const uint16_t *)(a.chain_h + Rh);
    a.res_local = res_local; a.name = (uint32_t *)out_lab; a.chain = a.name + R; a.number = (uint16_t *)(a.chain + R);
    const int64_t grid = (R + IFS_B - 1) / IFS_B * IFS_B;
    for (int64_t r = 0; r < grid; ++r) ifs_res_rows(a, r);
    return 0;
}

#ifdef IFSWEEP_CHECK_MAIN
/* a small generator of its own: the cases are the program's, whatever the C library */
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

/* M pair-structure atoms over an input of n atoms, cut into n_sides sides (some empty); classes 0, 1, 2 */
static int check_class(long long M, int n, int n_sides)
{
    int32_t *pair_atom = new int32_t[(size_t)M];
    unsigned char *cls = new unsigned char[(size_t)n], *pcls = new unsigned char[(size_t)M];
    double *buried = new double[(size_t)M], *out = new double[3 * (size_t)n_sides];
    int64_t *side_off = new int64_t[(size_t)n_sides + 1];
    for (int i = 0; i < n; ++i) cls[i] = (unsigned char)(rnd() % 3);
    for (long long m = 0; m < M; ++m) { pair_atom[m] = (int32_t)(rnd() % (unsigned)n); buried[m] = (double)(rnd() % 100000) / 977.0; }
    side_off[0] = 0; side_off[n_sides] = M;
    for (int q = 1; q < n_sides; ++q) side_off[q] = (int64_t)(rnd() % (unsigned)(M + 1));
    for (int q = 1; q < n_sides; ++q) /* (ascending: an insertion sort of a few cuts) */
        for (int j = q; j > 1 && side_off[j] < side_off[j - 1]; --j) { const int64_t t = side_off[j]; side_off[j] = side_off[j - 1]; side_off[j - 1] = t; }
    int bad = emu_ifs_side_class(pair_atom, M, cls, pcls);
    for (long long m = 0; m < M && !bad; ++m) bad = pcls[m] != cls[pair_atom[m]];
    bad |= emu_ifs_side_class_sums(pair_atom, M, cls, buried, side_off, n_sides, out);
    for (int q = 0; q < n_sides && !bad; ++q) { /* (the order of the adds is the class kernel's: here only that every atom is counted once) */
        double w[3] = {0, 0, 0}, tol = 0;
        for (int64_t m = side_off[q]; m < side_off[q + 1]; ++m) { w[cls[pair_atom[m]]] += buried[m]; tol += buried[m]; }
        for (int k = 0; k < 3; ++k) bad |= !(out[3 * q + k] - w[k] <= 1e-12 * tol + 1e-300 && w[k] - out[3 * q + k] <= 1e-12 * tol + 1e-300);
    }
    delete[] pair_atom; delete[] cls; delete[] pcls; delete[] buried; delete[] out; delete[] side_off;
    printf("class-%lld %s (sides %d)\n", M, bad ? "FAILED" : "ok", n_sides);
    return bad;
}

/* R rows over n_structs structures (some without atoms, some without a pair) of residues of 1 .. 4 atoms; the first Rd residues
   are the device parser's; sides without a row at the start, in the middle and at the end */
static int check_rows(const char *name, long long R, int n_structs, long long rd_share_pct)
{
    std::vector<int64_t> offsets(1, 0), res_first;
    std::vector<int> res_struct, first_res((size_t)n_structs, 0);
    for (int s = 0; s < n_structs; ++s) {
        first_res[(size_t)s] = (int)res_first.size();
        const int nres = s % 3 == 1 ? 0 : 1 + (int)(rnd() % 9);
        int64_t at = offsets.back();
        for (int j = 0; j < nres; ++j) { res_first.push_back(at); res_struct.push_back(s); at += 1 + (int)(rnd() % 4); }
        offsets.push_back(at);
    }
    const long long n_res = (long long)res_first.size(), Rd = n_res * rd_share_pct / 100, Rh = n_res - Rd;
    res_first.push_back(offsets.back());
    /* pairs: a structure with residues owns pairs; rows dealt to the sides so that some sides stay empty */
    std::vector<int32_t> pair_struct;
    for (int s = 0; s < n_structs; ++s)
        if (s % 3 != 1 && s % 5 != 4) for (int p = 0; p < 1 + s % 2; ++p) pair_struct.push_back(s);
    if (pair_struct.empty()) pair_struct.push_back(0);
    const long long P = (long long)pair_struct.size(), n_sides = 2 * P;
    int64_t *res_off = new int64_t[(size_t)n_sides + 1];
    int32_t *res_index = new int32_t[(size_t)R], *res_local = new int32_t[(size_t)R];
    std::vector<long long> per((size_t)n_sides, 0);
    for (long long r = 0; r < R; ++r) {
        long long q = 1 + (long long)(rnd() % (unsigned)(n_sides > 2 ? n_sides - 2 : 1)); /* (the first and the last side stay empty where there are more than two) */
        if (n_sides <= 2) q = (long long)(rnd() % 2);
        if (n_sides > 4 && q == n_sides / 2) q -= 1; /* (one empty in the middle) */
        per[(size_t)q]++;
    }
    res_off[0] = 0;
    for (long long q = 0; q < n_sides; ++q) res_off[q + 1] = res_off[q] + per[(size_t)q];
    for (long long q = 0; q < n_sides; ++q) {
        const int s = pair_struct[(size_t)(q / 2)];
        const int f = first_res[(size_t)s], cnt = (s + 1 < n_structs ? first_res[(size_t)s + 1] : (int)n_res) - f;
        for (int64_t r = res_off[q]; r < res_off[q + 1]; ++r) res_index[r] = f + (int)(rnd() % (unsigned)cnt);
    }
    unsigned char *lab_d = Rd ? new unsigned char[14 * (size_t)Rd] : nullptr, *lab_h = Rh ? new unsigned char[14 * (size_t)Rh] : nullptr;
    unsigned char *out_lab = new unsigned char[14 * (size_t)R];
    for (size_t i = 0; i < 14 * (size_t)Rd; ++i) lab_d[i] = (unsigned char)(rnd() % 7 == 0 ? ' ' : rnd());
    for (size_t i = 0; i < 14 * (size_t)Rh; ++i) lab_h[i] = (unsigned char)(rnd() % 7 == 0 ? ' ' : rnd());
    int bad = emu_ifs_res_rows(R, n_sides, res_off, pair_struct.data(), offsets.data(), res_first.data(), n_res, Rd, res_index, lab_d, lab_h,
                               res_local, out_lab);
    for (long long q = 0; q < n_sides && !bad; ++q)
        for (int64_t r = res_off[q]; r < res_off[q + 1] && !bad; ++r) {
            const int j = res_index[r], s = pair_struct[(size_t)(q / 2)];
            const unsigned char *src = j < Rd ? lab_d : lab_h;
            const size_t k = j < Rd ? (size_t)j : (size_t)(j - Rd), n = j < Rd ? (size_t)Rd : (size_t)Rh;
            bad = res_local[r] != j - first_res[(size_t)s] || memcmp(out_lab + 4 * r, src + 4 * k, 4) != 0 ||
                  memcmp(out_lab + 4 * R + 4 * r, src + 4 * n + 4 * k, 4) != 0 || memcmp(out_lab + 8 * R + 6 * r, src + 8 * n + 6 * k, 6) != 0;
        }
    delete[] res_off; delete[] res_index; delete[] res_local; delete[] lab_d; delete[] lab_h; delete[] out_lab;
    printf("%s-%lld %s (structures %d, pairs %lld, residues %lld of them %lld the device's)\n", name, R, bad ? "FAILED" : "ok", n_structs, P, n_res, Rd);
    return bad;
}

int main()
{
    int bad = 0;
    const long long sizes[] = {1, IFS_B - 1, IFS_B, IFS_B + 1};
    for (long long M : sizes) bad |= check_class(M, 50, M < 3 ? 1 : 6);
    const long long rows[] = {1, 63, 64, 65, IFS_B - 1, IFS_B, IFS_B + 1, 1000};
    for (long long R : rows) {
        bad |= check_rows("rows", R, 12, 50);
        bad |= check_rows("rows-all-host", R, 12, 0);
        bad |= check_rows("rows-all-device", R, 12, 100);
    }
    bad |= check_rows("one-structure", 10, 1, 50);
    return bad;
}
#endif
