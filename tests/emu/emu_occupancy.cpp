/* TESTS ONLY: the phase functions of the residue contact occupancy map (freesasa_amd/csrc/occupancy_kernels.h) driven on the CPU as
 * gpu_occupancy.hip drives the kernels: per chunk occ_first one thread per chunk row, the block scan of the flags through
 * ifr_scan_levels like kl_iface_res_scan, the next set of arrays sized for exactly U + N rows, occ_rank one thread per old and per
 * chunk row, occ_accumulate one thread per row of the next table, the sets swapped; occ_keys one thread per folded row and per frame
 * boundary for a chunk that comes as a folded table; occ_reverse at a snapshot.  Every grid is rounded up to whole workgroups, idle
 * threads included, and every array is a heap block of its exact size.
 * With -DOCC_CHECK_MAIN: a stand-alone program (tests/emu/occ_check, built with AddressSanitizer + UBSan) that drives the same phases
 * over generated frames against a std::map, in several cuts: one line per case.
 * Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <map>
#include <vector>

#include "../../freesasa_amd/csrc/occupancy_kernels.h"

using namespace sasa;

/* kl_iface_res_scan: a [n + 1] in place */
static void scan_in_place(int *a, int64_t n)
{
    int64_t cnt[IFR_MAX_LEVELS];
    int *lvl[IFR_MAX_LEVELS];
    int part[IF_B];
    const int top = ifr_scan_levels(n, cnt);
    int *scratch = new int[(size_t)ifr_scan_scratch(n) + 1];
    lvl[0] = a;
    for (int l = 1; l <= top; ++l) lvl[l] = l == 1 ? scratch : lvl[l - 1] + cnt[l - 1];
    auto apply = [&](int *x, int64_t m, const int *base, int *total, int64_t blocks) {
        for (int64_t b = 0; b < blocks; ++b) {
            for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase0(x, m, part, b, t);
            for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase1(part, total, t);
            for (int t = 0; t < IF_B; ++t) ifr_scan_apply_phase2(x, m, part, base, b, t);
        }
    };
    for (int l = 0; l < top; ++l)
        for (int64_t b = 0; b < cnt[l + 1]; ++b) {
            for (int t = 0; t < IF_B; ++t) ifr_scan_sums_phase0(lvl[l], cnt[l], part, b, t);
            for (int t = 0; t < IF_B; ++t) ifr_scan_sums_phase1(part, lvl[l + 1], b, t);
        }
    apply(lvl[top], cnt[top], nullptr, a + n, 1);
    for (int l = top - 1; l >= 0; --l) apply(lvl[l], cnt[l], lvl[l + 1], nullptr, cnt[l + 1]);
    delete[] scratch;
}

static int64_t grid(int64_t n) { return (n + IF_B - 1) / IF_B * IF_B; }

struct EmuOcc {
    OccTable t;        /* the current set: exactly U rows */
    int64_t U = 0, n_frames = 0;
    EmuOcc() { memset(&t, 0, sizeof t); }
};
static void table_alloc(OccTable &t, int64_t cap)
{
    const size_t c = (size_t)cap;
    t.cap = cap;
    t.keys = new int[OCC_KEY * c]; t.frames = new int64_t[c]; t.either = new int64_t[c]; t.counts = new int64_t[2 * c];
    t.area = new double[3 * c]; t.span = new int64_t[2 * c];
}
static void table_free(OccTable &t)
{
    delete[] t.keys; delete[] t.frames; delete[] t.either; delete[] t.counts; delete[] t.area; delete[] t.span;
    memset(&t, 0, sizeof t);
}

/* one chunk: F frames, Q > 0 rows (occ_merge of gpu_occupancy.hip) */
static void merge_chunk(EmuOcc *o, int F, int64_t Q, const int64_t *ff, const int *ck, const int *cc, const double *ca)
{
    OccArgs a;
    memset(&a, 0, sizeof a);
    a.n_rows = Q; a.n_frames = F; a.frame0 = o->n_frames; a.n_old = o->U;
    a.ff = ff; a.ck = ck; a.cc = cc; a.ca = ca;
    a.fl = new int[(size_t)Q + 1];
    a.old = o->t;
    for (int64_t t = 0; t < grid(Q); ++t) occ_first(a, t);
    scan_in_place(a.fl, Q);
    a.n_new = o->U + a.fl[Q];
    table_alloc(a.next, a.n_new);
    for (int64_t t = 0; t < grid(a.n_old + Q); ++t) occ_rank(a, t);
    for (int64_t t = 0; t < grid(a.n_new); ++t) occ_accumulate(a, t);
    delete[] a.fl;
    table_free(o->t);
    o->t = a.next;
    o->U = a.n_new;
}

extern "C" void *emu_occ_open(void) { return new EmuOcc; }
extern "C" void emu_occ_close(void *h)
{
    EmuOcc *o = (EmuOcc *)h;
    table_free(o->t);
    delete o;
}
extern "C" long long emu_occ_rows(void *h) { return ((EmuOcc *)h)->U; }
extern "C" long long emu_occ_frames(void *h) { return ((EmuOcc *)h)->n_frames; }

/* freesasa_gpu_contact_occupancy_add_rows behind its checks: chunks of up to frames_per_batch frames, each arrays of its own */
extern "C" int emu_occ_add_rows(void *h, int n_frames, const int64_t *frame_first, const int32_t *keys, const int32_t *counts, const double *area,
                                int frames_per_batch)
{
    EmuOcc *o = (EmuOcc *)h;
    if (!o || n_frames < 0 || !frame_first || frames_per_batch <= 0) return -1;
    for (int f0 = 0; f0 < n_frames; f0 += frames_per_batch) {
        const int nf = n_frames - f0 < frames_per_batch ? n_frames - f0 : frames_per_batch;
        const int64_t t0 = frame_first[f0], Q = frame_first[f0 + nf] - t0;
        if (Q > 0) {
            const size_t q = (size_t)Q;
            int64_t *ff = new int64_t[(size_t)nf + 1];
            int *ck = new int[OCC_KEY * q], *cc = new int[2 * q];
            double *ca = new double[q];
            for (int f = 0; f <= nf; ++f) ff[f] = frame_first[f0 + f] - t0;
            memcpy(ck, keys + OCC_KEY * t0, 4 * OCC_KEY * q); memcpy(cc, counts + 2 * t0, 8 * q); memcpy(ca, area + t0, 8 * q);
            merge_chunk(o, nf, Q, ff, ck, cc, ca);
            delete[] ff; delete[] ck; delete[] cc; delete[] ca;
        }
        o->n_frames += nf;
    }
    return 0;
}

/* One chunk of freesasa_gpu_contact_occupancy_add_frames behind the interface pipeline: the folded table of a batch of n_frames
   structures - pair_struct [P], pair_groups [P][2], rescontact_offsets [2 P + 1], _residues / _counts [Q][2], _area [Q], Q > 0 - and
   the residues of one frame.  frame_counts [n_frames][2] receives (P_f, Q_f). */
extern "C" int emu_occ_add_table(void *h, int n_frames, int n_res, long long P, const int32_t *pair_struct, const int32_t *pair_groups,
                                 const int64_t *rc_off, const int32_t *rc_res, const int32_t *rc_cnt, const double *rc_area, int64_t *frame_counts)
{
    EmuOcc *o = (EmuOcc *)h;
    if (!o || n_frames <= 0 || n_res <= 0 || P <= 0 || !pair_struct || !pair_groups || !rc_off || !rc_res || !rc_cnt || !rc_area || rc_off[2 * P] <= 0)
        return -1;
    const int64_t Q = rc_off[2 * P];
    int *pf = new int[(size_t)n_frames + 1]();
    for (long long p = 0; p < P; ++p) ++pf[pair_struct[p] + 1];
    for (int f = 0; f < n_frames; ++f) pf[f + 1] += pf[f];
    OccKeyArgs k;
    memset(&k, 0, sizeof k);
    k.n_rows = Q; k.n_sides = 2 * P; k.n_frames = n_frames; k.n_res = n_res;
    k.rc_off = rc_off; k.rc_res = rc_res; k.pair_struct = pair_struct; k.pair_groups = pair_groups; k.pair_first = pf;
    k.ck = new int[OCC_KEY * (size_t)Q]; k.ff = new int64_t[(size_t)n_frames + 1];
    const int64_t n = Q > n_frames + 1 ? Q : n_frames + 1;
    for (int64_t t = 0; t < grid(n); ++t) occ_keys(k, t);
    if (frame_counts)
        for (int f = 0; f < n_frames; ++f) { frame_counts[2 * f] = pf[f + 1] - pf[f]; frame_counts[2 * f + 1] = k.ff[f + 1] - k.ff[f]; }
    merge_chunk(o, n_frames, Q, k.ff, k.ck, rc_cnt, rc_area);
    o->n_frames += n_frames;
    delete[] pf; delete[] k.ck; delete[] k.ff;
    return 0;
}

/* the snapshot: arrays of exactly emu_occ_rows() rows */
extern "C" void emu_occ_table(void *h, int32_t *keys, int64_t *frames, int64_t *either, int64_t *counts, double *area, int64_t *span, int32_t *reverse)
{
    EmuOcc *o = (EmuOcc *)h;
    const size_t U = (size_t)o->U;
    if (!U) return;
    OccArgs a;
    memset(&a, 0, sizeof a);
    a.n_new = o->U; a.next = o->t;
    a.reverse = new int[U];
    for (int64_t t = 0; t < grid(o->U); ++t) occ_reverse(a, t);
    memcpy(keys, o->t.keys, 4 * OCC_KEY * U); memcpy(frames, o->t.frames, 8 * U); memcpy(either, o->t.either, 8 * U);
    memcpy(counts, o->t.counts, 16 * U); memcpy(area, o->t.area, 24 * U); memcpy(span, o->t.span, 16 * U); memcpy(reverse, a.reverse, 4 * U);
    delete[] a.reverse;
}

#ifdef OCC_CHECK_MAIN
/* a small generator of its own: the cases are the program's, whatever the C library */
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

typedef std::array<int, OCC_KEY> Key;
struct Row { long long frames, either, n_rows, n_points, first, last; double sum, lo, hi; };
static Key rev_of(const Key &k) { return Key{k[0], k[1], 1 - k[2], k[4], k[3]}; }

/* n_frames frames that draw up to max_rows keys each from a universe of n_keys (groups up to g_max, residues up to r_max; one frame
   in five is empty), fed in cuts of `cut` frames to a call and frames_per_batch to a chunk, with a snapshot behind every call */
static int check_case(const char *name, int n_frames, int n_keys, int max_rows, int g_max, int r_max, int cut, int fpb)
{
    std::vector<Key> uni;
    for (int i = 0; i < n_keys; ++i) {
        const int g = (int)(rnd() % (unsigned)g_max), h = g + 1 + (int)(rnd() % 3);
        const Key k{g, h, (int)(rnd() & 1), r_max - (int)(rnd() % 12), r_max - (int)(rnd() % 12)};
        uni.push_back(k);
        if (rnd() % 3) uni.push_back(rev_of(k));
    }
    std::sort(uni.begin(), uni.end());
    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
    std::vector<int64_t> ff(1, 0);
    std::vector<int32_t> keys, counts;
    std::vector<double> area;
    std::map<Key, Row> want;
    for (int f = 0; f < n_frames; ++f) {
        std::vector<size_t> pick;
        const int rows = rnd() % 5 == 0 ? 0 : 1 + (int)(rnd() % (unsigned)max_rows);
        for (int r = 0; r < rows; ++r) pick.push_back(rnd() % uni.size());
        std::sort(pick.begin(), pick.end());
        pick.erase(std::unique(pick.begin(), pick.end()), pick.end());
        std::map<Key, int> touched;
        for (size_t i : pick) {
            const Key &k = uni[i];
            const int nr = 1 + (int)(rnd() % 9), np = nr + (int)(rnd() % 90);
            const double x = (rnd() % 4 == 0 ? 1e8 : rnd() % 4 == 1 ? -1e8 : 1.0) * (double)(1 + rnd() % 1000) / 7.0;
            for (int j = 0; j < OCC_KEY; ++j) keys.push_back(k[j]);
            counts.push_back(nr); counts.push_back(np); area.push_back(x);
            auto it = want.find(k);
            if (it == want.end()) it = want.insert(std::make_pair(k, Row{0, 0, 0, 0, f, f, 0.0, x, x})).first;
            Row &w = it->second;
            ++w.frames; w.n_rows += nr; w.n_points += np; w.sum = w.sum + x; w.last = f;
            if (x < w.lo) w.lo = x;
            if (x > w.hi) w.hi = x;
            touched[k] = 1; touched[rev_of(k)] = 1;
        }
        ff.push_back((int64_t)area.size());
        (void)touched;
    }
    /* frames_either: a second pass, frame by frame */
    for (int f = 0; f < n_frames; ++f) {
        std::map<Key, int> touched;
        for (int64_t t = ff[(size_t)f]; t < ff[(size_t)f + 1]; ++t) {
            Key k;
            for (int j = 0; j < OCC_KEY; ++j) k[j] = keys[OCC_KEY * (size_t)t + (size_t)j];
            touched[k] = 1; touched[rev_of(k)] = 1;
        }
        for (const auto &kv : touched) {
            auto it = want.find(kv.first);
            if (it != want.end()) ++it->second.either;
        }
    }
    if (keys.empty()) { keys.push_back(0); counts.push_back(0); area.push_back(0); } /* (never read: data() of an empty vector may be null) */
    void *h = emu_occ_open();
    int bad = 0;
    for (int f0 = 0; f0 < n_frames; f0 += cut) {
        const int nf = n_frames - f0 < cut ? n_frames - f0 : cut;
        std::vector<int64_t> sub(ff.begin() + f0, ff.begin() + f0 + nf + 1);
        const int64_t t0 = sub[0];
        for (int64_t &v : sub) v -= t0;
        bad |= emu_occ_add_rows(h, nf, sub.data(), keys.data() + OCC_KEY * t0, counts.data() + 2 * t0, area.data() + t0, fpb);
        /* a snapshot that nobody reads: it must not change what follows */
        const size_t u = (size_t)emu_occ_rows(h);
        if (u) {
            int32_t *k = new int32_t[OCC_KEY * u], *r = new int32_t[u];
            int64_t *a = new int64_t[u], *b = new int64_t[u], *c = new int64_t[2 * u], *s = new int64_t[2 * u];
            double *d = new double[3 * u];
            emu_occ_table(h, k, a, b, c, d, s, r);
            delete[] k; delete[] r; delete[] a; delete[] b; delete[] c; delete[] s; delete[] d;
        }
    }
    const size_t U = (size_t)emu_occ_rows(h);
    bad |= U != want.size() || emu_occ_frames(h) != n_frames;
    if (!bad && U) {
        int32_t *k = new int32_t[OCC_KEY * U], *r = new int32_t[U];
        int64_t *fr = new int64_t[U], *ei = new int64_t[U], *cn = new int64_t[2 * U], *sp = new int64_t[2 * U];
        double *ar = new double[3 * U];
        emu_occ_table(h, k, fr, ei, cn, ar, sp, r);
        std::map<Key, int> where;
        size_t i = 0;
        for (const auto &kv : want) where[kv.first] = (int)i++;
        i = 0;
        for (const auto &kv : want) {
            const Row &w = kv.second;
            const auto it = where.find(rev_of(kv.first));
            bad |= memcmp(k + OCC_KEY * i, kv.first.data(), 4 * OCC_KEY) != 0 || fr[i] != w.frames || ei[i] != w.either || cn[2 * i] != w.n_rows ||
                   cn[2 * i + 1] != w.n_points || memcmp(ar + 3 * i, &w.sum, 8) != 0 || memcmp(ar + 3 * i + 1, &w.lo, 8) != 0 ||
                   memcmp(ar + 3 * i + 2, &w.hi, 8) != 0 || sp[2 * i] != w.first || sp[2 * i + 1] != w.last ||
                   r[i] != (it == where.end() ? -1 : it->second);
            ++i;
        }
        delete[] k; delete[] r; delete[] fr; delete[] ei; delete[] cn; delete[] sp; delete[] ar;
    }
    emu_occ_close(h);
    printf("%s %s (frames %d, rows %lld, table rows %lld; %d frames to a call, %d to a chunk)\n", name, bad ? "FAILED" : "ok", n_frames,
           (long long)ff.back(), (long long)U, cut, fpb);
    return bad;
}

/* a folded table of n_frames structures with up to 2 pairs each, residues chunk-wide, through occ_keys against its plain re-keying */
static int check_keys_case(const char *name, int n_frames, int n_res)
{
    std::vector<int32_t> ps, pg, res, cnt;
    std::vector<int64_t> off(1, 0);
    std::vector<double> area;
    std::map<Key, long long> want; /* the key -> the frames that hold it */
    for (int f = 0; f < n_frames; ++f) {
        const int pairs = n_frames == 1 ? 2 : (int)(rnd() % 3);
        for (int p = 0; p < pairs; ++p) {
            ps.push_back(f); pg.push_back(p); pg.push_back(p + 1 + (int)(rnd() % 2));
            for (int side = 0; side < 2; ++side) {
                const int rows = (int)(rnd() % 4) * (int)(rnd() % 5);
                std::vector<std::pair<int, int>> rr;
                for (int r = 0; r < rows; ++r) rr.push_back(std::make_pair((int)(rnd() % (unsigned)n_res), (int)(rnd() % (unsigned)n_res)));
                std::sort(rr.begin(), rr.end());
                rr.erase(std::unique(rr.begin(), rr.end()), rr.end());
                for (const auto &ab : rr) {
                    res.push_back(f * n_res + ab.first); res.push_back(f * n_res + ab.second);
                    cnt.push_back(1); cnt.push_back(2); area.push_back(0.5);
                    ++want[Key{pg[pg.size() - 2], pg.back(), side, ab.first, ab.second}];
                }
                off.push_back((int64_t)area.size());
            }
        }
    }
    const long long P = (long long)ps.size();
    int bad = 0;
    size_t U = 0;
    if (P > 0 && off.back() > 0) {
        void *h = emu_occ_open();
        int64_t *fc = new int64_t[2 * (size_t)n_frames];
        bad |= emu_occ_add_table(h, n_frames, n_res, P, ps.data(), pg.data(), off.data(), res.data(), cnt.data(), area.data(), fc);
        U = (size_t)emu_occ_rows(h);
        bad |= U != want.size();
        long long q_sum = 0, p_sum = 0;
        for (int f = 0; f < n_frames; ++f) { p_sum += fc[2 * f]; q_sum += fc[2 * f + 1]; }
        bad |= p_sum != P || q_sum != off.back();
        if (!bad && U) {
            int32_t *k = new int32_t[OCC_KEY * U], *r = new int32_t[U];
            int64_t *fr = new int64_t[U], *ei = new int64_t[U], *cn = new int64_t[2 * U], *sp = new int64_t[2 * U];
            double *ar = new double[3 * U];
            emu_occ_table(h, k, fr, ei, cn, ar, sp, r);
            size_t i = 0;
            for (const auto &kv : want) { bad |= memcmp(k + OCC_KEY * i, kv.first.data(), 4 * OCC_KEY) != 0 || fr[i] != kv.second; ++i; }
            delete[] k; delete[] r; delete[] fr; delete[] ei; delete[] cn; delete[] sp; delete[] ar;
        }
        delete[] fc;
        emu_occ_close(h);
    } else bad = 1; /* (the case is made to have rows) */
    printf("%s %s (frames %d, pairs %lld, rows %lld, table rows %lld)\n", name, bad ? "FAILED" : "ok", n_frames, P, (long long)off.back(), (long long)U);
    return bad;
}

int main()
{
    int bad = 0;
    bad |= check_case("one-frame-calls", 12, 40, 30, 3, 50, 1, 1);
    bad |= check_case("all-at-once", 12, 40, 30, 3, 50, 12, 12);
    bad |= check_case("chunks-of-5", 23, 200, 300, 5, 1000, 7, 5);
    bad |= check_case("large-table", 9, 2500, 1500, 4000, 0x7fffffff, 4, 3);    /* U beyond 1024, several scan levels, extreme keys */
    bad |= check_case("sparse-frames", 40, 10, 2, 2, 20, 40, 64);
    bad |= check_keys_case("keys-of-a-folded-table", 17, 9);
    bad |= check_keys_case("keys-of-a-folded-table-one-frame", 1, 30);
    return bad;
}
#endif
