/*
 * gpu_sweep.hip — the structure sweep over PDB / mmCIF files (BASELINE configs[3], include/freesasa_gpu.h) over ONE
 * device or a LIST of devices, and the device-side parser's own entries.  Host code; gpu_drivers.hip says how the
 * drivers divide work among devices and what they share (engine_internal.h).
 *
 * A worker per entry of the device list takes batches of whole files from a shared counter, largest first.  Who parses is
 * an option (FREESASA_INGEST_PARSE_ON_DEVICE) and only decides how a batch BEGINS: its text staged and parsed on the device
 * (gpu_parse.hip), the files the device refuses read by the host parser - or every file read by the host parser.  From
 * there on a batch is "the atoms the device parsed, and behind them what the host parser read": ONE tail computes,
 * aggregates, copies back and records it, and sees the second case as the first with nothing parsed on the device.
 * With chain groups the tail runs the chain-group pipeline in place of the plain batch (groups_run), and with interfaces the
 * interface entries' one path in its place (ifaces_run: iface_run, gpu_interfaces.hip, whose step 1 is that pipeline).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <fcntl.h>
#include <memory>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>

#include "engine_internal.h"
#include "hostfault.h"
#include "select_program.h"

namespace {

struct Batch { /* a loader batch (freesasa_ingest.h) */
    freesasa_ingest_batch b;
    Batch() { memset(&b, 0, sizeof b); }
    Batch(const Batch &) = delete;
    Batch &operator=(const Batch &) = delete;
    ~Batch() { freesasa_ingest_free(&b); }
    void clear() { freesasa_ingest_free(&b); } /* (leaves it zeroed) */
    void take(Batch &o) { clear(); b = o.b; memset(&o.b, 0, sizeof o.b); }
};

/* ---- the device-side parser's input (gpu_parse.hip): a batch's files read - not parsed - into page-locked memory */
/* The text lives in one of the worker's CONTEXT's two page-locked staging buffers (stage_in / stage_out: they stay with the
   pooled context from call to call).  Until round 6's last session every sweep allocated and freed its own: hipHostMalloc
   and hipHostFree of 50 MB take 5 - 7 ms each and hold the runtime's lock while they do - in the kernel trace of a 70 ms
   sweep (tools/dev/sweep_trace.sh) the first 24 ms saw five batches where the steady state does twenty-two, and the last
   batch's tile kernel waited 11 ms for the OTHER worker to free its buffers. */
struct Staged {
    unsigned char *text = nullptr; /* page-locked: the files one after the other, each in a slot of its size + 1 and ending with '\n' */
    size_t T = 0;
    void **slot = nullptr;         /* the context's buffer and its capacity */
    size_t *slot_cap = nullptr;
    std::vector<ParseFile> files;  /* [n + 1] */
    int rc = 0;                    /* -1: no page-locked memory */
    Staged(void **slot_, size_t *cap_) : slot(slot_), slot_cap(cap_) {}
    Staged(const Staged &) = delete;
    Staged &operator=(const Staged &) = delete;
    void swap(Staged &o) { std::swap(text, o.text); std::swap(T, o.T); std::swap(slot, o.slot); std::swap(slot_cap, o.slot_cap); files.swap(o.files); std::swap(rc, o.rc); }
};
/* n files -> out, with `threads` readers (each file: one pread loop, then the one-line-at-a-time look at an mmCIF file's text
   before its _atom_site loop: freesasa_ingest_cif_locate); a file that cannot be read is left to the host parser, which
   reports it */
void stage_files(const char *const *paths, int n, int options, int threads, Staged *out)
{
    out->rc = 0;
    out->files.assign((size_t)n + 1, ParseFile());
    std::vector<long long> size((size_t)n, 0);
    size_t T = 0;
    for (int f = 0; f < n; ++f) {
        struct stat st;
        size[f] = (paths[f] && stat(paths[f], &st) == 0 && st.st_size > 0) ? (long long)st.st_size : 0;
        out->files[f].beg = (unsigned)T;
        T += (size_t)size[f] + 1;
    }
    if (T >= (1ULL << 31)) { out->rc = -2; return; }
    out->files[n].beg = (unsigned)T;
    out->T = T;
    if (T + 64 > *out->slot_cap) {
        if (*out->slot) (void)hipHostFree(*out->slot);
        *out->slot = nullptr; *out->slot_cap = 0;
        const size_t want = T + T / 8 + 4096;
        if (host_malloc(out->slot, want) != hipSuccess) { out->rc = -1; out->text = nullptr; return; }
        *out->slot_cap = want;
    }
    out->text = (unsigned char *)*out->slot;
    std::atomic<int> next(0);
    auto reader = [&]() noexcept {
        for (;;) {
            const int f = next.fetch_add(1);
            if (f >= n) break;
            ParseFile &pf = out->files[f];
            unsigned char *dst = out->text + pf.beg;
            const size_t slot = (size_t)size[f] + 1;
            size_t got = 0;
            bool ok = false;
            if (paths[f]) {
                const int fd = open(paths[f], O_RDONLY);
                if (fd >= 0) {
                    ok = true;
                    while (got < (size_t)size[f]) {
                        const ssize_t r = pread(fd, dst + got, (size_t)size[f] - got, (off_t)got);
                        if (r < 0) { ok = false; break; }
                        if (r == 0) break;
                        got += (size_t)r;
                    }
                    close(fd);
                }
            }
            pf.no_final_nl = (got > 0 && dst[got - 1] != '\n') ? 1 : 0;
            memset(dst + got, '\n', slot - got); /* (the slot's spare byte, and whatever a file that shrank left) */
            pf.kind = PARSE_HOST; pf.ncol = 0; pf.row0 = 0;
            if (!ok || (long long)got != size[f] || (options & FREESASA_INGEST_RADIUS_FROM_OCCUPANCY)) continue;
            int ncol = 0;
            size_t row0 = 0;
            const int kind = freesasa_ingest_cif_locate((const char *)dst, got, &ncol, pf.slot, &row0);
            if (kind == 0) pf.kind = PARSE_PDB;
            else if (kind == 1) { pf.kind = PARSE_CIF; pf.ncol = (short)ncol; pf.row0 = pf.beg + (unsigned)row0; }
        }
    };
    ThreadGroup tg;
    for (int t = 1; t < threads && t < n; ++t)
        if (!tg.spawn(reader)) break; /* (fewer readers then) */
    reader();
}
std::atomic<long long> g_parse_dev_files(0), g_parse_host_files(0);

/* ------------------------------------------------------------------ structure sweep: files */

struct SweepRec { double total, cls[3]; long long atoms; int status, pad; };
static_assert(sizeof(SweepRec) == 48, "result record");

/* The per-residue table of freesasa_gpu_sweep_files_residues.  Workers finish batches in any order and a file's place in
   the table depends on the residues of every file before it: each batch leaves a block of its own, and the table is
   assembled from them once all are done.  A batch's residues are in ITS order: the files the device parsed one after the
   other, behind them those of the files the host parser read (fstart says where a file's run begins). */
struct ResBatch {
    int first = 0, ns = 0;                  /* files [first, first + ns) */
    long long n_res = 0;
    std::vector<long long> fstart, fcount;  /* [ns] */
    std::vector<int64_t> res_first;         /* [n_res + 1] atoms, batch-wide */
    std::vector<double> areas;              /* abs [6 n_res] | rel [5 n_res] */
    std::vector<int16_t> ref;               /* [n_res] */
    std::vector<char> name, number, chain;  /* [4 | 6 | 4 per residue] */
    void size(long long R)
    {
        n_res = R;
        res_first.assign((size_t)R + 1, 0); areas.resize(11 * (size_t)R); ref.resize((size_t)R);
        name.resize(4 * (size_t)R); number.resize(6 * (size_t)R); chain.resize(4 * (size_t)R);
    }
};
struct ResCollector {
    std::mutex mu;
    std::vector<std::unique_ptr<ResBatch>> done;
    void add(std::unique_ptr<ResBatch> &rb) { std::lock_guard<std::mutex> lk(mu); done.push_back(std::move(rb)); }
};

/* The group table of freesasa_gpu_sweep_files_groups, collected like the residue table: a block per batch, its groups in the
   batch's structure order (fstart says where a file's run begins; a file whose group status is not 0 owns none). */
struct GrpBatch {
    int first = 0, ns = 0;
    std::vector<long long> fstart, fcount;  /* [ns] */
    std::vector<int32_t> atoms;             /* [groups] */
    std::vector<double> areas;              /* [3 groups] */
    std::vector<uint32_t> chain;            /* [groups] */
};
struct GrpCollector {
    std::mutex mu;
    std::vector<std::unique_ptr<GrpBatch>> done;
    void add(std::unique_ptr<GrpBatch> &gb) { std::lock_guard<std::mutex> lk(mu); done.push_back(std::move(gb)); }
};

/* The interface table of freesasa_gpu_sweep_files_interfaces, collected like the group table: a block per batch, its pairs in the
   batch's structure order and within a structure in the tests' order (fstart says where a file's run begins; a file whose
   interface status is not 0 owns none), the residue rows of the 2 P sides behind res_off. */
struct IfcBatch {
    int first = 0, ns = 0;
    std::vector<long long> fstart, fcount;      /* [ns] pairs */
    long long P = 0, R = 0;
    std::vector<int32_t> groups, atoms;         /* [2 P] */
    std::vector<uint32_t> chain;                /* [2 P] */
    std::vector<double> areas, cls;             /* [6 P] each */
    std::vector<int64_t> res_off;               /* [2 P + 1] */
    std::vector<int32_t> res_index, res_atoms;  /* [R] (the index: among the residues of the row's file) */
    std::vector<double> res_areas;              /* [3 R] */
    std::vector<char> labels;                   /* names [4 R] | chains [4 R] | numbers [6 R] */
    void size(long long P_, long long R_)
    {
        P = P_; R = R_;
        groups.assign(2 * (size_t)P, 0); atoms.assign(2 * (size_t)P, 0); chain.assign(2 * (size_t)P, 0);
        areas.resize(6 * (size_t)P); cls.resize(6 * (size_t)P);
        res_off.assign(2 * (size_t)P + 1, 0);
        res_index.resize((size_t)R); res_atoms.resize((size_t)R); res_areas.resize(3 * (size_t)R); labels.resize(14 * (size_t)R);
    }
};
struct IfcCollector {
    std::mutex mu;
    std::vector<std::unique_ptr<IfcBatch>> done;
    void add(std::unique_ptr<IfcBatch> &ib) { std::lock_guard<std::mutex> lk(mu); done.push_back(std::move(ib)); }
};
/* the interface request of a sweep with chain groups */
struct IfaceSpec {
    bool residues; double min_buried;
    IfcCollector *col; int *status_out; /* [n_paths] */
};

/* what a sweep entry was called with (read-only) */
struct SweepArgs {
    const char *const *paths; int n_paths, ingest_options, n_threads;
    int alg; double probe; int resolution; long long batch_atoms;
    double *totals_out, *class_sums_out; long long *atoms_out; int *status_out;
    const char *done_path; long long max_new_batches; /* (may be NULL / 0) */
    const int *devices; int n_devices;
    const freesasa_ingest_classifier *classifier;     /* (may be NULL) */
    ResCollector *rcol;                               /* (may be NULL) */
    const freesasa_ingest_selection *sel;             /* (may be NULL; never together with rcol) */
    double *sel_area_out; long long *sel_atoms_out;   /* [n_paths * selections] */
    const GroupSpec *grp;                             /* (may be NULL; never together with rcol or sel) */
    GrpCollector *gcol; int *group_status_out;        /* [n_paths] */
    const IfaceSpec *ifc;                             /* (may be NULL; only with grp) */
};
/* what the workers of one sweep share */
struct Sweep {
    const SweepArgs &a;
    bool dev_parse = false, want_cls = false;
    int options = 0;               /* the loader's (without FREESASA_INGEST_PARSE_ON_DEVICE) */
    int loader_threads = 1;
    std::vector<int> cut, todo;    /* batch b: files [cut[b], cut[b + 1]); the batches to compute, largest first */
    std::vector<double> tp;        /* S&R test points */
    std::atomic<size_t> next{0};
    FirstError fe;
    DoneList list;
    Fd res;                        /* <done_path>.bin */
    /* dev aid (FREESASA_AMD_SWEEP_PROFILE): where a worker's wall clock goes - staging of its first batch, parse (upload, line
       and atom counts back), the files left to the host parser, the tile kernels up to the totals, the done-list, waiting for
       the loader of the next batch */
    bool sprof = false;
    std::atomic<long long> tp_first{0}, tp_parse{0}, tp_host{0}, tp_run{0}, tp_rec{0}, tp_join{0}, tp_stage{0};
    explicit Sweep(const SweepArgs &a_) : a(a_) {}
};
long long now_ns() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (long long)ts.tv_sec * 1000000000LL + ts.tv_nsec; }

/* what a worker's loader thread prepares of the NEXT batch while this one is on the GPU: with the parser on the device the
   files' text in page-locked memory, else the batch as the host parser read it (nothing is ever copied to the device from
   `b` itself: the worker takes it over first) */
struct Ahead {
    Staged s;
    Batch b;
    int rc = 0; /* the loader's code */
    Ahead(void **slot, size_t *cap) : s(slot, cap) {}
    void swap(Ahead &o) { s.swap(o.s); std::swap(b.b, o.b.b); std::swap(rc, o.rc); }
};
void look_ahead(Sweep &S, int b, Ahead *out) noexcept
{
    const long long t0 = S.sprof ? now_ns() : 0;
    const char *const *paths = S.a.paths + S.cut[b];
    const int n = S.cut[b + 1] - S.cut[b];
    if (S.dev_parse) {
        try { stage_files(paths, n, S.options, S.loader_threads, &out->s); } catch (...) { out->s.rc = -3; }
    } else {
        out->rc = freesasa_ingest_pdb_files_ex(paths, n, S.options, S.loader_threads, S.a.classifier, &out->b.b); /* (C code: nothing to catch) */
    }
    if (S.sprof) S.tp_stage += now_ns() - t0;
}

/* one batch in its worker's hands */
struct Work {
    int b, first, ns;                     /* batch, its files [first, first + ns) */
    int nd = 0;                           /* structures the device parser made: one per file (a refused file an empty one) or none */
    long long total = 0;                  /* ... and their atoms */
    std::vector<int> atoms, status, host; /* [ns] the device parser's: atoms kept, loader status, 1 = left to the host parser */
    std::vector<int> fb;                  /* the files the host parser read, in its batch's order: structure nd + j is file fb[j] */
    std::vector<long long> atoms64;       /* [ns] results for the done-list's records */
    std::vector<double> cls;              /* [3 ns], empty: none computed */
    std::unique_ptr<ResBatch> rb;
    long long R = 0, Rd = 0;              /* residues of the batch, and how many of them are the device's */
    std::vector<double> sel_area;         /* [structures of the batch * selections] on their way back: areas, selected atoms */
    std::vector<long long> sel_count;
    std::unique_ptr<GrpBatch> gb;         /* chain groups: the batch's block, the words of its structures (status in | n_groups | group status) */
    std::vector<int32_t> gwords;
    std::unique_ptr<IfcBatch> ib;         /* interfaces: the batch's block, the groups of its structures as the screen counts them, P | M | R */
    std::vector<int32_t> screen;
    long long if_counts[3] = {0, 0, 0};
    Work(const Sweep &S, int b_) : b(b_), first(S.cut[b_]), ns(S.cut[b_ + 1] - S.cut[b_]), atoms((size_t)ns), status((size_t)ns), host((size_t)ns), atoms64((size_t)ns, 0)
    {
        if (S.a.gcol) {
            gb.reset(new GrpBatch);
            gb->first = first; gb->ns = ns; gb->fstart.assign((size_t)ns, 0); gb->fcount.assign((size_t)ns, 0);
        }
        if (S.a.ifc) {
            ib.reset(new IfcBatch);
            ib->first = first; ib->ns = ns; ib->fstart.assign((size_t)ns, 0); ib->fcount.assign((size_t)ns, 0); ib->size(0, 0);
        }
        if (!S.a.rcol) return;
        rb.reset(new ResBatch);
        rb->first = first; rb->ns = ns; rb->fstart.assign((size_t)ns, 0); rb->fcount.assign((size_t)ns, 0); rb->size(0);
    }
};

/* How a batch begins with the parser ON THE DEVICE (gpu_parse.hip): the text the loader staged is uploaded and parsed; the
   files the device refuses are read by the host parser now (hb) and go behind the device's atoms as further structures. */
int front_device(Sweep &S, freesasa_gpu_ctx *c, Ahead &cur, Work &w, Batch &hb)
{
    if (cur.s.rc)
        return ctx_fail(c, "%s", cur.s.rc == -1 ? "out of page-locked host memory (file staging)" : (cur.s.rc == -2 ? "a batch of files larger than 2 GB: use a smaller batch_atoms" : "out of host memory (file staging)"));
    long long tq = S.sprof ? now_ns() : 0;
    if (parse_batch_dev_begin(c, cur.s.text, cur.s.T, cur.s.files.data(), w.ns, S.options, S.a.classifier, w.atoms.data(), w.status.data(), w.host.data(), &w.total)) return -1;
    w.nd = w.ns;
    if (S.sprof) { const long long t1 = now_ns(); S.tp_parse += t1 - tq; tq = t1; }
    for (int k = 0; k < w.ns; ++k) if (w.host[(size_t)k]) w.fb.push_back(k);
    g_parse_dev_files += w.ns - (long long)w.fb.size(); g_parse_host_files += (long long)w.fb.size();
    hb.clear();
    if (!w.fb.empty()) {
        std::vector<const char *> fp;
        for (int k : w.fb) fp.push_back(S.a.paths[w.first + k]);
        const int lrc = freesasa_ingest_pdb_files_ex(fp.data(), (int)fp.size(), S.options, S.loader_threads, S.a.classifier, &hb.b);
        if (lrc) return ctx_fail(c, "loader failed with code %d", lrc);
    }
    if (S.sprof) S.tp_host += now_ns() - tq;
    return 0;
}
/* ... and with the host parser: the loader read every file; the device parsed nothing */
int front_host(freesasa_gpu_ctx *c, Ahead &cur, Work &w, Batch &hb)
{
    if (cur.rc) return ctx_fail(c, "loader failed with code %d", cur.rc);
    parse_batch_dev_none(c);
    hb.take(cur.b);
    w.host.assign((size_t)w.ns, 1);
    for (int k = 0; k < w.ns; ++k) w.fb.push_back(k);
    return 0;
}

/* residues, behind run_batch: the device's count came back under its wait; the host parser's go behind them.  Enqueues the
   areas (PBUF_RES_AREAS) and their way back into page-locked c->res_stage: areas | the device's res_first, reference rows,
   labels, first residue per file.  Sets w.R, w.Rd. */
int residues_enqueue(Sweep &S, freesasa_gpu_ctx *c, Work &w, const Batch &hb, std::vector<int64_t> &hrf)
{
    const long long Rd = parse_batch_dev_residues_found(c), Rh = hb.b.n_residues, R = Rd + Rh;
    if (R <= 0) return 0;
    if (Rd < 0 || R >= (1LL << 31)) return ctx_fail(c, "bad residue count from the device parser");
    DevBuf *B = c->parse;
    if (parse_batch_dev_residues_build(c, (int)Rd, Rh, S.a.classifier != nullptr) || ensure(c, B[PBUF_RES_AREAS], 88 * (size_t)R) ||
        ensure_pinned(c, &c->res_stage, &c->res_stage_cap, 88 * (size_t)R + 24 * (size_t)Rd + 8 + 4 * (size_t)w.ns))
        return -1;
    if (Rh > 0) {
        hrf.resize((size_t)Rh + 1);
        for (long long j = 0; j <= Rh; ++j) hrf[(size_t)j] = w.total + hb.b.res_first[j];
        if (hipMemcpyAsync((int64_t *)B[PBUF_RES_FIRST].p + Rd, hrf.data(), 8 * ((size_t)Rh + 1), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync((int16_t *)B[PBUF_RES_REF].p + Rd, hb.b.res_ref, 2 * (size_t)Rh, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return ctx_fail(c, "host-to-device copy failed");
    }
    double *d_abs = (double *)B[PBUF_RES_AREAS].p;
    if (residue_areas_resident(c, (double *)c->h_sasa.p, (const unsigned char *)c->h_counts.p, (const unsigned char *)B[PBUF_BACKBONE].p,
                               (const int64_t *)B[PBUF_RES_FIRST].p, (const short *)B[PBUF_RES_REF].p, (int)R, d_abs, d_abs + 6 * R))
        return -1;
    unsigned char *r_stage = (unsigned char *)c->res_stage, *q = r_stage + 88 * (size_t)R;
    bool ok = hipMemcpyAsync(r_stage, d_abs, 88 * (size_t)R, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (Rd > 0)
        ok = ok && hipMemcpyAsync(q, B[PBUF_RES_FIRST].p, 8 * ((size_t)Rd + 1), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
             hipMemcpyAsync(q + 8 * ((size_t)Rd + 1), B[PBUF_RES_REF].p, 2 * (size_t)Rd, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
             hipMemcpyAsync(q + 8 + 10 * (size_t)Rd, B[PBUF_RES_LABELS].p, 14 * (size_t)Rd, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
             hipMemcpyAsync(q + 8 + 24 * (size_t)Rd, B[PBUF_FILE_RES0].p, 4 * (size_t)w.ns, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (!ok) return ctx_fail(c, "device-to-host copy failed");
    w.rb->size(R);
    w.R = R; w.Rd = Rd;
    return 0;
}
/* ... and, the stream waited for, from the page-locked block and the host parser's batch into the batch's ResBatch */
int residues_collect(freesasa_gpu_ctx *c, Work &w, const Batch &hb)
{
    ResBatch *rb = w.rb.get();
    const long long R = w.R, Rd = w.Rd, Rh = R - Rd;
    const unsigned char *r_stage = (const unsigned char *)c->res_stage, *q = r_stage + 88 * (size_t)R;
    memcpy(rb->areas.data(), r_stage, 88 * (size_t)R);
    if (Rd > 0) {
        memcpy(rb->res_first.data(), q, 8 * ((size_t)Rd + 1));
        memcpy(rb->ref.data(), q + 8 * ((size_t)Rd + 1), 2 * (size_t)Rd);
        const unsigned char *lab = q + 8 + 10 * (size_t)Rd;
        memcpy(rb->name.data(), lab, 4 * (size_t)Rd);
        memcpy(rb->chain.data(), lab + 4 * (size_t)Rd, 4 * (size_t)Rd);
        memcpy(rb->number.data(), lab + 8 * (size_t)Rd, 6 * (size_t)Rd);
        /* a file's run ends where the next file that kept atoms begins */
        const int *frf = (const int *)(q + 8 + 24 * (size_t)Rd);
        long long end = Rd;
        bool sane = true;
        for (int k = w.ns - 1; k >= 0; --k) {
            if (w.host[(size_t)k] || w.atoms[(size_t)k] == 0) continue;
            if (frf[k] < 0 || frf[k] >= end) { sane = false; break; }
            rb->fstart[(size_t)k] = frf[k]; rb->fcount[(size_t)k] = end - frf[k];
            end = frf[k];
        }
        if (!sane || end != 0) return ctx_fail(c, "the device parser's residue table does not match its atoms");
    }
    for (long long j = 0; j < Rh; ++j) rb->res_first[(size_t)(Rd + j)] = w.total + hb.b.res_first[j];
    rb->res_first[(size_t)R] = w.total + hb.b.n_atoms;
    if (Rh > 0) {
        memcpy(rb->ref.data() + Rd, hb.b.res_ref, 2 * (size_t)Rh);
        memcpy(rb->name.data() + 4 * Rd, hb.b.res_name, 4 * (size_t)Rh);
        memcpy(rb->number.data() + 6 * Rd, hb.b.res_number, 6 * (size_t)Rh);
        memcpy(rb->chain.data() + 4 * Rd, hb.b.res_chain, 4 * (size_t)Rh);
    }
    for (size_t j = 0; j < w.fb.size(); ++j) {
        rb->fstart[(size_t)w.fb[j]] = Rd + hb.b.res_offsets[j];
        rb->fcount[(size_t)w.fb[j]] = hb.b.res_offsets[j + 1] - hb.b.res_offsets[j];
    }
    return 0;
}

/* selections, behind run_batch (the device's residue count came back under its wait): residue boundaries and labels as for
   the residue table; the host parser's residue labels and atom keys go up behind the device's; sel_mask and sel_sums
   (select_kernels.h) are enqueued and their results start their way back into w.sel_area / w.sel_count. */
int select_enqueue(Sweep &S, freesasa_gpu_ctx *c, Work &w, const Batch &hb, int nst, std::vector<int64_t> &hrf, std::vector<uint64_t> &hkeys)
{
    const SweepArgs &a = S.a;
    const long long total = w.total, extra = hb.b.n_atoms;
    const long long Rd = parse_batch_dev_residues_found(c), Rh = hb.b.n_residues, R = Rd + Rh;
    if (Rd < 0 || R <= 0 || R >= (1LL << 31)) return ctx_fail(c, "bad residue count from the device parser");
    DevBuf *B = c->parse;
    if (parse_batch_dev_residues_build(c, (int)Rd, Rh, a.classifier != nullptr)) return -1;
    if (Rh > 0) {
        if (ensure(c, B[PBUF_SEL_LABELS], 14 * (size_t)Rh)) return -1;
        hrf.resize((size_t)Rh + 1);
        for (long long j = 0; j <= Rh; ++j) hrf[(size_t)j] = total + hb.b.res_first[j];
        hkeys.resize((size_t)extra);
        sel_pack_atom_keys(hb.b.atom_name, hb.b.atom_symbol, extra, hkeys.data());
        char *lab = (char *)B[PBUF_SEL_LABELS].p;
        if (hipMemcpyAsync((int64_t *)B[PBUF_RES_FIRST].p + Rd, hrf.data(), 8 * ((size_t)Rh + 1), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync((uint64_t *)B[PBUF_ATOM_KEYS].p + total, hkeys.data(), 8 * (size_t)extra, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(lab, hb.b.res_name, 4 * (size_t)Rh, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(lab + 4 * (size_t)Rh, hb.b.res_chain, 4 * (size_t)Rh, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(lab + 8 * (size_t)Rh, hb.b.res_number, 6 * (size_t)Rh, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return ctx_fail(c, "host-to-device copy failed");
    }
    sasa::SelArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.akey = (const uint64_t *)B[PBUF_ATOM_KEYS].p;
    sa.offsets = (const int64_t *)c->offsets.p; /* (run_batch left the batch's offsets there) */
    sa.n_structs = nst; sa.n_atoms = total + extra;
    sa.res_first = (const int64_t *)B[PBUF_RES_FIRST].p; sa.n_res = R; sa.n_res_dev = Rd;
    sa.name_d = (const uint32_t *)B[PBUF_RES_LABELS].p; sa.chain_d = sa.name_d + Rd; sa.number_d = (const uint16_t *)(sa.chain_d + Rd);
    const char *lab = (const char *)B[PBUF_SEL_LABELS].p;
    sa.name_h = (const uint32_t *)lab; sa.chain_h = (const uint32_t *)(lab + 4 * (size_t)Rh); sa.number_h = (const uint16_t *)(lab + 8 * (size_t)Rh);
    sa.sasa = (const double *)c->h_sasa.p;
    if (select_resident(c, a.sel, sa)) return -1;
    const size_t cells = (size_t)nst * (size_t)sa.n_sel;
    w.sel_area.resize(cells); w.sel_count.resize(cells);
    if (hipMemcpyAsync(w.sel_area.data(), sa.area, 8 * cells, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(w.sel_count.data(), sa.count, 8 * cells, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        return ctx_fail(c, "device-to-host copy failed");
    return 0;
}

/* chain groups, IN PLACE of run_batch: the device's residue count is waited for (it sizes the residue arrays; nothing to wait
   for when the device parsed nothing), residue boundaries and labels as for the selections, the host parser's chain labels
   and the structures' status behind them; the ids kernel (group_kernels.h); n_groups and the group status of every structure
   back (they size the combined batch); then the complex and its groups as ONE batch (groups_resident, gpu_groups.hip).  The
   groups' atoms, and on the stream their three areas and - separate chains - their labels on the way into w.gb.  Leaves the
   complex's areas in c->g_sasa and its totals in d_tot. */
int sweep_batch_too_large(Sweep &S, freesasa_gpu_ctx *c, const Work &w, const char *what, long long count)
{
    const char *p0 = S.a.paths[w.first], *p1 = S.a.paths[w.first + w.ns - 1];
    return ctx_fail(c, "the batch of files %d .. %d (%.90s .. %.90s) needs %lld %s: use a smaller batch_atoms", w.first, w.first + w.ns - 1,
                    p0 ? p0 : "", p1 ? p1 : "", count, what);
}

/* interfaces, IN PLACE of groups_resident (which is iface_run's step 1: the group outputs come from the same buffers): the one
   run with capacities that hold anything and no output arrays; the batch's block sized from P and R; the sides' class sums
   (k_ifs_side_class, the class-sum kernel over the sides) and the rows' place and labels (k_ifs_res_rows); the delivery into the
   block enqueued.  ng [nst]: the groups of every structure (0 where the group status is not 0); cnt: the atoms of every group.
   `r` outlives the stream's work (the worker's). */
int ifaces_run(Sweep &S, freesasa_gpu_ctx *c, Work &w, int nst, const std::vector<int64_t> &off, const int32_t *d_group, const int32_t *ng,
               long long n_res, long long Rd, double *d_tot, IfaceRun &r, std::vector<int> *cnt)
{
    const SweepArgs &a = S.a;
    const long long n_all = off[(size_t)nst], Rh = n_res - Rd;
    w.screen.assign(ng, ng + nst);
    long long T = 0;
    for (int k = 0; k < nst; ++k) {
        if (w.screen[(size_t)k] > IF_MAX_GROUPS) w.screen[(size_t)k] = 0; /* (FREESASA_GPU_EIFACE_GROUPS: its groups are summed, its pairs not looked for) */
        T += (long long)w.screen[(size_t)k] * (w.screen[(size_t)k] - 1) / 2;
    }
    if (T > IF_MAX_TESTS) return sweep_batch_too_large(S, c, w, "pairs of groups to test (a batch takes up to 2^27)", T);
    if (ensure(c, c->h_iso, 8 * (size_t)n_all)) return -1;
    r = IfaceRun();
    IfaceCall k;
    k.xyz = (const double *)c->h_xyz.p; k.radii = (const double *)c->h_radii.p; k.offsets = off.data(); k.n_structs = nst;
    k.group = d_group; k.n_groups = ng; k.screen_groups = w.screen.data();
    k.alg = a.alg; k.probe = a.probe; k.resolution = a.resolution;
    k.sasa = (double *)c->h_sasa.p; k.iso = (double *)c->h_iso.p; k.totals = d_tot; k.group_totals = (double *)c->h_gtot.p;
    k.whole = true; k.residues = a.ifc->residues;
    k.res_first_dev = (const int64_t *)c->parse[PBUF_RES_FIRST].p; k.n_res = (int)n_res; k.min_buried = a.ifc->min_buried;
    k.pair_capacity = k.atom_capacity = k.res_capacity = 0x7fffffffffffffffLL;
    k.n_pairs = &w.if_counts[0]; k.n_pair_atoms = &w.if_counts[1]; k.n_res_rows = &w.if_counts[2];
    if (iface_run(c, k, r)) {
        const long long atoms = (long long)(r.pl.n + r.pl.n_iso + r.pl.M);
        return atoms > 1LL << 30 ? sweep_batch_too_large(S, c, w, "atoms in the batch, its groups and its pair structures together (a batch takes up to 2^30)", atoms) : -1;
    }
    const int64_t *gstart = r.pl.meta.data();
    cnt->resize((size_t)r.pl.G);
    for (int g = 0; g < r.pl.G; ++g) (*cnt)[(size_t)g] = (int)(gstart[g + 1] - gstart[g]);
    const size_t P = (size_t)r.pl.P, M = (size_t)r.pl.M, R = (size_t)r.rt.R;
    IfcBatch *ib = w.ib.get();
    ib->size((long long)P, (long long)R);
    if (P == 0) return 0; /* (nothing to launch, nothing to deliver) */
    hipStream_t st = c->stream;
    /* class sums [6 P] | pair_struct [P] | the rows' place [R] | names [4 R] | chains [4 R] | numbers [6 R] | the atoms' classes [M] */
    const size_t o_ps = 48 * P, o_loc = o_ps + 4 * P, o_lab = o_loc + 4 * R, o_cls = o_lab + 14 * R + (R & 1) * 2;
    if (ensure(c, c->ifs_work, o_cls + M + 8)) return -1;
    char *wk = (char *)c->ifs_work.p;
    sasa::IfsClassArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.n_pair_atoms = (int64_t)M; ca.pair_atom = (const int *)c->if_patom.p; ca.cls = (const unsigned char *)c->h_counts.p;
    ca.pcls = (unsigned char *)(wk + o_cls);
    HIP_TRY(c, kl_ifs_side_class(ca, st));
    HIP_TRY(c, kl_class_sums((const double *)c->if_pburied.p, ca.pcls, (const int64_t *)c->if_sides.p, (int)(2 * P), (double *)wk, st));
    HIP_TRY(c, hipMemcpyAsync(ib->cls.data(), wk, 48 * P, hipMemcpyDeviceToHost, st));
    IfaceCall d = k; /* the same call with the block's arrays */
    d.pair_areas = ib->areas.data();
    if (k.residues) { d.res_offsets = ib->res_off.data(); d.res_atoms = ib->res_atoms.data(); d.res_areas = ib->res_areas.data(); }
    if (iface_deliver(c, d, r, false)) return -1;
    if (R == 0) return 0;
    sasa::IfsRowArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.n_rows = (int64_t)R; ra.n_sides = (int64_t)(2 * P); ra.res_off = r.rt.off; ra.pair_struct = (const int *)(wk + o_ps);
    ra.offsets = (const int64_t *)c->gi_words.p; ra.res_first = k.res_first_dev; ra.n_res = n_res; ra.n_res_dev = Rd; ra.res_index = r.rt.index;
    ra.name_d = (const uint32_t *)c->parse[PBUF_RES_LABELS].p; ra.chain_d = ra.name_d + Rd; ra.number_d = (const uint16_t *)(ra.chain_d + Rd);
    ra.name_h = (const uint32_t *)c->parse[PBUF_SEL_LABELS].p; ra.chain_h = ra.name_h + Rh; ra.number_h = (const uint16_t *)(ra.chain_h + Rh);
    ra.res_local = (int *)(wk + o_loc); ra.name = (uint32_t *)(wk + o_lab); ra.chain = ra.name + R; ra.number = (uint16_t *)(ra.chain + R);
    HIP_TRY(c, hipMemcpyAsync(wk + o_ps, r.pl.pair_struct.data(), 4 * P, hipMemcpyHostToDevice, st));
    HIP_TRY(c, kl_ifs_res_rows(ra, st));
    HIP_TRY(c, hipMemcpyAsync(ib->res_index.data(), ra.res_local, 4 * R, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(ib->labels.data(), ra.name, 14 * R, hipMemcpyDeviceToHost, st));
    return 0;
}
/* ... and, the stream waited for: what the plan holds of the table, the pairs' labels from the group block, a file's run of pairs */
void ifaces_collect(Work &w, const IfaceRun &r)
{
    IfcBatch *ib = w.ib.get();
    const GrpBatch *gb = w.gb.get();
    for (long long p = 0; p < ib->P; ++p) {
        const int k = r.pl.pair_struct[(size_t)p];
        const size_t f = k < w.nd ? (size_t)k : (size_t)w.fb[(size_t)(k - w.nd)];
        if (ib->fcount[f]++ == 0) ib->fstart[f] = p;
        for (int side = 0; side < 2; ++side) {
            const size_t q = 2 * (size_t)p + side;
            ib->groups[q] = r.pl.pair_groups[q];
            ib->atoms[q] = (int32_t)(r.pl.side_off[q + 1] - r.pl.side_off[q]);
            ib->chain[q] = gb->chain[(size_t)(gb->fstart[f] + ib->groups[q])];
        }
    }
}

int groups_run(Sweep &S, freesasa_gpu_ctx *c, Work &w, const Batch &hb, int nst, const std::vector<int64_t> &off, std::vector<int64_t> &hrf, double *d_tot,
               IfaceRun &ir)
{
    const SweepArgs &a = S.a;
    const GroupSpec &gs = *a.grp;
    const long long total = w.total, n_all = off[(size_t)nst];
    if (c->parse_atoms > 0 && hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
    const long long Rd = parse_batch_dev_residues_found(c), Rh = hb.b.n_residues, R = Rd + Rh;
    if (Rd < 0 || R <= 0 || R >= (1LL << 31)) return ctx_fail(c, "bad residue count from the device parser");
    DevBuf *B = c->parse;
    if (parse_batch_dev_residues_build(c, (int)Rd, Rh, a.classifier != nullptr)) return -1;
    const size_t b_off = 8 * ((size_t)nst + 1);
    /* (interfaces: the rows' labels are gathered on the device, so the host parser's names and numbers go up beside its chains -
       the selection sweep's 14 bytes per residue, names | chains | numbers) */
    const bool ifc = a.ifc != nullptr;
    if (ensure(c, B[PBUF_SEL_LABELS], (ifc ? 14 : 4) * (size_t)Rh + 4) || ensure(c, c->h_group, 4 * (size_t)n_all) || ensure(c, c->gi_words, b_off + 12 * (size_t)nst)) return -1;
    char *hlab = (char *)B[PBUF_SEL_LABELS].p + (ifc ? 4 * (size_t)Rh : 0); /* the host parser's chains */
    if (Rh > 0) {
        hrf.resize((size_t)Rh + 1);
        for (long long j = 0; j <= Rh; ++j) hrf[(size_t)j] = total + hb.b.res_first[j];
        if (hipMemcpyAsync((int64_t *)B[PBUF_RES_FIRST].p + Rd, hrf.data(), 8 * ((size_t)Rh + 1), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(hlab, hb.b.res_chain, 4 * (size_t)Rh, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            (ifc && (hipMemcpyAsync(B[PBUF_SEL_LABELS].p, hb.b.res_name, 4 * (size_t)Rh, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                     hipMemcpyAsync(hlab + 4 * (size_t)Rh, hb.b.res_number, 6 * (size_t)Rh, hipMemcpyHostToDevice, c->stream) != hipSuccess)))
            return ctx_fail(c, "host-to-device copy failed");
    }
    /* structure k < nd is file k (one the device refused: an empty structure that failed), structure nd + j the j-th file the host read */
    w.gwords.assign(3 * (size_t)nst, 0);
    for (int k = 0; k < w.nd; ++k) w.gwords[(size_t)k] = w.host[(size_t)k] ? FREESASA_INGEST_EIO : w.status[(size_t)k];
    for (size_t j = 0; j < w.fb.size(); ++j) w.gwords[(size_t)w.nd + j] = hb.b.status[j];
    char *words = (char *)c->gi_words.p;
    if (hipMemcpyAsync(words, off.data(), b_off, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(words + b_off, w.gwords.data(), 4 * (size_t)nst, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return ctx_fail(c, "host-to-device copy failed");
    sasa::GidArgs ga;
    memset(&ga, 0, sizeof ga);
    ga.offsets = (const int64_t *)words; ga.n_structs = nst;
    ga.res_first = (const int64_t *)B[PBUF_RES_FIRST].p; ga.n_res = R; ga.n_res_dev = Rd;
    ga.chain_d = (const uint32_t *)B[PBUF_RES_LABELS].p + Rd; ga.chain_h = (const uint32_t *)hlab;
    ga.status = (const int32_t *)(words + b_off); ga.n_groups = (int32_t *)(words + b_off) + nst; ga.group_status = ga.n_groups + nst;
    ga.group = (int32_t *)c->h_group.p;
    if (group_ids_resident(c, gs, ga)) return -1;
    if (hipMemcpyAsync(w.gwords.data() + nst, ga.n_groups, 8 * (size_t)nst, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return ctx_fail(c, "device-to-host copy failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
    /* a structure whose group status is not 0 owns no groups */
    int32_t *ng = w.gwords.data() + nst;
    const int32_t *gst = ng + nst;
    long long G = 0;
    for (int k = 0; k < nst; ++k) { if (gst[k] != 0) ng[k] = 0; G += ng[k]; }
    if (ensure(c, c->h_gtot, 24 * (size_t)G + 8)) return -1;
    std::vector<int> cnt;
    if (ifc ? ifaces_run(S, c, w, nst, off, ga.group, ng, R, Rd, d_tot, ir, &cnt)
            : groups_resident(c, a.alg, (const double *)c->h_xyz.p, (const double *)c->h_radii.p, off.data(), nst, ga.group, ng, a.probe, a.resolution,
                              a.alg == 1 ? S.tp.data() : nullptr, nullptr, nullptr, d_tot, (double *)c->h_gtot.p, &cnt))
        return -1;
    GrpBatch *gb = w.gb.get();
    gb->atoms.assign(cnt.begin(), cnt.end());
    gb->areas.resize(3 * (size_t)G); gb->chain.assign((size_t)G, 0);
    long long at = 0;
    for (int k = 0; k < nst; ++k) {
        const size_t f = k < w.nd ? (size_t)k : (size_t)w.fb[(size_t)(k - w.nd)];
        if (k < w.nd && w.host[(size_t)k]) continue;
        gb->fstart[f] = at; gb->fcount[f] = ng[k];
        a.group_status_out[w.first + (int)f] = gst[k];
        if (ifc) a.ifc->status_out[w.first + (int)f] = gst[k] ? gst[k] : (ng[k] > IF_MAX_GROUPS ? FREESASA_GPU_EIFACE_GROUPS : 0);
        if (!gs.separate) for (int g = 0; g < ng[k]; ++g) gb->chain[(size_t)(at + g)] = gs.first_label[(size_t)g];
        at += ng[k];
    }
    if (G == 0) return 0;
    if (gs.separate) {
        if (ensure(c, c->gi_label, 4 * (size_t)G)) return -1;
        sasa::GidLabelArgs la;
        memset(&la, 0, sizeof la);
        la.coffsets = (const int64_t *)c->offsets.p; la.src = (const int *)c->g_src.p;
        if (ifc && ir.pl.P > 0) { /* (run_batch over the pair structures has left ITS offsets in c->offsets: the combined batch's, from the counts) */
            std::vector<int64_t> &comb = ir.res_first; /* (the run's spare host array: it outlives the stream's work) */
            comb.assign(off.begin(), off.end());
            for (long long g = 0; g < G; ++g) comb.push_back(comb.back() + cnt[(size_t)g]);
            if (ensure(c, c->ifs_comb, 8 * comb.size())) return -1;
            if (hipMemcpyAsync(c->ifs_comb.p, comb.data(), 8 * comb.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess) return ctx_fail(c, "host-to-device copy failed");
            la.coffsets = (const int64_t *)c->ifs_comb.p;
        }
        la.n_structs = nst; la.n_groups = (int)G; la.n_atoms = n_all;
        la.res_first = ga.res_first; la.n_res = R; la.n_res_dev = Rd; la.chain_d = ga.chain_d; la.chain_h = ga.chain_h;
        la.label = (uint32_t *)c->gi_label.p;
        if (kl_gid_label(la, c->stream) != hipSuccess) return ctx_fail(c, "kernel launch failed");
        if (hipMemcpyAsync(gb->chain.data(), la.label, 4 * (size_t)G, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return ctx_fail(c, "device-to-host copy failed");
    }
    if (hipMemcpyAsync(gb->areas.data(), c->h_gtot.p, 24 * (size_t)G, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return ctx_fail(c, "device-to-host copy failed");
    return 0;
}

/* The rest of a batch, whoever parsed: w.nd structures of w.total atoms are on the device (c->h_xyz, h_radii, h_counts;
   backbone flags and residue keys in c->parse[]), hb holds the files w.fb as the host parser read them and goes up behind
   them.  Results into the caller's arrays, w.atoms64 / w.cls and w.rb; on success the stream has been waited for. */
int tail(Sweep &S, freesasa_gpu_ctx *c, Work &w, const Batch &hb, std::vector<int64_t> &hrf, std::vector<uint64_t> &hkeys, IfaceRun &ir)
{
    const SweepArgs &a = S.a;
    const int ns = w.ns, first = w.first, nd = w.nd, nst = nd + (int)w.fb.size();
    const long long total = w.total, extra = hb.b.n_atoms, n_all = total + extra;
    if (parse_batch_dev_finish(c, extra)) return -1;
    if ((a.rcol || a.sel || a.grp) && parse_batch_dev_residues_count(c, extra)) return -1;
    if (a.sel && parse_batch_dev_atom_keys(c, extra)) return -1;
    const int n_sel = a.sel ? freesasa_ingest_selection_count(a.sel) : 0;
    std::vector<int64_t> off((size_t)nst + 1);
    off[0] = 0;
    for (int k = 0; k < nd; ++k) off[(size_t)k + 1] = off[(size_t)k] + w.atoms[(size_t)k];
    for (size_t j = 0; j < w.fb.size(); ++j) off[(size_t)nd + j + 1] = total + hb.b.offsets[j + 1];
    for (int k = 0; k < ns; ++k) {
        a.status_out[first + k] = w.status[(size_t)k];
        a.totals_out[first + k] = 0;
        w.atoms64[(size_t)k] = w.atoms[(size_t)k];
        if (a.class_sums_out) a.class_sums_out[3 * (first + k)] = a.class_sums_out[3 * (first + k) + 1] = a.class_sums_out[3 * (first + k) + 2] = 0;
        for (int q = 0; q < n_sel; ++q) { a.sel_area_out[(size_t)(first + k) * n_sel + q] = 0; a.sel_atoms_out[(size_t)(first + k) * n_sel + q] = 0; }
    }
    for (size_t j = 0; j < w.fb.size(); ++j) { a.status_out[first + w.fb[j]] = hb.b.status[j]; w.atoms64[(size_t)w.fb[j]] = hb.b.offsets[j + 1] - hb.b.offsets[j]; }
    if (a.grp) for (int k = 0; k < ns; ++k) a.group_status_out[first + k] = a.status_out[first + k]; /* (a batch without atoms: nobody loaded) */
    if (a.ifc) for (int k = 0; k < ns; ++k) a.ifc->status_out[first + k] = a.status_out[first + k];
    if (a.atoms_out) for (int k = 0; k < ns; ++k) a.atoms_out[first + k] = w.atoms64[(size_t)k];
    if (n_all == 0) return 0;
    if (extra > 0 &&
        (hipMemcpyAsync((double *)c->h_xyz.p + 3 * total, hb.b.xyz, 24 * (size_t)extra, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
         hipMemcpyAsync((double *)c->h_radii.p + total, hb.b.radii, 8 * (size_t)extra, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
         hipMemcpyAsync((unsigned char *)c->h_counts.p + total, hb.b.atom_class, (size_t)extra, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
         (a.rcol && hipMemcpyAsync((unsigned char *)c->parse[PBUF_BACKBONE].p + total, hb.b.atom_backbone, (size_t)extra, hipMemcpyHostToDevice, c->stream) != hipSuccess)))
        return ctx_fail(c, "host-to-device copy failed");
    if (ensure(c, c->h_sasa, 8 * (size_t)n_all) || ensure(c, c->h_totals, 8 * 4 * (size_t)nst)) return -1;
    double *d_tot = (double *)c->h_totals.p, *d_cls = d_tot + nst;
    const double *d_areas = (const double *)c->h_sasa.p;
    if (a.grp) {
        if (groups_run(S, c, w, hb, nst, off, hrf, d_tot, ir)) return -1;
        d_areas = (const double *)c->g_sasa.p;
    } else if (run_batch(c, a.alg == 0, (double *)c->h_xyz.p, (double *)c->h_radii.p, off.data(), nst, a.probe, a.resolution,
                         a.alg == 1 ? S.tp.data() : nullptr, (double *)c->h_sasa.p, nullptr, d_tot))
        return -1;
    if (a.rcol && residues_enqueue(S, c, w, hb, hrf)) return -1;
    if (a.sel && select_enqueue(S, c, w, hb, nst, hrf, hkeys)) return -1;
    std::vector<double> tot((size_t)nst), cls;
    if (S.want_cls) {
        cls.resize(3 * (size_t)nst);
        if (freesasa_gpu_class_sums_dev(c, d_areas, (const unsigned char *)c->h_counts.p, off.data(), nst, d_cls)) return -1;
        if (hipMemcpyAsync(cls.data(), d_cls, 8 * 3 * (size_t)nst, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return ctx_fail(c, "device-to-host copy failed");
    }
    if (hipMemcpyAsync(tot.data(), d_tot, 8 * (size_t)nst, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return ctx_fail(c, "device-to-host copy failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
    /* structure k < nd of the batch is file k; structure nd + j is the j-th file the host read */
    for (int k = 0; k < nd; ++k) a.totals_out[first + k] = tot[(size_t)k];
    for (size_t j = 0; j < w.fb.size(); ++j) a.totals_out[first + w.fb[j]] = tot[(size_t)nd + j];
    if (S.want_cls) {
        w.cls.assign(3 * (size_t)ns, 0);
        if (nd) memcpy(w.cls.data(), cls.data(), 8 * 3 * (size_t)nd);
        for (size_t j = 0; j < w.fb.size(); ++j) memcpy(&w.cls[3 * (size_t)w.fb[j]], &cls[3 * ((size_t)nd + j)], 8 * 3);
        if (a.class_sums_out) memcpy(a.class_sums_out + 3 * (size_t)first, w.cls.data(), 8 * 3 * (size_t)ns);
    }
    for (int k = 0; k < nst && n_sel; ++k) { /* (a structure without atoms has sums of nothing: the zeros are there already) */
        const size_t f = (size_t)first + (k < nd ? (size_t)k : (size_t)w.fb[(size_t)(k - nd)]);
        memcpy(a.sel_area_out + f * n_sel, &w.sel_area[(size_t)k * n_sel], 8 * (size_t)n_sel);
        memcpy(a.sel_atoms_out + f * n_sel, &w.sel_count[(size_t)k * n_sel], 8 * (size_t)n_sel);
    }
    if (a.ifc) ifaces_collect(w, ir);
    return w.R > 0 ? residues_collect(c, w, hb) : 0;
}

/* the results of a finished batch into the result file, then its line in the done-list */
int record(Sweep &S, freesasa_gpu_ctx *c, const Work &w)
{
    std::vector<SweepRec> recs((size_t)w.ns);
    for (int k = 0; k < w.ns; ++k) {
        SweepRec &r = recs[(size_t)k];
        memset(&r, 0, sizeof r);
        r.total = S.a.totals_out[w.first + k]; r.status = S.a.status_out[w.first + k];
        r.atoms = w.atoms64[(size_t)k];
        if (!w.cls.empty()) for (int q = 0; q < 3; ++q) r.cls[q] = w.cls[3 * (size_t)k + q];
    }
    /* (the records of a batch lie at their own offset: no lock; the list itself is appended to by one worker at a time) */
    if (!pwrite_all(S.res.fd, recs.data(), sizeof(SweepRec) * recs.size(), (long long)sizeof(SweepRec) * w.first) || fdatasync(S.res.fd) != 0 ||
        S.list.append(w.b, w.first, w.ns))
        return ctx_fail(c, "could not record the finished batch in the done-list");
    return 0;
}

/* A worker owns a pooled context of its device and a loader: while batch k is on the GPU the loader thread prepares the
   batch the worker took next (Ahead).  A batch is a chain on the context's stream: text or arrays over PCIe, parse, cell
   sort, tile kernels, aggregates, results back. */
void worker(Sweep &S, int wi) noexcept
{
  try {
    /* declared before the context, so freed after its stream is idle (PoolLease), whatever ends the worker: the host parser's
       part of the batch in hand and its res_first, shifted - copies to the device read both */
    Batch hb;
    std::vector<int64_t> hrf;
    std::vector<uint64_t> hkeys; /* (the host parser's atom keys, packed: selections) */
    IfaceRun ir;                 /* (interfaces: the run's plan - uploads read it) */
    DeviceNodeScope node(S.a.devices[wi]); /* this worker - its context's page-locked memory, its loader threads - on the device's NUMA node */
    PoolLease lease(S.a.devices[wi]);
    freesasa_gpu_ctx *c = lease.c;
    if (!c) { S.fe.set("could not create a GPU context"); return; }
    Ahead cur(&c->stage_in, &c->stage_in_cap), nxt(&c->stage_out, &c->stage_out_cap);
    size_t ti = S.next.fetch_add(1);
    { const long long t0 = S.sprof ? now_ns() : 0;
      if (ti < S.todo.size()) look_ahead(S, S.todo[ti], &cur);
      if (S.sprof) S.tp_first += now_ns() - t0; }
    while (ti < S.todo.size() && !S.fe.failed.load()) {
        const size_t tn = S.next.fetch_add(1); /* the batch this worker does next: prepared while this one computes */
        ThreadGroup loader; /* (joined before nxt can go away, whatever happens below) */
        if (tn < S.todo.size() && !loader.spawn(look_ahead, std::ref(S), S.todo[tn], &nxt)) { S.fe.set("could not start a loader thread"); break; }
        Work w(S, S.todo[ti]);
        int ret = hipSetDevice(c->device) == hipSuccess ? 0 : ctx_fail(c, "hipSetDevice failed");
        if (!ret) ret = S.dev_parse ? front_device(S, c, cur, w, hb) : front_host(c, cur, w, hb);
        long long tr = S.sprof ? now_ns() : 0;
        if (!ret) {
            /* (copies into the batch's blocks may be on the stream when a host allocation fails: they end before `w` does) */
            try { ret = tail(S, c, w, hb, hrf, hkeys, ir); } catch (...) { (void)hipStreamSynchronize(c->stream); throw; }
        }
        if (ret) (void)hipStreamSynchronize(c->stream); /* no copy may still read the batch when it is freed */
        if (S.sprof) { const long long t1 = now_ns(); S.tp_run += t1 - tr; tr = t1; }
        if (!ret && S.list.active()) ret = record(S, c, w);
        if (!ret && S.a.rcol) S.a.rcol->add(w.rb);
        if (!ret && S.a.gcol) S.a.gcol->add(w.gb);
        if (!ret && S.a.ifc) S.a.ifc->col->add(w.ib);
        if (ret) S.fe.set(c->err[0] ? c->err : "GPU sweep failed");
        if (S.sprof) { const long long t1 = now_ns(); S.tp_rec += t1 - tr; tr = t1; }
        loader.join();
        if (S.sprof) S.tp_join += now_ns() - tr;
        cur.swap(nxt);
        ti = tn;
    }
  } catch (...) { /* (an exception that leaves a thread's function ends the process: it ends the sweep instead) */
    S.fe.set_exception();
  }
}

/* The done-list of this sweep (gpu_drivers.hip says what a done-list is) and its result file <done_path>.bin: per file total
   | class sums (3) | atoms | status (SweepRec), written before the batch is listed.  -1: another run's list, or files that
   cannot be opened. */
int open_done_list(Sweep &S, int n_batches, char *err_out, int err_len)
{
    const SweepArgs &a = S.a;
    unsigned long long h = 1469598103934665603ULL; /* FNV-1a over the files' names, sizes and modification times: the done-list belongs to THESE files as they are now */
    for (int k = 0; k < a.n_paths; ++k) {
        for (const char *q = a.paths[k] ? a.paths[k] : ""; ; ++q) { h = (h ^ (unsigned char)*q) * 1099511628211ULL; if (!*q) break; }
        struct stat st;
        long long id[3] = {-1, -1, -1};
        if (a.paths[k] && stat(a.paths[k], &st) == 0) { id[0] = (long long)st.st_size; id[1] = (long long)st.st_mtim.tv_sec; id[2] = (long long)st.st_mtim.tv_nsec; }
        for (size_t q = 0; q < sizeof id; ++q) h = (h ^ ((const unsigned char *)id)[q]) * 1099511628211ULL;
    }
    char head[256];
    snprintf(head, sizeof head, "freesasa_amd sweep done-list v2 n_files=%d batches=%d files=%016llx options=%d alg=%d resolution=%d probe=%.17g\n",
             a.n_paths, n_batches, h, S.options, a.alg, a.resolution, a.probe); /* (who parses does not change a result: not part of the run's name) */
    if (a.classifier) { /* (without one the line is what it always was: earlier done-lists resume) */
        const size_t hl = strlen(head);
        snprintf(head + hl - 1, sizeof head - (hl - 1), " classifier=%016llx\n", (unsigned long long)freesasa_ingest_classifier_digest(a.classifier));
    }
    const std::vector<int> &cut = S.cut;
    if (S.list.read(a.done_path, head, n_batches, [&cut](long long b, long long first, long long count) { return first == cut[(size_t)b] && count == cut[(size_t)b + 1] - cut[(size_t)b]; }) == DoneList::REFUSED)
        return set_err(err_out, err_len, "the done-list belongs to a sweep with other parameters or other (changed) input files");
    const std::string res_path = std::string(a.done_path) + ".bin";
    S.res.fd = open(res_path.c_str(), S.list.resumed() ? O_RDWR | O_CREAT : O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (S.res.fd < 0 || S.list.open()) return set_err(err_out, err_len, "cannot open the done-list or its result file");
    return 0;
}
/* the results of a batch the done-list names, from the result file (false: unreadable - the batch is computed again) */
bool load_recorded(Sweep &S, int b)
{
    const SweepArgs &a = S.a;
    std::vector<SweepRec> recs((size_t)(S.cut[b + 1] - S.cut[b]));
    if (!pread_all(S.res.fd, recs.data(), sizeof(SweepRec) * recs.size(), (long long)sizeof(SweepRec) * S.cut[b])) return false;
    for (size_t k = 0; k < recs.size(); ++k) {
        const int f = S.cut[b] + (int)k;
        a.totals_out[f] = recs[k].total; a.status_out[f] = recs[k].status;
        if (a.atoms_out) a.atoms_out[f] = recs[k].atoms;
        if (a.class_sums_out) for (int q = 0; q < 3; ++q) a.class_sums_out[3 * f + q] = recs[k].cls[q];
    }
    return true;
}

/* Files -> per-structure totals.  Inputs that fail to load get total 0 and their loader status; the call only fails for GPU
 * errors.  With a done-list (a.done_path) a call that finds the list of the same run takes the listed batches' results from
 * the result file and only computes the others.
 * Returns 0 done, 1 stopped after max_new_batches, -1 error. */
int sweep_impl(SweepArgs a, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!a.paths || a.n_paths < 0 || !a.totals_out || !a.status_out) return set_err(err_out, err_len, "null argument");
    if (a.alg != 0 && a.alg != 1) return set_err(err_out, err_len, "unknown algorithm");
    if (check_devices(a.devices, a.n_devices, err_out, err_len)) return -1;
    if (a.n_paths == 0) return 0;
    /* (round 6, MI355X box, 1.2e7 protein atoms in 7172 files, 16 CPUs, two workers on the device, parser on the device,
       batches of 5e5 / 1e6 / 1.5e6 / 2e6 atoms: 2.2 / 2.5 / 2.4 / 2.3e8 atoms/s once the workers' page-locked staging stays
       with their contexts - tools/dev/sweep_profile.py; with a staging buffer allocated and freed per call, as until the
       round's last session: 1.7 / 1.5 / - / 1.1e8; host parser 1.25 / 1.34 / - / 1.31e8) */
    if (a.batch_atoms <= 0) a.batch_atoms = 1000000;
    /* ONE device in the list: two workers on it, so that the upload of one batch runs under the kernels of the other */
    const int two[2] = {a.devices[0], a.devices[0]};
    if (a.n_devices == 1 && !getenv("FREESASA_AMD_SWEEP_ONE_WORKER")) { a.devices = two; a.n_devices = 2; }
    return guarded(err_out, err_len, [&]() -> int {
    Sweep S(a);
    S.dev_parse = (a.ingest_options & FREESASA_INGEST_PARSE_ON_DEVICE) != 0;
    S.options = a.ingest_options & ~FREESASA_INGEST_PARSE_ON_DEVICE;
    S.want_cls = a.class_sums_out != nullptr || a.done_path != nullptr;
    S.sprof = getenv("FREESASA_AMD_SWEEP_PROFILE") != nullptr;
    /* batches of roughly batch_atoms atoms, estimated from the file sizes (~81 bytes per ATOM line) */
    S.cut.assign(1, 0);
    std::vector<long long> batch_bytes;
    long long bytes = 0;
    for (int k = 0; k < a.n_paths; ++k) {
        struct stat st;
        bytes += (a.paths[k] && stat(a.paths[k], &st) == 0) ? (long long)st.st_size : 0;
        if (bytes >= a.batch_atoms * 81 && k + 1 < a.n_paths) { S.cut.push_back(k + 1); batch_bytes.push_back(bytes); bytes = 0; }
    }
    S.cut.push_back(a.n_paths);
    batch_bytes.push_back(bytes);
    const int n_batches = (int)S.cut.size() - 1;
    if (a.done_path && open_done_list(S, n_batches, err_out, err_len)) return -1;
    for (int b = 0; b < n_batches; ++b)
        if (!S.list.done(b) || !load_recorded(S, b)) S.todo.push_back(b);
    bool stopped = false;
    if (a.max_new_batches > 0 && (long long)S.todo.size() > a.max_new_batches) { S.todo.resize((size_t)a.max_new_batches); stopped = true; }
    if (S.todo.empty()) return stopped ? 1 : 0;
    /* largest first (LPT): whoever is free takes the largest batch left */
    std::stable_sort(S.todo.begin(), S.todo.end(), [&](int x, int y) { return batch_bytes[(size_t)x] > batch_bytes[(size_t)y]; });
    const int n_workers = a.n_devices < (int)S.todo.size() ? a.n_devices : (int)S.todo.size();
    S.loader_threads = threads_per_worker(a.n_threads, n_workers);
    if (a.alg == 1) { S.tp.resize(3 * (size_t)(a.resolution > 0 ? a.resolution : 1)); if (a.resolution > 0) freesasa_gpu_test_points(a.resolution, S.tp.data()); }
    run_lanes(n_workers, S.fe, [&S](int w) noexcept { worker(S, w); });
    if (S.sprof && S.dev_parse)
        fprintf(stderr, "sweep profile (%d workers, %zu batches, %d loader threads each; ms summed over the workers): first batch staged %.1f | parse %.1f | host parser %.1f | "
                        "kernels to totals %.1f | done-list %.1f | waiting for the loader %.1f || staging itself (loader threads) %.1f\n",
                n_workers, S.todo.size(), S.loader_threads, S.tp_first / 1e6, S.tp_parse / 1e6, S.tp_host / 1e6, S.tp_run / 1e6, S.tp_rec / 1e6, S.tp_join / 1e6, S.tp_stage / 1e6);
    if (S.fe.failed.load()) return set_err(err_out, err_len, S.fe.text);
    return stopped ? 1 : 0;
    });
}

} /* namespace */

/* ------------------------------------------------------------------ entry points */

/* The device-side parser on its own (tests, tools): n files -> coordinates, radii and classes of the atoms it keeps (host
   arrays of `cap` atoms), offsets_out [n + 1], status_out [n] (the loader's codes), host_out [n] (1: the device refuses the
   file - the sweep would hand it to the host parser - and it contributes nothing here).  Returns the atoms written, -1 on
   error, -2 if cap is too small (offsets_out[n] says how many are needed). */
extern "C" long long freesasa_gpu_parse_files_classified(const char *const *paths, int n_paths, int ingest_options, int n_threads, int device,
                                                         double *xyz_out, double *radii_out, unsigned char *class_out, long long cap,
                                                         long long *offsets_out, int *status_out, int *host_out,
                                                         const freesasa_ingest_classifier *classifier, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!paths || n_paths <= 0 || !offsets_out || !status_out || !host_out) return set_err(err_out, err_len, "bad argument");
    if (check_devices(&device, 1, err_out, err_len)) return -1;
    long long written = -1;
    const int rc = guarded(err_out, err_len, [&]() -> int {
        PoolLease lease(device);
        freesasa_gpu_ctx *c = lease.c;
        if (!c) return set_err(err_out, err_len, "could not create a GPU context");
        Staged s(&c->stage_in, &c->stage_in_cap);
        if (hipSetDevice(c->device) != hipSuccess) return set_err(err_out, err_len, "hipSetDevice failed");
        stage_files(paths, n_paths, ingest_options & ~FREESASA_INGEST_PARSE_ON_DEVICE, threads_per_worker(n_threads, 1), &s);
        if (s.rc) return set_err(err_out, err_len, "could not stage the files");
        std::vector<int> atoms((size_t)n_paths);
        long long total = 0;
        if (parse_batch_dev_begin(c, s.text, s.T, s.files.data(), n_paths, ingest_options & ~FREESASA_INGEST_PARSE_ON_DEVICE, classifier, atoms.data(), status_out, host_out, &total) ||
            parse_batch_dev_finish(c, 0))
            return set_err(err_out, err_len, c->err);
        offsets_out[0] = 0;
        for (int k = 0; k < n_paths; ++k) offsets_out[k + 1] = offsets_out[k] + atoms[(size_t)k];
        if (total > cap) { written = -2; return 0; }
        if (total > 0 &&
            ((xyz_out && hipMemcpyAsync(xyz_out, c->h_xyz.p, 24 * (size_t)total, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
             (radii_out && hipMemcpyAsync(radii_out, c->h_radii.p, 8 * (size_t)total, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
             (class_out && hipMemcpyAsync(class_out, c->h_counts.p, (size_t)total, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
             hipStreamSynchronize(c->stream) != hipSuccess))
            return set_err(err_out, err_len, "device-to-host copy failed");
        written = total;
        return 0;
    });
    return rc ? -1 : written;
}

extern "C" long long freesasa_gpu_parse_files(const char *const *paths, int n_paths, int ingest_options, int n_threads, int device,
                                              double *xyz_out, double *radii_out, unsigned char *class_out, long long cap,
                                              long long *offsets_out, int *status_out, int *host_out, char *err_out, int err_len)
{
    return freesasa_gpu_parse_files_classified(paths, n_paths, ingest_options, n_threads, device, xyz_out, radii_out, class_out, cap,
                                               offsets_out, status_out, host_out, nullptr, err_out, err_len);
}

/* files the sweeps of this process parsed on the device / left to the host parser since the last call (FREESASA_INGEST_PARSE_ON_DEVICE) */
extern "C" void freesasa_gpu_sweep_parse_stats(long long *device_files, long long *host_files)
{
    if (device_files) *device_files = g_parse_dev_files.exchange(0);
    if (host_files) *host_files = g_parse_host_files.exchange(0);
}

extern "C" int freesasa_gpu_sweep_files_classified(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                                   int alg, double probe, int resolution, long long batch_atoms,
                                                   double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                                   const char *done_path, long long max_new_batches, const int *devices, int n_devices,
                                                   const freesasa_ingest_classifier *classifier, char *err_out, int err_len)
{
    return sweep_impl({paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out, atoms_out, status_out,
                       done_path, max_new_batches, devices, n_devices, classifier, nullptr, nullptr, nullptr, nullptr}, err_out, err_len);
}

extern "C" int freesasa_gpu_sweep_files_devices(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                                int alg, double probe, int resolution, long long batch_atoms,
                                                double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                                const char *done_path, long long max_new_batches, const int *devices, int n_devices,
                                                char *err_out, int err_len)
{
    return freesasa_gpu_sweep_files_classified(paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out,
                                               atoms_out, status_out, done_path, max_new_batches, devices, n_devices, nullptr, err_out, err_len);
}

extern "C" int freesasa_gpu_sweep_files_resumable(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                                  int alg, double probe, int resolution, long long batch_atoms,
                                                  double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                                  const char *done_path, long long max_new_batches, int device, char *err_out, int err_len)
{
    return freesasa_gpu_sweep_files_devices(paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out,
                                            atoms_out, status_out, done_path, max_new_batches, &device, 1, err_out, err_len);
}

extern "C" int freesasa_gpu_sweep_files(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                        int alg, double probe, int resolution, long long batch_atoms,
                                        double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                        int device, char *err_out, int err_len)
{
    return freesasa_gpu_sweep_files_resumable(paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out,
                                              atoms_out, status_out, nullptr, 0, device, err_out, err_len);
}

/* The sweep with the per-residue table (include/freesasa_gpu.h): the batches' blocks (ResBatch) into ONE block behind
   res_offsets, files in the caller's order, each file's residues in the file's order. */
static int assemble_residue_table(int n_paths, std::vector<std::unique_ptr<ResBatch>> &done, freesasa_gpu_residue_table *t, char *err_out, int err_len)
{
    std::vector<long long> count((size_t)n_paths, 0);
    std::vector<char> seen((size_t)n_paths, 0);
    for (auto &rb : done)
        for (int k = 0; k < rb->ns; ++k) { count[(size_t)(rb->first + k)] = rb->fcount[(size_t)k]; seen[(size_t)(rb->first + k)] = 1; }
    long long R = 0;
    for (int f = 0; f < n_paths; ++f) {
        if (!seen[(size_t)f]) return set_err(err_out, err_len, "a batch of the sweep left no residue block");
        R += count[(size_t)f];
    }
    const size_t n = (size_t)n_paths, r = (size_t)R;
    const size_t o_abs = 8 * (n + 1), o_rel = o_abs + 48 * r, o_atoms = o_rel + 40 * r, o_ref = o_atoms + 4 * r, o_name = o_ref + 2 * r,
                 o_number = o_name + 4 * r, o_chain = o_number + 6 * r, bytes = o_chain + 4 * r;
    char *blk = (char *)hf_malloc(bytes + 8);
    if (!blk) return set_err(err_out, err_len, "out of host memory (residue table)");
    t->n_files = n_paths; t->n_residues = R;
    t->res_offsets = (int64_t *)blk; t->abs = (double *)(blk + o_abs); t->rel = (double *)(blk + o_rel);
    t->res_atoms = (int32_t *)(blk + o_atoms); t->res_ref = (int16_t *)(blk + o_ref);
    t->res_name = blk + o_name; t->res_number = blk + o_number; t->res_chain = blk + o_chain;
    t->res_offsets[0] = 0;
    for (int f = 0; f < n_paths; ++f) t->res_offsets[f + 1] = t->res_offsets[f] + count[(size_t)f];
    for (auto &rb : done) {
        const double *b_abs = rb->areas.data(), *b_rel = b_abs + 6 * rb->n_res;
        for (int k = 0; k < rb->ns; ++k) {
            const size_t m = (size_t)rb->fcount[(size_t)k], src = (size_t)rb->fstart[(size_t)k], dst = (size_t)t->res_offsets[rb->first + k];
            if (!m) continue;
            memcpy(t->abs + 6 * dst, b_abs + 6 * src, 48 * m);
            memcpy(t->rel + 5 * dst, b_rel + 5 * src, 40 * m);
            memcpy(t->res_ref + dst, rb->ref.data() + src, 2 * m);
            memcpy(t->res_name + 4 * dst, rb->name.data() + 4 * src, 4 * m);
            memcpy(t->res_number + 6 * dst, rb->number.data() + 6 * src, 6 * m);
            memcpy(t->res_chain + 4 * dst, rb->chain.data() + 4 * src, 4 * m);
            for (size_t q = 0; q < m; ++q) t->res_atoms[dst + q] = (int32_t)(rb->res_first[src + q + 1] - rb->res_first[src + q]);
        }
    }
    return 0;
}

extern "C" void freesasa_gpu_residue_table_free(freesasa_gpu_residue_table *table)
{
    if (!table) return;
    free(table->res_offsets); /* (the one block: assemble_residue_table) */
    memset(table, 0, sizeof *table);
}

extern "C" int freesasa_gpu_sweep_files_residues(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                                 int alg, double probe, int resolution, long long batch_atoms,
                                                 double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                                 const int *devices, int n_devices, const freesasa_ingest_classifier *classifier,
                                                 freesasa_gpu_residue_table *table_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (table_out) memset(table_out, 0, sizeof *table_out);
    if (!table_out) return set_err(err_out, err_len, "null argument");
    const int rc = guarded(err_out, err_len, [&]() -> int {
        ResCollector col;
        if (sweep_impl({paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out, atoms_out, status_out,
                        nullptr, 0, devices, n_devices, classifier, &col, nullptr, nullptr, nullptr}, err_out, err_len))
            return -1;
        return assemble_residue_table(n_paths, col.done, table_out, err_out, err_len);
    });
    if (rc) freesasa_gpu_residue_table_free(table_out);
    return rc ? -1 : 0;
}

/* The sweep with selections (include/freesasa_gpu.h): a SweepArgs member away from the residue sweep. */
extern "C" int freesasa_gpu_sweep_files_select(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                               int alg, double probe, int resolution, long long batch_atoms,
                                               double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                               const int *devices, int n_devices, const freesasa_ingest_classifier *classifier,
                                               const freesasa_ingest_selection *sel, double *sel_area_out, long long *sel_atoms_out,
                                               char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!sel || !sel_area_out || !sel_atoms_out) return set_err(err_out, err_len, "null argument");
    if (freesasa_ingest_selection_count(sel) < 1) return set_err(err_out, err_len, "empty selection set");
    const int rc = sweep_impl({paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out, atoms_out, status_out,
                               nullptr, 0, devices, n_devices, classifier, nullptr, sel, sel_area_out, sel_atoms_out}, err_out, err_len);
    return rc ? -1 : 0;
}

/* The sweep with chain groups (include/freesasa_gpu.h): the batches' blocks (GrpBatch) into ONE block behind group_offsets,
   files in the caller's order, each file's groups in their order. */
static int assemble_group_table(int n_paths, std::vector<std::unique_ptr<GrpBatch>> &done, freesasa_gpu_group_table *t, char *err_out, int err_len)
{
    std::vector<long long> count((size_t)n_paths, 0);
    std::vector<char> seen((size_t)n_paths, 0);
    for (auto &gb : done)
        for (int k = 0; k < gb->ns; ++k) { count[(size_t)(gb->first + k)] = gb->fcount[(size_t)k]; seen[(size_t)(gb->first + k)] = 1; }
    long long G = 0;
    for (int f = 0; f < n_paths; ++f) {
        if (!seen[(size_t)f]) return set_err(err_out, err_len, "a batch of the sweep left no group block");
        G += count[(size_t)f];
    }
    const size_t n = (size_t)n_paths, g = (size_t)G;
    const size_t o_areas = 8 * (n + 1), o_atoms = o_areas + 24 * g, o_chain = o_atoms + 4 * g, bytes = o_chain + 4 * g;
    char *blk = (char *)hf_malloc(bytes + 8);
    if (!blk) return set_err(err_out, err_len, "out of host memory (group table)");
    t->n_files = n_paths; t->n_groups = G;
    t->group_offsets = (int64_t *)blk; t->areas = (double *)(blk + o_areas); t->group_atoms = (int32_t *)(blk + o_atoms); t->chain = blk + o_chain;
    t->group_offsets[0] = 0;
    for (int f = 0; f < n_paths; ++f) t->group_offsets[f + 1] = t->group_offsets[f] + count[(size_t)f];
    for (auto &gb : done)
        for (int k = 0; k < gb->ns; ++k) {
            const size_t m = (size_t)gb->fcount[(size_t)k], src = (size_t)gb->fstart[(size_t)k], dst = (size_t)t->group_offsets[gb->first + k];
            if (!m) continue;
            memcpy(t->areas + 3 * dst, gb->areas.data() + 3 * src, 24 * m);
            memcpy(t->group_atoms + dst, gb->atoms.data() + src, 4 * m);
            memcpy(t->chain + 4 * dst, gb->chain.data() + src, 4 * m);
        }
    return 0;
}

extern "C" void freesasa_gpu_group_table_free(freesasa_gpu_group_table *table)
{
    if (!table) return;
    free(table->group_offsets); /* (the one block: assemble_group_table) */
    memset(table, 0, sizeof *table);
}

extern "C" int freesasa_gpu_sweep_files_groups(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                               int alg, double probe, int resolution, long long batch_atoms,
                                               double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                               const int *devices, int n_devices, const freesasa_ingest_classifier *classifier,
                                               const char *spec, int group_flags, int *group_status_out,
                                               freesasa_gpu_group_table *table_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (table_out) memset(table_out, 0, sizeof *table_out);
    if (!table_out || !group_status_out) return set_err(err_out, err_len, "null argument");
    const int rc = guarded(err_out, err_len, [&]() -> int {
        GroupSpec gs; /* (outlives the workers and their contexts' streams) */
        if (group_spec_parse(spec, group_flags, &gs, err_out, err_len)) return -1;
        GrpCollector col;
        SweepArgs a = {paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out, atoms_out, status_out,
                       nullptr, 0, devices, n_devices, classifier, nullptr, nullptr, nullptr, nullptr, &gs, &col, group_status_out};
        if (sweep_impl(a, err_out, err_len)) return -1;
        return assemble_group_table(n_paths, col.done, table_out, err_out, err_len);
    });
    if (rc) freesasa_gpu_group_table_free(table_out);
    return rc ? -1 : 0;
}

/* The sweep with the interfaces between chain groups (include/freesasa_gpu.h): the batches' blocks (IfcBatch) into ONE block
   behind pair_offsets, files in the caller's order, each file's pairs in the tests' order, the residue rows of their sides behind
   res_offsets. */
static int assemble_interface_table(int n_paths, bool residues, std::vector<std::unique_ptr<IfcBatch>> &done, freesasa_gpu_interface_table *t,
                                    char *err_out, int err_len)
{
    std::vector<long long> count((size_t)n_paths, 0), rows((size_t)n_paths, 0);
    std::vector<char> seen((size_t)n_paths, 0);
    for (auto &ib : done)
        for (int k = 0; k < ib->ns; ++k) {
            const size_t f = (size_t)(ib->first + k), p0 = (size_t)ib->fstart[(size_t)k], m = (size_t)ib->fcount[(size_t)k];
            count[f] = (long long)m; seen[f] = 1;
            if (residues && m) rows[f] = ib->res_off[2 * (p0 + m)] - ib->res_off[2 * p0];
        }
    long long P = 0, R = 0;
    for (int f = 0; f < n_paths; ++f) {
        if (!seen[(size_t)f]) return set_err(err_out, err_len, "a batch of the sweep left no interface block");
        P += count[(size_t)f]; R += rows[(size_t)f];
    }
    const size_t n = (size_t)n_paths, p = (size_t)P, r = (size_t)R;
    const size_t o_areas = 8 * (n + 1), o_cls = o_areas + 48 * p, o_roff = o_cls + 48 * p, o_rareas = o_roff + (residues ? 8 * (2 * p + 1) : 0),
                 o_groups = o_rareas + 24 * r, o_atoms = o_groups + 8 * p, o_chain = o_atoms + 8 * p, o_rindex = o_chain + 8 * p,
                 o_ratoms = o_rindex + 4 * r, o_rname = o_ratoms + 4 * r, o_rchain = o_rname + 4 * r, o_rnumber = o_rchain + 4 * r,
                 bytes = o_rnumber + 6 * r;
    char *blk = (char *)hf_malloc(bytes + 8);
    if (!blk) return set_err(err_out, err_len, "out of host memory (interface table)");
    t->n_files = n_paths; t->n_pairs = P; t->n_res_rows = R;
    t->pair_offsets = (int64_t *)blk; t->pair_areas = (double *)(blk + o_areas); t->pair_class_buried = (double *)(blk + o_cls);
    t->pair_groups = (int32_t *)(blk + o_groups); t->pair_atoms = (int32_t *)(blk + o_atoms); t->pair_chain = blk + o_chain;
    if (residues) {
        t->res_offsets = (int64_t *)(blk + o_roff); t->res_areas = (double *)(blk + o_rareas);
        t->res_index = (int32_t *)(blk + o_rindex); t->res_atoms = (int32_t *)(blk + o_ratoms);
        t->res_name = blk + o_rname; t->res_chain = blk + o_rchain; t->res_number = blk + o_rnumber;
    }
    t->pair_offsets[0] = 0;
    for (int f = 0; f < n_paths; ++f) t->pair_offsets[f + 1] = t->pair_offsets[f] + count[(size_t)f];
    std::vector<long long> row0((size_t)n_paths + 1, 0);
    for (int f = 0; f < n_paths; ++f) row0[(size_t)f + 1] = row0[(size_t)f] + rows[(size_t)f];
    if (residues) t->res_offsets[2 * p] = R;
    for (auto &ib : done)
        for (int k = 0; k < ib->ns; ++k) {
            const size_t f = (size_t)(ib->first + k), m = (size_t)ib->fcount[(size_t)k], src = (size_t)ib->fstart[(size_t)k], dst = (size_t)t->pair_offsets[f];
            if (!m) continue;
            memcpy(t->pair_areas + 6 * dst, ib->areas.data() + 6 * src, 48 * m);
            memcpy(t->pair_class_buried + 6 * dst, ib->cls.data() + 6 * src, 48 * m);
            memcpy(t->pair_groups + 2 * dst, ib->groups.data() + 2 * src, 8 * m);
            memcpy(t->pair_atoms + 2 * dst, ib->atoms.data() + 2 * src, 8 * m);
            memcpy(t->pair_chain + 8 * dst, ib->chain.data() + 2 * src, 8 * m);
            if (!residues) continue;
            const long long b0 = ib->res_off[2 * src];
            const size_t rs = (size_t)b0, rd = (size_t)row0[f], rm = (size_t)rows[f], RB = (size_t)ib->R;
            for (size_t q = 0; q < 2 * m; ++q) t->res_offsets[2 * dst + q] = row0[f] + (ib->res_off[2 * src + q] - b0);
            if (!rm) continue;
            memcpy(t->res_index + rd, ib->res_index.data() + rs, 4 * rm);
            memcpy(t->res_atoms + rd, ib->res_atoms.data() + rs, 4 * rm);
            memcpy(t->res_areas + 3 * rd, ib->res_areas.data() + 3 * rs, 24 * rm);
            memcpy(t->res_name + 4 * rd, ib->labels.data() + 4 * rs, 4 * rm);
            memcpy(t->res_chain + 4 * rd, ib->labels.data() + 4 * RB + 4 * rs, 4 * rm);
            memcpy(t->res_number + 6 * rd, ib->labels.data() + 8 * RB + 6 * rs, 6 * rm);
        }
    return 0;
}

extern "C" void freesasa_gpu_interface_table_free(freesasa_gpu_interface_table *table)
{
    if (!table) return;
    free(table->pair_offsets); /* (the one block: assemble_interface_table) */
    memset(table, 0, sizeof *table);
}

extern "C" int freesasa_gpu_sweep_files_interfaces(const char *const *paths, int n_paths, int ingest_options, int n_threads,
                                                   int alg, double probe, int resolution, long long batch_atoms,
                                                   double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out,
                                                   const int *devices, int n_devices, const freesasa_ingest_classifier *classifier,
                                                   const char *spec, int group_flags, int *group_status_out,
                                                   freesasa_gpu_group_table *table_out, int residue_rows, double min_buried,
                                                   int *iface_status_out, freesasa_gpu_interface_table *itable_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (table_out) memset(table_out, 0, sizeof *table_out);
    if (itable_out) memset(itable_out, 0, sizeof *itable_out);
    if (!group_status_out) return set_err(err_out, err_len, "null argument");
    const int rc = guarded(err_out, err_len, [&]() -> int {
        GroupSpec gs; /* (outlives the workers and their contexts' streams) */
        if (group_spec_parse(spec, group_flags, &gs, err_out, err_len)) return -1;
        if (!(min_buried >= 0.0) || min_buried > 1.7976931348623157e308) return set_err(err_out, err_len, "min_buried must be finite and >= 0");
        if (!itable_out || !iface_status_out) return set_err(err_out, err_len, "null argument");
        GrpCollector col;
        IfcCollector icol;
        const IfaceSpec is = {residue_rows != 0, min_buried, &icol, iface_status_out};
        SweepArgs a = {paths, n_paths, ingest_options, n_threads, alg, probe, resolution, batch_atoms, totals_out, class_sums_out, atoms_out, status_out,
                       nullptr, 0, devices, n_devices, classifier, nullptr, nullptr, nullptr, nullptr, &gs, &col, group_status_out, &is};
        if (sweep_impl(a, err_out, err_len)) return -1;
        if (table_out && assemble_group_table(n_paths, col.done, table_out, err_out, err_len)) return -1;
        return assemble_interface_table(n_paths, is.residues, icol.done, itable_out, err_out, err_len);
    });
    if (rc) { freesasa_gpu_group_table_free(table_out); freesasa_gpu_interface_table_free(itable_out); }
    return rc ? -1 : 0;
}
