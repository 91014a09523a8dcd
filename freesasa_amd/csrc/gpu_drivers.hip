/*
 * gpu_drivers.hip — the drivers for BASELINE configs[3] and configs[4] (include/freesasa_gpu.h): the structure sweep
 * over PDB / mmCIF files (gpu_sweep.hip), the same sweep from a binary cache, and the trajectory drivers (both here, with
 * what all three share: engine_internal.h) — each over ONE device or a LIST of devices of the node.  Host code; kernels
 * in gpu_kernels.hip.
 *
 * What replaces what: the reference reads one file per run of its CLI (src/main.cc:763-779) and spreads ONE structure
 * over <= 16 pthreads (src/sasa_lr.c:219-253).  Here the unit of parallel work is a batch of whole structures (a
 * shard of whole frames), and the units are independent: there is no exchange between devices, only a shared list of
 * work.  One worker (sweep) or a few lanes (trajectory, cache sweep) per entry of devices[] take the next unit from a
 * shared counter — largest first for the file sweep (LPT on the file sizes: atoms are proportional to bytes) — so
 * that a device that finishes early takes more; every result lands at its own place of the caller's arrays / the
 * result files (pwrite at the unit's offset), and ONE done-list, appended to under a mutex after a unit's results
 * are on disk, serves all devices.  The host CPUs THE CGROUP GRANTS (freesasa_ingest_usable_cpus: a GPU box shows 256
 * and grants 16) are divided among the devices' loaders.  A device may appear in the list more than once (its units
 * then overlap their copies and kernels; the tests run device lists [0, 0, 0] and [0] * 8 on a one-GPU box).
 * Results are bit-identical to the single-device drivers': a unit's numbers do not depend on who computed it.
 */
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>

#include "engine_internal.h"
#include "select_program.h"

bool pread_all(int fd, void *buf, size_t bytes, long long off)
{
    char *p = (char *)buf;
    while (bytes) {
        const ssize_t r = pread(fd, p, bytes, (off_t)off);
        if (r <= 0) return false;
        p += r; off += r; bytes -= (size_t)r;
    }
    return true;
}
bool pwrite_all(int fd, const void *buf, size_t bytes, long long off)
{
    const char *p = (const char *)buf;
    while (bytes) {
        const ssize_t r = pwrite(fd, p, bytes, (off_t)off);
        if (r <= 0) return false;
        p += r; off += r; bytes -= (size_t)r;
    }
    return true;
}

int check_devices(const int *devices, int n_devices, char *err_out, int err_len)
{
    const int n_dev = freesasa_gpu_device_count();
    if (n_dev <= 0) return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    if (!devices || n_devices <= 0 || n_devices > 64) return set_err(err_out, err_len, "bad device list (1 .. 64 entries)");
    for (int k = 0; k < n_devices; ++k)
        if (devices[k] < -1 || devices[k] >= n_dev) return set_err(err_out, err_len, "device index out of range");
    return 0;
}

/* CPUs THIS PROCESS may count on: what the cgroup grants (freesasa_ingest_usable_cpus), divided among the ranks of the node
   when a launcher says there are several (one process per GPU: torchrun exports LOCAL_WORLD_SIZE).  What every default
   below - loader threads, lanes per device - starts from: eight ranks of a box that grants 16 CPUs get two each, not
   sixteen each (the host budget). */
int process_cpus()
{
    int total = freesasa_ingest_usable_cpus();
    if (const char *lws = getenv("LOCAL_WORLD_SIZE")) {
        const int ranks = atoi(lws);
        if (ranks > 1) total /= ranks;
    }
    return total < 1 ? 1 : total;
}
int threads_per_worker(int n_threads, int n_workers)
{
    const int total = n_threads > 0 ? n_threads : process_cpus();
    const int per = total / (n_workers > 0 ? n_workers : 1);
    return per < 1 ? 1 : per;
}

/* (engine_internal.h) */
int DoneList::read(const char *path, const char *head, long long n_units, const std::function<bool(long long, long long, long long)> &valid)
{
    path_ = path; head_ = head; resumed_ = false;
    done_.assign((size_t)n_units, 0);
    FILE *fp = fopen(path, "r");
    if (!fp) return FRESH;
    char line[512];
    if (fgets(line, sizeof line, fp)) {
        if (head_ != line) { fclose(fp); return REFUSED; }
        resumed_ = true;
        long long k, a, b;
        while (fgets(line, sizeof line, fp))
            if (sscanf(line, "shard %lld %lld %lld", &k, &a, &b) == 3 && k >= 0 && k < n_units && valid(k, a, b) && line[strlen(line) - 1] == '\n')
                done_[(size_t)k] = 1;
    }
    fclose(fp);
    return resumed_ ? RESUMED : FRESH;
}
int DoneList::open()
{
    f.fd = ::open(path_.c_str(), resumed_ ? O_WRONLY | O_APPEND : O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) return -1;
    return !resumed_ && write(f.fd, head_.data(), head_.size()) != (ssize_t)head_.size() ? -2 : 0;
}
int DoneList::append(long long k, long long a, long long b)
{
    char line[96];
    const int len = snprintf(line, sizeof line, "shard %lld %lld %lld\n", k, a, b);
    std::lock_guard<std::mutex> lk(mu);
    if (write(f.fd, line, (size_t)len) != len || fdatasync(f.fd) != 0) return -1;
    done_[(size_t)k] = 1;
    return 0;
}

namespace {

struct Cache {
    freesasa_ingest_cache *c = nullptr;
    Cache() = default;
    Cache(const Cache &) = delete;
    Cache &operator=(const Cache &) = delete;
    ~Cache() { if (c) freesasa_ingest_cache_close(c); }
};

/* ------------------------------------------------------------------ structure sweep: from a binary cache */

/* The sweep of a cache file (freesasa_ingest_save): no parsing, no classification — what is left on the host is to get
 * 33 bytes per atom (coordinates, radius, class) from the file into page-locked memory, which one thread does at
 * ~1e8 atoms/s (pread from the page cache + checksum) against 4.5e8 atoms/s of one GPU at protein density.  So every
 * device gets several lanes (threads), each with its own pooled context and page-locked staging: a lane takes the
 * next batch of structures from the shared counter, reads and verifies exactly its run of atoms
 * (freesasa_ingest_cache_read_atoms: piece checksums) into its staging buffer, copies it to the device and computes,
 * while the other lanes are in another stage. */
int sweep_cache_impl(const char *cache_path, int alg, double probe, int resolution, long long batch_atoms,
                     double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out, int n_out,
                     const int *devices, int n_devices, int lanes_per_device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!cache_path || !totals_out) return set_err(err_out, err_len, "null argument");
    if (alg != 0 && alg != 1) return set_err(err_out, err_len, "unknown algorithm");
    if (resolution <= 0) return set_err(err_out, err_len, "resolution must be > 0");
    if (check_devices(devices, n_devices, err_out, err_len)) return -1;
    return guarded(err_out, err_len, [&]() -> int {
    Cache cache_h; /* (closed on every way out) */
    const int orc = freesasa_ingest_cache_open(cache_path, &cache_h.c);
    if (orc) {
        char msg[96];
        snprintf(msg, sizeof msg, "cannot open the cache file (freesasa_ingest code %d)", orc);
        return set_err(err_out, err_len, msg);
    }
    freesasa_ingest_cache *const cache = cache_h.c;
    const int S = freesasa_ingest_cache_n_structs(cache);
    const int64_t *offs = freesasa_ingest_cache_offsets(cache);
    const int32_t *stat = freesasa_ingest_cache_status(cache);
    if (n_out < S) return set_err(err_out, err_len, "the output arrays are shorter than the cache's structure count");
    if (batch_atoms <= 0) batch_atoms = 1000000; /* (measured, round 5, 1.2e7 protein atoms on one MI355X with 16 CPUs: 8 lanes x 1e6 atoms 3.5e8 atoms/s, 4 x 2e6 3.1e8, 2 x 2e6 2.6e8; the kernels alone run 4.5e8 at this density) */
    if (batch_atoms > (1LL << 30)) batch_atoms = 1LL << 30;
    std::vector<int> cut(1, 0);
    for (int s = 0; s < S; ++s) {
        if (offs[s + 1] - offs[s] > (1LL << 30)) return set_err(err_out, err_len, "a structure of the cache is too large for one batch");
        if (offs[s + 1] - offs[cut.back()] > batch_atoms && s > cut.back()) cut.push_back(s); /* (a batch never exceeds batch_atoms unless one structure does) */
    }
    cut.push_back(S);
    const int n_batches = (int)cut.size() - 1;
    for (int s = 0; s < S; ++s) {
        totals_out[s] = 0;
        if (status_out) status_out[s] = stat[s];
        if (atoms_out) atoms_out[s] = offs[s + 1] - offs[s];
        if (class_sums_out) class_sums_out[3 * s] = class_sums_out[3 * s + 1] = class_sums_out[3 * s + 2] = 0;
    }
    if (lanes_per_device <= 0) {
        /* the granted CPUs divided among the devices, 8 at most; two where they allow (one lane reads while the other
           computes) - but never more lanes in all than twice the CPUs: eight devices on four CPUs get one lane each, not
           sixteen threads that read and checksum in turns (round-5 advisor) */
        const int cpus = process_cpus();
        lanes_per_device = cpus / n_devices;
        if (lanes_per_device > 8) lanes_per_device = 8;
        if (lanes_per_device < 2) lanes_per_device = 2 * cpus >= 2 * n_devices ? 2 : 1;
    }
    if (lanes_per_device > 8) lanes_per_device = 8;
    int n_lanes = lanes_per_device * n_devices;
    if (n_lanes > n_batches) n_lanes = n_batches;
    std::vector<double> tp;
    if (alg == 1) { tp.resize(3 * (size_t)resolution); freesasa_gpu_test_points(resolution, tp.data()); }
    std::atomic<int> next(0);
    FirstError fe;
    auto lane = [&](int id) noexcept {
      try {
        DeviceNodeScope node(devices[id % n_devices]); /* the lane and its page-locked staging on the device's NUMA node */
        PoolLease lease(devices[id % n_devices]);
        freesasa_gpu_ctx *c = lease.c;
        if (!c) { fe.set("could not create a GPU context"); return; }
        std::vector<int64_t> off;
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= n_batches || fe.failed.load()) break;
            const int s0 = cut[b], ns = cut[b + 1] - cut[b];
            const int64_t a0 = offs[s0];
            const size_t n = (size_t)(offs[s0 + ns] - a0);
            if (n == 0) continue;
            off.resize((size_t)ns + 1);
            for (int i = 0; i <= ns; ++i) off[i] = offs[s0 + i] - a0;
            int rc = -1;
            do {
                if (hipSetDevice(c->device) != hipSuccess) { ctx_fail(c, "hipSetDevice failed"); break; }
                if (ensure(c, c->h_xyz, 24 * n) || ensure(c, c->h_radii, 8 * n) || ensure(c, c->h_sasa, 8 * n) ||
                    ensure(c, c->h_counts, n) || ensure(c, c->h_totals, 8 * 4 * (size_t)ns))
                    break;
                if (ensure_pinned(c, &c->stage_in, &c->stage_in_cap, 33 * n + 64) || ensure_pinned(c, &c->stage_out, &c->stage_out_cap, 8 * 4 * (size_t)ns)) break;
                double *h_xyz = (double *)c->stage_in, *h_r = h_xyz + 3 * n;
                uint8_t *h_cls = (uint8_t *)(h_r + n);
                const int rrc = freesasa_ingest_cache_read_atoms(cache, a0, a0 + (int64_t)n, h_xyz, h_r, class_sums_out ? h_cls : nullptr);
                if (rrc) { ctx_fail(c, "the cache file failed its checksum or could not be read (freesasa_ingest code %d)", rrc); break; }
                if (hipMemcpyAsync(c->h_xyz.p, h_xyz, 24 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                    hipMemcpyAsync(c->h_radii.p, h_r, 8 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                    (class_sums_out && hipMemcpyAsync(c->h_counts.p, h_cls, n, hipMemcpyHostToDevice, c->stream) != hipSuccess)) {
                    ctx_fail(c, "host-to-device copy failed");
                    break;
                }
                double *d_tot = (double *)c->h_totals.p, *d_cls = d_tot + ns;
                if (run_batch(c, alg == 0, (double *)c->h_xyz.p, (double *)c->h_radii.p, off.data(), ns, probe, resolution,
                              alg == 1 ? tp.data() : nullptr, (double *)c->h_sasa.p, nullptr, d_tot))
                    break;
                if (class_sums_out && freesasa_gpu_class_sums_dev(c, (double *)c->h_sasa.p, (const unsigned char *)c->h_counts.p, off.data(), ns, d_cls)) break;
                double *h_out = (double *)c->stage_out;
                if (hipMemcpyAsync(h_out, d_tot, 8 * (size_t)(class_sums_out ? 4 * ns : ns), hipMemcpyDeviceToHost, c->stream) != hipSuccess) { ctx_fail(c, "device-to-host copy failed"); break; }
                if (hipStreamSynchronize(c->stream) != hipSuccess) { ctx_fail(c, "stream synchronize failed"); break; }
                memcpy(totals_out + s0, h_out, 8 * (size_t)ns);
                if (class_sums_out) memcpy(class_sums_out + 3 * (size_t)s0, h_out + ns, 8 * 3 * (size_t)ns);
                rc = 0;
            } while (0);
            if (rc) {
                (void)hipStreamSynchronize(c->stream);
                fe.set(c->err[0] ? c->err : "GPU cache sweep failed");
                break;
            }
        }
      } catch (...) {
        fe.set_exception();
      }
    };
    {
        ThreadGroup tg;
        for (int k = 1; k < n_lanes; ++k)
            if (!tg.spawn(lane, k)) { fe.set("could not start a worker thread"); break; }
        if (n_lanes > 0 && !fe.failed.load()) lane(0);
    }
    if (fe.failed.load()) return set_err(err_out, err_len, fe.text);
    return 0;
    });
}

/* ------------------------------------------------------------------ trajectory driver */

/* Frames of ONE system (same atoms, same radii) are independent structures: a SHARD is a run of frames_per_batch
 * frames that goes through the engine as one batch.  A few host lanes PER DEVICE take shards from a shared counter; a
 * lane owns a pooled context (stream, workspace, page-locked staging) of its device and does, for its shard,
 *     read (memory or frame file) -> host-to-device -> [fp32 frames widened to fp64 on the device: an INPUT format,
 *     the arithmetic stays fp64] -> cell sort + tile kernels -> device-to-host -> write (memory or files)
 * while the other lanes are in another stage.  The radii live once per device context (shared by every frame of
 * a batch).  With a done-list file every finished shard is recorded after its results are on disk; a later call
 * with the same parameters skips the recorded shards: an interrupted run resumes — on any list of devices. */
struct TrajIO {
    const double *mem_in = nullptr; /* frames in host memory (fp64) ... */
    int fd_in = -1;                 /* ... or in a file of raw frames */
    int in_f32 = 0;
    long long in_header = 0;
    double *totals_mem = nullptr, *sasa_mem = nullptr;
    int fd_totals = -1, fd_sasa = -1;
    DoneList *list = nullptr;       /* (file runs with a done-list) */
    int out_f32 = 0;                /* per-atom areas written as fp32 (narrowed on the device; an output format) */
    /* runs with a topology: class sums [3], residue areas [6 R], selection areas [S] per frame; the selections' atoms once */
    double *cls_mem = nullptr, *res_mem = nullptr, *sel_mem = nullptr;
    long long *sel_atoms = nullptr;
    int fd_cls = -1, fd_res = -1, fd_sel = -1;
};

/* The TOPOLOGY of a trajectory (include/freesasa_gpu.h, freesasa_gpu_trajectory_topology): one structure of a loaded batch
 * - its radii, classes, backbone flags, atom keys, its residues rebased to the structure - and the index that says which
 * atom of an input frame each of its atoms is.  Constant over the run: a lane uploads it once (topo_upload) and runs the
 * selection set's program over it once; per shard only the gather and the per-frame sums (traj_kernels.h) are enqueued. */
struct TrajTopo {
    int n = 0, frame_atoms = 0, n_res = 0, n_sel = 0;
    const int32_t *index = nullptr;  /* NULL: the identity (frame_atoms == n): frames go to the engine as they are */
    const double *radii = nullptr;
    const uint8_t *cls = nullptr, *bb = nullptr;
    std::vector<int64_t> seg;        /* res_first [n_res + 1] within the structure, then its offsets as a batch of one: 0, n */
    const freesasa_ingest_selection *sel = nullptr;
    std::vector<uint64_t> keys;      /* (selections) name | symbol of every atom */
    const char *res_name = nullptr, *res_chain = nullptr, *res_number = nullptr; /* the structure's first residue's */
};

unsigned long long fnv1a(const void *p, size_t bytes, unsigned long long h = 1469598103934665603ULL)
{
    for (size_t q = 0; q < bytes; ++q) h = (h ^ ((const unsigned char *)p)[q]) * 1099511628211ULL;
    return h;
}

/* the argument checks of a topology, on the host: 0, or -1 with the message */
int topo_make(const freesasa_ingest_batch *b, int structure, int frame_atoms, const int32_t *atom_index,
              const freesasa_ingest_selection *sel, TrajTopo *tp, char *err_out, int err_len)
{
    if (!b) return set_err(err_out, err_len, "null argument: the topology needs a loaded batch");
    if (structure < 0 || structure >= b->n_structs) return set_err(err_out, err_len, "structure out of range");
    if (!b->offsets || !b->res_first || !b->res_offsets || !b->radii || !b->atom_class || !b->atom_backbone || !b->status)
        return set_err(err_out, err_len, "inconsistent batch");
    if (b->status[structure] != 0) return set_err(err_out, err_len, "the topology's structure failed to load (its status is not 0)");
    const int64_t a0 = b->offsets[structure], n = b->offsets[structure + 1] - a0;
    if (n <= 0) return set_err(err_out, err_len, "the topology's structure has no atoms");
    if (n > (1LL << 30)) return set_err(err_out, err_len, "the topology's structure is too large");
    if (frame_atoms < n) return set_err(err_out, err_len, "frame_atoms is smaller than the structure's atom count");
    if (!atom_index && frame_atoms != n) return set_err(err_out, err_len, "without an atom index frame_atoms must be the structure's atom count");
    if (atom_index) {
        std::vector<char> seen((size_t)frame_atoms, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t k = atom_index[i];
            if (k < 0 || k >= frame_atoms) return set_err(err_out, err_len, "atom index out of range");
            if (seen[(size_t)k]) return set_err(err_out, err_len, "an atom index occurs twice");
            seen[(size_t)k] = 1;
        }
    }
    const int64_t r0 = b->res_offsets[structure], R = b->res_offsets[structure + 1] - r0;
    if (R <= 0 || R > n || b->res_first[r0] != a0 || b->res_first[r0 + R] != a0 + n) return set_err(err_out, err_len, "inconsistent batch");
    tp->seg.resize((size_t)R + 3);
    for (int64_t r = 0; r <= R; ++r) {
        if (r && b->res_first[r0 + r] < b->res_first[r0 + r - 1]) return set_err(err_out, err_len, "residue offsets must be non-decreasing");
        tp->seg[(size_t)r] = b->res_first[r0 + r] - a0; /* (rebased: the batch-wide arrays do not start at 0 for structure > 0) */
    }
    tp->seg[(size_t)R + 1] = 0; tp->seg[(size_t)R + 2] = n;
    tp->n = (int)n; tp->frame_atoms = frame_atoms; tp->n_res = (int)R; tp->index = atom_index;
    tp->radii = b->radii + a0; tp->cls = b->atom_class + a0; tp->bb = b->atom_backbone + a0;
    if (sel) {
        if (!b->atom_name || !b->atom_symbol || !b->res_name || !b->res_chain || !b->res_number) return set_err(err_out, err_len, "inconsistent batch");
        tp->sel = sel; tp->n_sel = freesasa_ingest_selection_count(sel);
        if (tp->n_sel < 1 || tp->n_sel > SEL_MAX_SELECTIONS) return set_err(err_out, err_len, "bad selection set");
        tp->keys.resize((size_t)n);
        sel_pack_atom_keys(b->atom_name + 4 * a0, b->atom_symbol + 2 * a0, n, tp->keys.data());
        tp->res_name = b->res_name + 4 * r0; tp->res_chain = b->res_chain + 4 * r0; tp->res_number = b->res_number + 6 * r0;
    }
    return 0;
}

/* Once per lane: the topology onto the lane's context - c->seg: residue boundaries | the one structure's offsets | index |
   classes | backbone flags; with selections the keys, labels and program where freesasa_gpu_select_batch puts them, and
   sel_mask_atom over the topology: the mask words stay in c->parse[PBUF_SEL_BITS].  (run_batch touches none of these.)
   Fills the constant part of `ta`.  Enqueued on the context's stream, nothing waited for. */
int topo_upload(freesasa_gpu_ctx *c, const TrajTopo &tp, sasa::TrajArgs &ta)
{
    const size_t n = (size_t)tp.n, R = (size_t)tp.n_res;
    const size_t b_seg = 8 * (R + 3), b_idx = tp.index ? (4 * n + 7) & ~(size_t)7 : 0;
    if (ensure(c, c->seg, b_seg + b_idx + 2 * n)) return -1;
    char *base = (char *)c->seg.p;
    hipStream_t st = c->stream;
    HIP_TRY(c, hipMemcpyAsync(base, tp.seg.data(), b_seg, hipMemcpyHostToDevice, st));
    if (tp.index) HIP_TRY(c, hipMemcpyAsync(base + b_seg, tp.index, 4 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(base + b_seg + b_idx, tp.cls, n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(base + b_seg + b_idx + n, tp.bb, n, hipMemcpyHostToDevice, st));
    memset(&ta, 0, sizeof ta);
    ta.n = tp.n; ta.frame_atoms = tp.frame_atoms; ta.n_res = tp.n_res; ta.n_sel = tp.n_sel;
    ta.res_first = (const int64_t *)base;
    ta.index = tp.index ? (const int32_t *)(base + b_seg) : nullptr;
    ta.cls = (const unsigned char *)(base + b_seg + b_idx); ta.bb = ta.cls + n;
    if (!tp.sel) return 0;
    int n_words = 0, flags = 0;
    const freesasa_sel_word *prog = (const freesasa_sel_word *)freesasa_ingest_selection_program(tp.sel, &n_words, &flags);
    if (!prog || n_words < 1) return ctx_fail(c, "bad selection set");
    DevBuf *B = c->parse;
    if (ensure(c, B[PBUF_ATOM_KEYS], 8 * n) || ensure(c, B[PBUF_SEL_LABELS], 14 * R) ||
        ensure(c, B[PBUF_SEL_PROG], sizeof(freesasa_sel_word) * (size_t)n_words) || ensure(c, B[PBUF_SEL_BITS], 8 * n))
        return -1;
    char *lab = (char *)B[PBUF_SEL_LABELS].p;
    HIP_TRY(c, hipMemcpyAsync(B[PBUF_ATOM_KEYS].p, tp.keys.data(), 8 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(lab, tp.res_name, 4 * R, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(lab + 4 * R, tp.res_chain, 4 * R, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(lab + 8 * R, tp.res_number, 6 * R, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(B[PBUF_SEL_PROG].p, prog, sizeof(freesasa_sel_word) * (size_t)n_words, hipMemcpyHostToDevice, st));
    sasa::SelArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.prog = (const freesasa_sel_word *)B[PBUF_SEL_PROG].p; sa.n_words = n_words; sa.flags = flags; sa.n_sel = tp.n_sel;
    sa.akey = (const uint64_t *)B[PBUF_ATOM_KEYS].p;
    sa.offsets = (const int64_t *)base + R + 1; sa.n_structs = 1; sa.n_atoms = tp.n;
    sa.res_first = (const int64_t *)base; sa.n_res = tp.n_res; sa.n_res_dev = 0;
    sa.name_h = (const uint32_t *)lab; sa.chain_h = (const uint32_t *)(lab + 4 * R); sa.number_h = (const uint16_t *)(lab + 8 * R);
    sa.bits = (uint64_t *)B[PBUF_SEL_BITS].p;
    HIP_TRY(c, kl_sel_mask(sa, st));
    ta.bits = sa.bits;
    return 0;
}

/* returns 0: all shards done, 1: stopped after max_new shards (more left), -1: error */
int traj_run(TrajIO &io, const double *radii, int n_atoms, long long n_frames, int alg, double probe, int resolution,
             int frames_per_batch, int lanes_per_device, long long max_new, const int *devices, int n_devices, char *err_out, int err_len,
             const TrajTopo *topo = nullptr)
{
    return guarded(err_out, err_len, [&]() -> int {
    const size_t n = (size_t)n_atoms, FB = (size_t)frames_per_batch;
    const long long n_shards = (n_frames + frames_per_batch - 1) / frames_per_batch;
    if (lanes_per_device <= 0) {
        /* three lanes keep one device's PCIe in, kernels and PCIe out busy (measured, round 2; round 6, from and to files on the
           MI355X box, 600 frames x 100 000 atoms: 3 lanes 2.97e8, 6 lanes 3.10e8 atom-frames/s with two of the three contexts
           cold - the kernel trace shows the tile kernels of the lanes back to back, 2.9 ms per shard of 1.2e6 atoms: the
           driver runs at the rate of the kernels); with several devices the lanes also share the granted
           CPUs (a lane reads, copies and writes on the host): two each at least */
        const int per = process_cpus() / n_devices;
        lanes_per_device = per >= 3 ? 3 : 2;
        if (const char *e = getenv("FREESASA_AMD_TRAJ_LANES")) lanes_per_device = atoi(e) > 0 ? atoi(e) : lanes_per_device; /* tuning aid */
    }
    if (lanes_per_device > 8) lanes_per_device = 8;
    int n_lanes = lanes_per_device * n_devices;
    if (n_lanes > n_shards) n_lanes = (int)n_shards;
    std::vector<double> tp;
    if (alg == 1) { tp.resize(3 * (size_t)resolution); freesasa_gpu_test_points(resolution, tp.data()); }
    std::vector<int64_t> offs(FB + 1);
    for (size_t k = 0; k <= FB; ++k) offs[k] = (int64_t)(k * n);
    const bool in_pinned = io.mem_in && host_pinned(io.mem_in);
    const bool out_pinned = io.totals_mem && host_pinned(io.totals_mem) && (!io.sasa_mem || host_pinned(io.sasa_mem));
    const bool want_sasa = io.sasa_mem || io.fd_sasa >= 0;
    /* a topology: frames of fa atoms come in (the gather makes the engine's n of them), and per frame xw more numbers go out */
    const bool gather = topo && topo->index;
    const size_t fa = topo ? (size_t)topo->frame_atoms : n, esz = io.in_f32 ? 12 : 24;
    const size_t widen_bytes = io.in_f32 && !gather ? 12 * n * FB : 0; /* (fp32 frames without an index: kl_widen_f32's input) */
    const bool want_cls = topo && (io.cls_mem || io.fd_cls >= 0), want_res = topo && (io.res_mem || io.fd_res >= 0);
    const bool want_sel = topo && topo->sel && (io.sel_mem || io.fd_sel >= 0 || io.sel_atoms);
    const size_t R = topo ? (size_t)topo->n_res : 0, S = want_sel ? (size_t)topo->n_sel : 0;
    const size_t xw = (want_cls ? 3 : 0) + (want_res ? 6 * R : 0) + 2 * S;
    std::atomic<long long> next(0), fresh(0);
    std::atomic<int> stopped(0), counts_out(0);
    FirstError fe;
    /* dev aid (FREESASA_AMD_TRAJ_PROFILE): where the lanes' host time goes - read, waiting for the device, write, flush */
    const bool prof = getenv("FREESASA_AMD_TRAJ_PROFILE") != nullptr;
    std::atomic<long long> t_read(0), t_dev(0), t_write(0), t_flush(0);
    auto now_ns = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (long long)ts.tv_sec * 1000000000LL + ts.tv_nsec; };
    auto lane = [&](int id) noexcept {
      try {
        DeviceNodeScope node(devices[id % n_devices]); /* the lane and its page-locked staging on the device's NUMA node */
        PoolLease lease(devices[id % n_devices]); /* lanes 0 .. n_devices-1 open one device each, the next n_devices the second lane of each, ... */
        freesasa_gpu_ctx *c = lease.c;
        if (!c) { fe.set("could not create a GPU context"); return; }
        bool radii_up = false, topo_up = false;
        sasa::TrajArgs ta;
        for (;;) {
            const long long k = next.fetch_add(1);
            if (k >= n_shards || fe.failed.load()) break;
            if (io.list && io.list->done(k)) continue;
            if (max_new > 0 && fresh.fetch_add(1) >= max_new) { stopped = 1; break; }
            const long long f0 = k * frames_per_batch;
            const int nf = (int)(n_frames - f0 < frames_per_batch ? n_frames - f0 : frames_per_batch);
            const size_t na = n * (size_t)nf;
            const size_t in_bytes = esz * fa * (size_t)nf;
            int rc = -1;
            do {
                if (hipSetDevice(c->device) != hipSuccess) { ctx_fail(c, "hipSetDevice failed"); break; }
                if (ensure(c, c->h_xyz, 24 * n * FB) || ensure(c, c->h_radii, 8 * n) || ensure(c, c->h_sasa, 8 * n * FB) ||
                    ensure(c, c->h_totals, 8 * FB) || ((widen_bytes || io.out_f32) && ensure(c, c->h_counts, widen_bytes + (io.out_f32 ? 4 * n * FB : 0))) ||
                    (gather && ensure(c, c->g_xyz, esz * fa * FB)) || (xw && ensure(c, c->h_gtot, 8 * xw * FB)))
                    break;
                if (!radii_up) { /* once per lane: the radii of the system */
                    if (hipMemcpyAsync(c->h_radii.p, radii, 8 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) { ctx_fail(c, "radii upload failed"); break; }
                    radii_up = true;
                }
                if (topo && !topo_up) { /* ... and its topology */
                    if (topo_upload(c, *topo, ta)) break;
                    topo_up = true;
                }
                const void *src;
                long long tp0 = prof ? now_ns() : 0;
                if (io.mem_in && in_pinned) {
                    src = io.mem_in + 3 * fa * (size_t)f0;
                } else {
                    if (ensure_pinned(c, &c->stage_in, &c->stage_in_cap, in_bytes)) break;
                    if (io.mem_in) memcpy(c->stage_in, io.mem_in + 3 * fa * (size_t)f0, in_bytes);
                    else if (!pread_all(io.fd_in, c->stage_in, in_bytes, io.in_header + (long long)esz * (long long)fa * f0)) {
                        ctx_fail(c, "could not read frames %lld..%lld of the frame file", f0, f0 + nf - 1);
                        break;
                    }
                    src = c->stage_in;
                }
                if (prof) { const long long t = now_ns(); t_read += t - tp0; tp0 = t; }
                if (gather) { /* full frames up as they were read; one kernel drops the solvent and widens fp32 */
                    if (hipMemcpyAsync(c->g_xyz.p, src, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { ctx_fail(c, "host-to-device copy failed"); break; }
                    ta.n_frames = nf;
                    if (kl_traj_gather(ta, c->g_xyz.p, io.in_f32 != 0, (double *)c->h_xyz.p, c->stream) != hipSuccess) { ctx_fail(c, "gather launch failed"); break; }
                } else if (io.in_f32) {
                    if (hipMemcpyAsync(c->h_counts.p, src, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { ctx_fail(c, "host-to-device copy failed"); break; }
                    if (kl_widen_f32((const float *)c->h_counts.p, (double *)c->h_xyz.p, (long long)(3 * na), c->stream) != hipSuccess) { ctx_fail(c, "widening launch failed"); break; }
                } else if (hipMemcpyAsync(c->h_xyz.p, src, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
                    ctx_fail(c, "host-to-device copy failed");
                    break;
                }
                c->shared_radii = true;
                const int rb = run_batch(c, alg == 0, (double *)c->h_xyz.p, (double *)c->h_radii.p, offs.data(), nf, probe, resolution,
                                         alg == 1 ? tp.data() : nullptr, (double *)c->h_sasa.p, nullptr, (double *)c->h_totals.p);
                c->shared_radii = false;
                if (rb) break;
                double *dst_tot = io.totals_mem ? io.totals_mem + f0 : nullptr, *dst_sasa = io.sasa_mem ? io.sasa_mem + n * (size_t)f0 : nullptr;
                const bool staged = !(io.totals_mem && out_pinned);
                const size_t eb = io.out_f32 ? 4 : 8; /* bytes per per-atom area in the result file */
                if (staged) {
                    if (ensure_pinned(c, &c->stage_out, &c->stage_out_cap, 8 * (size_t)nf + (want_sasa ? 8 * na : 0))) break;
                    dst_tot = (double *)c->stage_out;
                    dst_sasa = want_sasa ? (double *)c->stage_out + nf : nullptr;
                }
                const void *d_areas = c->h_sasa.p;
                if (want_sasa && io.out_f32) { /* (file output only) narrowed on the device: half the bytes over PCIe and into the file */
                    if (ensure(c, c->h_counts, 4 * n * FB + widen_bytes)) break;
                    float *d32 = (float *)((char *)c->h_counts.p + widen_bytes);
                    if (kl_narrow_f64((const double *)c->h_sasa.p, d32, (long long)na, c->stream) != hipSuccess) { ctx_fail(c, "narrowing launch failed"); break; }
                    d_areas = d32;
                }
                bool ok = hipMemcpyAsync(dst_tot, c->h_totals.p, 8 * (size_t)nf, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
                if (ok && want_sasa) ok = hipMemcpyAsync(dst_sasa, d_areas, eb * na, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
                /* the topology's per-frame sums, behind the tile kernels on this stream; cut to this shard's nf frames they lie
                   one behind the other in c->h_gtot - classes | residues | selection areas | selected atoms - and come back
                   in ONE copy, in front of the shard's one synchronisation */
                double *x_out = nullptr;
                const size_t o_res = want_cls ? 3 * (size_t)nf : 0, o_sel = o_res + (want_res ? 6 * R * (size_t)nf : 0), o_cnt = o_sel + S * (size_t)nf;
                if (ok && xw) {
                    if (ensure_pinned(c, &c->res_stage, &c->res_stage_cap, 8 * xw * (size_t)nf)) break;
                    x_out = (double *)c->res_stage;
                    double *d_x = (double *)c->h_gtot.p;
                    ta.n_frames = nf; ta.sasa = (const double *)c->h_sasa.p;
                    ta.cls_out = d_x; ta.res_out = d_x + o_res; ta.sel_out = d_x + o_sel; ta.sel_count = (long long *)(d_x + o_cnt);
                    if ((want_res && kl_traj_residues(ta, c->stream) != hipSuccess) || (want_cls && kl_traj_class(ta, c->stream) != hipSuccess) ||
                        (want_sel && kl_traj_sel(ta, c->stream) != hipSuccess)) {
                        ctx_fail(c, "launch of the per-frame sums failed"); break;
                    }
                    ok = hipMemcpyAsync(x_out, d_x, 8 * (o_cnt + S), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
                }
                if (!ok) { ctx_fail(c, "device-to-host copy failed"); break; }
                if (hipStreamSynchronize(c->stream) != hipSuccess) { ctx_fail(c, "stream synchronize failed"); break; }
                if (prof) { const long long t = now_ns(); t_dev += t - tp0; tp0 = t; }
                const long long sasa_off = (long long)eb * (long long)n * f0;
                if (staged) {
                    if (io.totals_mem) memcpy(io.totals_mem + f0, dst_tot, 8 * (size_t)nf);
                    if (io.sasa_mem) memcpy(io.sasa_mem + n * (size_t)f0, dst_sasa, 8 * na);
                    if (io.fd_totals >= 0 && !pwrite_all(io.fd_totals, dst_tot, 8 * (size_t)nf, 8 * f0)) { ctx_fail(c, "could not write the totals file"); break; }
                    if (io.fd_sasa >= 0 && !pwrite_all(io.fd_sasa, dst_sasa, eb * na, sasa_off)) { ctx_fail(c, "could not write the per-atom file"); break; }
                }
                if (xw) {
                    if (io.cls_mem) memcpy(io.cls_mem + 3 * (size_t)f0, x_out, 8 * 3 * (size_t)nf);
                    if (io.res_mem) memcpy(io.res_mem + 6 * R * (size_t)f0, x_out + o_res, 8 * 6 * R * (size_t)nf);
                    if (io.sel_mem) memcpy(io.sel_mem + S * (size_t)f0, x_out + o_sel, 8 * S * (size_t)nf);
                    if (io.sel_atoms && S && !counts_out.exchange(1)) memcpy(io.sel_atoms, x_out + o_cnt, 8 * S); /* (frame-independent: once) */
                    if (io.fd_cls >= 0 && !pwrite_all(io.fd_cls, x_out, 8 * 3 * (size_t)nf, 8 * 3 * f0)) { ctx_fail(c, "could not write the class-sums file"); break; }
                    if (io.fd_res >= 0 && !pwrite_all(io.fd_res, x_out + o_res, 8 * 6 * R * (size_t)nf, 8 * 6 * (long long)R * f0)) { ctx_fail(c, "could not write the residues file"); break; }
                    if (io.fd_sel >= 0 && !pwrite_all(io.fd_sel, x_out + o_sel, 8 * S * (size_t)nf, 8 * (long long)S * f0)) { ctx_fail(c, "could not write the selections file"); break; }
                }
                if (prof) { const long long t = now_ns(); t_write += t - tp0; tp0 = t; }
                if (io.list) { /* results first, then the record: a shard is listed only when its numbers are on disk */
                    const bool flushed = (io.fd_totals < 0 || fdatasync(io.fd_totals) == 0) && (io.fd_sasa < 0 || fdatasync(io.fd_sasa) == 0) &&
                                         (io.fd_cls < 0 || fdatasync(io.fd_cls) == 0) && (io.fd_res < 0 || fdatasync(io.fd_res) == 0) &&
                                         (io.fd_sel < 0 || fdatasync(io.fd_sel) == 0);
                    if (!flushed) {
                        ctx_fail(c, "could not flush the result files: the shard is not listed as done"); break;
                    }
                    if (io.list->append(k, f0, nf)) { ctx_fail(c, "could not append to the done-list"); break; }
                }
                if (prof) t_flush += now_ns() - tp0;
                rc = 0;
            } while (0);
            if (rc) {
                c->shared_radii = false;
                (void)hipStreamSynchronize(c->stream);
                fe.set(c->err[0] ? c->err : "trajectory shard failed");
                break;
            }
        }
      } catch (...) {
        fe.set_exception();
      }
    };
    {
        ThreadGroup tg;
        for (int k = 1; k < n_lanes; ++k)
            if (!tg.spawn(lane, k)) { fe.set("could not start a worker thread"); break; }
        if (!fe.failed.load()) lane(0);
    }
    if (prof) fprintf(stderr, "trajectory lanes %d: per lane, ms: read %.1f  device (copies + kernels) %.1f  write %.1f  flush + done-list %.1f\n", n_lanes,
                      1e-6 * t_read.load() / n_lanes, 1e-6 * t_dev.load() / n_lanes, 1e-6 * t_write.load() / n_lanes, 1e-6 * t_flush.load() / n_lanes);
    if (fe.failed.load()) return set_err(err_out, err_len, fe.text);
    return stopped.load() ? 1 : 0;
    });
}

} /* namespace */

/* ------------------------------------------------------------------ entry points */

extern "C" int freesasa_gpu_sweep_cache_devices(const char *cache_path, int alg, double probe, int resolution, long long batch_atoms,
                                                double *totals_out, double *class_sums_out, long long *atoms_out, int *status_out, int n_out,
                                                const int *devices, int n_devices, int lanes_per_device, char *err_out, int err_len)
{
    return sweep_cache_impl(cache_path, alg, probe, resolution, batch_atoms, totals_out, class_sums_out, atoms_out, status_out, n_out,
                            devices, n_devices, lanes_per_device, err_out, err_len);
}

/* ------------------------------------------------------------------ entry points: trajectories */

static int trajectory_mem(const double *xyz_frames, const double *radii, int n_atoms, int n_frames, int alg, double probe, int resolution,
                          int frames_per_batch, double *totals_out, double *sasa_out, const int *devices, int n_devices, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz_frames || !radii || !totals_out) return set_err(err_out, err_len, "null argument");
    if (n_atoms <= 0 || n_frames <= 0) return set_err(err_out, err_len, "n_atoms and n_frames must be > 0");
    if (alg != 0 && alg != 1) return set_err(err_out, err_len, "unknown algorithm");
    if (resolution <= 0) return set_err(err_out, err_len, "resolution must be > 0");
    if (check_devices(devices, n_devices, err_out, err_len)) return -1;
    if (frames_per_batch <= 0) frames_per_batch = (int)(1250000 / n_atoms) + 1;
    if (frames_per_batch > n_frames) frames_per_batch = n_frames;
    if ((long long)frames_per_batch * n_atoms > (1LL << 30)) return set_err(err_out, err_len, "batch too large");
    return guarded(err_out, err_len, [&]() -> int {
        TrajIO io;
        io.mem_in = xyz_frames; io.totals_mem = totals_out; io.sasa_mem = sasa_out;
        return traj_run(io, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, 0, 0, devices, n_devices, err_out, err_len) < 0 ? -1 : 0;
    });
}

extern "C" int freesasa_gpu_trajectory(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                                       int alg, double probe, int resolution, int frames_per_batch,
                                       double *totals_out, double *sasa_out, int device, char *err_out, int err_len)
{
    return trajectory_mem(xyz_frames, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, totals_out, sasa_out, &device, 1, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_devices(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                                               int alg, double probe, int resolution, int frames_per_batch,
                                               double *totals_out, double *sasa_out, const int *devices, int n_devices, char *err_out, int err_len)
{
    return trajectory_mem(xyz_frames, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, totals_out, sasa_out, devices, n_devices, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_topology(const double *xyz_frames, int n_frames, const freesasa_ingest_batch *batch, int structure,
                                                int frame_atoms, const int32_t *atom_index, const freesasa_ingest_selection *sel,
                                                int alg, double probe, int resolution, int frames_per_batch,
                                                double *totals_out, double *sasa_out, double *class_sums_out, double *residues_out,
                                                double *sel_area_out, long long *sel_atoms_out,
                                                const int *devices, int n_devices, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    return guarded(err_out, err_len, [&]() -> int {
        TrajTopo tp;
        if (topo_make(batch, structure, frame_atoms, atom_index, sel, &tp, err_out, err_len)) return -1;
        if (!xyz_frames || !totals_out) return set_err(err_out, err_len, "null argument");
        if ((sel_area_out || sel_atoms_out) && !sel) return set_err(err_out, err_len, "selection outputs need a selection set");
        if (n_frames <= 0) return set_err(err_out, err_len, "n_frames must be > 0");
        if (alg != 0 && alg != 1) return set_err(err_out, err_len, "unknown algorithm");
        if (resolution <= 0) return set_err(err_out, err_len, "resolution must be > 0");
        if (check_devices(devices, n_devices, err_out, err_len)) return -1;
        /* by the atoms that come IN: the staging of a mostly-solvent frame stays what the plain drivers' is (not measured
           whether sizing by the kept atoms, i.e. longer shards for the engine, would be faster) */
        if (frames_per_batch <= 0) frames_per_batch = (int)(1250000 / frame_atoms) + 1;
        if (frames_per_batch > n_frames) frames_per_batch = n_frames;
        if ((long long)frames_per_batch * frame_atoms > (1LL << 30)) return set_err(err_out, err_len, "batch too large");
        TrajIO io;
        io.mem_in = xyz_frames; io.totals_mem = totals_out; io.sasa_mem = sasa_out;
        io.cls_mem = class_sums_out; io.res_mem = residues_out; io.sel_mem = sel_area_out; io.sel_atoms = sel_atoms_out;
        return traj_run(io, tp.radii, tp.n, n_frames, alg, probe, resolution, frames_per_batch, 0, 0, devices, n_devices, err_out, err_len, &tp) < 0 ? -1 : 0;
    });
}

/* Frame file -> result files, resumable (include/freesasa_gpu.h has the formats).  The done-list names its run: the
 * parameters, the frame file's size and modification time and a checksum of the radii — NOT the devices: a run
 * interrupted on eight GPUs may be finished on one, with the same files byte for byte. */
/* (tp: a run with a topology - frames of tp->frame_atoms atoms, three more result files, a longer first line) */
static int trajectory_file_run(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                               int n_atoms, long long n_frames, int alg, double probe, int resolution,
                               int frames_per_batch, const char *totals_path, const char *sasa_path,
                               const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                               long long *frames_total_out, char *err_out, int err_len,
                               const TrajTopo *tp = nullptr, const char *cls_path = nullptr, const char *res_path = nullptr,
                               const char *sel_path = nullptr, long long *sel_atoms_out = nullptr)
{
    if (!frames_path || !radii || !totals_path) return set_err(err_out, err_len, "null argument");
    if (n_atoms <= 0 || header_bytes < 0) return set_err(err_out, err_len, "bad argument");
    if (alg != 0 && alg != 1) return set_err(err_out, err_len, "unknown algorithm");
    if (resolution <= 0) return set_err(err_out, err_len, "resolution must be > 0");
    if (check_devices(devices, n_devices, err_out, err_len)) return -1;
    return guarded(err_out, err_len, [&]() -> int {
    TrajIO io;
    Fd f_in, f_totals, f_sasa, f_cls, f_res, f_sel; /* (closed on every way out) */
    const long long frame_atoms = tp ? tp->frame_atoms : n_atoms;
    DoneList list;
    f_in.fd = io.fd_in = open(frames_path, O_RDONLY);
    if (io.fd_in < 0) return set_err(err_out, err_len, "cannot open the frame file");
    struct stat st;
    if (fstat(io.fd_in, &st) != 0) return set_err(err_out, err_len, "cannot stat the frame file");
    const long long frame_bytes = ((frames_f32 & 1) ? 12LL : 24LL) * frame_atoms;
    const long long in_file = ((long long)st.st_size - header_bytes) / frame_bytes;
    if (n_frames <= 0) n_frames = in_file;
    if (n_frames <= 0 || n_frames > in_file) return set_err(err_out, err_len, "the frame file holds fewer frames than asked for");
    if (frames_total_out) *frames_total_out = n_frames;
    /* (a topology: by the atoms that come IN, so that the staging of a mostly-solvent frame stays what it is without one; not
       measured whether sizing by the kept atoms, i.e. longer shards for the engine, would be faster) */
    if (frames_per_batch <= 0) frames_per_batch = (int)(1250000 / frame_atoms) + 1;
    if (frames_per_batch > n_frames) frames_per_batch = (int)n_frames;
    if ((long long)frames_per_batch * frame_atoms > (1LL << 30)) return set_err(err_out, err_len, "batch too large");
    io.in_f32 = (frames_f32 & 1) ? 1 : 0; io.in_header = header_bytes;
    io.out_f32 = (frames_f32 & 2) ? 1 : 0;
    const long long n_shards = (n_frames + frames_per_batch - 1) / frames_per_batch;
    if (done_path) {
        unsigned long long hr = 1469598103934665603ULL; /* FNV-1a over the radii */
        for (size_t q = 0; q < 8 * (size_t)n_atoms; ++q) hr = (hr ^ ((const unsigned char *)radii)[q]) * 1099511628211ULL;
        char head[500];
        int len = snprintf(head, sizeof head, "freesasa_amd trajectory done-list v2 n_atoms=%d n_frames=%lld frames_per_batch=%d alg=%d resolution=%d probe=%.17g f32=%d "
                 "header_bytes=%lld frames_size=%lld frames_mtime=%lld.%09ld radii=%016llx\n",
                 n_atoms, n_frames, frames_per_batch, alg, resolution, probe, io.in_f32 | (io.out_f32 << 1), header_bytes, (long long)st.st_size,
                 (long long)st.st_mtim.tv_sec, (long)st.st_mtim.tv_nsec, hr);
        if (tp && len > 0 && len < (int)sizeof head) { /* ... and what the topology's outputs depend on, in front of the line's end */
            unsigned long long h_res = fnv1a(tp->seg.data(), 8 * ((size_t)tp->n_res + 1));
            h_res = fnv1a(tp->bb, (size_t)tp->n, fnv1a(tp->cls, (size_t)tp->n, h_res));
            unsigned long long h_sel = 0;
            if (tp->sel) {
                int n_words = 0, flags = 0;
                const void *prog = freesasa_ingest_selection_program(tp->sel, &n_words, &flags);
                const int key[3] = {tp->n_sel, n_words, flags};
                h_sel = fnv1a(prog, sizeof(freesasa_sel_word) * (size_t)n_words, fnv1a(key, sizeof key));
            }
            len += snprintf(head + len - 1, sizeof head - (size_t)len + 1, " topology frame_atoms=%d index=%016llx residues=%016llx selection=%016llx outputs=%d\n",
                            tp->frame_atoms, tp->index ? fnv1a(tp->index, 4 * (size_t)tp->n) : 0ULL, h_res, h_sel,
                            (sasa_path ? 1 : 0) | (cls_path ? 2 : 0) | (res_path ? 4 : 0) | (sel_path ? 8 : 0)) - 1;
        }
        if (len <= 0 || len >= (int)sizeof head) return set_err(err_out, err_len, "cannot write the done-list");
        const int fpb = frames_per_batch;
        if (list.read(done_path, head, n_shards, [fpb](long long k, long long f0, long long) { return f0 == k * fpb; }) == DoneList::REFUSED)
            return set_err(err_out, err_len, tp ? "the done-list belongs to a run with other parameters, radii, topology, selections, outputs or frame file"
                                                : "the done-list belongs to a run with other parameters, radii or frame file");
    }
    const int flags = list.resumed() ? O_WRONLY | O_CREAT : O_WRONLY | O_CREAT | O_TRUNC;
    f_totals.fd = io.fd_totals = open(totals_path, flags, 0644);
    if (io.fd_totals < 0) return set_err(err_out, err_len, "cannot open the totals file");
    if (sasa_path) {
        f_sasa.fd = io.fd_sasa = open(sasa_path, flags, 0644);
        if (io.fd_sasa < 0) return set_err(err_out, err_len, "cannot open the per-atom file");
    }
    if (cls_path) {
        f_cls.fd = io.fd_cls = open(cls_path, flags, 0644);
        if (io.fd_cls < 0) return set_err(err_out, err_len, "cannot open the class-sums file");
    }
    if (res_path) {
        f_res.fd = io.fd_res = open(res_path, flags, 0644);
        if (io.fd_res < 0) return set_err(err_out, err_len, "cannot open the residues file");
    }
    if (sel_path) {
        f_sel.fd = io.fd_sel = open(sel_path, flags, 0644);
        if (io.fd_sel < 0) return set_err(err_out, err_len, "cannot open the selections file");
    }
    io.sel_atoms = sel_atoms_out;
    if (done_path) {
        const int orc = list.open();
        if (orc) return set_err(err_out, err_len, orc == -1 ? "cannot open the done-list" : "cannot write the done-list");
        io.list = &list;
    }
    return traj_run(io, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, 0, max_new_shards, devices, n_devices, err_out, err_len, tp);
    });
}

extern "C" int freesasa_gpu_trajectory_file_devices(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                                                    int n_atoms, long long n_frames, int alg, double probe, int resolution,
                                                    int frames_per_batch, const char *totals_path, const char *sasa_path,
                                                    const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                    long long *frames_total_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    return trajectory_file_run(frames_path, frames_f32, header_bytes, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch,
                               totals_path, sasa_path, done_path, max_new_shards, devices, n_devices, frames_total_out, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_file_topology(const char *frames_path, int frames_f32, long long header_bytes, long long n_frames,
                                                     const freesasa_ingest_batch *batch, int structure,
                                                     int frame_atoms, const int32_t *atom_index, const freesasa_ingest_selection *sel,
                                                     int alg, double probe, int resolution, int frames_per_batch,
                                                     const char *totals_path, const char *sasa_path, const char *class_sums_path,
                                                     const char *residues_path, const char *sel_area_path, long long *sel_atoms_out,
                                                     const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                     long long *frames_total_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    return guarded(err_out, err_len, [&]() -> int {
        TrajTopo tp; /* (outlives the run: the lanes upload from it) */
        if (topo_make(batch, structure, frame_atoms, atom_index, sel, &tp, err_out, err_len)) return -1;
        if ((sel_area_path || sel_atoms_out) && !sel) return set_err(err_out, err_len, "selection outputs need a selection set");
        return trajectory_file_run(frames_path, frames_f32, header_bytes, tp.radii, tp.n, n_frames, alg, probe, resolution, frames_per_batch,
                                   totals_path, sasa_path, done_path, max_new_shards, devices, n_devices, frames_total_out, err_out, err_len,
                                   &tp, class_sums_path, residues_path, sel_area_path, sel_atoms_out);
    });
}

extern "C" int freesasa_gpu_trajectory_file(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                                            int n_atoms, long long n_frames, int alg, double probe, int resolution,
                                            int frames_per_batch, const char *totals_path, const char *sasa_path,
                                            const char *done_path, long long max_new_shards, int device,
                                            long long *frames_total_out, char *err_out, int err_len)
{
    return freesasa_gpu_trajectory_file_devices(frames_path, frames_f32, header_bytes, radii, n_atoms, n_frames, alg, probe, resolution,
                                                frames_per_batch, totals_path, sasa_path, done_path, max_new_shards, &device, 1,
                                                frames_total_out, err_out, err_len);
}
