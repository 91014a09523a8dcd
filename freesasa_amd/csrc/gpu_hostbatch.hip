/*
 * gpu_hostbatch.hip — host-pointer batches (include/freesasa_gpu.h): the pool of contexts behind the re-entrant
 * entry points; the chunk path (BatchCall, Chunk and the chunk_* stages, engine_internal.h) and the entries on top of it:
 * one batch on one device, a batch cut over a list of devices, the pipelined form whose PCIe copies run under the kernels
 * of other chunks, and the sweep of a binary cache.  Host code; kernels in gpu_kernels.hip.
 */
#include <hip/hip_runtime.h>

#include <atomic>
#include <exception>
#include <mutex>
#include <new>
#include <sched.h>
#include <stdlib.h>
#include <system_error>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <thread>
#include <vector>

#include "engine_internal.h"

/* ------------------------------------------------------------------ host-pointer batch */

/* A small pool of contexts so that concurrent host threads (the reference library is
 * re-entrant, doc/doxy-main.md:741-756) each get their own stream and workspace. */
static std::mutex g_pool_mu;
static std::vector<freesasa_gpu_ctx *> g_pool;

freesasa_gpu_ctx *pool_get(int device)
{
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t k = 0; k < g_pool.size(); ++k)
            if (device < 0 || g_pool[k]->device == device) {
                freesasa_gpu_ctx *c = g_pool[k];
                g_pool.erase(g_pool.begin() + k);
                return c;
            }
    }
    return freesasa_gpu_ctx_create(device, nullptr);
}
void pool_put(freesasa_gpu_ctx *c) /* (called from destructors: must not throw - a context the pool cannot list is destroyed) */
{
    try {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pool.push_back(c);
    } catch (...) {
        freesasa_gpu_ctx_destroy(c);
    }
}

/* Destroy the idle contexts of the pool (their streams, workspaces and staging buffers): device memory goes back
 * to the runtime; the next host-pointer call builds what it needs again. */
extern "C" void freesasa_gpu_release_pool(void)
{
    std::vector<freesasa_gpu_ctx *> idle;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        idle.swap(g_pool);
    }
    for (freesasa_gpu_ctx *c : idle) freesasa_gpu_ctx_destroy(c);
}

int set_err(char *out, int len, const char *msg)
{
    if (out && len > 0) snprintf(out, (size_t)len, "%s", msg);
    return -1;
}

const char *exception_text(char *buf, size_t len) noexcept
{
    try { throw; }
    catch (const std::bad_alloc &) { snprintf(buf, len, "out of host memory"); }
    catch (const std::system_error &e) { snprintf(buf, len, "system error: %s", e.what()); }
    catch (const std::exception &e) { snprintf(buf, len, "internal error: %s", e.what()); }
    catch (...) { snprintf(buf, len, "internal error (unknown C++ exception)"); }
    return buf;
}

/* ------------------------------------------------------------------ the NUMA node of a device (engine_internal.h) */

static bool read_small_file(const char *path, char *buf, size_t len)
{
    FILE *f = fopen(path, "r");
    if (!f) return false;
    const size_t n = fread(buf, 1, len - 1, f);
    fclose(f);
    buf[n] = 0;
    return n > 0;
}
/* "0-63,128-191\n" -> CPU numbers; returns how many the list names (the first `cap` are stored), -1 on a malformed list */
static int parse_cpulist(const char *text, int *cpus_out, int cap)
{
    int n = 0;
    const char *p = text;
    while (*p && *p != '\n') {
        char *e;
        const long a = strtol(p, &e, 10);
        if (e == p || a < 0) return -1;
        long b = a;
        p = e;
        if (*p == '-') { b = strtol(p + 1, &e, 10); if (e == p + 1 || b < a) return -1; p = e; }
        for (long c = a; c <= b; ++c) { if (n < cap && cpus_out) cpus_out[n] = (int)c; ++n; }
        if (*p == ',') ++p;
        else if (*p && *p != '\n') return -1;
    }
    return n;
}
int node_cpus_for_pci(const char *sysfs_root, const char *pci_address, int *cpus_out, int cap)
{
    if (!sysfs_root || !pci_address) return -1;
    char path[512], buf[4096], addr[64];
    size_t k = 0;
    for (; pci_address[k] && k + 1 < sizeof addr; ++k) addr[k] = (char)(pci_address[k] >= 'A' && pci_address[k] <= 'F' ? pci_address[k] + 32 : pci_address[k]); /* sysfs names are lower case */
    addr[k] = 0;
    snprintf(path, sizeof path, "%s/bus/pci/devices/%s/numa_node", sysfs_root, addr);
    if (!read_small_file(path, buf, sizeof buf)) return -1;
    const int node = atoi(buf);
    if (node < 0) return 0; /* the platform names no node for the device */
    snprintf(path, sizeof path, "%s/devices/system/node/node%d/cpulist", sysfs_root, node);
    if (!read_small_file(path, buf, sizeof buf)) return -1;
    return parse_cpulist(buf, cpus_out, cap);
}
extern "C" int freesasa_gpu_test_node_cpus(const char *sysfs_root, const char *pci_address, int *cpus_out, int cap)
{
    return node_cpus_for_pci(sysfs_root, pci_address, cpus_out, cap);
}

DeviceNodeScope::DeviceNodeScope(int device)
{
    static_assert(sizeof(cpu_set_t) <= sizeof old_mask, "cpu_set_t");
    if (getenv("FREESASA_AMD_NO_AFFINITY")) return;
    char addr[64] = {0};
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return;
    if (hipDeviceGetPCIBusId(addr, (int)sizeof addr, device) != hipSuccess) { (void)hipGetLastError(); return; }
    int cpus[1024];
    const char *root = getenv("FREESASA_AMD_SYSFS_ROOT"); /* (tests) */
    const int n = node_cpus_for_pci(root ? root : "/sys", addr, cpus, 1024);
    if (n <= 0) return;
    cpu_set_t now, want;
    if (sched_getaffinity(0, sizeof now, &now) != 0) return;
    CPU_ZERO(&want);
    int common = 0;
    for (int k = 0; k < n && k < 1024; ++k)
        if (cpus[k] < CPU_SETSIZE && CPU_ISSET(cpus[k], &now)) { CPU_SET(cpus[k], &want); ++common; }
    if (common == 0 || common == CPU_COUNT(&now)) return; /* (nothing to narrow) */
    if (sched_setaffinity(0, sizeof want, &want) != 0) return;
    memcpy(old_mask, &now, sizeof now);
    bound = true;
}
DeviceNodeScope::~DeviceNodeScope()
{
    if (!bound) return;
    cpu_set_t old;
    memcpy(&old, old_mask, sizeof old);
    (void)sched_setaffinity(0, sizeof old, &old);
}

/* ------------------------------------------------------------------ the chunk path (engine_internal.h) */

std::vector<double> call_test_points(int alg, int resolution)
{
    std::vector<double> tp;
    if (alg != 1) return tp;
    tp.resize(3 * (size_t)(resolution > 0 ? resolution : 1));
    if (resolution > 0) freesasa_gpu_test_points(resolution, tp.data());
    return tp;
}

/* the arguments every entry has, as a call */
static BatchCall batch_call(const double *xyz, const double *radii, const int64_t *offsets, int alg, double probe, int resolution,
                            double *sasa_out, int *counts_out, double *totals_out)
{
    BatchCall b;
    b.xyz = xyz; b.radii = radii; b.offsets = offsets;
    b.alg = alg; b.probe = probe; b.resolution = resolution; b.tp = call_test_points(alg, resolution);
    b.sasa_out = sasa_out; b.counts_out = counts_out; b.totals_out = totals_out;
    return b;
}

/* structures [s0, s0 + ns) of a call as a chunk; `store` (a lane's, reused from chunk to chunk) holds its offsets */
static Chunk chunk_of(const BatchCall &b, int s0, int ns, std::vector<int64_t> &store)
{
    Chunk h;
    h.s0 = s0; h.ns = ns; h.a0 = b.offsets[s0]; h.n = (size_t)(b.offsets[s0 + ns] - h.a0);
    store.resize((size_t)ns + 1);
    for (int i = 0; i <= ns; ++i) store[(size_t)i] = b.offsets[s0 + i] - h.a0;
    h.off = store.data();
    return h;
}

/* a chunk without atoms never sees a device: its structures' totals are 0 */
static bool chunk_empty(const BatchCall &b, const Chunk &h)
{
    if (h.n) return false;
    for (int i = 0; i < h.ns && b.totals_out; ++i) b.totals_out[h.s0 + i] = 0;
    return true;
}

int chunk_size(const BatchCall &b, freesasa_gpu_ctx *c, const Chunk &h)
{
    const size_t n = h.n, aux = b.want_counts() ? 4 : b.class_sums_out ? 1 : 0, tot_bytes = 8 * b.cols() * (size_t)h.ns;
    if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
    if (ensure(c, c->h_xyz, 24 * n) || ensure(c, c->h_radii, 8 * n) || ensure(c, c->h_sasa, 8 * n) ||
        (aux && ensure(c, c->h_counts, aux * n)) || ensure(c, c->h_totals, tot_bytes))
        return -1;
    /* coordinates | radii [| the cache's classes] in, per-atom areas | counts | totals and class sums out */
    if (b.stage_in && ensure_pinned(c, &c->stage_in, &c->stage_in_cap, b.cache ? 33 * n + 64 : 32 * n)) return -1;
    if (b.stage_out && ensure_pinned(c, &c->stage_out, &c->stage_out_cap, (b.sasa_out ? 8 * n : 0) + (b.want_counts() ? 4 * n : 0) + (b.totals_out ? tot_bytes : 0)))
        return -1;
    return 0;
}

/* The chunk's inputs where the device can copy them from - the only stage that knows the source: the caller's arrays in
   place, the caller's arrays through the context's staging, or the cache file read (and verified: piece checksums) into it. */
static int chunk_fill(const BatchCall &b, freesasa_gpu_ctx *c, Chunk &h)
{
    if (!b.stage_in) { h.xyz = b.xyz + 3 * h.a0; h.radii = b.radii + h.a0; return 0; }
    double *xyz = (double *)c->stage_in, *radii = xyz + 3 * h.n;
    unsigned char *cls = b.class_sums_out ? (unsigned char *)(radii + h.n) : nullptr;
    h.xyz = xyz; h.radii = radii; h.cls = cls;
    if (b.cache) {
        const int rc = freesasa_ingest_cache_read_atoms(b.cache, h.a0, h.a0 + (int64_t)h.n, xyz, radii, cls);
        return rc ? ctx_fail(c, "the cache file failed its checksum or could not be read (freesasa_ingest code %d)", rc) : 0;
    }
    memcpy(xyz, b.xyz + 3 * h.a0, 24 * h.n);
    memcpy(radii, b.radii + h.a0, 8 * h.n);
    return 0;
}

int chunk_upload(freesasa_gpu_ctx *c, const Chunk &h)
{
    if (hipMemcpyAsync(c->h_xyz.p, h.xyz, 24 * h.n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->h_radii.p, h.radii, 8 * h.n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        (h.cls && hipMemcpyAsync(c->h_counts.p, h.cls, h.n, hipMemcpyHostToDevice, c->stream) != hipSuccess))
        return ctx_fail(c, "host-to-device copy failed");
    return 0;
}

const char *chunk_failed(const BatchCall &b, freesasa_gpu_ctx *c)
{
    (void)hipStreamSynchronize(c->stream);
    return c->err[0] ? c->err : b.fallback;
}

/* the engine on the chunk as a batch of its own; behind it the class sums of a cache sweep, beside the totals in c->h_totals */
static int chunk_compute(const BatchCall &b, freesasa_gpu_ctx *c, const Chunk &h)
{
    if (b.alg != 0 && b.alg != 1) return ctx_fail(c, "unknown algorithm %d", b.alg); /* (freesasa_gpu_calc_batch's check: the other entries refuse it before they begin) */
    double *d_sasa = (double *)c->h_sasa.p, *d_tot = b.totals_out ? (double *)c->h_totals.p : nullptr;
    if (run_batch(c, b.alg == 0, (double *)c->h_xyz.p, (double *)c->h_radii.p, h.off, h.ns, b.probe, b.resolution, b.alg == 1 ? b.tp.data() : nullptr,
                  d_sasa, b.want_counts() ? (int *)c->h_counts.p : nullptr, d_tot))
        return -1;
    if (b.class_sums_out && freesasa_gpu_class_sums_dev(c, d_sasa, (const unsigned char *)c->h_counts.p, h.off, h.ns, d_tot + h.ns)) return -1;
    return 0;
}

/* The results to the host - into the caller's arrays in place, or one behind the other into the context's staging - and
   the chunk's one synchronisation. */
static int chunk_download(const BatchCall &b, freesasa_gpu_ctx *c, Chunk &h)
{
    const size_t n = h.n, tot_bytes = 8 * b.cols() * (size_t)h.ns;
    h.sasa = b.sasa_out ? b.sasa_out + h.a0 : nullptr;
    h.counts = b.want_counts() ? b.counts_out + h.a0 : nullptr;
    h.totals = b.totals_out ? b.totals_out + h.s0 : nullptr;
    if (b.stage_out) {
        char *p = (char *)c->stage_out;
        if (h.sasa) { h.sasa = (double *)p; p += 8 * n; }
        if (h.counts) { h.counts = (int *)p; p += 4 * n; }
        if (h.totals) h.totals = (double *)p;
    }
    if ((h.sasa && hipMemcpyAsync(h.sasa, c->h_sasa.p, 8 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        (h.counts && hipMemcpyAsync(h.counts, c->h_counts.p, 4 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        (h.totals && hipMemcpyAsync(h.totals, c->h_totals.p, tot_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
        return ctx_fail(c, "device-to-host copy failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
    return 0;
}

/* ... and from the staging to the caller's arrays */
static void chunk_deliver(const BatchCall &b, const Chunk &h)
{
    if (!b.stage_out) return;
    if (h.sasa) memcpy(b.sasa_out + h.a0, h.sasa, 8 * h.n);
    if (h.counts) memcpy(b.counts_out + h.a0, h.counts, 4 * h.n);
    if (h.totals) memcpy(b.totals_out + h.s0, h.totals, 8 * (size_t)h.ns);
    if (b.class_sums_out) memcpy(b.class_sums_out + 3 * (size_t)h.s0, h.totals + h.ns, 8 * 3 * (size_t)h.ns);
}

/* the stages of one chunk on a context; -1: the caller owes chunk_failed */
static int chunk_run(const BatchCall &b, freesasa_gpu_ctx *c, Chunk &h)
{
    if (chunk_size(b, c, h) || chunk_fill(b, c, h) || chunk_upload(c, h) || chunk_compute(b, c, h) || chunk_download(b, c, h)) return -1;
    chunk_deliver(b, h);
    return 0;
}

/* A lane owns a pooled context of its device and takes the chunks [cut[k], cut[k + 1]) from the shared counter until none is
   left or a lane has failed. */
static void chunk_lane(const BatchCall &b, const std::vector<int> &cut, std::atomic<int> &next, FirstError &fe, int device) noexcept
{
  try {
    PoolLease lease(device);
    if (!lease.c) { fe.set("could not create a GPU context"); return; }
    std::vector<int64_t> off;
    for (;;) {
        const int k = next.fetch_add(1);
        if (k + 1 >= (int)cut.size() || fe.failed.load()) break;
        Chunk h = chunk_of(b, cut[k], cut[k + 1] - cut[k], off);
        if (chunk_empty(b, h)) continue;
        if (chunk_run(b, lease.c, h)) { fe.set(chunk_failed(b, lease.c)); break; }
    }
  } catch (...) { /* (the lease has left the stream idle and returned the context) */
    fe.set_exception();
  }
}

/* ------------------------------------------------------------------ one batch, one device: the batch as it is, in place */

extern "C" int freesasa_gpu_calc_batch(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                       int alg, double probe, int resolution, double *sasa_out, int *counts_out,
                                       double *totals_out, int device, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz || !radii || !offsets || !sasa_out) return set_err(err_out, err_len, "null argument");
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    return guarded(err_out, err_len, [&]() -> int {
    PoolLease lease(device); /* (returned to the pool, its stream idle, on every way out - an exception included) */
    if (!lease.c) return set_err(err_out, err_len, "could not create a GPU context");
    if (n_structs <= 0 || offsets[n_structs] <= 0) return set_err(err_out, err_len, "empty batch");
    const BatchCall b = batch_call(xyz, radii, offsets, alg, probe, resolution, sasa_out, counts_out, totals_out);
    Chunk h;
    h.ns = n_structs; h.n = (size_t)offsets[n_structs]; h.off = offsets;
    return chunk_run(b, lease.c, h) ? set_err(err_out, err_len, chunk_failed(b, lease.c)) : 0;
    });
}

/* ------------------------------------------------------------------ several GPUs, one process */

/* Independent structures shard with no exchange: the batch is cut into contiguous runs of
 * structures with about equal atom counts, one run per entry of the device list, each run one chunk on its
 * own host thread (its own pooled context, stream and workspace).
 * Contiguous runs need no gather: every device reads and writes its slice of the caller's arrays. */
/* cuts[k] = first structure of shard k (cuts[n_parts] = n_structs): where the running atom count passes
 * k/n_parts of the total; shards may be empty when there are fewer structures than parts */
extern "C" void freesasa_gpu_shard_cuts(const int64_t *offsets, int n_structs, int n_parts, int *cuts)
{
    cuts[0] = 0;
    const int64_t base = offsets[0], total = offsets[n_structs] - base;
    for (int k = 1, s = 0; k < n_parts; ++k) {
        const int64_t want = base + total * k / n_parts;
        while (s < n_structs && offsets[s] < want) ++s;
        cuts[k] = s < cuts[k - 1] ? cuts[k - 1] : s;
    }
    cuts[n_parts] = n_structs;
}

extern "C" int freesasa_gpu_calc_batch_devices(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                               int alg, double probe, int resolution, double *sasa_out, int *counts_out,
                                               double *totals_out, const int *devices, int n_devices, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz || !radii || !offsets || !sasa_out || n_structs <= 0 || !devices || n_devices <= 0)
        return set_err(err_out, err_len, "bad argument");
    const int n_dev = freesasa_gpu_device_count();
    if (n_dev <= 0) return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    for (int k = 0; k < n_devices; ++k)
        if (devices[k] < 0 || devices[k] >= n_dev) return set_err(err_out, err_len, "device index out of range");
    return guarded(err_out, err_len, [&]() -> int {
    BatchCall b = batch_call(xyz, radii, offsets, alg, probe, resolution, sasa_out, counts_out, totals_out);
    b.fallback = "a device shard failed";
    std::vector<int> cut((size_t)n_devices + 1);
    freesasa_gpu_shard_cuts(offsets, n_structs, n_devices, cut.data());
    FirstError fe;
    run_lanes(n_devices, fe, [&](int k) noexcept { /* shard k on devices[k]; a shard without atoms opens no context */
      try {
        std::vector<int64_t> off;
        Chunk h = chunk_of(b, cut[k], cut[k + 1] - cut[k], off);
        if (chunk_empty(b, h)) return;
        PoolLease lease(devices[k]);
        if (!lease.c) fe.set("could not create a GPU context");
        else if (chunk_run(b, lease.c, h)) fe.set(chunk_failed(b, lease.c));
      } catch (...) {
        fe.set_exception();
      }
    });
    return fe.failed.load() ? set_err(err_out, err_len, fe.text) : 0;
    });
}

extern "C" int freesasa_gpu_calc_batch_multi(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                             int alg, double probe, int resolution, double *sasa_out, int *counts_out,
                                             double *totals_out, unsigned device_mask, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    const int n_dev = freesasa_gpu_device_count();
    if (n_dev <= 0) return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    int devs[32], nd = 0;
    for (int d = 0; d < 32 && d < n_dev; ++d)
        if (device_mask & (1u << d)) devs[nd++] = d;
    if (nd == 0) return set_err(err_out, err_len, "device mask selects no available device");
    return freesasa_gpu_calc_batch_devices(xyz, radii, offsets, n_structs, alg, probe, resolution, sasa_out, counts_out,
                                           totals_out, devs, nd, err_out, err_len);
}

/* ------------------------------------------------------------------ host arrays in, host arrays out, pipelined */

/* One host pointer: page-locked already (hipHostMalloc / hipHostRegister, e.g. a pinned tensor)? */
bool host_pinned(const void *p)
{
    hipPointerAttribute_t at;
    if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

/* Grow a context's page-locked staging buffer (for callers whose arrays are pageable). */
int ensure_pinned(freesasa_gpu_ctx *c, void **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return 0;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (host_malloc(p, want) != hipSuccess) return ctx_fail(c, "out of page-locked host memory (%zu bytes)", want);
    *cap = want;
    return 0;
}

/* The batch is cut into chunks of whole structures (about chunk_atoms atoms each) that n_lanes host threads take
 * from a shared counter; every lane owns a pooled context (stream, workspace, staging) and runs
 *     host -> device copy,  cell sort + tile kernels,  device -> host copy
 * for its chunk while the other lanes are in a different stage: PCIe in, kernels and PCIe out of different
 * chunks overlap.  Page-locked caller arrays are copied by DMA in place; pageable ones go through the lane's
 * page-locked staging buffers (the memcpy of one lane overlaps the DMA of another). */
extern "C" int freesasa_gpu_calc_batch_pipelined(const double *xyz, const double *radii, const int64_t *offsets, int n_structs,
                                                 int alg, double probe, int resolution, double *sasa_out, int *counts_out,
                                                 double *totals_out, int device, int n_lanes, long long chunk_atoms,
                                                 char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz || !radii || !offsets || !sasa_out || n_structs <= 0) return set_err(err_out, err_len, "bad argument");
    if (alg != 0 && alg != 1) return set_err(err_out, err_len, "unknown algorithm");
    if (freesasa_gpu_device_count() <= 0)
        return set_err(err_out, err_len, "no HIP device available: libfreesasa_amd has no CPU path");
    const bool pin_in = host_pinned(xyz) && host_pinned(radii);
    const bool pin_out = host_pinned(sasa_out) && (!counts_out || host_pinned(counts_out)) && (!totals_out || host_pinned(totals_out));
    if (n_lanes <= 0) n_lanes = pin_in && pin_out ? 3 : 4; /* (measured, 1e7 atoms: 1 / 2 / 3 / 4 / 6 lanes with DMA in place 24.0 / 22.4 /
                                                              15.9 / 17.1 / 16.6 ms - one lane each in PCIe in, kernels, PCIe out;
                                                              staging through page-locked buffers also spends host memcpy time) */
    if (n_lanes > 8) n_lanes = 8;
    if (chunk_atoms <= 0) chunk_atoms = 1250000;
    return guarded(err_out, err_len, [&]() -> int {
    BatchCall b = batch_call(xyz, radii, offsets, alg, probe, resolution, sasa_out, counts_out, totals_out);
    b.stage_in = !pin_in; b.stage_out = !pin_out;
    std::vector<int> cut(1, 0);
    for (int s = 0; s < n_structs; ++s)
        if (offsets[s + 1] - offsets[cut.back()] >= chunk_atoms && s + 1 < n_structs) cut.push_back(s + 1);
    cut.push_back(n_structs);
    const int n_chunks = (int)cut.size() - 1;
    std::atomic<int> next(0);
    FirstError fe;
    run_lanes(n_lanes > n_chunks ? n_chunks : n_lanes, fe, [&](int) noexcept { chunk_lane(b, cut, next, fe, device); });
    return fe.failed.load() ? set_err(err_out, err_len, fe.text) : 0;
    });
}

/* ------------------------------------------------------------------ structure sweep: from a binary cache */

namespace {
struct Cache {
    freesasa_ingest_cache *c = nullptr;
    Cache() = default;
    Cache(const Cache &) = delete;
    Cache &operator=(const Cache &) = delete;
    ~Cache() { if (c) freesasa_ingest_cache_close(c); }
};
} /* namespace */

/* The sweep of a cache file (freesasa_ingest_save): no parsing, no classification — what is left on the host is to get
 * 33 bytes per atom (coordinates, radius, class) from the file into page-locked memory, which one thread does at
 * ~1e8 atoms/s (pread from the page cache + checksum) against 4.5e8 atoms/s of one GPU at protein density.  So every
 * device gets several lanes (threads), each with its own pooled context and page-locked staging: a lane takes the
 * next batch of structures from the shared counter, reads and verifies exactly its run of atoms
 * (freesasa_ingest_cache_read_atoms: piece checksums) into its staging buffer, copies it to the device and computes,
 * while the other lanes are in another stage: the pipelined entry's lanes over chunks whose source is the file. */
extern "C" int freesasa_gpu_sweep_cache_devices(const char *cache_path, int alg, double probe, int resolution, long long batch_atoms,
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
    const int S = freesasa_ingest_cache_n_structs(cache_h.c);
    const int64_t *offs = freesasa_ingest_cache_offsets(cache_h.c);
    const int32_t *stat = freesasa_ingest_cache_status(cache_h.c);
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
    const int n_lanes = lanes_per_device * n_devices;
    /* the cache as a call: every chunk read into the lane's staging, its totals (and class sums) through stage_out */
    BatchCall b = batch_call(nullptr, nullptr, offs, alg, probe, resolution, nullptr, nullptr, totals_out);
    b.cache = cache_h.c; b.class_sums_out = class_sums_out;
    b.stage_in = b.stage_out = true;
    b.fallback = "GPU cache sweep failed";
    std::atomic<int> next(0);
    FirstError fe;
    run_lanes(n_lanes > n_batches ? n_batches : n_lanes, fe, [&](int id) noexcept {
        DeviceNodeScope node(devices[id % n_devices]); /* the lane and its page-locked staging on the device's NUMA node */
        chunk_lane(b, cut, next, fe, devices[id % n_devices]);
    });
    return fe.failed.load() ? set_err(err_out, err_len, fe.text) : 0;
    });
}
