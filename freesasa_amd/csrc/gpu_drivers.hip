/*
 * gpu_drivers.hip — the drivers for BASELINE configs[3] and configs[4] (include/freesasa_gpu.h): the structure sweep
 * over PDB / mmCIF files (gpu_sweep.hip), the same sweep from a binary cache (gpu_hostbatch.hip: chunks of the host-batch
 * path whose source is the file) and the trajectory drivers (here, with what all three share: engine_internal.h; where
 * their frames come from: gpu_frames.hip) — each over ONE device or a LIST of devices of the node.  Host code; kernels in gpu_kernels.hip.
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
 * The lanes of every driver are started by run_lanes (engine_internal.h): lane 0 is the calling thread.
 */
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>

#include <algorithm>
#include <utility>

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
    char line[1024];
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

/* ------------------------------------------------------------------ trajectory driver */

/* Frames of ONE system (same atoms, same radii) are independent structures: a SHARD is a run of frames_per_batch
 * frames that goes through the engine as one batch.  A few host lanes PER DEVICE take shards from a shared counter; a
 * lane owns a pooled context (stream, workspace, page-locked staging) of its device and does, for its shard,
 *     read (memory or frame file) -> host-to-device -> [whatever came in made into compact fp64 frames on the device: the
 *     FRAME SOURCE's two steps (gpu_frames.hip), the only code that knows the format of the input; the arithmetic is fp64]
 *     -> cell sort + tile kernels -> device-to-host -> write (memory or files)
 * while the other lanes are in another stage.  The radii live once per device context (shared by every frame of
 * a batch).  With a done-list file every finished shard is recorded after its results are on disk; a later call
 * with the same parameters skips the recorded shards: an interrupted run resumes — on any list of devices.
 *
 * The shape is the file sweep's (gpu_sweep.hip): TrajSpec is what an entry was called with, TrajIO where the frames come
 * from and ONE TABLE of the per-frame outputs (TrajOut), TrajRun what the lanes of a run share, TrajLane a lane's context,
 * TrajShard the shard in its hands.  A shard goes through shard_size -> _read -> _upload -> _compute -> _download -> _write
 * -> _record (shard_run), each 0 or -1 with the context's message; traj_lane takes shards until none is left and on a
 * failure drains its stream and sets the run's first error.  Above them, with the entry points: TrajCall, the one description of a call
 * that every entry with a topology fills, and trajectory_call, which makes TrajTopo, TrajSpec and TrajIO of it. */

/* One per-frame OUTPUT of a run: a row of TrajIO's table.  An entry point says where it goes - the caller's array or a
   result file - and everything else that is per output (opening the files, is it wanted, its place in a shard's blocks, the
   copy or the pwrite at the frame's offset, the flush, the done-list's outputs= word) is a loop over the table. */
enum { OUT_TOTALS, OUT_SASA, OUT_ISO, OUT_MASK, OUT_CLS, OUT_RES, OUT_SEL, OUT_GRP, OUT_PAIR, OUT_PRES, OUT_VOL, N_OUT }; /* (per atom | from OUT_CLS on: the block of sums) */
/* what is constant of an output: ONE table for TrajIO, for the check of a statistics word and for the done-list's first line */
struct TrajOutDef {
    const char *name;           /* in messages: "cannot open the %s file", "could not write the %s file" */
    int bit;                    /* in the outputs= word of a done-list's first line */
    int sbit;                   /* in the statistics word (FREESASA_GPU_STATS_*); 0: the output has no run statistics */
    size_t esz;                 /* bytes per value */
    /* an output of the Shrake-Rupley test points alone (the volume, the masks): what its entries say when they have nowhere to
       put it, to Lee-Richards, to periodic images and to more test points than a cap holds (%d: the cap, the points asked for) */
    const char *nowhere, *not_lr, *not_periodic, *too_many;
};
static const TrajOutDef OUT_DEF[N_OUT] = {
    {"totals", 0, FREESASA_GPU_STATS_TOTALS, 8}, {"per-atom", 1, FREESASA_GPU_STATS_ATOMS, 8}, {"isolated", 32, FREESASA_GPU_STATS_ISOLATED, 8},
    {"masks", 128, 0, 4, "null argument: the exposure masks have nowhere to go",
     "the exposure masks are those of the Shrake-Rupley test points: Lee-Richards is not offered",
     "bit 3 and bit 4 of frames_f32 (periodic images) are not offered with the exposure masks",
     "the exposure masks are offered up to %d test points (%d asked for)"},
    {"class-sums", 2, FREESASA_GPU_STATS_CLASSES, 8}, {"residues", 4, FREESASA_GPU_STATS_RESIDUES, 8}, {"selections", 8, FREESASA_GPU_STATS_SELECTIONS, 8},
    {"groups", 16, FREESASA_GPU_STATS_GROUPS, 8}, {"interfaces", 256, FREESASA_GPU_STATS_PAIRS, 8}, {"interface-residues", 512, FREESASA_GPU_STATS_PAIR_RESIDUES, 8},
    {"volumes", 64, 0, 8, "null argument: the volumes have nowhere to go",
     "the volume is made of the Shrake-Rupley test points: Lee-Richards is not offered",
     "bit 3 and bit 4 of frames_f32 (periodic images) are not offered with the volume: among periodic images the surface is not closed within the cell",
     "the volume is offered up to %d test points (%d asked for)"}};
struct TrajOut : TrajOutDef {   /* (esz of a run: 4 where the per-atom areas are asked for as fp32) */
    void *mem = nullptr;        /* the caller's array [n_frames * per_frame] ... */
    const char *path = nullptr; /* ... or a result file, */
    Fd f;                       /* open for the length of the run */
    size_t per_frame = 0;       /* (TrajRun) values per frame, 0: not computed */
    bool stat = false;          /* (TrajRun) its run statistics are asked for: computed, whether or not it is delivered ... */
    size_t s0 = 0;              /* ... and its first column of a shard's partial */
    bool wanted() const { return mem || path; }
    size_t deliver() const { return wanted() ? per_frame : 0; } /* values per frame that go down and out (0: computed at most) */
};
struct TrajIO {
    FrameSource src; /* the frames: host memory or a frame file of any format (engine_internal.h, gpu_frames.hip) */
    /* per frame: total [1], per-atom areas [n]; runs with a topology: class sums [3], residue areas [6 R], selection areas [S];
       with chain groups: every atom's area in its isolated group [n], and isolated, complex, buried per group [3 G]; with
       interface pairs: six doubles per pair [6 K] (traj_kernels.h, traj_pair_rows) and, where asked for, four doubles per segment of a side
       that lies in one residue [4 S] (traj_pair_res) - their statistics bits are accepted by the interface-residue entries only; the volume
       entries: the frame's volume [1] (gpu_volume.hip; it has no run statistics: no bit of the statistics word); the mask entries:
       every atom's exposure mask, four uint32 words [4 n] (gpu_dots.hip; per atom, 4 bytes a value, copied as it lies; no statistics) */
    TrajOut out[N_OUT];
    TrajIO() { for (int k = 0; k < N_OUT; ++k) static_cast<TrajOutDef &>(out[k]) = OUT_DEF[k]; }
    /* run statistics (include/freesasa_gpu.h): the word; every shard's partial [4][W] at k * 4 W doubles of a host array or of
       the partials file; the merged result to the caller's array (memory form: the entry merges) or the statistics file */
    int stats = 0;
    double *parts_mem = nullptr;
    const char *stats_path = nullptr, *parts_path = nullptr;
    Fd parts_f;
    long long *sel_atoms = nullptr; /* the selections' atoms [S]: frame-independent, delivered once */
    bool out_f32() const { return out[OUT_SASA].esz == 4; } /* per-atom and isolated areas written as fp32 (narrowed on the device; an output format) */
    DoneList list;                  /* (active: a file run with a done-list) */
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
    /* chain groups (group_make): the ids, and the cut of the structure into its groups (traj_kernels.h, traj_group_cut) */
    const int32_t *group = nullptr;  /* [n], -1: in no group; NULL: a run without groups */
    int n_groups = 0, n_iso = 0;     /* G; atoms with an id >= 0 */
    std::vector<int64_t> gfirst;     /* [G + 1] */
    std::vector<int32_t> src;        /* [n_iso] */
    /* interfaces between chain groups (pair_make): the pairs, and the cut of a frame's pair structures (traj_kernels.h, traj_pair_cut) */
    const int32_t *pairs = nullptr;  /* [K, 2] g < h; NULL: a run without pairs */
    int n_pairs = 0, n_pair = 0;     /* K; atoms of a frame's pair structures: the sum over the pairs of |g| + |h| */
    std::vector<int64_t> pfirst, pside; /* [K + 1], [2 K + 1] */
    std::vector<int32_t> psrc;       /* [n_pair] */
    /* their per-residue table (pair_res_make): the segments of the sides (traj_kernels.h, traj_pair_res_cut) */
    bool pres = false;               /* the table is computed: delivered, or its statistics asked for */
    double min_buried = 0;
    int n_seg = 0;                   /* S */
    std::vector<int64_t> seg_first, seg_iso; /* [S + 1], [S] */
    std::vector<int32_t> seg_res, seg_side;  /* [S], [S] */
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

/* the argument checks of chain groups and the cut, on the host: 0 (tp->group stays NULL when no groups are asked for), or -1
   with the message.  areas / iso: is that output asked for? */
int group_make(const int32_t *group, int n_groups, bool areas, bool iso, TrajTopo *tp, char *err_out, int err_len)
{
    if (!group && !areas && !iso) return 0;
    if (!group) return set_err(err_out, err_len, "group areas and isolated areas need group ids (group is NULL)");
    if (!areas) return set_err(err_out, err_len, "group ids are given but the group areas have nowhere to go (NULL)");
    if (n_groups < 1 || n_groups > 65535) return set_err(err_out, err_len, "n_groups must be 1 .. 65535");
    tp->gfirst.resize((size_t)n_groups + 1);
    tp->src.resize((size_t)tp->n);
    int64_t bad = 0;
    const int64_t n_iso = sasa::traj_group_cut(group, tp->n, n_groups, tp->gfirst.data(), tp->src.data(), &bad);
    if (n_iso < 0) {
        char msg[160];
        snprintf(msg, sizeof msg, "atom %lld has group id %d: ids are -1 .. n_groups - 1 = %d", (long long)bad, group[bad], n_groups - 1);
        return set_err(err_out, err_len, msg);
    }
    tp->group = group; tp->n_groups = n_groups; tp->n_iso = (int)n_iso;
    return 0;
}

/* What the interface entries refuse before a device is touched or a file opened, each with its own message: 0, or -1.
   periodic: the entry is one of the two among periodic images (the only ones bits 3 / 4 of frames_f32 get through for) */
int pair_check(const int32_t *group, int n_groups, const int32_t *pairs, int n_pairs, int frames_f32, const void *out, char *err_out, int err_len,
               bool periodic = false)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!group) return set_err(err_out, err_len, "interfaces need chain groups: group ids (group is NULL)");
    if (n_pairs < 1) return set_err(err_out, err_len, "interfaces need at least one pair of groups (n_pairs < 1)");
    if (!pairs) return set_err(err_out, err_len, "null argument: the pairs");
    if (!out) return set_err(err_out, err_len, "null argument: the pair areas have nowhere to go");
    if (!periodic && (frames_f32 & (FREESASA_GPU_FRAMES_PBC | FREESASA_GPU_FRAMES_TRICLINIC)))
        return set_err(err_out, err_len, "bit 3 and bit 4 of frames_f32: interfaces among periodic images are not offered by this entry: "
                                         "freesasa_gpu_trajectory_file_interfaces_periodic and _interface_residues_periodic are the ones");
    char msg[200];
    for (int k = 0; k < n_pairs; ++k) {
        const int32_t g = pairs[2 * k], h = pairs[2 * k + 1];
        if (g < 0 || h < 0 || g >= n_groups || h >= n_groups || g >= h) {
            snprintf(msg, sizeof msg, "pair %d is (%d, %d): a pair is (g, h) with 0 <= g < h < n_groups = %d", k, g, h, n_groups);
            return set_err(err_out, err_len, msg);
        }
    }
    return guarded(err_out, err_len, [&]() -> int {
        std::vector<std::pair<int64_t, int>> key((size_t)n_pairs);
        for (int k = 0; k < n_pairs; ++k) key[(size_t)k] = {(int64_t)pairs[2 * k] * n_groups + pairs[2 * k + 1], k};
        std::sort(key.begin(), key.end());
        for (int k = 1; k < n_pairs; ++k)
            if (key[(size_t)k].first == key[(size_t)k - 1].first) {
                snprintf(msg, sizeof msg, "pairs %d and %d are the same pair (%d, %d): a pair is named at most once", key[(size_t)k - 1].second,
                         key[(size_t)k].second, pairs[2 * key[(size_t)k].second], pairs[2 * key[(size_t)k].second + 1]);
                return set_err(err_out, err_len, msg);
            }
        return 0;
    });
}
/* ... and the cut of the pair structures, behind group_make and pair_check: nothing is left to refuse */
void pair_make(const int32_t *pairs, int n_pairs, TrajTopo *tp)
{
    if (!pairs || n_pairs < 1) return;
    tp->pfirst.resize((size_t)n_pairs + 1);
    tp->pside.resize(2 * (size_t)n_pairs + 1);
    const int64_t n_pair = sasa::traj_pair_cut(pairs, n_pairs, tp->gfirst.data(), tp->src.data(), tp->pfirst.data(), tp->pside.data(), nullptr);
    tp->psrc.resize((size_t)n_pair);
    sasa::traj_pair_cut(pairs, n_pairs, tp->gfirst.data(), tp->src.data(), tp->pfirst.data(), tp->pside.data(), tp->psrc.data());
    tp->pairs = pairs; tp->n_pairs = n_pairs; tp->n_pair = (int)n_pair;
}

/* ... and, for the interface-residue entries, the segments of the sides: behind pair_make */
void pair_res_make(double min_buried, TrajTopo *tp)
{
    if (!tp->pairs) return;
    const int64_t *res_first = tp->seg.data();
    const int64_t S = sasa::traj_pair_res_cut(tp->pairs, tp->n_pairs, tp->gfirst.data(), tp->pside.data(), tp->psrc.data(), res_first, tp->n_res,
                                              nullptr, nullptr, nullptr, nullptr);
    tp->seg_first.resize((size_t)S + 1); tp->seg_iso.resize((size_t)S); tp->seg_res.resize((size_t)S); tp->seg_side.resize((size_t)S);
    sasa::traj_pair_res_cut(tp->pairs, tp->n_pairs, tp->gfirst.data(), tp->pside.data(), tp->psrc.data(), res_first, tp->n_res,
                            tp->seg_first.data(), tp->seg_res.data(), tp->seg_side.data(), tp->seg_iso.data());
    tp->pres = true; tp->min_buried = min_buried; tp->n_seg = (int)S;
}
/* The argument checks of a statistics word, on the host: 0, or -1 with a message that names the output.  tp NULL: a run without
   a topology; has_sel, has_group: was a selection set, were group ids given?  more: the bits the entry knows beyond the
   seven (the interface-residue entries: pairs, pair residues - those runs have their pairs, so nothing is left to need) */
int stats_check(int stats, const TrajTopo *tp, bool has_sel, bool has_group, char *err_out, int err_len, int more = 0)
{
    if (stats & ~(127 | more)) return set_err(err_out, err_len, "unknown bit in the statistics word");
    char msg[160];
    for (int k = 0; k < N_OUT; ++k) {
        if (!(stats & OUT_DEF[k].sbit)) continue;
        const char *needs = (k == OUT_ISO || k == OUT_GRP) && !has_group ? "chain groups" : k >= OUT_CLS && !tp ? "a topology"
                          : k == OUT_SEL && !has_sel ? "a selection set" : nullptr;
        if (!needs) continue;
        snprintf(msg, sizeof msg, "statistics of the %s output need %s", OUT_DEF[k].name, needs);
        return set_err(err_out, err_len, msg);
    }
    return 0;
}
/* W of a run's statistics word, every output's first column into first[9], in the order of the word's bits (trajstats.c: the one place that knows the layout) */
size_t stats_width(int stats, int n_atoms, const TrajTopo *tp, long long *first)
{
    const long long W = freesasa_gpu_traj_stats_width_pairs(stats, n_atoms, tp ? tp->n_res : 0, tp ? tp->n_sel : 0, tp ? tp->n_groups : 0,
                                                            tp ? tp->n_pairs : 0, tp ? tp->n_seg : 0, first);
    return W > 0 ? (size_t)W : 0;
}

/* Once per lane: the topology onto the lane's context - c->seg: residue boundaries | the one structure's offsets | index |
   classes | backbone flags [| radii | group ids | src: the constant part of `ga` [| pside | pairs | psrc: that of `xa` [| seg_first | seg_iso: that of `ra`]]]; with selections the keys, labels and program where freesasa_gpu_select_batch puts them, and
   sel_mask_atom over the topology: the mask words stay in c->parse[PBUF_SEL_BITS].  (run_batch touches none of these.)
   Fills the constant part of `ta`.  Enqueued on the context's stream, nothing waited for. */
int topo_upload(freesasa_gpu_ctx *c, const TrajTopo &tp, sasa::TrajArgs &ta, sasa::TrajGroupArgs &ga, sasa::TrajPairArgs &xa, sasa::TrajPairResArgs &ra)
{
    const size_t n = (size_t)tp.n, R = (size_t)tp.n_res;
    const size_t b_seg = 8 * (R + 3), b_idx = tp.index ? (4 * n + 7) & ~(size_t)7 : 0;
    /* chain groups, behind the flags: the structure's radii (the combined batch's are made of them on the device) | ids | src */
    const size_t b_flags = (2 * n + 7) & ~(size_t)7, b_grp = tp.group ? 8 * n + 4 * n + 4 * (size_t)tp.n_iso : 0;
    /* interface pairs, behind the groups' part at the next multiple of 8: the sides' begins | the pairs | psrc */
    const size_t K = (size_t)tp.n_pairs, b_grp8 = (b_grp + 7) & ~(size_t)7, b_pair = K ? b_grp8 - b_grp + 8 * (2 * K + 1) + 8 * K + 4 * (size_t)tp.n_pair : 0;
    /* the segments of the per-residue table, behind the pairs' part at the next multiple of 8: seg_first | seg_iso */
    const size_t NS = tp.pres ? (size_t)tp.n_seg : 0, b_end = b_grp + b_pair, b_end8 = (b_end + 7) & ~(size_t)7, b_pres = tp.pres ? b_end8 - b_end + 8 * (2 * NS + 1) : 0;
    if (ensure(c, c->seg, b_seg + b_idx + (tp.group ? b_flags : 2 * n) + b_grp + b_pair + b_pres)) return -1;
    char *base = (char *)c->seg.p;
    hipStream_t st = c->stream;
    memset(&ga, 0, sizeof ga);
    memset(&xa, 0, sizeof xa);
    memset(&ra, 0, sizeof ra);
    if (tp.pres) {
        char *r = base + b_seg + b_idx + b_flags + b_end8;
        HIP_TRY(c, hipMemcpyAsync(r, tp.seg_first.data(), 8 * (NS + 1), hipMemcpyHostToDevice, st));
        if (NS) HIP_TRY(c, hipMemcpyAsync(r + 8 * (NS + 1), tp.seg_iso.data(), 8 * NS, hipMemcpyHostToDevice, st));
        ra.n = tp.n; ra.n_iso = tp.n_iso; ra.n_pair = tp.n_pair; ra.n_seg = tp.n_seg; ra.min_buried = tp.min_buried;
        ra.seg_first = (const int64_t *)r; ra.seg_iso = ra.seg_first + NS + 1;
    }
    if (K) {
        char *x = base + b_seg + b_idx + b_flags + b_grp8;
        HIP_TRY(c, hipMemcpyAsync(x, tp.pside.data(), 8 * (2 * K + 1), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(x + 8 * (2 * K + 1), tp.pairs, 8 * K, hipMemcpyHostToDevice, st));
        if (tp.n_pair) HIP_TRY(c, hipMemcpyAsync(x + 8 * (2 * K + 1) + 8 * K, tp.psrc.data(), 4 * (size_t)tp.n_pair, hipMemcpyHostToDevice, st));
        xa.n = tp.n; xa.n_iso = tp.n_iso; xa.n_pair = tp.n_pair; xa.n_groups = tp.n_groups; xa.n_pairs = tp.n_pairs;
        xa.pside = (const int64_t *)x; xa.pairs = (const int32_t *)(x + 8 * (2 * K + 1)); xa.psrc = xa.pairs + 2 * K;
        xa.radii = (const double *)(base + b_seg + b_idx + b_flags);
    }
    if (tp.group) {
        char *g = base + b_seg + b_idx + b_flags;
        HIP_TRY(c, hipMemcpyAsync(g, tp.radii, 8 * n, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(g + 8 * n, tp.group, 4 * n, hipMemcpyHostToDevice, st));
        if (tp.n_iso) HIP_TRY(c, hipMemcpyAsync(g + 12 * n, tp.src.data(), 4 * (size_t)tp.n_iso, hipMemcpyHostToDevice, st));
        ga.n = tp.n; ga.n_iso = tp.n_iso; ga.n_groups = tp.n_groups;
        ga.radii = (const double *)g; ga.group = (const int32_t *)(g + 8 * n); ga.src = (const int32_t *)(g + 12 * n);
    }
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

/* what a trajectory entry was called with */
struct TrajSpec {
    const double *radii; int n_atoms; long long n_frames; int alg; double probe; int resolution, frames_per_batch;
    const int *devices; int n_devices;
    const TrajTopo *topo = nullptr;
    long long max_new = 0; /* (file runs) stop after this many new shards */
};

/* The checks every entry makes of its arguments, in every entry's order.  sizes_msg: the entry's wording for "no atoms or no
   frames" (NULL: it has made that check in its own terms). */
int traj_check_args(const TrajSpec &s, const char *sizes_msg, char *err_out, int err_len)
{
    if (sizes_msg && (s.n_atoms <= 0 || s.n_frames <= 0)) return set_err(err_out, err_len, sizes_msg);
    if (s.alg != 0 && s.alg != 1) return set_err(err_out, err_len, "unknown algorithm");
    if (s.resolution <= 0) return set_err(err_out, err_len, "resolution must be > 0");
    return check_devices(s.devices, s.n_devices, err_out, err_len);
}
/* ... and the size of a shard, once the number of frames is known (a file run asks the file).  The default goes by the atoms
   that come IN: with a topology the staging of a mostly-solvent frame stays what the plain drivers' is (not measured whether
   sizing by the kept atoms, i.e. longer shards for the engine, would be faster). */
int traj_shard_size(TrajSpec &s, long long frame_atoms, char *err_out, int err_len)
{
    /* (with interface pairs the engine's batch can be many times the frames - all pairs of G groups: G - 1 times the atoms in
       groups more - and the default goes by the combined atoms of a frame where those are more than come in) */
    const long long comb = s.topo && s.topo->n_pairs ? (long long)s.topo->n + s.topo->n_iso + s.topo->n_pair : 0;
    if (s.frames_per_batch <= 0) s.frames_per_batch = (int)(1250000 / (comb > frame_atoms ? comb : frame_atoms)) + 1;
    if (s.frames_per_batch > s.n_frames) s.frames_per_batch = (int)s.n_frames;
    if ((long long)s.frames_per_batch * frame_atoms > (1LL << 30)) return set_err(err_out, err_len, "batch too large");
    /* chain groups: the engine sees a shard's frames AND their isolated groups as one batch - up to twice the atoms */
    if (s.topo && s.topo->group && ((long long)s.frames_per_batch * ((long long)s.topo->n + s.topo->n_iso) > (1LL << 30) ||
                                    (long long)s.frames_per_batch * (1 + s.topo->n_groups) > (1LL << 30)))
        return set_err(err_out, err_len, "batch too large with chain groups: frames_per_batch x (atoms + atoms in groups) and frames_per_batch x (1 + groups) "
                                         "must not exceed 2^30");
    if (comb && ((long long)s.frames_per_batch * comb > (1LL << 30) || (long long)s.frames_per_batch * (1 + s.topo->n_groups + s.topo->n_pairs) > (1LL << 30)))
        return set_err(err_out, err_len, "batch too large with interface pairs: frames_per_batch x (atoms + atoms in groups + atoms in pair structures) and "
                                         "frames_per_batch x (1 + groups + pairs) must not exceed 2^30");
    return 0;
}

/* what the lanes of one run share */
struct TrajRun {
    const TrajSpec &s;
    TrajIO &io;
    const TrajTopo *const topo = s.topo;
    const size_t n = (size_t)s.n_atoms, FB = (size_t)s.frames_per_batch; /* atoms of a frame as the engine sees it, frames of a full shard */
    /* chain groups: behind a shard's frames every group of every frame as a structure of its own (traj_kernels.h) */
    const bool groups = topo && topo->group;
    /* ... and with interface pairs, behind those, every pair structure of every frame */
    const size_t G = groups ? (size_t)topo->n_groups : 0, n_iso = groups ? (size_t)topo->n_iso : 0;
    const size_t K = groups ? (size_t)topo->n_pairs : 0, n_pair = groups ? (size_t)topo->n_pair : 0, nc = n + n_iso + n_pair; /* nc: combined atoms per frame */
    const long long n_shards = (s.n_frames + s.frames_per_batch - 1) / s.frames_per_batch;
    FrameSource &src = io.src; /* (planned below: what its shards are, a topology's index, the cutoff of periodic images) */
    /* the caller's arrays are page-locked: no staging */
    const bool direct_out = io.out[OUT_TOTALS].mem && host_pinned(io.out[OUT_TOTALS].mem) && (!io.out[OUT_SASA].mem || host_pinned(io.out[OUT_SASA].mem)) &&
                            (!io.out[OUT_ISO].mem || host_pinned(io.out[OUT_ISO].mem)) && (!io.out[OUT_MASK].mem || host_pinned(io.out[OUT_MASK].mem));
    const size_t S = topo && topo->sel && (io.out[OUT_SEL].wanted() || io.sel_atoms || (io.stats & FREESASA_GPU_STATS_SELECTIONS)) ? (size_t)topo->n_sel : 0; /* selections computed */
    /* A shard's sums lie one behind the other in ONE block, cut to its nf frames: classes | residues | selection areas |
       groups | interfaces | interface residues | volumes | selected atoms.  Output k's begin at x0[k] * nf doubles (k = N_OUT: the atom counts); xw doubles per frame hold it all. */
    size_t x0[N_OUT + 1] = {0, 0, 0}, xw;
    /* does the block of sums go to the host?  (not when its outputs are computed for their statistics alone) */
    const bool sums_down = io.out[OUT_CLS].wanted() || io.out[OUT_RES].wanted() || io.out[OUT_SEL].wanted() || io.out[OUT_GRP].wanted() || io.out[OUT_PAIR].wanted() ||
                           io.out[OUT_PRES].wanted() || io.out[OUT_VOL].wanted() || io.sel_atoms;
    size_t sW = 0; /* run statistics: columns of a shard's partial; it lies behind a FULL shard's block of sums, at xw * FB doubles of c->h_gtot */
    const std::vector<double> tp = call_test_points(s.alg, s.resolution);
    /* a full shard as a batch: k n; with chain groups behind them FB n + f n_iso + gfirst[g], with interface pairs behind those
       FB (n + n_iso) + f n_pair + pfirst[k] - and the same for the run's short last shard, whose isolated structures begin earlier
       (without groups a short shard is a prefix of the full one) */
    std::vector<int64_t> offs, offs_last;
    int grp_chunks = 0, grp_chunks_last = 0; /* (interface pairs) chunks of the engine's chunk table that belong to the frames and the isolated structures */
    std::atomic<long long> next{0}, fresh{0};
    std::atomic<int> stopped{0}, counts_out{0};
    FirstError fe;
    /* A run reports the failure of its LOWEST failed shard, whichever lane got there first: shards are handed out in ascending
       order, a shard in a lane's hands is run to its end, and a lane that holds a shard BELOW the lowest failed one runs it even
       after the failure (traj_lane), so every shard below a failed one has reported by the time the lanes are joined - the message of a run does not depend on how its lanes happen to be scheduled (a file whose every frame is
       refused is refused "at frame 0"). */
    std::mutex shard_err_mu;
    std::atomic<long long> shard_err_k{-1};
    char shard_err[256] = {0};
    void shard_failed(long long k, const char *msg)
    {
        {
            std::lock_guard<std::mutex> lk(shard_err_mu);
            if (shard_err_k.load() < 0 || k < shard_err_k.load()) { snprintf(shard_err, sizeof shard_err, "%s", msg); shard_err_k = k; }
        }
        fe.set(msg);
    }
    /* dev aid (FREESASA_AMD_TRAJ_PROFILE): where the lanes' host time goes - read, waiting for the device, write, flush */
    const bool prof = getenv("FREESASA_AMD_TRAJ_PROFILE") != nullptr;
    std::atomic<long long> t_read{0}, t_dev{0}, t_write{0}, t_flush{0};

    void batch_offsets(size_t nf, std::vector<int64_t> &o) const
    {
        o.resize(nf * (1 + G + K) + 1);
        for (size_t k = 0; k <= nf; ++k) o[k] = (int64_t)(k * n);
        for (size_t f = 0; f < nf && G; ++f)
            for (size_t g = 1; g <= G; ++g) o[nf + f * G + g] = (int64_t)(nf * n + f * n_iso) + topo->gfirst[g];
        for (size_t f = 0; f < nf && K; ++f)
            for (size_t k = 1; k <= K; ++k) o[nf * (1 + G) + f * K + k] = (int64_t)(nf * (n + n_iso) + f * n_pair) + topo->pfirst[k];
    }
    /* the chunks of the first nf (1 + G) structures, as cell_sort_enqueue (gpu_engine.hip) cuts a batch's structures */
    int chunks_before_pairs(size_t nf, const std::vector<int64_t> &o) const
    {
        int64_t k = 0;
        for (size_t s = 0; s < nf * (1 + G); ++s) k += (o[s + 1] - o[s] + SASA_BOUNDS_CHUNK - 1) / SASA_BOUNDS_CHUNK;
        return (int)k;
    }
    TrajRun(const TrajSpec &s_, TrajIO &io_) : s(s_), io(io_)
    {
        batch_offsets(FB, offs);
        if (groups && (size_t)(s.n_frames % s.frames_per_batch)) batch_offsets((size_t)(s.n_frames % s.frames_per_batch), offs_last);
        if (K) grp_chunks = chunks_before_pairs(FB, offs);
        if (K && !offs_last.empty()) grp_chunks_last = chunks_before_pairs((size_t)(s.n_frames % s.frames_per_batch), offs_last);
        const size_t per[N_OUT] = {1, n, groups ? n : 0, SR_CAP_WORDS * n, topo ? (size_t)3 : 0, topo ? 6 * (size_t)topo->n_res : 0, S, 3 * G, 6 * K,
                                   K && topo->pres ? 4 * (size_t)topo->n_seg : 0, 1};
        /* (an output's place in the order of the statistics word's outputs, which is trajstats.c's and not the table's: the
           masks and the volumes have no statistics) */
        static const int scol[N_OUT] = {0, 1, 2, -1, 3, 4, 5, 6, 7, 8, -1};
        long long first[N_OUT] = {0};
        sW = stats_width(io.stats, s.n_atoms, topo, first);
        for (int k = 0; k < N_OUT; ++k) {
            /* computed: delivered, or its statistics asked for (the selections' and the groups' kernels write theirs whenever they run) */
            io.out[k].stat = (io.stats & io.out[k].sbit) != 0;
            io.out[k].s0 = io.out[k].stat && scol[k] >= 0 ? (size_t)first[scol[k]] : 0;
            io.out[k].per_frame = io.out[k].wanted() || io.out[k].stat || k == OUT_SEL || k == OUT_GRP || k == OUT_PAIR ? per[k] : 0;
            if (k >= OUT_CLS) x0[k + 1] = x0[k] + io.out[k].per_frame;
        }
        xw = x0[N_OUT] + S;
        src.plan(n, topo && topo->index, s.n_frames, s.frames_per_batch, s.radii, s.probe);
    }
};
/* a lane: its pooled context and what it has put there once */
struct TrajLane {
    freesasa_gpu_ctx *c;
    bool radii_up = false, topo_up = false;
    sasa::TrajArgs ta;
    sasa::TrajGroupArgs ga; /* (chain groups) */
    sasa::TrajPairArgs xa;  /* (interface pairs) */
    sasa::TrajPairResArgs ra; /* (... and their per-residue table) */
    int radii_nf = 0;       /* ... the shard length the combined batch's radii are laid out for */
};
/* a shard in its lane's hands: frames [f0, f0 + nf) */
struct TrajShard {
    long long k, f0; int nf;
    size_t na, in_bytes; /* its atoms as the engine sees them, the bytes that come in */
    const void *src;     /* its frames on the host (page-locked) */
    const void *d_areas, *d_iso; /* its per-atom (and isolated) areas on the device, as they go out */
    char *host[N_OUT];   /* where every output's values are after the download (page-locked) */
    char *stat_host;     /* ... and the shard's partial statistics [4][W] */
};
long long now_ns() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (long long)ts.tv_sec * 1000000000LL + ts.tv_nsec; }

/* the device buffers, for a FULL shard (a short last one fits); once per lane the radii of the system and its topology */
int shard_size(TrajRun &T, TrajLane &L)
{
    freesasa_gpu_ctx *c = L.c;
    const size_t n = T.n, FB = T.FB, nc = T.nc, iso = T.io.out[OUT_ISO].per_frame;
    const size_t narrow_bytes = T.io.out_f32() ? 4 * (n + iso) * FB : 0; /* (the isolated areas' behind the per-atom areas') */
    if (hipSetDevice(c->device) != hipSuccess) return ctx_fail(c, "hipSetDevice failed");
    /* (with chain groups nc = n + n_iso [+ n_pair] atoms and 1 + G [+ K] structures per frame, and radii per atom: the isolated structures are not n atoms long) */
    if (ensure(c, c->h_xyz, 24 * nc * FB) || ensure(c, c->h_radii, T.groups ? 8 * nc * FB : 8 * n) || ensure(c, c->h_sasa, 8 * nc * FB) ||
        ensure(c, c->h_totals, 8 * (1 + T.G + T.K) * FB) ||
        (T.K && (ensure(c, c->if_sides, 8 * (2 * T.K * FB + 1)) || ensure(c, c->if_inpair, 16 * T.K * FB))) ||
        (T.src.widen_bytes() + narrow_bytes && ensure(c, c->h_counts, T.src.widen_bytes() + narrow_bytes)) ||
        (T.src.xyz_bytes() && ensure(c, c->g_xyz, T.src.xyz_bytes())) || (T.xw + T.sW && ensure(c, c->h_gtot, 8 * (T.xw * FB + 4 * T.sW))) ||
        (T.groups && (ensure(c, c->g_gath, 8 * nc * FB) || ensure(c, c->g_tot2, 8 * (1 + T.G) * FB))) || (iso && ensure(c, c->h_iso, 8 * n * FB)) ||
        (T.io.out[OUT_MASK].per_frame && ensure(c, c->dt_masks, 4 * SR_CAP_WORDS * n * FB)))
        return -1;
    if (!T.groups && !L.radii_up && hipMemcpyAsync(c->h_radii.p, T.s.radii, 8 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ctx_fail(c, "radii upload failed");
    if (T.topo && !L.topo_up && topo_upload(c, *T.topo, L.ta, L.ga, L.xa, L.ra)) return -1;
    L.radii_up = L.topo_up = true;
    return 0;
}

/* the shard's frames in page-locked memory, checked: the frame source's (gpu_frames.hip) */
int shard_read(TrajRun &T, freesasa_gpu_ctx *c, TrajShard &h)
{
    return T.src.read(c, h.f0, h.nf, h.in_bytes, &h.src);
}

/* ... to the device, into the compact fp64 frames the engine reads (c->h_xyz): the frame source's copy and kernels; with chain
   groups, behind them, every group's atoms of every frame */
int shard_upload(TrajRun &T, TrajLane &L, const TrajShard &h)
{
    freesasa_gpu_ctx *c = L.c;
    L.ta.n_frames = h.nf;
    if (T.src.to_frames(c, L.ta, h.f0, h.nf, h.in_bytes, h.src)) return -1;
    if (!T.groups) return 0;
    /* chain groups: behind the compact frames, whoever made them, every group's atoms of every frame; the radii of the
       combined batch once per shard length (the isolated structures begin at nf n) */
    sasa::TrajGroupArgs &ga = L.ga;
    ga.n_frames = h.nf; ga.xyz = (double *)c->h_xyz.p; ga.cradii = (double *)c->h_radii.p;
    const bool radii_due = L.radii_nf != h.nf;
    if (radii_due && kl_traj_group_radii(ga, c->stream) != hipSuccess) return ctx_fail(c, "launch of the groups' radii failed");
    L.radii_nf = h.nf;
    if (kl_traj_group_gather(ga, c->stream) != hipSuccess) return ctx_fail(c, "launch of the groups' gather failed");
    if (!T.K) return 0;
    /* interface pairs: behind the isolated structures every pair structure of every frame; their radii and the sides'
       boundaries once per shard length too */
    sasa::TrajPairArgs &xa = L.xa;
    xa.n_frames = h.nf; xa.xyz = ga.xyz; xa.cradii = ga.cradii; xa.side_off = (int64_t *)c->if_sides.p;
    if (radii_due && kl_traj_pair_radii(xa, c->stream) != hipSuccess) return ctx_fail(c, "launch of the pairs' radii failed");
    if (kl_traj_pair_gather(xa, c->stream) != hipSuccess) return ctx_fail(c, "launch of the pairs' gather failed");
    return 0;
}

/* the engine on the shard as a batch of nf structures that share their radii; behind it on the stream what is made of the
   areas on the device: fp32 per-atom areas, the topology's per-frame sums into their block (c->h_gtot, TrajRun::x0) */
int shard_compute(TrajRun &T, TrajLane &L, TrajShard &h)
{
    freesasa_gpu_ctx *c = L.c;
    const TrajOut *out = T.io.out;
    const size_t nf = (size_t)h.nf;
    /* (chain groups: ONE batch of the nf frames and their nf G isolated groups, radii per atom) */
    c->shared_radii = !T.groups;
    /* periodic images: the compact frames expanded by their cells, the engine on the expanded shard (radii per atom, offsets
       that vary), the real atoms' areas and totals collected where the plain path puts them (gpu_periodic.hip) */
    const bool pbc = T.src.pbc;
    const double *cells = pbc ? T.src.host_cells(c, h.in_bytes) : nullptr, *d_cells = pbc ? T.src.dev_cells(c, h.in_bytes) : nullptr;
    /* chain groups among periodic images: the combined batch - the frames, behind them every group of every frame - through the
       same stage, every group in its frame's cell; behind the engine the fused finish has put areas, isolated areas, gathered
       complex areas and both sets of totals where the groups' path below has them after its own finish (gpu_periodic.hip) */
    const bool gpbc = pbc && T.groups;
    sasa::GpbcArgs gx;
    memset(&gx, 0, sizeof gx);
    if (gpbc) {
        /* (interface pairs among periodic images: behind the groups the K pair structures of every frame, each in its frame's cell
           among its own images; the finish gives their atoms' areas to the compact combined areas alone, pbc_kernels.h) */
        gx.n_cplx = h.nf; gx.n_comb = (int)(nf * (1 + T.G + T.K)); gx.g_fixed = (int)T.G;
        gx.k_fixed = (int)T.K; gx.pair_first = (int64_t)(nf * (T.n + T.n_iso));
        gx.n_atoms = (int64_t)(nf * T.n); gx.n_all = (int64_t)(nf * T.nc);
        gx.src = L.ga.src; gx.n_fixed = (int)T.n; gx.n_iso_fixed = (int)T.n_iso; gx.key = L.ga.group;
        gx.carea = (double *)c->h_sasa.p; gx.cgath = (double *)c->g_gath.p; gx.iso = out[OUT_ISO].per_frame ? (double *)c->h_iso.p : nullptr;
    }
    const int rb = gpbc ? groups_periodic_stage(c, T.src.tri, T.s.alg, (double *)c->h_xyz.p, (double *)c->h_radii.p, (nf != T.FB ? T.offs_last : T.offs).data(),
                                                cells, d_cells, gx,
                                                T.s.probe, T.s.resolution, T.s.alg == 1 ? T.tp.data() : nullptr, (double *)c->h_totals.p,
                                                (double *)c->g_tot2.p, nullptr)
                 : pbc ? (T.src.tri ? periodic_resident_tri : periodic_resident)(c, T.s.alg, (double *)c->h_xyz.p, (double *)c->h_radii.p, T.offs.data(), h.nf, (int)T.n,
                                             cells, d_cells,
                                             T.s.probe, T.s.resolution, T.s.alg == 1 ? T.tp.data() : nullptr, (double *)c->h_sasa.p,
                                             (double *)c->h_totals.p, nullptr)
                 : out[OUT_VOL].per_frame /* (the volume entries: the batch with its exposed-point vectors kept, the frames' volumes into the block of sums) */
                     ? volume_resident(c, (double *)c->h_xyz.p, (double *)c->h_radii.p, T.offs.data(), h.nf, T.s.probe, T.s.resolution, T.tp.data(),
                                       (double *)c->h_sasa.p, nullptr, nullptr, nullptr, (double *)c->h_totals.p, (double *)c->h_gtot.p + T.x0[OUT_VOL] * nf)
                 : out[OUT_MASK].per_frame /* (the mask entries: the batch with its exposure masks kept, where they go down from) */
                     ? masks_resident(c, (double *)c->h_xyz.p, (double *)c->h_radii.p, T.offs.data(), h.nf, T.s.probe, T.s.resolution, T.tp.data(),
                                      (double *)c->h_sasa.p, nullptr, (double *)c->h_totals.p, (unsigned *)c->dt_masks.p)
                 : run_batch(c, T.s.alg == 0, (double *)c->h_xyz.p, (double *)c->h_radii.p, (T.groups && nf != T.FB ? T.offs_last : T.offs).data(),
                             (int)(nf * (1 + T.G + T.K)), T.s.probe, T.s.resolution, T.s.alg == 1 ? T.tp.data() : nullptr, (double *)c->h_sasa.p, nullptr,
                             (double *)c->h_totals.p);
    c->shared_radii = false;
    if (rb) return -1;
    h.d_iso = nullptr;
    if (T.groups) {
        /* grp_finish_atom per frame, each group's complex area reduced like its isolated total (the combined batch's chunk
           tables, which run_batch left on the device: gpu_groups.hip does the same), the three columns into the block of sums */
        sasa::TrajGroupArgs &ga = L.ga; /* (n_frames: shard_upload's) */
        ga.csasa = (const double *)c->h_sasa.p; ga.cgath = (double *)c->g_gath.p; ga.iso = out[OUT_ISO].per_frame ? (double *)c->h_iso.p : nullptr;
        ga.ctot = (const double *)c->h_totals.p; ga.ctot2 = (const double *)c->g_tot2.p; ga.out = (double *)c->h_gtot.p + T.x0[OUT_GRP] * nf;
        sasa::PipeArgs pa;
        memset(&pa, 0, sizeof pa);
        /* (interface pairs: the pair structures' chunks lie behind the others in the tables and are kept out - cgath has no
           values there, and the groups' sums are what they are without pairs) */
        pa.n_structs = (int)(nf * (1 + T.G)); pa.n_atoms = (int)(nf * (T.n + T.n_iso)); pa.offsets = (const int64_t *)c->offsets.p;
        pa.n_chunks = !T.K ? c->n_chunks : nf != T.FB ? T.grp_chunks_last : T.grp_chunks; pa.chunk_struct = (const int *)c->chunk_struct.p; pa.chunk_begin = (const int64_t *)c->chunk_begin.p;
        pa.chunk_len = (const int *)c->chunk_len.p; pa.struct_chunk0 = (const int *)c->struct_chunk0.p;
        /* (among periodic images the finish and both reductions are done: run_batch's chunk tables describe the expanded batch) */
        if ((!gpbc && (kl_traj_group_finish(ga, c->stream) != hipSuccess ||
                       kl_totals(pa, pa.n_chunks, pa.n_structs, (const double *)c->g_gath.p, (double *)c->bpart.p, (double *)c->g_tot2.p, c->stream) != hipSuccess)) ||
            kl_traj_group_totals(ga, c->stream) != hipSuccess)
            return ctx_fail(c, "launch of the groups' sums failed");
        h.d_iso = ga.iso;
        if (T.K) {
            /* every side's area in its pair structure, summed as k_totals sums a segment whatever its length (a row does not
               depend on what else is in the shard), then the six columns per (frame, pair) */
            sasa::TrajPairArgs &xa = L.xa; /* (n_frames, side_off: shard_upload's) */
            xa.ctot = (const double *)c->h_totals.p; xa.inpair = (const double *)c->if_inpair.p; xa.out = (double *)c->h_gtot.p + T.x0[OUT_PAIR] * nf;
            if (kl_segment_sums((const double *)c->h_sasa.p, xa.side_off, (int)(2 * T.K * nf), false, (double *)c->if_inpair.p, c->stream) != hipSuccess ||
                kl_traj_pair_rows(xa, c->stream) != hipSuccess)
                return ctx_fail(c, "launch of the pairs' sums failed");
            /* ... and, where the table is delivered or its statistics are asked for, the four columns per (frame, segment) from the
               engine's areas of the isolated part and of the pair part */
            if (out[OUT_PRES].per_frame) {
                sasa::TrajPairResArgs &ra = L.ra;
                ra.n_frames = h.nf; ra.csasa = (const double *)c->h_sasa.p; ra.out = (double *)c->h_gtot.p + T.x0[OUT_PRES] * nf;
                if (kl_traj_pair_res(ra, c->stream) != hipSuccess) return ctx_fail(c, "launch of the pairs' per-residue sums failed");
            }
        }
    }
    /* (file output only) per-atom areas narrowed on the device: half the bytes over PCIe and into the file */
    const bool narrow = out[OUT_SASA].deliver() && T.io.out_f32();
    h.d_areas = narrow ? (char *)c->h_counts.p + T.src.widen_bytes() : c->h_sasa.p;
    if (narrow && kl_narrow_f64((const double *)c->h_sasa.p, (float *)h.d_areas, (long long)h.na, c->stream) != hipSuccess) return ctx_fail(c, "narrowing launch failed");
    if (h.d_iso && out[OUT_ISO].deliver() && T.io.out_f32()) {
        h.d_iso = (char *)c->h_counts.p + T.src.widen_bytes() + 4 * T.n * T.FB;
        if (kl_narrow_f64((const double *)c->h_iso.p, (float *)h.d_iso, (long long)h.na, c->stream) != hipSuccess) return ctx_fail(c, "narrowing launch failed");
    }
    double *const d_x = (double *)c->h_gtot.p;
    if (T.xw) {
        sasa::TrajArgs &ta = L.ta; /* (n_frames: shard_upload's) */
        ta.sasa = (const double *)c->h_sasa.p;
        ta.cls_out = d_x; ta.res_out = d_x + T.x0[OUT_RES] * nf; ta.sel_out = d_x + T.x0[OUT_SEL] * nf; ta.sel_count = (long long *)(d_x + T.x0[N_OUT] * nf);
        if ((out[OUT_RES].per_frame && kl_traj_residues(ta, c->stream) != hipSuccess) || (out[OUT_CLS].per_frame && kl_traj_class(ta, c->stream) != hipSuccess) ||
            (T.S && kl_traj_sel(ta, c->stream) != hipSuccess))
            return ctx_fail(c, "launch of the per-frame sums failed");
    }
    if (!T.sW) return 0;
    /* run statistics: the shard's partial of every output asked for, in ONE launch behind the kernels that wrote the blocks -
       the fp64 areas and sums where they lie, never the narrowed copies */
    sasa::TrajStatsArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.n_frames = h.nf; sa.W = (int64_t)T.sW; sa.out = d_x + T.xw * T.FB;
    for (int k = 0; k < N_OUT; ++k) {
        if (!out[k].stat) continue;
        const double *src = k == OUT_TOTALS ? (const double *)c->h_totals.p : k == OUT_SASA ? (const double *)c->h_sasa.p
                          : k == OUT_ISO ? (const double *)c->h_iso.p : d_x + T.x0[k] * nf;
        sa.seg[sa.n_seg++] = {src, (int64_t)out[k].per_frame, (int64_t)out[k].s0};
    }
    if (kl_traj_stats(sa, c->stream) != hipSuccess) return ctx_fail(c, "launch of the statistics failed");
    return 0;
}

/* The results to the host: totals and per-atom (and isolated) areas straight into the caller's arrays when those are page-locked, else into
   c->stage_out one behind the other; the block of sums in ONE copy into c->res_stage; then the shard's one synchronisation. */
int shard_download(TrajRun &T, freesasa_gpu_ctx *c, TrajShard &h)
{
    const TrajOut *out = T.io.out;
    const size_t nf = (size_t)h.nf, sasa_bytes = out[OUT_SASA].esz * out[OUT_SASA].deliver() * nf, iso_bytes = out[OUT_ISO].esz * out[OUT_ISO].deliver() * nf,
                 mask_bytes = out[OUT_MASK].esz * out[OUT_MASK].deliver() * nf;
    if (!T.direct_out && ensure_pinned(c, &c->stage_out, &c->stage_out_cap, 8 * nf + 8 * (out[OUT_SASA].deliver() + out[OUT_ISO].deliver()) * nf + mask_bytes)) return -1;
    if (T.xw + T.sW && ensure_pinned(c, &c->res_stage, &c->res_stage_cap, 8 * (T.xw * nf + 4 * T.sW))) return -1;
    for (int k = 0; k < N_OUT; ++k)
        h.host[k] = k >= OUT_CLS ? (char *)c->res_stage + 8 * T.x0[k] * nf
                  : T.direct_out ? (char *)out[k].mem + out[k].esz * out[k].deliver() * (size_t)h.f0 /* (memory forms: 8 bytes a value but the masks' 4) */
                  : (char *)c->stage_out + (k == OUT_SASA ? 8 * nf : k == OUT_ISO ? 8 * nf + 8 * out[OUT_SASA].deliver() * nf
                                            : k == OUT_MASK ? 8 * nf + 8 * (out[OUT_SASA].deliver() + out[OUT_ISO].deliver()) * nf : 0);
    h.stat_host = (char *)c->res_stage + 8 * T.xw * nf; /* (behind the shard's block of sums) */
    if (hipMemcpyAsync(h.host[OUT_TOTALS], c->h_totals.p, 8 * nf, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        (sasa_bytes && hipMemcpyAsync(h.host[OUT_SASA], h.d_areas, sasa_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        (iso_bytes && hipMemcpyAsync(h.host[OUT_ISO], h.d_iso, iso_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        (mask_bytes && hipMemcpyAsync(h.host[OUT_MASK], c->dt_masks.p, mask_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        (T.xw && T.sums_down && hipMemcpyAsync(c->res_stage, c->h_gtot.p, 8 * (T.x0[N_OUT] * nf + T.S), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        (T.sW && hipMemcpyAsync(h.stat_host, (const double *)c->h_gtot.p + T.xw * T.FB, 32 * T.sW, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
        return ctx_fail(c, "device-to-host copy failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, "stream synchronize failed");
    return 0;
}

/* every output to its place, at the frame's offset: the caller's array (unless it came straight there) or the result file */
int shard_write(TrajRun &T, freesasa_gpu_ctx *c, const TrajShard &h)
{
    for (int k = 0; k < N_OUT; ++k) {
        const TrajOut &o = T.io.out[k];
        const size_t bytes = o.esz * o.deliver() * (size_t)h.nf;
        const long long at = (long long)(o.esz * o.deliver()) * h.f0;
        if (o.mem && bytes && (char *)o.mem + at != h.host[k]) memcpy((char *)o.mem + at, h.host[k], bytes);
        if (o.f.fd >= 0 && bytes && !pwrite_all(o.f.fd, h.host[k], bytes, at)) return ctx_fail(c, "could not write the %s file", o.name);
    }
    if (T.sW) { /* the shard's partial statistics at its place of the partials */
        if (T.io.parts_mem) memcpy(T.io.parts_mem + 4 * T.sW * (size_t)h.k, h.stat_host, 32 * T.sW);
        if (T.io.parts_f.fd >= 0 && !pwrite_all(T.io.parts_f.fd, h.stat_host, 32 * T.sW, (long long)(32 * T.sW) * h.k)) return ctx_fail(c, "could not write the partials file");
    }
    if (T.io.sel_atoms && T.S && !T.counts_out.exchange(1)) memcpy(T.io.sel_atoms, (char *)c->res_stage + 8 * T.x0[N_OUT] * (size_t)h.nf, 8 * T.S); /* (frame-independent: once) */
    return 0;
}

/* results first, then the record: a shard is listed only when its numbers are on disk */
int shard_record(TrajRun &T, freesasa_gpu_ctx *c, const TrajShard &h)
{
    if (!T.io.list.active()) return 0;
    for (const TrajOut &o : T.io.out)
        if (o.f.fd >= 0 && fdatasync(o.f.fd) != 0) return ctx_fail(c, "could not flush the result files: the shard is not listed as done");
    if (T.io.parts_f.fd >= 0 && fdatasync(T.io.parts_f.fd) != 0) return ctx_fail(c, "could not flush the partials file: the shard is not listed as done");
    return T.io.list.append(h.k, h.f0, h.nf) ? ctx_fail(c, "could not append to the done-list") : 0;
}

/* the stages of one shard, the profile's clocks between them */
int shard_run(TrajRun &T, TrajLane &L, TrajShard &h)
{
    if (shard_size(T, L)) return -1;
    long long t0 = T.prof ? now_ns() : 0;
    auto lap = [&](std::atomic<long long> &sum) { if (T.prof) { const long long t = now_ns(); sum += t - t0; t0 = t; } };
    if (shard_read(T, L.c, h)) return -1;
    lap(T.t_read);
    if (shard_upload(T, L, h) || shard_compute(T, L, h) || shard_download(T, L.c, h)) return -1;
    lap(T.t_dev);
    if (shard_write(T, L.c, h)) return -1;
    lap(T.t_write);
    if (shard_record(T, L.c, h)) return -1;
    lap(T.t_flush);
    return 0;
}

/* A lane owns a pooled context of its device: lanes 0 .. n_devices-1 open one device each, the next n_devices the second
   lane of each, ...  It takes shards from the shared counter until none is left, max_new were begun or a lane has failed. */
void traj_lane(TrajRun &T, int id) noexcept
{
  try {
    const TrajSpec &s = T.s;
    DeviceNodeScope node(s.devices[id % s.n_devices]); /* the lane and its page-locked staging on the device's NUMA node */
    PoolLease lease(s.devices[id % s.n_devices]);
    TrajLane L = {lease.c};
    if (!L.c) { T.fe.set("could not create a GPU context"); return; }
    for (;;) {
        TrajShard h;
        h.k = T.next.fetch_add(1);
        if (h.k >= T.n_shards || (T.fe.failed.load() && h.k >= T.shard_err_k.load())) break; /* (shard_err_k -1: a failure that is no shard's ends every lane) */
        if (T.io.list.done(h.k)) continue;
        if (s.max_new > 0 && T.fresh.fetch_add(1) >= s.max_new) { T.stopped = 1; break; }
        h.f0 = h.k * s.frames_per_batch;
        h.nf = (int)(s.n_frames - h.f0 < s.frames_per_batch ? s.n_frames - h.f0 : s.frames_per_batch);
        h.na = T.n * (size_t)h.nf; h.in_bytes = T.src.shard_bytes(h.f0, h.nf);
        if (shard_run(T, L, h)) {
            (void)hipStreamSynchronize(L.c->stream); /* nothing of the shard may still run when the lane lets go */
            T.shard_failed(h.k, L.c->err[0] ? L.c->err : "trajectory shard failed");
            break;
        }
    }
  } catch (...) {
    T.fe.set_exception();
  }
}

/* returns 0: all shards done, 1: stopped after max_new shards (more left), -1: error */
int traj_run(TrajIO &io, const TrajSpec &s, char *err_out, int err_len)
{
    return guarded(err_out, err_len, [&]() -> int {
    TrajRun T(s, io);
    /* three lanes keep one device's PCIe in, kernels and PCIe out busy (measured, round 2; round 6, from and to files on the
       MI355X box, 600 frames x 100 000 atoms: 3 lanes 2.97e8, 6 lanes 3.10e8 atom-frames/s with two of the three contexts
       cold - the kernel trace shows the tile kernels of the lanes back to back, 2.9 ms per shard of 1.2e6 atoms: the
       driver runs at the rate of the kernels); with several devices the lanes also share the granted
       CPUs (a lane reads, copies and writes on the host): two each at least */
    int per_device = process_cpus() / s.n_devices >= 3 ? 3 : 2;
    if (const char *e = getenv("FREESASA_AMD_TRAJ_LANES")) per_device = atoi(e) > 0 ? atoi(e) : per_device; /* tuning aid */
    int n_lanes = (per_device > 8 ? 8 : per_device) * s.n_devices;
    if (n_lanes > T.n_shards) n_lanes = (int)T.n_shards;
    run_lanes(n_lanes, T.fe, [&T](int id) noexcept { traj_lane(T, id); });
    if (T.prof) fprintf(stderr, "trajectory lanes %d: per lane, ms: read %.1f  device (copies + kernels) %.1f  write %.1f  flush + done-list %.1f\n", n_lanes,
                        1e-6 * T.t_read.load() / n_lanes, 1e-6 * T.t_dev.load() / n_lanes, 1e-6 * T.t_write.load() / n_lanes, 1e-6 * T.t_flush.load() / n_lanes);
    if (T.fe.failed.load()) return set_err(err_out, err_len, T.shard_err_k.load() >= 0 ? T.shard_err : T.fe.text);
    return T.stopped.load() ? 1 : 0;
    });
}

/* run statistics: the frames of every shard of a run, for the merge (trajstats.c) */
std::vector<long long> shard_frames(const TrajSpec &s)
{
    const long long n_shards = (s.n_frames + s.frames_per_batch - 1) / s.frames_per_batch;
    std::vector<long long> nf((size_t)n_shards, s.frames_per_batch);
    nf.back() = s.n_frames - (n_shards - 1) * s.frames_per_batch;
    return nf;
}

/* a memory-form run with its statistics: the partials into the caller's array or one of the call's own, merged when the run is through */
int traj_run_mem(TrajIO &io, const TrajSpec &s, double *stats_out, double *partials_out, char *err_out, int err_len)
{
    if (!io.stats) return traj_run(io, s, err_out, err_len) < 0 ? -1 : 0;
    std::vector<double> own;
    const size_t W = stats_width(io.stats, s.n_atoms, s.topo, nullptr);
    const std::vector<long long> nf = shard_frames(s);
    if (W && !partials_out) own.resize(4 * W * nf.size());
    io.parts_mem = W ? (partials_out ? partials_out : own.data()) : nullptr;
    if (traj_run(io, s, err_out, err_len) < 0) return -1;
    if (W && freesasa_gpu_traj_stats_merge(io.parts_mem, nf.data(), (long long)nf.size(), (long long)W, stats_out, nullptr))
        return set_err(err_out, err_len, "could not merge the partial statistics");
    return 0;
}

} /* namespace */

/* ------------------------------------------------------------------ entry points: trajectories */

extern "C" int freesasa_gpu_trajectory_stats(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                                             int alg, double probe, int resolution, int frames_per_batch,
                                             double *totals_out, double *sasa_out, const int *devices, int n_devices,
                                             int stats, double *stats_out, double *partials_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (!xyz_frames || !radii || !totals_out) return set_err(err_out, err_len, "null argument");
    if (stats_check(stats, nullptr, false, false, err_out, err_len)) return -1;
    if (stats && !stats_out) return set_err(err_out, err_len, "statistics are asked for but have nowhere to go (stats_out is NULL)");
    TrajSpec s = {radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, devices, n_devices};
    if (traj_check_args(s, "n_atoms and n_frames must be > 0", err_out, err_len) || traj_shard_size(s, n_atoms, err_out, err_len)) return -1;
    return guarded(err_out, err_len, [&]() -> int {
        TrajIO io;
        io.src.open_memory(xyz_frames, (size_t)n_atoms); io.out[OUT_TOTALS].mem = totals_out; io.out[OUT_SASA].mem = sasa_out; io.stats = stats;
        return traj_run_mem(io, s, stats_out, partials_out, err_out, err_len);
    });
}

extern "C" int freesasa_gpu_trajectory_devices(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                                               int alg, double probe, int resolution, int frames_per_batch,
                                               double *totals_out, double *sasa_out, const int *devices, int n_devices, char *err_out, int err_len)
{
    return freesasa_gpu_trajectory_stats(xyz_frames, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, totals_out, sasa_out, devices, n_devices,
                                         0, nullptr, nullptr, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory(const double *xyz_frames, const double *radii, int n_atoms, int n_frames,
                                       int alg, double probe, int resolution, int frames_per_batch,
                                       double *totals_out, double *sasa_out, int device, char *err_out, int err_len)
{
    return freesasa_gpu_trajectory_devices(xyz_frames, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, totals_out, sasa_out, &device, 1, err_out, err_len);
}

/* the segments of such a run, on the host: the run's own checks and cuts, no device */
extern "C" int freesasa_gpu_trajectory_interface_segments(const freesasa_ingest_batch *batch, int structure, const int32_t *group, int n_groups,
                                                          const int32_t *pairs, int n_pairs, long long seg_capacity, long long *n_segments_out,
                                                          long long *seg_offsets_out, int32_t *seg_res_out, int32_t *seg_atoms_out, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (pair_check(group, n_groups, pairs, n_pairs, 0, "", err_out, err_len)) return -1;
    if (!n_segments_out) return set_err(err_out, err_len, "null argument: n_segments_out");
    return guarded(err_out, err_len, [&]() -> int {
        TrajTopo tp;
        /* (the frames are the structure's atoms: topo_make has nothing to say about an index) */
        const bool sized = batch && structure >= 0 && structure < batch->n_structs && batch->offsets;
        const long long n = sized ? (long long)(batch->offsets[structure + 1] - batch->offsets[structure]) : 0;
        if (topo_make(batch, structure, n > 0 && n <= (1LL << 30) ? (int)n : 0, nullptr, nullptr, &tp, err_out, err_len)) return -1;
        if (group_make(group, n_groups, true, false, &tp, err_out, err_len)) return -1;
        pair_make(pairs, n_pairs, &tp);
        pair_res_make(0.0, &tp);
        *n_segments_out = tp.n_seg;
        if (seg_capacity < tp.n_seg) {
            char msg[160];
            snprintf(msg, sizeof msg, "seg_capacity %lld is too small: the run has %d segments", seg_capacity, tp.n_seg);
            return set_err(err_out, err_len, msg);
        }
        if (seg_offsets_out) {
            for (int j = 0; j <= 2 * n_pairs; ++j) seg_offsets_out[j] = 0;
            for (int s = 0; s < tp.n_seg; ++s) ++seg_offsets_out[tp.seg_side[(size_t)s] + 1];
            for (int j = 0; j < 2 * n_pairs; ++j) seg_offsets_out[j + 1] += seg_offsets_out[j];
        }
        for (int s = 0; s < tp.n_seg; ++s) {
            if (seg_res_out) seg_res_out[s] = tp.seg_res[(size_t)s];
            if (seg_atoms_out) seg_atoms_out[s] = (int32_t)(tp.seg_first[(size_t)s + 1] - tp.seg_first[(size_t)s]);
        }
        return 0;
    });
}

/* The first line of a trajectory file run's done-list names the run: the parameters, the frame file's size and modification
   time and a checksum of the radii - NOT the devices: a run interrupted on eight GPUs may be finished on one, with the same
   files byte for byte.  With a topology, in front of the line's end, what its outputs depend on: digests of the index, of
   residue boundaries + classes + backbone flags, of the selection set's program, and which result files the run writes; with
   chain groups, behind that, a digest of the group count and the ids; with interface pairs, behind that, a digest of the pair count
   and the pairs; with run statistics, last, the word as stats=.  The f32= word:
   the frame source's bits (the input's format, periodic images) and bit 1, fp32 per-atom output; header_bytes=: the byte of frame 0. */
static int traj_done_head(char *head, size_t cap, const TrajSpec &s, const TrajIO &io, const struct stat &st)
{
    int len = snprintf(head, cap, "freesasa_amd trajectory done-list v2 n_atoms=%d n_frames=%lld frames_per_batch=%d alg=%d resolution=%d probe=%.17g f32=%d "
                       "header_bytes=%lld frames_size=%lld frames_mtime=%lld.%09ld radii=%016llx\n",
                       s.n_atoms, s.n_frames, s.frames_per_batch, s.alg, s.resolution, s.probe, io.src.head_f32() | (io.out_f32() << 1), io.src.head_bytes(), (long long)st.st_size,
                       (long long)st.st_mtim.tv_sec, (long)st.st_mtim.tv_nsec, fnv1a(s.radii, 8 * (size_t)s.n_atoms));
    const TrajTopo *tp = s.topo;
    if (tp && len > 0 && len < (int)cap) {
        unsigned long long h_res = fnv1a(tp->seg.data(), 8 * ((size_t)tp->n_res + 1));
        h_res = fnv1a(tp->bb, (size_t)tp->n, fnv1a(tp->cls, (size_t)tp->n, h_res));
        unsigned long long h_sel = 0;
        if (tp->sel) {
            int n_words = 0, flags = 0;
            const void *prog = freesasa_ingest_selection_program(tp->sel, &n_words, &flags);
            const int key[3] = {tp->n_sel, n_words, flags};
            h_sel = fnv1a(prog, sizeof(freesasa_sel_word) * (size_t)n_words, fnv1a(key, sizeof key));
        }
        int outputs = 0;
        for (int k = 0; k < N_OUT; ++k) outputs |= io.out[k].path ? OUT_DEF[k].bit : 0;
        len += snprintf(head + len - 1, cap - (size_t)len + 1, " topology frame_atoms=%d index=%016llx residues=%016llx selection=%016llx outputs=%d\n",
                        tp->frame_atoms, tp->index ? fnv1a(tp->index, 4 * (size_t)tp->n) : 0ULL, h_res, h_sel, outputs) - 1;
        /* ... and with chain groups a digest of G and the ids (a run without groups keeps the line it had) */
        if (tp->group && len > 0 && len < (int)cap)
            len += snprintf(head + len - 1, cap - (size_t)len + 1, " groups=%016llx\n", fnv1a(tp->group, 4 * (size_t)tp->n, fnv1a(&tp->n_groups, sizeof tp->n_groups))) - 1;
        /* ... and with interface pairs a digest of K and the pairs (a run without pairs keeps the line it had) */
        if (tp->pairs && len > 0 && len < (int)cap)
            len += snprintf(head + len - 1, cap - (size_t)len + 1, " pairs=%016llx\n", fnv1a(tp->pairs, 8 * (size_t)tp->n_pairs, fnv1a(&tp->n_pairs, sizeof tp->n_pairs))) - 1;
        /* ... and where their per-residue table is computed the threshold of its fourth column, bit for bit (the plain interfaces
           run keeps the line it had) */
        if (tp->pres && len > 0 && len < (int)cap) {
            unsigned long long u;
            memcpy(&u, &tp->min_buried, 8);
            len += snprintf(head + len - 1, cap - (size_t)len + 1, " minburied=%016llx\n", u) - 1;
        }
    }
    /* ... and with run statistics the word (a run without statistics keeps the line it had) */
    if (io.stats && len > 0 && len < (int)cap) len += snprintf(head + len - 1, cap - (size_t)len + 1, " stats=%d\n", io.stats) - 1;
    return len > 0 && len < (int)cap ? 0 : -1;
}

/* Frame file (of any format the frame source opens: include/freesasa_gpu.h has them) -> result files, resumable.  The caller has
   put the result files' paths into io.out[]; s.topo: a run with a topology - frames of its frame_atoms atoms, a longer first line of the done-list. */
static int trajectory_file_run(const char *frames_path, int frames_f32, long long header_bytes, TrajSpec s, TrajIO &io,
                               const char *done_path, long long *frames_total_out, char *err_out, int err_len)
{
    if (!frames_path || !s.radii || !io.out[OUT_TOTALS].path) return set_err(err_out, err_len, "null argument");
    if (s.n_atoms <= 0 || header_bytes < 0) return set_err(err_out, err_len, "bad argument");
    if (io.stats && (!io.stats_path || !io.parts_path)) return set_err(err_out, err_len, "statistics need a statistics path and a partials path");
    const long long frame_atoms = s.topo ? s.topo->frame_atoms : s.n_atoms;
    if (io.src.open(frames_path, frames_f32, header_bytes, frame_atoms, err_out, err_len)) return -1;
    if (traj_check_args(s, nullptr, err_out, err_len)) return -1;
    return guarded(err_out, err_len, [&]() -> int {
    io.src.file.fd = open(frames_path, O_RDONLY);
    if (io.src.file.fd < 0) return set_err(err_out, err_len, "cannot open the frame file");
    struct stat st;
    if (fstat(io.src.file.fd, &st) != 0) return set_err(err_out, err_len, "cannot stat the frame file");
    io.out[OUT_SASA].esz = io.out[OUT_ISO].esz = (frames_f32 & 2) ? 4 : 8;
    const long long in_file = io.src.frames_in_file((long long)st.st_size);
    if (s.n_frames <= 0) s.n_frames = in_file;
    if (s.n_frames <= 0 || s.n_frames > in_file) return set_err(err_out, err_len, "the frame file holds fewer frames than asked for");
    if (frames_total_out) *frames_total_out = s.n_frames;
    if (traj_shard_size(s, frame_atoms, err_out, err_len)) return -1;
    if (done_path) {
        char head[640];
        if (traj_done_head(head, sizeof head, s, io, st)) return set_err(err_out, err_len, "cannot write the done-list");
        const int fpb = s.frames_per_batch;
        if (io.list.read(done_path, head, (s.n_frames + fpb - 1) / fpb, [fpb](long long k, long long f0, long long) { return f0 == k * fpb; }) == DoneList::REFUSED)
            return set_err(err_out, err_len, s.topo && s.topo->pres ? "the done-list belongs to a run with other parameters, radii, topology, selections, chain groups, interface pairs, "
                                                                      "min_buried, outputs, statistics or frame file"
                                           : io.stats ? "the done-list belongs to a run with other parameters, radii, topology, outputs, statistics or frame file"
                                           : s.topo && s.topo->pairs ? "the done-list belongs to a run with other parameters, radii, topology, selections, chain groups, interface pairs, outputs or frame file"
                                           : s.topo && s.topo->group ? "the done-list belongs to a run with other parameters, radii, topology, selections, chain groups, outputs or frame file"
                                           : s.topo ? "the done-list belongs to a run with other parameters, radii, topology, selections, outputs or frame file"
                                                    : "the done-list belongs to a run with other parameters, radii or frame file");
    }
    for (TrajOut &o : io.out) { /* (a resumed run's files keep what the listed shards wrote) */
        if (!o.path) continue;
        o.f.fd = open(o.path, io.list.resumed() ? O_WRONLY | O_CREAT : O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (o.f.fd < 0) return set_err(err_out, err_len, ("cannot open the " + std::string(o.name) + " file").c_str());
    }
    if (io.stats) { /* the partials like a result file; a statistics file of an earlier run does not outlive the start of a fresh one */
        if (!io.list.resumed()) (void)unlink(io.stats_path);
        io.parts_f.fd = open(io.parts_path, io.list.resumed() ? O_RDWR | O_CREAT : O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (io.parts_f.fd < 0) return set_err(err_out, err_len, "cannot open the partials file");
    }
    if (done_path) {
        const int orc = io.list.open();
        if (orc) return set_err(err_out, err_len, orc == -1 ? "cannot open the done-list" : "cannot write the done-list");
    }
    const int rc = traj_run(io, s, err_out, err_len);
    if (rc != 0 || !io.stats) return rc;
    /* every shard is done - by this call or by earlier ones: the partials back from their file, merged, the statistics file */
    const size_t W = stats_width(io.stats, s.n_atoms, s.topo, nullptr);
    const std::vector<long long> nf = shard_frames(s);
    /* (mapped, not read: the partials of a long run are tens of megabytes that the merge walks once) */
    const size_t part_bytes = 32 * W * nf.size();
    struct stat pst;
    if (fstat(io.parts_f.fd, &pst) != 0 || (size_t)pst.st_size < part_bytes) return set_err(err_out, err_len, "the partials file is shorter than its shards: it is not this run's");
    std::vector<double> merged(4 * W);
    void *parts = mmap(nullptr, part_bytes, PROT_READ, MAP_SHARED | MAP_POPULATE, io.parts_f.fd, 0);
    if (parts == MAP_FAILED) return set_err(err_out, err_len, "could not read the partials file");
    const int mrc = freesasa_gpu_traj_stats_merge((const double *)parts, nf.data(), (long long)nf.size(), (long long)W, merged.data(), nullptr);
    (void)munmap(parts, part_bytes);
    if (mrc) return set_err(err_out, err_len, "could not merge the partial statistics");
    Fd out;
    out.fd = open(io.stats_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (out.fd < 0) return set_err(err_out, err_len, "cannot open the statistics file");
    /* (flushed like the result files: in a run with a done-list) */
    if (!pwrite_all(out.fd, merged.data(), 8 * merged.size(), 0) || (io.list.active() && fdatasync(out.fd) != 0)) return set_err(err_out, err_len, "could not write the statistics file");
    return 0;
    });
}

extern "C" int freesasa_gpu_trajectory_file_stats(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                                                  int n_atoms, long long n_frames, int alg, double probe, int resolution,
                                                  int frames_per_batch, const char *totals_path, const char *sasa_path,
                                                  const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                  long long *frames_total_out,
                                                  int stats, const char *stats_path, const char *partials_path, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (stats_check(stats, nullptr, false, false, err_out, err_len)) return -1;
    TrajSpec s = {radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch, devices, n_devices, nullptr, max_new_shards};
    return guarded(err_out, err_len, [&]() -> int {
        TrajIO io;
        io.out[OUT_TOTALS].path = totals_path; io.out[OUT_SASA].path = sasa_path;
        io.stats = stats; io.stats_path = stats_path; io.parts_path = partials_path;
        return trajectory_file_run(frames_path, frames_f32, header_bytes, s, io, done_path, frames_total_out, err_out, err_len);
    });
}

extern "C" int freesasa_gpu_trajectory_file_devices(const char *frames_path, int frames_f32, long long header_bytes, const double *radii,
                                                    int n_atoms, long long n_frames, int alg, double probe, int resolution,
                                                    int frames_per_batch, const char *totals_path, const char *sasa_path,
                                                    const char *done_path, long long max_new_shards, const int *devices, int n_devices,
                                                    long long *frames_total_out, char *err_out, int err_len)
{
    return freesasa_gpu_trajectory_file_stats(frames_path, frames_f32, header_bytes, radii, n_atoms, n_frames, alg, probe, resolution, frames_per_batch,
                                              totals_path, sasa_path, done_path, max_new_shards, devices, n_devices, frames_total_out,
                                              0, nullptr, nullptr, err_out, err_len);
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

/* ------------------------------------------------------------------ the entries with a topology */

namespace {

/* ONE call of any entry with a topology: what it was called with, under the names of include/freesasa_gpu.h, and the entry's own
   rules.  A plain aggregate - nothing in it allocates -, so an entry fills it before anything is guarded; trajectory_call does
   the rest.  The memory form fills xyz and mem[], the file form the frame file's four and path[]. */
struct TrajCall {
    bool file = false;              /* the file form: frames from a frame file, results to files, resumable */
    const double *xyz = nullptr;
    const char *frames_path = nullptr; int frames_f32 = 0; long long header_bytes = 0;
    long long n_frames = 0;
    const freesasa_ingest_batch *batch = nullptr; int structure = 0, frame_atoms = 0; const int32_t *atom_index = nullptr;
    const freesasa_ingest_selection *sel = nullptr;
    const int32_t *group = nullptr; int n_groups = 0;
    const int32_t *pairs = nullptr; int n_pairs = 0; double min_buried = 0;
    int alg = 0; double probe = 0; int resolution = 0, frames_per_batch = 0;
    void *mem[N_OUT] = {};          /* where every output goes, by the table's OUT_*: the caller's array ... */
    const char *path[N_OUT] = {};   /* ... or a result file; NULL in both: not delivered */
    long long *sel_atoms_out = nullptr;
    const char *done_path = nullptr; long long max_new_shards = 0;
    const int *devices = nullptr; int n_devices = 0; long long *frames_total_out = nullptr;
    int stats = 0; double *stats_out = nullptr, *partials_out = nullptr; const char *stats_path = nullptr, *partials_path = nullptr;
    /* the entry's own rules */
    int more_stats = 0;             /* the statistics bits it knows beyond the seven */
    /* bits 3 and 4 of frames_f32, periodic images, with chain groups: fine (an entry without groups; the interface entries and
       the outputs of the test points refuse the bits in words of their own), refused where the call has to do with groups,
       refused whatever the call, or bit 3 REQUIRED: the entry is one among periodic images, and without the bit the run is its
       `sibling`'s - an entry's name, for the message */
    enum { IMAGES_FINE, IMAGES_NOT_WITH_GROUPS, IMAGES_NEVER, IMAGES_REQUIRED } images = IMAGES_FINE;
    const char *sibling = nullptr;
    int sr_only = -1;               /* OUT_VOL, OUT_MASK: the entry of that output of the Shrake-Rupley test points */
    enum { NO_PAIRS, PAIRS, PAIR_RESIDUES } kind = NO_PAIRS; /* an interface entry, an interface-residue entry */
    const void *to(int k) const { return mem[k] ? mem[k] : path[k]; }
};

/* what an entry refuses by its own rules, before everything else: 0, or -1 with the message */
int traj_call_rules(const TrajCall &a, char *err_out, int err_len)
{
    char msg[200];
    const bool periodic = a.images == TrajCall::IMAGES_REQUIRED;
    if (periodic && !(a.frames_f32 & FREESASA_GPU_FRAMES_PBC)) {
        snprintf(msg, sizeof msg, "%s among periodic images need bit 3 of frames_f32 (periodic images): without it the run is %s's",
                 a.kind ? "interfaces" : "chain groups", a.sibling);
        return set_err(err_out, err_len, msg);
    }
    if (periodic && !a.kind && !a.group)
        return set_err(err_out, err_len, "chain groups among periodic images need group ids (group is NULL): without them the run is freesasa_gpu_trajectory_file_topology's");
    /* (group NULL and neither group output: the run is freesasa_gpu_trajectory_file_topology's, periodic images included) */
    const bool with_groups = a.group || a.to(OUT_GRP) || a.to(OUT_ISO) || (a.stats & (FREESASA_GPU_STATS_GROUPS | FREESASA_GPU_STATS_ISOLATED));
    if (a.images == TrajCall::IMAGES_NEVER || (a.images == TrajCall::IMAGES_NOT_WITH_GROUPS && with_groups)) {
        if (a.frames_f32 & FREESASA_GPU_FRAMES_TRICLINIC)
            return set_err(err_out, err_len, "bit 4 of frames_f32 (triclinic cells) is not offered with chain groups by this entry: freesasa_gpu_trajectory_file_groups_periodic is the one");
        if (a.frames_f32 & FREESASA_GPU_FRAMES_PBC)
            return set_err(err_out, err_len, "bit 3 of frames_f32 (periodic images) is not offered with chain groups by this entry: freesasa_gpu_trajectory_file_groups_periodic is the one");
    }
    if (a.kind) {
        /* (the interface-residue entries may have no place for the pair areas: they ask below for either output) */
        if (pair_check(a.group, a.n_groups, a.pairs, a.n_pairs, a.frames_f32, a.kind == TrajCall::PAIR_RESIDUES ? "" : a.to(OUT_PAIR), err_out, err_len, periodic)) return -1;
        if (a.kind == TrajCall::PAIRS) return 0;
        if (!a.to(OUT_PAIR) && !a.to(OUT_PRES) && !(a.stats & (FREESASA_GPU_STATS_PAIRS | FREESASA_GPU_STATS_PAIR_RESIDUES)))
            return set_err(err_out, err_len, "neither the pair areas nor the pair residues are delivered or named in the statistics word: they have nowhere to go");
        if (!std::isfinite(a.min_buried)) return set_err(err_out, err_len, "min_buried must be finite");
    }
    if (a.sr_only >= 0) { /* the volume, the masks: in the output's words */
        const TrajOutDef &o = OUT_DEF[a.sr_only];
        if (!a.to(a.sr_only)) return set_err(err_out, err_len, o.nowhere);
        if (a.alg != 1) return set_err(err_out, err_len, o.not_lr);
        if (a.frames_f32 & (FREESASA_GPU_FRAMES_PBC | FREESASA_GPU_FRAMES_TRICLINIC)) return set_err(err_out, err_len, o.not_periodic);
        if (a.resolution > SR_CAP_POINTS_MAX) {
            snprintf(msg, sizeof msg, o.too_many, SR_CAP_POINTS_MAX, a.resolution);
            return set_err(err_out, err_len, msg);
        }
    }
    return 0;
}

/* The run of a TrajCall, either form: the entry's rules, the topology with its groups and pairs (TrajTopo outlives the run: the
   lanes upload from it), TrajSpec and TrajIO, and then the memory form's run or the file form's.  The order of the checks is
   interface, and the two forms differ in it: the memory form asks for stats_out behind the statistics word and for the frames
   and the totals behind the pairs; the file form leaves its paths, header_bytes and the format to trajectory_file_run. */
int trajectory_call(const TrajCall &a, char *err_out, int err_len)
{
    if (err_out && err_len > 0) err_out[0] = 0;
    if (traj_call_rules(a, err_out, err_len)) return -1;
    return guarded(err_out, err_len, [&]() -> int {
        TrajTopo tp;
        if (topo_make(a.batch, a.structure, a.frame_atoms, a.atom_index, a.sel, &tp, err_out, err_len)) return -1;
        if (stats_check(a.stats, &tp, a.sel != nullptr, a.group != nullptr, err_out, err_len, a.more_stats)) return -1;
        if (!a.file && a.stats && !a.stats_out) return set_err(err_out, err_len, "statistics are asked for but have nowhere to go (stats_out is NULL)");
        /* (statistics of either group output make the groups' areas wanted: their kernels run) */
        /* (... and so do interface pairs: a row's isolated areas are the groups') */
        if (group_make(a.group, a.n_groups, a.to(OUT_GRP) || a.pairs || (a.stats & (FREESASA_GPU_STATS_GROUPS | FREESASA_GPU_STATS_ISOLATED)),
                       a.to(OUT_ISO) || (a.stats & FREESASA_GPU_STATS_ISOLATED), &tp, err_out, err_len)) return -1;
        pair_make(a.pairs, a.n_pairs, &tp);
        if (a.to(OUT_PRES) || (a.stats & FREESASA_GPU_STATS_PAIR_RESIDUES)) pair_res_make(a.min_buried, &tp);
        if (!a.file && (!a.xyz || !a.mem[OUT_TOTALS])) return set_err(err_out, err_len, "null argument");
        if ((a.to(OUT_SEL) || a.sel_atoms_out) && !a.sel) return set_err(err_out, err_len, "selection outputs need a selection set");
        TrajSpec s = {tp.radii, tp.n, a.n_frames, a.alg, a.probe, a.resolution, a.frames_per_batch, a.devices, a.n_devices, &tp, a.max_new_shards};
        TrajIO io;
        for (int k = 0; k < N_OUT; ++k) { io.out[k].mem = a.mem[k]; io.out[k].path = a.path[k]; }
        io.sel_atoms = a.sel_atoms_out; io.stats = a.stats; io.stats_path = a.stats_path; io.parts_path = a.partials_path;
        if (a.file) return trajectory_file_run(a.frames_path, a.frames_f32, a.header_bytes, s, io, a.done_path, a.frames_total_out, err_out, err_len);
        if (traj_check_args(s, "n_frames must be > 0", err_out, err_len) || traj_shard_size(s, a.frame_atoms, err_out, err_len)) return -1;
        io.src.open_memory(a.xyz, (size_t)a.frame_atoms);
        return traj_run_mem(io, s, a.stats_out, a.partials_out, err_out, err_len);
    });
}

} /* namespace */

/* The entries, from PIECES: a piece is a run of arguments that every entry which has it has under the same names
   (include/freesasa_gpu.h spells the prototypes out, and a definition here that differs from its prototype does not compile), once
   as the parameters, P_, and once as their way into the TrajCall, TC_ - by name, so an argument cannot end up in another one's
   field.  An output is `x_out`, an array, in the memory form and `x_path` in the file form: sfx is `out` or `path`. */
#define T_out double *
#define T_path const char *
#define TO_out mem
#define TO_path path
#define P_MEMORY const double *xyz_frames, int n_frames
#define TC_MEMORY a.xyz = xyz_frames; a.n_frames = n_frames
#define P_FILE const char *frames_path, int frames_f32, long long header_bytes, long long n_frames
#define TC_FILE a.file = true; a.frames_path = frames_path; a.frames_f32 = frames_f32; a.header_bytes = header_bytes; a.n_frames = n_frames
#define P_TOPOLOGY const freesasa_ingest_batch *batch, int structure, int frame_atoms, const int32_t *atom_index, const freesasa_ingest_selection *sel
#define TC_TOPOLOGY a.batch = batch; a.structure = structure; a.frame_atoms = frame_atoms; a.atom_index = atom_index; a.sel = sel
#define P_GROUPS const int32_t *group, int n_groups
#define TC_GROUPS a.group = group; a.n_groups = n_groups
#define P_PARAMETERS int alg, double probe, int resolution, int frames_per_batch
#define TC_PARAMETERS a.alg = alg; a.probe = probe; a.resolution = resolution; a.frames_per_batch = frames_per_batch
#define P_OUTPUTS(sfx) T_##sfx totals_##sfx, T_##sfx sasa_##sfx, T_##sfx class_sums_##sfx, T_##sfx residues_##sfx, T_##sfx sel_area_##sfx, long long *sel_atoms_out
#define TC_OUTPUTS(sfx) \
    a.TO_##sfx[OUT_TOTALS] = totals_##sfx; a.TO_##sfx[OUT_SASA] = sasa_##sfx; a.TO_##sfx[OUT_CLS] = class_sums_##sfx; a.TO_##sfx[OUT_RES] = residues_##sfx; \
    a.TO_##sfx[OUT_SEL] = sel_area_##sfx; a.sel_atoms_out = sel_atoms_out
#define P_GROUP_OUTPUTS(sfx) T_##sfx group_areas_##sfx, T_##sfx iso_##sfx
#define TC_GROUP_OUTPUTS(sfx) a.TO_##sfx[OUT_GRP] = group_areas_##sfx; a.TO_##sfx[OUT_ISO] = iso_##sfx
#define P_DEVICES const int *devices, int n_devices
#define TC_DEVICES a.devices = devices; a.n_devices = n_devices
#define P_FILE_TAIL const char *done_path, long long max_new_shards, P_DEVICES, long long *frames_total_out
#define TC_FILE_TAIL a.done_path = done_path; a.max_new_shards = max_new_shards; TC_DEVICES; a.frames_total_out = frames_total_out
#define P_STATISTICS(sfx) int stats, T_##sfx stats_##sfx, T_##sfx partials_##sfx
#define TC_STATISTICS(sfx) a.stats = stats; a.stats_##sfx = stats_##sfx; a.partials_##sfx = partials_##sfx
#define P_PAIRS(sfx) const int32_t *pairs, int n_pairs, T_##sfx pair_areas_##sfx
#define TC_PAIRS(sfx) a.kind = TrajCall::PAIRS; a.pairs = pairs; a.n_pairs = n_pairs; a.TO_##sfx[OUT_PAIR] = pair_areas_##sfx
#define P_PAIR_RESIDUES(sfx) double min_buried, T_##sfx pair_res_##sfx
#define TC_PAIR_RESIDUES(sfx) \
    a.kind = TrajCall::PAIR_RESIDUES; a.more_stats = FREESASA_GPU_STATS_PAIRS | FREESASA_GPU_STATS_PAIR_RESIDUES; a.min_buried = min_buried; \
    a.TO_##sfx[OUT_PRES] = pair_res_##sfx
#define P_ERR char *err_out, int err_len
/* an entry without groups: the memory form (..., the output of its own, if any, ...) and the file form */
#define P_MEMORY_PLAIN(...) P_MEMORY, P_TOPOLOGY, P_PARAMETERS, P_OUTPUTS(out), ##__VA_ARGS__, P_DEVICES, P_ERR
#define TC_MEMORY_PLAIN TC_MEMORY; TC_TOPOLOGY; TC_PARAMETERS; TC_OUTPUTS(out); TC_DEVICES
#define P_FILE_PLAIN(...) P_FILE, P_TOPOLOGY, P_PARAMETERS, P_OUTPUTS(path), ##__VA_ARGS__, P_FILE_TAIL, P_ERR
#define TC_FILE_PLAIN TC_FILE; TC_TOPOLOGY; TC_PARAMETERS; TC_OUTPUTS(path); TC_FILE_TAIL
/* an entry with groups: behind the tail its statistics, pairs and pair residues, if any */
#define P_MEMORY_GROUPS P_MEMORY, P_TOPOLOGY, P_GROUPS, P_PARAMETERS, P_OUTPUTS(out), P_GROUP_OUTPUTS(out), P_DEVICES
#define TC_MEMORY_GROUPS TC_MEMORY; TC_TOPOLOGY; TC_GROUPS; TC_PARAMETERS; TC_OUTPUTS(out); TC_GROUP_OUTPUTS(out); TC_DEVICES
#define P_FILE_GROUPS P_FILE, P_TOPOLOGY, P_GROUPS, P_PARAMETERS, P_OUTPUTS(path), P_GROUP_OUTPUTS(path), P_FILE_TAIL
#define TC_FILE_GROUPS TC_FILE; TC_TOPOLOGY; TC_GROUPS; TC_PARAMETERS; TC_OUTPUTS(path); TC_GROUP_OUTPUTS(path); TC_FILE_TAIL

extern "C" int freesasa_gpu_trajectory_topology(P_MEMORY_PLAIN())
{
    TrajCall a;
    TC_MEMORY_PLAIN;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_volume(P_MEMORY_PLAIN(double *volumes_out))
{
    TrajCall a;
    TC_MEMORY_PLAIN; a.mem[OUT_VOL] = volumes_out; a.sr_only = OUT_VOL;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_masks(P_MEMORY_PLAIN(uint32_t *masks_out))
{
    TrajCall a;
    TC_MEMORY_PLAIN; a.mem[OUT_MASK] = masks_out; a.sr_only = OUT_MASK;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_groups(P_MEMORY_GROUPS, P_ERR)
{
    TrajCall a;
    TC_MEMORY_GROUPS;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_groups_stats(P_MEMORY_GROUPS, P_STATISTICS(out), P_ERR)
{
    TrajCall a;
    TC_MEMORY_GROUPS; TC_STATISTICS(out);
    return trajectory_call(a, err_out, err_len);
}

/* the groups' run with the interfaces between the pairs of groups the caller names: six doubles per frame and pair */
extern "C" int freesasa_gpu_trajectory_interfaces(P_MEMORY_GROUPS, P_STATISTICS(out), P_PAIRS(out), P_ERR)
{
    TrajCall a;
    TC_MEMORY_GROUPS; TC_STATISTICS(out); TC_PAIRS(out);
    return trajectory_call(a, err_out, err_len);
}

/* ... and with the per-residue table of the interfaces, its occupancy column and the statistics of both pair outputs */
extern "C" int freesasa_gpu_trajectory_interface_residues(P_MEMORY_GROUPS, P_STATISTICS(out), P_PAIRS(out), P_PAIR_RESIDUES(out), P_ERR)
{
    TrajCall a;
    TC_MEMORY_GROUPS; TC_STATISTICS(out); TC_PAIRS(out); TC_PAIR_RESIDUES(out);
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_file_topology(P_FILE_PLAIN())
{
    TrajCall a;
    TC_FILE_PLAIN;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_file_volume(P_FILE_PLAIN(const char *volumes_path))
{
    TrajCall a;
    TC_FILE_PLAIN; a.path[OUT_VOL] = volumes_path; a.sr_only = OUT_VOL;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_file_masks(P_FILE_PLAIN(const char *masks_path))
{
    TrajCall a;
    TC_FILE_PLAIN; a.path[OUT_MASK] = masks_path; a.sr_only = OUT_MASK;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_file_groups(P_FILE_GROUPS, P_ERR)
{
    TrajCall a;
    TC_FILE_GROUPS; a.images = TrajCall::IMAGES_NEVER;
    return trajectory_call(a, err_out, err_len);
}

extern "C" int freesasa_gpu_trajectory_file_groups_stats(P_FILE_GROUPS, P_STATISTICS(path), P_ERR)
{
    TrajCall a;
    TC_FILE_GROUPS; TC_STATISTICS(path); a.images = TrajCall::IMAGES_NOT_WITH_GROUPS;
    return trajectory_call(a, err_out, err_len);
}

/* ... with the interfaces between the pairs of groups the caller names, six doubles per frame and pair into their own file */
extern "C" int freesasa_gpu_trajectory_file_interfaces(P_FILE_GROUPS, P_STATISTICS(path), P_PAIRS(path), P_ERR)
{
    TrajCall a;
    TC_FILE_GROUPS; TC_STATISTICS(path); TC_PAIRS(path);
    return trajectory_call(a, err_out, err_len);
}

/* ... with the per-residue table of the interfaces into its own file, and the statistics of both pair outputs */
extern "C" int freesasa_gpu_trajectory_file_interface_residues(P_FILE_GROUPS, P_STATISTICS(path), P_PAIRS(path), P_PAIR_RESIDUES(path), P_ERR)
{
    TrajCall a;
    TC_FILE_GROUPS; TC_STATISTICS(path); TC_PAIRS(path); TC_PAIR_RESIDUES(path);
    return trajectory_call(a, err_out, err_len);
}

/* chain groups among periodic images: the groups' run with every frame - and every group of it, taken on its own - among the
   images of the frame's cell (shard_compute: groups_periodic_stage) */
extern "C" int freesasa_gpu_trajectory_file_groups_periodic(P_FILE_GROUPS, P_STATISTICS(path), P_ERR)
{
    TrajCall a;
    TC_FILE_GROUPS; TC_STATISTICS(path);
    a.images = TrajCall::IMAGES_REQUIRED; a.sibling = "freesasa_gpu_trajectory_file_groups_stats";
    return trajectory_call(a, err_out, err_len);
}

/* interfaces between chain groups among periodic images: that run with, behind every frame's groups, its pair structures - each
   in the frame's cell among its own images (shard_compute: the pair part of groups_periodic_stage's combined batch); behind the
   stage the pairs' sums are the ones of the run without cells */
extern "C" int freesasa_gpu_trajectory_file_interfaces_periodic(P_FILE_GROUPS, P_STATISTICS(path), P_PAIRS(path), P_ERR)
{
    TrajCall a;
    TC_FILE_GROUPS; TC_STATISTICS(path); TC_PAIRS(path);
    a.images = TrajCall::IMAGES_REQUIRED; a.sibling = "freesasa_gpu_trajectory_file_interfaces";
    return trajectory_call(a, err_out, err_len);
}

/* ... with the per-residue table of the interfaces, read from the periodic isolated and pair areas, and the statistics of both pair outputs */
extern "C" int freesasa_gpu_trajectory_file_interface_residues_periodic(P_FILE_GROUPS, P_STATISTICS(path), P_PAIRS(path), P_PAIR_RESIDUES(path), P_ERR)
{
    TrajCall a;
    TC_FILE_GROUPS; TC_STATISTICS(path); TC_PAIRS(path); TC_PAIR_RESIDUES(path);
    a.images = TrajCall::IMAGES_REQUIRED; a.sibling = "freesasa_gpu_trajectory_file_interface_residues";
    return trajectory_call(a, err_out, err_len);
}
