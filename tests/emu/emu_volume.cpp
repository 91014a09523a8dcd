/* TESTS ONLY: the phase functions of the molecular volume (freesasa_amd/csrc/vol_kernels.h) driven on the CPU as gpu_volume.hip
 * drives the kernels: vol_origin_phase0 / 1 one workgroup of SASA_TOT_B threads per structure (the barrier between the phases is
 * the loop's end), vol_atom one thread per atom of k_vol_atom's grid, then the engine's totals over the terms as kl_totals takes
 * them (totals_chunk_phase0 / 1 per chunk of the bounds chunk table, totals_struct per structure).
 * And the Shrake-Rupley tile kernel's phases with the store phase of k_sr_tile_vol: emu.cpp, as it is, compiled into this
 * library a second time with its call of sr_caps_store sent through a hook that runs sr_caps_store<true> while a place for
 * the exposed-point vectors is set (emu_set_sr_evec) - launch_sr picks the kernel by that pointer in the same way.
 * Never linked into the product. */
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../freesasa_amd/csrc/vol_kernels.h"

static double *emu_sr_evec = nullptr; /* [3 n]: where the next emu_run_batch calls of THIS library keep the vectors */
extern "C" void emu_set_sr_evec(double *evec) { emu_sr_evec = evec; }
static inline void emu_store_hook(const sasa::TileArgs &a, sasa::TileMem &m, int tile, int tid)
{
    if (emu_sr_evec) sasa::sr_caps_store<true>(a, m, tile, tid, emu_sr_evec);
    else sasa::sr_caps_store<false>(a, m, tile, tid);
}
#define sr_caps_store(a, m, tile, tid) emu_store_hook(a, m, tile, tid) /* (emu.cpp's one call; the templates above are spelled with <>) */
#include "emu.cpp"
#undef sr_caps_store

/* xyz [3 n], radii [n] (shared_radii: one structure's), offsets [n_structs + 1], counts [n], evec [3 n].
 * Out: origin [3 n_structs], vol [n], volumes [n_structs].  0, -1 on a bad argument. */
extern "C" int emu_volume(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, int shared_radii, double probe,
                          int n_points, const int *counts, const double *evec, double *origin, double *vol, double *volumes)
{
    if (!xyz || !radii || !offsets || n_structs <= 0 || n_points <= 0 || !counts || !evec || !origin || !vol || !volumes) return -1;
    VolArgs a;
    memset(&a, 0, sizeof a);
    a.xyz = xyz; a.radii = radii; a.offsets = offsets; a.n_structs = n_structs; a.shared_radii = shared_radii; a.n_points = n_points;
    a.n_atoms = offsets[n_structs]; a.probe = probe; a.counts = counts; a.evec = evec; a.origin = origin; a.vol = vol;
    std::vector<double> part(6 * SASA_TOT_B);
    for (int s = 0; s < n_structs; ++s) { /* (k_vol_origin: one workgroup per structure) */
        for (int tid = 0; tid < SASA_TOT_B; ++tid) vol_origin_phase0(a, part.data(), s, tid);
        for (int tid = 0; tid < SASA_TOT_B; ++tid) vol_origin_phase1(a, part.data(), s, tid);
    }
    for (int64_t t = 0; t < (a.n_atoms + VOL_B - 1) / VOL_B * VOL_B; ++t) vol_atom(a, t); /* (k_vol_atom's grid, idle threads included) */
    /* the chunk tables as gpu_engine.hip makes them of the offsets */
    std::vector<int> cl, sc0((size_t)n_structs + 1);
    std::vector<int64_t> cb;
    for (int s = 0; s < n_structs; ++s) {
        sc0[(size_t)s] = (int)cb.size();
        for (int64_t b = offsets[s]; b < offsets[s + 1]; b += SASA_BOUNDS_CHUNK) {
            const int64_t e = b + SASA_BOUNDS_CHUNK < offsets[s + 1] ? b + SASA_BOUNDS_CHUNK : offsets[s + 1];
            cb.push_back(b); cl.push_back((int)(e - b));
        }
    }
    sc0[(size_t)n_structs] = (int)cb.size();
    PipeArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.n_structs = n_structs; pa.n_chunks = (int)cb.size(); pa.chunk_begin = cb.data(); pa.chunk_len = cl.data(); pa.struct_chunk0 = sc0.data();
    std::vector<double> chunk_tot(cb.size() + 1), tp(SASA_TOT_B);
    for (int c = 0; c < pa.n_chunks; ++c) {
        for (int tid = 0; tid < SASA_TOT_B; ++tid) totals_chunk_phase0(pa, vol, tp.data(), c, tid);
        for (int tid = 0; tid < SASA_TOT_B; ++tid) totals_chunk_phase1(tp.data(), chunk_tot.data(), c, tid);
    }
    for (int s = 0; s < (n_structs + 255) / 256 * 256; ++s) totals_struct(pa, chunk_tot.data(), volumes, s);
    return 0;
}
