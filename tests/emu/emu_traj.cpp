/* TESTS ONLY: the phase functions of the trajectory drivers' topology (freesasa_amd/csrc/traj_kernels.h) driven thread by
 * thread on the CPU, in the launch order of gpu_kernels.hip: sel_mask_atom once over structure `structure` of a loaded batch
 * taken as a batch of one (what a lane does once), k_traj_gather over full frames, then k_traj_residues, k_traj_class and
 * k_traj_sel over per-atom areas.  The rebase of the structure's residues is done HERE, independently of the driver's.
 * Never linked into the product. */
#include <stdint.h>
#include <string.h>
#include <vector>

#include "freesasa_ingest.h"
#include "../../freesasa_amd/csrc/traj_kernels.h"

using namespace sasa;

/* The gather alone: in [n_frames][frame_atoms][3] (floats when in_f32) -> out [n_frames][n][3] doubles. */
extern "C" int emu_traj_gather(const void *in, int in_f32, int n_frames, int frame_atoms, const int32_t *index, int n, double *out)
{
    if (!in || !index || !out || n < 1 || n_frames < 1 || frame_atoms < n) return -1;
    TrajArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.n_frames = n_frames; a.frame_atoms = frame_atoms; a.index = index;
    const int64_t blocks = (3 * (int64_t)n_frames * n + TRAJ_B - 1) / TRAJ_B;
    for (int64_t blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < TRAJ_B; ++t) {
            if (in_f32) traj_gather(a, (const float *)in, out, blk * TRAJ_B + t);
            else traj_gather(a, (const double *)in, out, blk * TRAJ_B + t);
        }
    return 0;
}

/* The per-frame sums: sasa [n_frames * n] -> cls_out [n_frames * 3], res_out [n_frames * R * 6] and, with a program,
 * bits_out [n], sel_out / count_out [n_frames * n_sel].  Returns the structure's residue count R, -1 on a bad argument. */
extern "C" int emu_traj_sums(const freesasa_ingest_batch *b, int structure, const freesasa_sel_word *prog, int n_words, int flags, int n_sel,
                             const double *sasa, int n_frames, double *cls_out, double *res_out, uint64_t *bits_out, double *sel_out,
                             long long *count_out)
{
    if (!b || structure < 0 || structure >= b->n_structs || !sasa || n_frames < 1) return -1;
    const int64_t a0 = b->offsets[structure], n = b->offsets[structure + 1] - a0;
    const int64_t r0 = b->res_offsets[structure], R = b->res_offsets[structure + 1] - r0;
    if (n < 1 || R < 1) return -1;
    std::vector<int64_t> first((size_t)R + 1);
    for (int64_t r = 0; r <= R; ++r) first[(size_t)r] = b->res_first[r0 + r] - a0;
    const int64_t offs[2] = {0, n};
    TrajArgs a;
    memset(&a, 0, sizeof a);
    a.n = (int)n; a.n_frames = n_frames; a.frame_atoms = (int)n; a.n_res = (int)R; a.res_first = first.data();
    a.cls = b->atom_class + a0; a.bb = b->atom_backbone + a0;
    a.sasa = sasa; a.cls_out = cls_out; a.res_out = res_out;
    if (res_out) {
        const int64_t blocks = ((int64_t)n_frames * R + TRAJ_B - 1) / TRAJ_B;
        for (int64_t blk = 0; blk < blocks; ++blk)
            for (int t = 0; t < TRAJ_B; ++t) traj_residue(a, blk * TRAJ_B + t);
    }
    if (cls_out) {
        std::vector<double> part(3 * SASA_TOT_B);
        for (int f = 0; f < n_frames; ++f) {
            for (int t = 0; t < SASA_TOT_B; ++t) traj_class_phase0(a, part.data(), f, t);
            for (int t = 0; t < SASA_TOT_B; ++t) class_phase1(part.data(), cls_out, f, t);
        }
    }
    if (!prog) return (int)R;
    if (n_words < 1 || n_sel < 1 || n_sel > SEL_MAX_SELECTIONS || !bits_out || !sel_out || !count_out) return -1;
    /* once per topology: the program over the structure as a batch of one */
    std::vector<uint64_t> keys((size_t)n);
    sel_pack_atom_keys(b->atom_name + 4 * a0, b->atom_symbol + 2 * a0, n, keys.data());
    std::vector<uint32_t> name((size_t)R), chain((size_t)R);
    std::vector<uint16_t> number(3 * (size_t)R);
    memcpy(name.data(), b->res_name + 4 * r0, 4 * (size_t)R);
    memcpy(chain.data(), b->res_chain + 4 * r0, 4 * (size_t)R);
    memcpy(number.data(), b->res_number + 6 * r0, 6 * (size_t)R);
    SelArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.prog = prog; sa.n_words = n_words; sa.flags = flags; sa.n_sel = n_sel;
    sa.akey = keys.data(); sa.offsets = offs; sa.n_structs = 1; sa.n_atoms = n;
    sa.res_first = first.data(); sa.n_res = R; sa.n_res_dev = 0;
    sa.name_h = name.data(); sa.chain_h = chain.data(); sa.number_h = number.data();
    sa.bits = bits_out;
    for (int64_t blk = 0; blk < (n + SEL_B - 1) / SEL_B; ++blk)
        for (int t = 0; t < SEL_B; ++t) sel_mask_atom(sa, blk * SEL_B + t);
    a.bits = bits_out; a.n_sel = n_sel; a.sel_out = sel_out; a.sel_count = count_out;
    std::vector<double> part((size_t)SEL_G * SASA_TOT_B);
    std::vector<int> cnt((size_t)SEL_G * SASA_TOT_B);
    for (int f = 0; f < n_frames; ++f)
        for (int g0 = 0; g0 < n_sel; g0 += SEL_G) {
            for (int t = 0; t < SASA_TOT_B; ++t) traj_sel_phase0(a, part.data(), cnt.data(), f, g0, t);
            for (int t = 0; t < SASA_TOT_B; ++t) traj_sel_phase1(a, part.data(), cnt.data(), f, g0, t);
        }
    return (int)R;
}
