/* TESTS ONLY: the phase functions of the selection kernels (freesasa_amd/csrc/select_kernels.h) driven thread by thread on
 * the CPU over a loaded batch, in the launch order of gpu_kernels.hip (k_sel_mask, then k_sel_sums per structure and group
 * of SEL_G selections).  The program comes from the product library (freesasa_ingest_selection_compile); this file only
 * runs it.  Never linked into the product. */
#include <stdint.h>
#include <string.h>
#include <vector>

#include "freesasa_ingest.h"
#include "../../freesasa_amd/csrc/select_kernels.h"

using namespace sasa;

/* prog [n_words] with its flags, n_sel selections; the batch's arrays; sasa [n_atoms] (may be NULL: no sums).
 * bits_out [n_atoms]; area_out / count_out [n_structs * n_sel] (may be NULL).  Returns 0, -1 on a bad argument. */
extern "C" int emu_select(const freesasa_sel_word *prog, int n_words, int flags, int n_sel, const freesasa_ingest_batch *b,
                          const double *sasa, uint64_t *bits_out, double *area_out, long long *count_out)
{
    if (!prog || !b || !bits_out || n_words < 1 || n_sel < 1 || n_sel > SEL_MAX_SELECTIONS) return -1;
    const int64_t n = b->n_atoms, R = b->n_residues;
    if (n == 0) return 0;
    if (R < 1 || b->n_structs < 1) return -1;
    std::vector<uint64_t> keys((size_t)n);
    sel_pack_atom_keys(b->atom_name, b->atom_symbol, n, keys.data());
    /* labels in the layout the device gets them in: names | chains | numbers, read as words */
    std::vector<uint32_t> name((size_t)R), chain((size_t)R);
    std::vector<uint16_t> number(3 * (size_t)R);
    memcpy(name.data(), b->res_name, 4 * (size_t)R);
    memcpy(chain.data(), b->res_chain, 4 * (size_t)R);
    memcpy(number.data(), b->res_number, 6 * (size_t)R);
    SelArgs a;
    memset(&a, 0, sizeof a);
    a.prog = prog; a.n_words = n_words; a.flags = flags; a.n_sel = n_sel;
    a.akey = keys.data();
    a.offsets = b->offsets; a.n_structs = b->n_structs; a.n_atoms = n;
    a.res_first = b->res_first; a.n_res = R; a.n_res_dev = 0;
    a.name_h = name.data(); a.chain_h = chain.data(); a.number_h = number.data();
    a.bits = bits_out; a.sasa = sasa; a.area = area_out; a.count = count_out;
    const int64_t blocks = (n + SEL_B - 1) / SEL_B;
    for (int64_t blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < SEL_B; ++t) sel_mask_atom(a, blk * SEL_B + t);
    if (!sasa || !area_out || !count_out) return 0;
    std::vector<double> part((size_t)SEL_G * SASA_TOT_B);
    std::vector<int> cnt((size_t)SEL_G * SASA_TOT_B);
    for (int s = 0; s < b->n_structs; ++s)
        for (int g0 = 0; g0 < n_sel; g0 += SEL_G) {
            for (int t = 0; t < SASA_TOT_B; ++t) sel_sums_phase0(a, part.data(), cnt.data(), s, g0, t);
            for (int t = 0; t < SASA_TOT_B; ++t) sel_sums_phase1(a, part.data(), cnt.data(), s, g0, t);
        }
    return 0;
}
