/* TESTS ONLY: the two phase functions of chain groups among periodic images (freesasa_amd/csrc/pbc_kernels.h, GpbcArgs) with the
 * PAIR PART of a trajectory shard's combined batch - frames | isolated groups | pair structures - driven on the CPU as
 * gpu_periodic.hip drives the kernels for freesasa_gpu_trajectory_file_interfaces_periodic: gpbc_cell_struct one thread per
 * combined structure, gpbc_finish_atom one thread per combined atom, both over their kernels' whole grids, idle threads
 * included.  k_fixed = 0 is the groups' run: emu_groups_pbc.cpp's two entries, taken in with the file, are its yardstick.
 * Never linked into the product. */
#include "emu_groups_pbc.cpp"

/* a shard's frames: nf complexes, g_fixed groups and k_fixed pair structures each; cells [W nf] -> ccells [W n_comb] */
extern "C" int emu_gpbc_pair_cells(int nf, int g_fixed, int k_fixed, int W, const double *cells, double *ccells)
{
    if (nf <= 0 || g_fixed <= 0 || k_fixed < 0 || !cells || !ccells || (W != 3 && W != PBC_TRI_CELL)) return -1;
    GpbcArgs a;
    memset(&a, 0, sizeof a);
    a.n_cplx = nf; a.n_comb = nf * (1 + g_fixed + k_fixed); a.g_fixed = g_fixed; a.k_fixed = k_fixed; a.W = W; a.cells = cells; a.ccells = ccells;
    for (int k = 0; k < (a.n_comb + PBC_B - 1) / PBC_B * PBC_B; ++k) gpbc_cell_struct(a, k);
    return 0;
}

/* coff, eoff [n_comb + 1] with n_comb = nf (1 + g_fixed + k_fixed); src [n_iso_fixed], key [n_fixed]: the topology's; esasa
 * [eoff[n_comb]] -> carea, cgath [n_all], sasa, iso [nf n_fixed] (either may be NULL) */
extern "C" int emu_gpbc_pair_finish(int nf, int g_fixed, int k_fixed, const int64_t *coff, const int64_t *eoff, const int *src, int n_fixed,
                                    int n_iso_fixed, const int *key, const double *esasa, double *carea, double *cgath, double *sasa, double *iso)
{
    if (nf <= 0 || g_fixed <= 0 || k_fixed < 0 || n_fixed <= 0 || n_iso_fixed < 0 || !coff || !eoff || !src || !key || !esasa || !carea || !cgath)
        return -1;
    GpbcArgs a;
    memset(&a, 0, sizeof a);
    a.n_cplx = nf; a.n_comb = nf * (1 + g_fixed + k_fixed); a.coff = coff; a.eoff = eoff; a.g_fixed = g_fixed; a.k_fixed = k_fixed;
    a.n_atoms = (int64_t)nf * n_fixed; a.n_all = coff[a.n_comb]; a.pair_first = a.n_atoms + (int64_t)nf * n_iso_fixed;
    if (coff[nf] != a.n_atoms || coff[nf * (1 + g_fixed)] != a.pair_first) return -1;
    a.src = src; a.n_fixed = n_fixed; a.n_iso_fixed = n_iso_fixed; a.key = key;
    a.esasa = esasa; a.carea = carea; a.cgath = cgath; a.sasa = sasa; a.iso = iso;
    for (int64_t t = 0; t < (a.n_all + PBC_B - 1) / PBC_B * PBC_B; ++t) gpbc_finish_atom(a, t);
    return 0;
}
