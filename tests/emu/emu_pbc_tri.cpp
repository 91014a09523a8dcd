/* TESTS ONLY: the phase functions of periodic images in a triclinic cell (freesasa_amd/csrc/pbc_tri_kernels.h) driven on the
 * CPU as gpu_periodic.hip drives the kernels: pbc_tri_count_struct one workgroup of PBC_B threads per structure, the expanded
 * offsets made of its image counts, pbc_tri_emit_atom one thread per atom.  The workgroup's fibers are emu_pbc.cpp's, taken
 * in with the file (so this library also holds emu_pbc_expand and emu_pbc_collect, built from the same source as
 * libpbc_emu.so).  Never linked into the product. */
#include "emu_pbc.cpp"

#include "../../freesasa_amd/csrc/pbc_tri_kernels.h"

struct TriRun { const PbcTriArgs *a; double *lds_d; int *lds_w; int s; };
static void tri_count_body(int tid, void *ctx)
{
    const TriRun *r = (const TriRun *)ctx;
    pbc_tri_count_struct(*r->a, r->lds_d, r->lds_w, r->s, tid);
}

/* As emu_pbc_expand, with cell9 [9 n_structs]: per structure ax, bx, by, cx, cy, cz and the widths d_a, d_b, d_c. */
extern "C" long long emu_pbc_tri_expand(const double *xyz, const double *radii, const int64_t *offsets, int n_structs, int n_fixed, int shared_radii,
                                        const double *cell9, double probe, int64_t *n_img, double *rmax, int *ibase, int64_t *eoff,
                                        double *exyz, double *eradii, long long cap)
{
    if (!xyz || !radii || !cell9 || n_structs <= 0 || !n_img || !rmax || !ibase || !eoff || (!offsets && n_fixed <= 0)) return -1;
    PbcTriArgs t;
    memset(&t, 0, sizeof t);
    PbcArgs &a = t.b;
    t.cell9 = cell9;
    a.xyz = xyz; a.radii = radii; a.offsets = offsets;
    a.n_structs = n_structs; a.n_fixed = offsets ? 0 : n_fixed; a.shared_radii = shared_radii;
    a.n_atoms = offsets ? offsets[n_structs] : (int64_t)n_structs * n_fixed;
    a.probe = probe;
    a.ibase = ibase; a.n_img = n_img; a.rmax = rmax;
    double lds_d[PBC_B];
    int lds_w[PBC_WAVES];
    for (int s = 0; s < n_structs; ++s) { /* (k_pbc_tri_count: one workgroup per structure) */
        TriRun r = {&t, lds_d, lds_w, s};
        sasa_emu::run_group(tri_count_body, &r);
    }
    eoff[0] = 0;
    for (int s = 0; s < n_structs; ++s) eoff[s + 1] = eoff[s] + (pbc_begin(a, s + 1) - pbc_begin(a, s)) + n_img[s];
    if (exyz && eradii && eoff[n_structs] <= cap) {
        a.eoff = eoff; a.exyz = exyz; a.eradii = eradii;
        for (int64_t i = 0; i < (a.n_atoms + PBC_B - 1) / PBC_B * PBC_B; ++i) pbc_tri_emit_atom(t, i); /* (k_pbc_tri_emit's grid, idle threads included) */
    }
    return eoff[n_structs];
}
