/* TESTS ONLY: the two phase functions of chain groups among periodic images (freesasa_amd/csrc/pbc_kernels.h, GpbcArgs) driven
 * on the CPU as gpu_periodic.hip drives the kernels: gpbc_cell_struct one thread per combined structure, gpbc_finish_atom one
 * thread per combined atom - both over their kernels' whole grids, idle threads included.  The expansion of the combined batch
 * between them is emu_pbc.cpp's and emu_pbc_tri.cpp's, taken in with the file.  Never linked into the product. */
#include "emu_pbc_tri.cpp"

/* cells [W n_cplx] -> ccells [W n_comb]; gbase [n_cplx + 1] or NULL with g_fixed groups per complex */
extern "C" int emu_gpbc_cells(int n_cplx, int n_comb, const int64_t *gbase, int g_fixed, int W, const double *cells, double *ccells)
{
    if (n_cplx <= 0 || n_comb < n_cplx || !cells || !ccells || (W != 3 && W != PBC_TRI_CELL) || (!gbase && n_comb > n_cplx && g_fixed <= 0)) return -1;
    GpbcArgs a;
    memset(&a, 0, sizeof a);
    a.n_cplx = n_cplx; a.n_comb = n_comb; a.gbase = gbase; a.g_fixed = g_fixed; a.W = W; a.cells = cells; a.ccells = ccells;
    for (int k = 0; k < (n_comb + PBC_B - 1) / PBC_B * PBC_B; ++k) gpbc_cell_struct(a, k);
    return 0;
}

/* coff, eoff [n_comb + 1]; src [n_all - n_atoms] (n_fixed > 0: [n_iso_fixed]); key [n_atoms] (n_fixed > 0: [n_fixed]); esasa
 * [eoff[n_comb]] -> carea, cgath [n_all], sasa, iso [n_atoms] (either may be NULL) */
extern "C" int emu_gpbc_finish(int n_cplx, int n_comb, const int64_t *coff, const int64_t *eoff, const int64_t *gbase, int g_fixed,
                               const int *src, int n_fixed, int n_iso_fixed, const int *key, const double *esasa, double *carea,
                               double *cgath, double *sasa, double *iso)
{
    if (n_cplx <= 0 || n_comb < n_cplx || !coff || !eoff || !key || !esasa || !carea || !cgath) return -1;
    GpbcArgs a;
    memset(&a, 0, sizeof a);
    a.n_cplx = n_cplx; a.n_comb = n_comb; a.coff = coff; a.eoff = eoff; a.gbase = gbase; a.g_fixed = g_fixed;
    a.n_atoms = coff[n_cplx]; a.n_all = coff[n_comb];
    a.src = src; a.n_fixed = n_fixed; a.n_iso_fixed = n_iso_fixed; a.key = key;
    a.esasa = esasa; a.carea = carea; a.cgath = cgath; a.sasa = sasa; a.iso = iso;
    for (int64_t t = 0; t < (a.n_all + PBC_B - 1) / PBC_B * PBC_B; ++t) gpbc_finish_atom(a, t);
    return 0;
}

#ifdef GPBC_CHECK_MAIN
/* The same phases under AddressSanitizer + UBSan in a stand-alone program (make tests/emu/groups_pbc_check): a batch of three
 * complexes - 0 groups; 70 atoms in groups of 41, 0 and 1 with the rest in none; none of its atoms - in cells whose x edge is below
 * 2 c, every array of exactly its size.  One line per stage; exit status 0 when the areas that name their slot come back right. */
#include <stdio.h>
int main()
{
    const int ns = 3, G = 4, NS = ns + G;
    const int64_t off[ns + 1] = {0, 9, 79, 79}, gbase[ns + 1] = {0, 0, 3, 4};
    const int n = 79;
    std::vector<double> xyz(3 * n), radii(n), cells = {30, 9, 50, 12, 14, 16, 7, 7.5, 8};
    std::vector<int> key(n, -1);
    unsigned long long seed = 12345;
    auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
    for (int i = 0; i < n; ++i) {
        const double *L = &cells[3 * (i < 9 ? 0 : 1)];
        for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (rnd() * 2.0 - 0.5) * L[k];
        radii[i] = 1.2 + 0.8 * rnd();
        if (i >= 9) key[i] = (i - 9) % 7 == 3 ? -1 : (i == 20 ? 2 : 0);
    }
    std::vector<int64_t> comb(off, off + ns + 1);
    std::vector<int> src;
    std::vector<double> cxyz(xyz), cradii(radii);
    for (int g = 0; g < G; ++g) {
        int64_t cnt = 0;
        for (int i = 9; g < 3 && i < n; ++i)
            if (key[i] == g) { src.push_back(i); cxyz.insert(cxyz.end(), &xyz[3 * i], &xyz[3 * i] + 3); cradii.push_back(radii[i]); ++cnt; }
        comb.push_back(comb.back() + cnt);
    }
    const int64_t N = comb[NS];
    std::vector<double> ccells(3 * NS);
    if (emu_gpbc_cells(ns, NS, gbase, 0, 3, cells.data(), ccells.data())) return 1;
    for (int k = 0; k < NS; ++k)
        for (int w = 0; w < 3; ++w)
            if (ccells[3 * k + w] != cells[3 * (k < ns ? k : k < ns + 3 ? 1 : 2) + w]) { printf("cells: structure %d wrong\n", k); return 1; }
    printf("cells ok: %d structures\n", NS);
    std::vector<int64_t> n_img(NS), eoff(NS + 1);
    std::vector<double> rmax(NS);
    std::vector<int> ibase(N);
    long long E = emu_pbc_expand(cxyz.data(), cradii.data(), comb.data(), NS, 0, 0, ccells.data(), 1.4, n_img.data(), rmax.data(), ibase.data(),
                                 eoff.data(), nullptr, nullptr, 0);
    if (E < N) return 1;
    std::vector<double> exyz(3 * E), eradii(E), esasa(E);
    if (emu_pbc_expand(cxyz.data(), cradii.data(), comb.data(), NS, 0, 0, ccells.data(), 1.4, n_img.data(), rmax.data(), ibase.data(), eoff.data(),
                       exyz.data(), eradii.data(), E) != E) return 1;
    printf("expand ok: %lld atoms, %lld with their images\n", (long long)N, E);
    for (long long j = 0; j < E; ++j) esasa[j] = (double)j + 0.25;
    std::vector<double> carea(N), cgath(N), sasa(n), iso(n);
    if (emu_gpbc_finish(ns, NS, comb.data(), eoff.data(), gbase, 0, src.data(), 0, 0, key.data(), esasa.data(), carea.data(), cgath.data(),
                        sasa.data(), iso.data())) return 1;
    for (int i = 0; i < n; ++i) {
        const int s = i < 9 ? 0 : 1;
        if (sasa[i] != (double)(eoff[s] + i - off[s]) + 0.25 || (key[i] < 0 && iso[i] != sasa[i])) { printf("finish: atom %d wrong\n", i); return 1; }
    }
    for (int64_t t = n; t < N; ++t) {
        int k = ns;
        while (comb[k + 1] <= t) ++k;
        if (iso[src[t - n]] != (double)(eoff[k] + t - comb[k]) + 0.25 || cgath[t] != sasa[src[t - n]] || carea[t] != iso[src[t - n]]) { printf("finish: isolated atom %lld wrong\n", (long long)t); return 1; }
    }
    printf("finish ok: %d atoms, %lld isolated\n", n, (long long)(N - n));
    return 0;
}
#endif
