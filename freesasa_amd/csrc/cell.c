/*
 * cell.c — the host arithmetic of triclinic cells (include/freesasa_gpu.h: freesasa_gpu_cell_widths,
 * freesasa_gpu_cell_from_dcd, freesasa_gpu_cell_from_lengths_angles).  A cell is six numbers ax, bx, by, cx, cy, cz: the lower-triangular box matrix with rows
 * a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz).  Plain C without allocation, compiled with -ffp-contract=off like all of
 * the engine: every operation below is rounded on its own, in the order written (pbc_tri_kernels.h and the tests pin it).
 */
#include <math.h>
#include <stdio.h>

#include "../../include/freesasa_gpu.h"

/* (engine_internal.h) 0, -(k + 1) when entry k is not finite, k + 1 when the diagonal entry k (0, 2, 5) is not positive */
int periodic_cell6_bad(const double *h);
int periodic_cell6_bad(const double *h)
{
    for (int k = 0; k < 6; ++k)
        if (!isfinite(h[k])) return -(k + 1);
    for (int k = 0; k < 6; ++k)
        if ((k == 0 || k == 2 || k == 5) && !(h[k] > 0)) return k + 1;
    return 0;
}

int freesasa_gpu_cell_widths(const double cell6[6], double widths_out[3])
{
    if (!cell6 || !widths_out) return -1;
    const double ax = cell6[0], bx = cell6[1], by = cell6[2], cx = cell6[3], cy = cell6[4], cz = cell6[5];
    if (periodic_cell6_bad(cell6)) {
        widths_out[0] = widths_out[1] = widths_out[2] = NAN;
        return -1;
    }
    const double t = bx * cy - by * cx;
    widths_out[2] = cz;
    widths_out[1] = by * (cz / sqrt(cy * cy + cz * cz));
    widths_out[0] = ax * ((by * cz) / sqrt(((by * cz) * (by * cz) + (bx * cz) * (bx * cz)) + t * t));
    return 0;
}

/* the cosine of an angle given in degrees; 0 / -1 with the reason, which ends in `expected` */
static int degrees_cosine(double v, const char *name, const char *expected, double *cosine, char *why, int why_len)
{
    if (!(v > 0.0 && v < 180.0)) { /* (a NaN comes here) */
        if (why && why_len > 0) snprintf(why, (size_t)why_len, "angle %s of its cell is %.9g: %s", name, v, expected);
        return -1;
    }
    *cosine = fabs(v - 90.0) <= 1e-4 ? 0.0 : cos(v * 3.14159265358979323846 / 180.0);
    return 0;
}

/* the cosine an angle field of a CHARMM cell record stands for; 0 / -1 with the reason */
static int angle_cosine(double v, const char *name, double *cosine, char *why, int why_len)
{
    if (fabs(v) <= 1.0) { /* a cosine (the orthorhombic decoder's |v| <= 1e-6: a right angle) */
        *cosine = fabs(v) <= 1e-6 ? 0.0 : v;
        return 0;
    }
    return degrees_cosine(v, name, "neither a cosine nor degrees in (0, 180)", cosine, why, why_len);
}

static int edges_finite(double A, double B, double C, char *why, int why_len)
{
    const double edge[3] = {A, B, C};
    for (int k = 0; k < 3; ++k)
        if (!isfinite(edge[k])) {
            if (why && why_len > 0) snprintf(why, (size_t)why_len, "edge %c of its cell is not finite", "ABC"[k]);
            return -1;
        }
    return 0;
}

/* the six numbers from the edges and the cosines; g, b, a: the angles as they were given, for the reason */
static int cell_from_cosines(double A, double B, double C, double cg, double cb, double ca, double g, double b, double a, double cell6_out[6],
                             char *why, int why_len)
{
    const double sg = sqrt(1.0 - cg * cg);
    const double ax = A, bx = B * cg, by = B * sg, cx = C * cb, cy = C * ((ca - cb * cg) / sg);
    const double cz2 = (C * C - cx * cx) - cy * cy;
    if (!(cz2 > 0.0) || !isfinite(cz2) || !isfinite(bx) || !isfinite(by) || !isfinite(cx) || !isfinite(cy)) {
        if (why && why_len > 0)
            snprintf(why, (size_t)why_len, "the angles of its cell span no cell (gamma, beta, alpha fields %.9g, %.9g, %.9g)", g, b, a);
        return -1;
    }
    cell6_out[0] = ax; cell6_out[1] = bx; cell6_out[2] = by; cell6_out[3] = cx; cell6_out[4] = cy; cell6_out[5] = sqrt(cz2);
    return 0;
}

int freesasa_gpu_cell_from_dcd(const double rec[6], double cell6_out[6], char *why, int why_len)
{
    if (why && why_len > 0) why[0] = 0;
    if (!rec || !cell6_out) {
        if (why && why_len > 0) snprintf(why, (size_t)why_len, "null argument");
        return -1;
    }
    if (edges_finite(rec[0], rec[2], rec[5], why, why_len)) return -1;
    double cg, cb, ca;
    if (angle_cosine(rec[1], "gamma", &cg, why, why_len) || angle_cosine(rec[3], "beta", &cb, why, why_len) ||
        angle_cosine(rec[4], "alpha", &ca, why, why_len))
        return -1;
    return cell_from_cosines(rec[0], rec[2], rec[5], cg, cb, ca, rec[1], rec[3], rec[4], cell6_out, why, why_len);
}

int freesasa_gpu_cell_from_lengths_angles(const double len[3], const double deg[3], double cell6_out[6], char *why, int why_len)
{
    if (why && why_len > 0) why[0] = 0;
    if (!len || !deg || !cell6_out) {
        if (why && why_len > 0) snprintf(why, (size_t)why_len, "null argument");
        return -1;
    }
    if (edges_finite(len[0], len[1], len[2], why, why_len)) return -1;
    double cg, cb, ca; /* (gamma, beta, alpha: the order the DCD entry takes them in) */
    if (degrees_cosine(deg[2], "gamma", "not degrees in (0, 180)", &cg, why, why_len) || degrees_cosine(deg[1], "beta", "not degrees in (0, 180)", &cb, why, why_len) ||
        degrees_cosine(deg[0], "alpha", "not degrees in (0, 180)", &ca, why, why_len))
        return -1;
    return cell_from_cosines(len[0], len[1], len[2], cg, cb, ca, deg[2], deg[1], deg[0], cell6_out, why, why_len);
}
