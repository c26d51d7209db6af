/*
 * CPU oracle (plain C) for the 2D TE-mode FDTD leapfrog -- TEST INFRASTRUCTURE ONLY.
 *
 * A scalar, per-cell restatement of the reference algorithm.  It is the checker
 * for the HIP path at sizes where the NumPy oracle is too slow, and the
 * multi-threaded "port" leg of bench.py's cpu_baseline.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it; the
 * product library (libfdtd2d.so) never links or calls it.
 *
 * Parity status: PINNED -- tests/test_oracle_golden.py checks every entry point
 * bit-for-bit against vectors produced by running the reference itself
 * (tests/golden/make_golden.py), for float64 and for float32 arrays.
 *
 * Reference map (relative to the reference checkout):
 *   orc_update_h_*   <- python-src/main.py:66-76   update_Hx_Hy
 *   orc_update_e_*   <- python-src/main.py:12-63   update_Ez (curl, Mur bands, corners)
 *   orc_mur_coef_*   <- python-src/main.py:30-31
 *   orc_add_point_*  <- python-src/fdtd.py:34 + main.py:185-186
 *   orc_ricker       <- python-src/main.py:183-184
 *   orc_run_*        <- python-src/fdtd.py:30-34   (H, E, source; t = i*dt)
 *
 * Layout = the reference's: row-major, Ez R x C, Hx R x (C-1), Hy (R-1) x C,
 * eps/mu R x C.  Arithmetic type = the array type: the float instantiation
 * rounds dt and dx to float first and then works in float throughout, which
 * is what NumPy does when the reference is handed float32 arrays (Python
 * scalars are weak).  Build with -ffp-contract=off: NumPy never fuses a*b+c.
 *
 * The boundary stages below run in the reference's own sequential order
 * (ascending band index, reading the not-yet-overwritten inward neighbour),
 * so unlike the staged NumPy oracle this file has no 11x11 minimum.
 *
 * Fused variant (suffixes _f32_fma / _f64_fma: orc_update_h_*, orc_update_e_*, orc_run_*): the arithmetic of
 * libfdtd2d_fused.so stated exactly.  The same per-cell code with four forms as ONE correctly rounded libm
 * fmaf / fma each --
 *     hx = fma(-ch, dr, hx)      hy = fma(ch, dc, hy)      e = fma(dhy - dhx, ce, e)
 *     Mur band cell = fma(k, inward_new - own_old, inward_old)
 * -- and everything else (the differences, ch, ce, k, the corner mean, the source add through double) with one
 * rounding per operation as before.  The file is compiled with -ffp-contract=off, so only these calls fuse.
 * Nothing of this comes from the reference, which has no such mode; tests/test_fused_oracle_cpu.py checks the
 * variant against exact rational arithmetic.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define BAND 5

double orc_ricker(double t, double fc)
{
    const double pi = 3.141592653589793;
    double tau = pi * fc * (t - 1 / fc);
    return (1 - 2 * (tau * tau)) * exp(-(tau * tau));
}

/* the four multiply-add forms of a cell-step: two roundings each (the reference), or one (the fused variant) */
#define HX_PLAIN(ch, dr, hx)   ((hx) - (ch) * (dr))
#define HY_PLAIN(ch, dc, hy)   ((hy) + (ch) * (dc))
#define EZ_PLAIN(d, ce, e)     ((e) + (d) * (ce))
#define MUR_PLAIN(k, d, p)     ((p) + (k) * (d))
#define HX_FMAF(ch, dr, hx)    fmaf(-(ch), (dr), (hx))
#define HY_FMAF(ch, dc, hy)    fmaf((ch), (dc), (hy))
#define EZ_FMAF(d, ce, e)      fmaf((d), (ce), (e))
#define MUR_FMAF(k, d, p)      fmaf((k), (d), (p))
#define HX_FMA(ch, dr, hx)     fma(-(ch), (dr), (hx))
#define HY_FMA(ch, dc, hy)     fma((ch), (dc), (hy))
#define EZ_FMA(d, ce, e)       fma((d), (ce), (e))
#define MUR_FMA(k, d, p)       fma((k), (d), (p))

/* shared by both variants: BASE = f32 | f64 */
#define DEFINE_SHARED(T, SUF, SQRT)                                                         \
                                                                                            \
T orc_mur_coef_##SUF(T mu00, T eps00, double dt_, double dx_)                               \
{                                                                                           \
    T dt = (T)dt_, dx = (T)dx_;                                                             \
    T c = (T)1 / SQRT(mu00 * eps00);                                                        \
    T cdt = c * dt;                                                                         \
    return (cdt - dx) / (cdt + dx);                                                         \
}                                                                                           \
                                                                                            \
int orc_add_point_##SUF(T *Ez, int R, int C, int row, int col, double amp)                  \
{                                                                                           \
    if (row < 0 || row >= R || col < 0 || col >= C) return -1;                              \
    size_t o = (size_t)row * C + col;                                                       \
    Ez[o] = (T)((double)Ez[o] + amp);                                                       \
    return 0;                                                                               \
}

/* SUF = BASE (plain forms) or BASE_fma (fused forms) */
#define DEFINE_ORACLE(T, SUF, BASE, HXF, HYF, EZF, MURF)                                    \
                                                                                            \
int orc_update_h_##SUF(const T *Ez, T *Hx, T *Hy, const T *mu, int R, int C,                \
                       double dt_, double dx_)                                              \
{                                                                                           \
    const T dt = (T)dt_, dx = (T)dx_;                                                       \
    _Pragma("omp parallel for schedule(static)")                                            \
    for (int i = 0; i < R - 1; ++i) {                                                       \
        const T *e0 = Ez + (size_t)i * C, *e1 = e0 + C;                                     \
        const T *m = mu + (size_t)i * C;                                                    \
        T *hx = Hx + (size_t)i * (C - 1);                                                   \
        T *hy = Hy + (size_t)i * C;                                                         \
        for (int j = 0; j < C - 1; ++j) {                                                   \
            T ch = dt / (m[j] * dx);                                                        \
            T dr = e1[j] - e0[j];                                                           \
            T dc = e0[j + 1] - e0[j];                                                       \
            hx[j] = HXF(ch, dr, hx[j]);                                                     \
            hy[j] = HYF(ch, dc, hy[j]);                                                     \
        }                                                                                   \
    }                                                                                       \
    return 0;                                                                               \
}                                                                                           \
                                                                                            \
/* P: caller scratch of R*C elements, or NULL (allocated here). */                          \
int orc_update_e_##SUF(T *Ez, const T *Hx, const T *Hy, const T *mu, const T *eps,          \
                       int R, int C, double dt_, double dx_, T *P)                          \
{                                                                                           \
    const T dt = (T)dt_, dx = (T)dx_;                                                       \
    int own = 0;                                                                            \
    if (R < BAND + 1 || C < BAND + 1) return -1;                                            \
    if (!P) { P = (T *)malloc((size_t)R * C * sizeof(T)); own = 1; if (!P) return -2; }     \
    memcpy(P, Ez, (size_t)R * C * sizeof(T));                                               \
    /* interior curl */                                                                     \
    _Pragma("omp parallel for schedule(static)")                                            \
    for (int i = 1; i < R - 1; ++i) {                                                       \
        T *e = Ez + (size_t)i * C;                                                          \
        const T *ep = eps + (size_t)i * C;                                                  \
        const T *hy = Hy + (size_t)i * C;                                                   \
        const T *hx = Hx + (size_t)i * (C - 1), *hxu = hx - (C - 1);                        \
        for (int j = 1; j < C - 1; ++j) {                                                   \
            T dhy = hy[j] - hy[j - 1];                                                      \
            T dhx = hx[j] - hxu[j];                                                         \
            T ce = dt / (ep[j] * dx);                                                       \
            e[j] = EZF(dhy - dhx, ce, e[j]);                                                \
        }                                                                                   \
    }                                                                                       \
    const T k = orc_mur_coef_##BASE(mu[0], eps[0], dt_, dx_);                               \
    /* left, then right band: rows 1..R-2 */                                                \
    for (int b = 0; b < BAND; ++b)                                                          \
        for (int i = 1; i < R - 1; ++i) {                                                   \
            size_t o = (size_t)i * C;                                                       \
            Ez[o + b] = MURF(k, Ez[o + b + 1] - P[o + b], P[o + b + 1]);                    \
        }                                                                                   \
    for (int b = 0; b < BAND; ++b)                                                          \
        for (int i = 1; i < R - 1; ++i) {                                                   \
            size_t o = (size_t)i * C + (C - 1 - b);                                         \
            Ez[o] = MURF(k, Ez[o - 1] - P[o], P[o - 1]);                                    \
        }                                                                                   \
    /* top, then bottom band: columns 1..C-2 */                                             \
    for (int b = 0; b < BAND; ++b) {                                                        \
        size_t o = (size_t)b * C;                                                           \
        for (int j = 1; j < C - 1; ++j)                                                     \
            Ez[o + j] = MURF(k, Ez[o + C + j] - P[o + j], P[o + C + j]);                    \
    }                                                                                       \
    for (int b = 0; b < BAND; ++b) {                                                        \
        size_t o = (size_t)(R - 1 - b) * C;                                                 \
        for (int j = 1; j < C - 1; ++j)                                                     \
            Ez[o + j] = MURF(k, Ez[o - C + j] - P[o + j], P[o - C + j]);                    \
    }                                                                                       \
    /* corner blocks: mean of the inward row- and column-neighbour */                       \
    for (int a = 0; a < BAND; ++a)                                                          \
        for (int b = 0; b < BAND; ++b) {                                                    \
            size_t t = (size_t)a * C, u = (size_t)(R - 1 - a) * C;                          \
            int l = b, r = C - 1 - b;                                                       \
            Ez[t + l] = (Ez[t + l + 1] + Ez[t + C + l]) / 2;                                \
            Ez[t + r] = (Ez[t + r - 1] + Ez[t + C + r]) / 2;                                \
            Ez[u + l] = (Ez[u - C + l] + Ez[u + l + 1]) / 2;                                \
            Ez[u + r] = (Ez[u - C + r] + Ez[u + r - 1]) / 2;                                \
        }                                                                                   \
    if (own) free(P);                                                                       \
    return 0;                                                                               \
}                                                                                           \
                                                                                            \
/* amps: nsteps doubles, or NULL for ricker(fc) at t = (step0 + n) * dt. */                 \
int orc_run_##SUF(T *Ez, T *Hx, T *Hy, const T *eps, const T *mu, int R, int C,             \
                  double dt, double dx, int nsteps, int src_row, int src_col,               \
                  const double *amps, double fc, long long step0)                           \
{                                                                                           \
    T *P = (T *)malloc((size_t)R * C * sizeof(T));                                          \
    if (!P) return -2;                                                                      \
    int rc = 0;                                                                             \
    for (int n = 0; n < nsteps && rc == 0; ++n) {                                           \
        rc = orc_update_h_##SUF(Ez, Hx, Hy, mu, R, C, dt, dx);                              \
        if (!rc) rc = orc_update_e_##SUF(Ez, Hx, Hy, mu, eps, R, C, dt, dx, P);             \
        double a = amps ? amps[n] : orc_ricker((double)(step0 + n) * dt, fc);               \
        if (!rc) rc = orc_add_point_##BASE(Ez, R, C, src_row, src_col, a);                  \
    }                                                                                       \
    free(P);                                                                                \
    return rc;                                                                              \
}

DEFINE_SHARED(float, f32, sqrtf)
DEFINE_SHARED(double, f64, sqrt)
DEFINE_ORACLE(float, f32, f32, HX_PLAIN, HY_PLAIN, EZ_PLAIN, MUR_PLAIN)
DEFINE_ORACLE(double, f64, f64, HX_PLAIN, HY_PLAIN, EZ_PLAIN, MUR_PLAIN)
DEFINE_ORACLE(float, f32_fma, f32, HX_FMAF, HY_FMAF, EZ_FMAF, MUR_FMAF)
DEFINE_ORACLE(double, f64_fma, f64, HX_FMA, HY_FMA, EZ_FMA, MUR_FMA)

void orc_set_threads(int n)
{
    extern void omp_set_num_threads(int);
    if (n > 0) omp_set_num_threads(n);
}

int orc_num_threads(void)
{
#ifdef _OPENMP
    extern int omp_get_max_threads(void);
    return omp_get_max_threads();
#else
    return 1;
#endif
}
