/* fdtd2d_batch_dispersive_adjoint.h -- what an adjoint run needs on a batch with a Drude-Lorentz pole, a companion of
 * fdtd2d_batch_dispersive.h.
 *
 * fdtd2d_batch_hold_dft_window and fdtd2d_batch_dft_window_product keep refusing a batch with a pole; their counterparts
 * are the calls below, which need one (FDTD2D_E_STATE without) and real fields (the pole of
 * fdtd2d_batch_bloch_dispersive.h is refused: its kernels take no point sources).
 *
 * Why they suffice.  With z = exp(i omega dt), D = eps dx / dt, G = sigma dx / 2 and the member's a, bq, ck of
 * fdtd2d_batch_dispersive.h (cj = dx bq EPS0 wp2), eliminating H, Jh and Q from one step gives
 *     (D (z - 2 + 1/z) + G (z - 1/z) + cj (z - 1)^2 / ((z - a)(z - 1) + ck z) - L) E = D (z - 1) S
 * The pole's term is diagonal, so the operator stays symmetric: the adjoint field is an ordinary dispersive run of the
 * same member with sources at the probe cells (fdtd2d_batch_set_point_sources, fdtd2d_batch_run_channels, which the
 * dispersive kernels take), and every gradient is a product of the same two window DFTs:
 *     dJ/d eps[i]   = (dx / dt)     sum_k Re( -(z_k - 2 + 1/z_k) / (z_k - 1)                     E_k[i] Eadj_k[i] )
 *     dJ/d sigma[i] = (dx / 2)      sum_k Re( -(z_k + 1) / z_k                                   E_k[i] Eadj_k[i] )
 *     dJ/d wp2[i]   = (dx bq EPS0)  sum_k Re( -(z_k - 1) / ((z_k - a)(z_k - 1) + ck z_k)         E_k[i] Eadj_k[i] )
 * so one call forms up to three of them in one pass over the windows.
 *
 * Definitions.
 *   held window   fdtd2d_batch_hold_dispersive_window keeps a device copy of the window accumulators in a buffer of its
 *                 own: the buffer of fdtd2d_batch_hold_dft_window and FDTD2D_BATCH_INFO_HELD_WINDOW are not touched.
 *   the product   Per member b, window cell w and coefficient set c, with the held pair hr, hi and the current pair cr, ci
 *                 of frequency k:
 *                     tr = hr*cr - hi*ci   ti = hr*ci + hi*cr   term = coef_re[c][b][k]*tr - coef_im[c][b][k]*ti
 *                 s_c = 0.0; s_c = s_c + term for k ascending; out[c][b][w] = scale[b][c] * s_c.  All in float64, one
 *                 rounding per operation (the fused build contracts as it does in fdtd2d_batch_dft_window_product).  With
 *                 one set and scale 1 the result equals fdtd2d_batch_dft_window_product's on the same buffers bit for bit. */
#ifndef FDTD2D_BATCH_DISPERSIVE_ADJOINT_H
#define FDTD2D_BATCH_DISPERSIVE_ADJOINT_H

#include "fdtd2d_batch_dispersive.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: 1 while a held dispersive window exists (20: the ids 0..19 are taken by fdtd2d.h and the other
 * companions); and the most coefficient sets of one fdtd2d_batch_dispersive_window_product.  Enumerators, not macros:
 * the companions' checks of their own ids scan every header for FDTD2D_BATCH_INFO_* macros and pin the largest. */
enum {
    FDTD2D_BATCH_INFO_HELD_DISPERSIVE_WINDOW = 20,
    FDTD2D_BATCH_MAX_PRODUCT_SETS = 3
};

/* Keeps the window DFT as it is now; the copy survives fdtd2d_batch_reset, fdtd2d_batch_set_point_sources and further
 * runs, and goes with the window (fdtd2d_batch_set_dft_window) or the pole (fdtd2d_batch_set_dispersion with NULLs).
 * FDTD2D_E_STATE, the batch unchanged: without a pole (use fdtd2d_batch_hold_dft_window), on a batch with complex
 * fields, without a window DFT. */
int fdtd2d_batch_hold_dispersive_window(fdtd2d_batch_t *b);

/* out (ncoef x count x nrows x ncols float64) as defined above.  ncoef: 1..FDTD2D_BATCH_MAX_PRODUCT_SETS; coef_re,
 * coef_im: ncoef x count x nfreq; scale: count x ncoef.  One launch and one read-back.  FDTD2D_E_ARG for a NULL or a bad
 * ncoef; FDTD2D_E_STATE without a held dispersive window (and for what fdtd2d_batch_hold_dispersive_window refuses). */
int fdtd2d_batch_dispersive_window_product(fdtd2d_batch_t *b, int ncoef, const double *coef_re, const double *coef_im,
                                           const double *scale, double *out);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_DISPERSIVE_ADJOINT_H */
