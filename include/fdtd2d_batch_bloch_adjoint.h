/* fdtd2d_batch_bloch_adjoint.h -- what an adjoint run needs on a Bloch batch, a companion of fdtd2d_batch_bloch.h.
 *
 * The calls of fdtd2d_batch_adjoint.h and fdtd2d_batch_design.h keep refusing a batch that carries a Bloch phase; their
 * complex counterparts are the calls below, which need one (FDTD2D_E_STATE without).
 *
 * Why they suffice.  With rho = (c, s) the one-step operator couples across the seam with conj(rho) * k in the row of
 * column 0 and rho * k in the row of column C-2, so it is not symmetric; its transpose is the same operator with rho
 * replaced by conj(rho) = (c, -s), exactly, also with c and s rounded to the batch dtype (negation is exact).  The adjoint
 * field is therefore an ordinary Bloch run of the same member with the rotation conjugated and sources at the probe
 * cells, and the gradient is the plain, unconjugated product of the two complex window DFTs.
 *
 * Definitions.
 *   point sources   After the E half-step and the rectangle source of step n of fdtd2d_batch_run_bloch_channels, point
 *                   cell p takes s = 0.0; s = s + w[p][c] * chan[c][n] for c ascending, in float64, then
 *                   Ez_re = (T)((double)Ez_re + s).  The imaginary part takes nothing.  Then the window DFT and the
 *                   probes of both parts sample.  Weights and channels are real: a real series added to the real part
 *                   drives the complex field through the seam.
 *   the image       A point cell in column 0 is also added to the image slot (which holds the unrotated copy of column
 *                   0), so the image stays that copy bit for bit; such a cell counts twice against the 64 entries.
 *   conjugate       A run with conjugate != 0 steps with (c, -s) in place of (c, s) everywhere the step applies rho.
 *                   Every download after it delivers the image column rotated by the rotation that run used, until the
 *                   next run, fdtd2d_batch_reset or fdtd2d_batch_set_bloch.
 *   held window     fdtd2d_batch_hold_bloch_window keeps device copies of both parts' accumulators.
 *   the product     With the held a = W(re), b = W(im) (accumulator pairs ar, ai and br, bi): hr = ar - bi, hi = ai + br;
 *                   the current windows give cr', ci' the same way; then per member and window cell
 *                       tr = hr*cr' - hi*ci'   ti = hr*ci' + hi*cr'   term = coef_re*tr - coef_im*ti
 *                   summed over k ascending from 0.0, all in float64, one rounding per operation.  The fused build:
 *                   tr = fma(hr, cr', -(hi*ci')), ti = fma(hr, ci', hi*cr'), term = fma(coef_re, tr, -(coef_im*ti)).
 *   probe spectra   fdtd2d_batch_probe_spectra's transform S of the real traces and of the imaginary traces:
 *                   X_re = S(re)_re - S(im)_im, X_im = S(re)_im + S(im)_re; the peak is the larger of the two parts'.
 *   field maxima    fdtd2d_batch_field_absmax of each part, the larger of the two; of Ez over columns 0..C-2 (the image
 *                   slot holds a copy of column 0). */
#ifndef FDTD2D_BATCH_BLOCH_ADJOINT_H
#define FDTD2D_BATCH_BLOCH_ADJOINT_H

#include "fdtd2d_batch_bloch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: the point cells per member of a Bloch batch (FDTD2D_BATCH_INFO_POINT_SOURCES reports 0 there), and
 * 1 while a held Bloch window exists (FDTD2D_BATCH_INFO_HELD_WINDOW reports 0 there).  _RESIDENT, _RESIDENT_MAX_CELLS
 * and _LDS_BYTES count the 8 bytes per table entry while Bloch point sources are set. */
#define FDTD2D_BATCH_INFO_BLOCH_POINT_SOURCES 17
#define FDTD2D_BATCH_INFO_HELD_BLOCH_WINDOW 18

/* The arguments and checks of fdtd2d_batch_set_point_sources; FDTD2D_E_STATE without a Bloch phase, FDTD2D_E_ARG
 * (naming the member) for a cell in column C-1.  ncell = 0 removes them.  Turning the phase off drops them; a later
 * fdtd2d_batch_set_bloch that changes the rotations keeps them. */
int fdtd2d_batch_set_bloch_point_sources(fdtd2d_batch_t *b, int ncell, const int *cells, int nchan,
                                         const double *weights);

/* fdtd2d_batch_run_bloch plus the point sources: chan as fdtd2d_batch_run_channels takes it (nchan x nsteps shared, or
 * count x nchan x nsteps with chan_per_member != 0).  conjugate != 0 runs with (c, -s).  One launch per run on the
 * resident path, two per step on the streamed one. */
int fdtd2d_batch_run_bloch_channels(fdtd2d_batch_t *b, int nsteps, const double *amps_re, const double *amps_im,
                                    const double *chan, int chan_per_member, int conjugate);

/* Keeps both parts of the window DFT as they are now; the copy survives fdtd2d_batch_reset and further runs, and goes
 * with the window (fdtd2d_batch_set_dft_window) or the phase. */
int fdtd2d_batch_hold_bloch_window(fdtd2d_batch_t *b);

/* out (count x nrows x ncols float64) = sum_k Re(coef[b][k] * held[b][k] * current[b][k]) as defined above; coef_re,
 * coef_im: count x nfreq. */
int fdtd2d_batch_bloch_window_product(fdtd2d_batch_t *b, const double *coef_re, const double *coef_im, double *out);

/* The arguments of fdtd2d_batch_probe_spectra; re, im receive the complex spectra of the complex traces. */
int fdtd2d_batch_bloch_probe_spectra(fdtd2d_batch_t *b, int nfreq, const double *omega, long long first,
                                     long long count_samples, double *re, double *im, double *peak);

/* out[count]: max(max |Re field|, max |Im field|) per member; which = FDTD2D_FIELD_EZ, _HX or _HY. */
int fdtd2d_batch_bloch_field_absmax(fdtd2d_batch_t *b, int which, double *out);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_BLOCH_ADJOINT_H */
