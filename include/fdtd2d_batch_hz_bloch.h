/* fdtd2d_batch_hz_bloch.h -- a Bloch phase for periodic batches in the Hz polarisation, a companion of fdtd2d_batch_hz.h
 * and fdtd2d_batch_bloch.h.
 *
 * An Hz Bloch batch is a periodic batch in the Hz polarisation (Hz with Ex and Ey, the electric field in the plane)
 * whose fields are complex and repeat as F(x + period) = F(x) * e^{i phi}, one phi per member: Brewster incidence,
 * grating-coupled surface plasmons, the angle sweep of a wire-grid polariser.  The conductivity and the Drude-Lorentz
 * pole of fdtd2d_batch_hz.h act on Ex and Ey under the phase.
 *
 * Definition.  Every field is a pair (re, im) of the batch dtype T.  Member b has a rotation rho_b = (c_b, s_b) of type
 * T: the float64 cos(phi_b) and sin(phi_b) as given, rounded to T.  Every coefficient (ch, cb, ca, cj, a, ck, the row
 * factors) is real, so the step of fdtd2d_batch_hz.h on a periodic batch acts on the real part and on the imaginary
 * part separately, operations and order unchanged: the E half-step with its two pole updates, the H half-step with the
 * split update in the layer, the source, the image, the monitors.  The two parts meet at the seam only:
 *   E half-step, j = C-2   the right neighbour of Hz is rho * (image slot):
 *                              re' = c*re - s*im        im' = s*re + c*im
 *                          two products and one sum each, each rounded to T.  It is formed first, then
 *                          dyj = rotated - Hz[i, C-2].
 *   H half-step, column 0  the left neighbour of Ey is conj(rho) * Ey[i, C-2]:
 *                              re' = c*er + s*ei        im' = c*ei - s*er
 *                          formed first, then dey = Ey[i, 0] - that.
 *   the fused build        writes these as explicit fma: re' = fma(c, re, -(s*im)), im' = fma(s, re, c*im), and
 *                          re' = fma(c, er, s*ei), im' = fma(c, ei, -(s*er)); the resident and the streamed path agree.
 *   state without images   Ex, Ey, Jx, Qx, Jy and Qy have no image column and never cross the seam.
 *   the rectangle source   adds to Hz after the H half-step, with complex amplitudes a[n] (float64 re, im) and a complex
 *                          float64 weight w_b[j] per column 0..C-2 of each member (default 1):
 *                              Hz_re = (T)((double)Hz_re + (ar*wr - ai*wi))
 *                              Hz_im = (T)((double)Hz_im + (ar*wi + ai*wr))
 *                          (the fused build: fma(ar, wr, -(ai*wi)) and fma(ar, wi, ai*wr)).
 *   the window DFT         is the real window DFT of fdtd2d_batch_monitor.h on Hz, once for the real part and once for
 *                          the imaginary part, same arithmetic and order; the complex transform is W(re) + i W(im).
 *   the probes             record both parts of Hz.
 *
 * Storage.  The image slot of Hz and Hzx holds the UNROTATED copy of column 0, on the device and in LDS: the thread that
 * owns (i, C-1) recomputes column 0's H update with its own value as the old one and column 0's source weight.  rho is
 * applied where the image is read (the Ey update at j = C-2, and download), conj(rho) to Ey[i, C-2] in column 0's H
 * update.  Every download delivers column C-1 of Hz and Hzx rotated by rho.  Upload, the Hzx transfer and reset write the
 * image slot from column 0 as for any periodic batch.
 *
 * Identities.
 *   (a) With c = 1, s = 0, real amplitudes and unit weights the real parts equal the plain periodic Hz run of
 *       fdtd2d_batch_hz.h value for value (signed zeros aside) and the imaginary parts are zero.
 *   (b) Without a conductivity and without a pole a run is bit-identical, in the exact build, to the Ez Bloch run of
 *       fdtd2d_batch_bloch.h with eps and mu exchanged: Hz = Ez, Ex = -Hx, Ey = -Hy.  Negation commutes with the
 *       rotation exactly.
 *   (c) With sigma = 0, wp2 = 0 and zero state a run is bit-identical to the run without a pole.
 *
 * Capacity of the resident path: 11 arrays in LDS (Hz, Ex, Ey, Hzx twice, then ch, cb, ca) and with a pole 20 (those,
 * cj, and Jx, Qx, Jy, Qy twice); behind them the 4R row factors, the 2 (C-1) float64 source weights, the phasor table
 * and, when they fit too, twice the window accumulators.  At most about 3700 float32 or 1850 float64 cells, and with a
 * pole about 1900 float32 or 950 float64 cells: never more than 4 cells per thread, with a pole never more than 2.
 *
 * While the phase is set these keep working, in either order with it: fdtd2d_batch_set_hz_conductivity,
 * fdtd2d_batch_set_hz_dispersion (which allocates both parts of the state), fdtd2d_batch_set_pml and clearing the layer,
 * fdtd2d_batch_set_materials, _set_eps_window, _set_dft_window, _set_probes, _set_option, _reset (zeroes both parts).
 * fdtd2d_batch_upload, _download and _transfer_ezx move the real parts of (Hz, Ex, Ey) and Hzx,
 * fdtd2d_batch_transfer_hz_dispersion the real parts of the pole state.
 *
 * Refused while the phase is set, before anything changes: a window or a probe touching column C-1 (FDTD2D_E_ARG); the
 * whole-grid fdtd2d_batch_set_dft, fdtd2d_batch_set_point_sources and fdtd2d_batch_run_channels,
 * fdtd2d_batch_set_hz_flux_lines (and this header's phase while such lines are set), fdtd2d_batch_set_polarization to
 * the Ez polarisation, fdtd2d_batch_set_periodic(b, 0), and everything the Hz polarisation refuses without a phase,
 * fdtd2d_batch_set_bloch and the other entry points of the Ez Bloch headers included (all FDTD2D_E_STATE).  Flux lines
 * under the phase are fdtd2d_batch_hz_bloch_flux.h's (fdtd2d_batch_set_hz_bloch_flux_lines); while they are set, turning
 * the phase off is refused (FDTD2D_E_STATE) and a new phase keeps them.  The lattice mode of this polarisation (a second
 * phase, across the rows) is fdtd2d_batch_hz_lattice.h's: it excludes this header's phase and takes its complex traffic
 * through the entry points below.  Not available: adjoints. */
#ifndef FDTD2D_BATCH_HZ_BLOCH_H
#define FDTD2D_BATCH_HZ_BLOCH_H

#include "fdtd2d_batch_bloch.h"
#include "fdtd2d_batch_flux.h"
#include "fdtd2d_batch_hz.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: 1 while the phase of this header is set (FDTD2D_BATCH_INFO_BLOCH stays 0 in the Hz polarisation).
 * _RESIDENT, _RESIDENT_MAX_CELLS and _LDS_BYTES then report the rule above.  The id is 24, the one behind
 * FDTD2D_BATCH_INFO_FLUX_LINE_SOURCES, and is written as that header writes its own. */
enum { FDTD2D_BATCH_INFO_HZ_BLOCH = FDTD2D_BATCH_INFO_FLUX_LDS + 2 };

/* cos_phi, sin_phi: count float64 values each, rounded to the batch dtype.  Needs the Hz polarisation and periodic
 * columns (FDTD2D_E_STATE otherwise), no whole-grid transform, point sources or lines of fdtd2d_batch_hz_flux.h
 * (FDTD2D_E_STATE), no window or probe touching column C-1 and finite values (FDTD2D_E_ARG).  The first call allocates
 * the imaginary Hz, Ex, Ey and Hzx as zero, the unit source weights, the imaginary parts of the monitors that are set
 * and, if a pole is set, the imaginary Jx, Qx, Jy, Qy as zero; a later call changes the rotations alone.  NULL, NULL
 * turns the phase off and frees them: the batch is a plain periodic Hz batch again, its real parts as they are.
 * Synchronous. */
int fdtd2d_batch_set_hz_bloch(fdtd2d_batch_t *b, const double *cos_phi, const double *sin_phi);

/* The source weights: wr, wi of shape (count, C-1), float64, finite; NULL, NULL restores ones.  Needs the phase. */
int fdtd2d_batch_set_hz_bloch_source(fdtd2d_batch_t *b, const double *wr, const double *wi);

/* fdtd2d_batch_run with complex amplitudes: amps_re, amps_im (count x nsteps float64 each; amps_im NULL = zero; both
 * NULL = no source).  fdtd2d_batch_run and fdtd2d_batch_run_waveform on such a batch are this call with a zero imaginary
 * part. */
int fdtd2d_batch_run_hz_bloch(fdtd2d_batch_t *b, int nsteps, const double *amps_re, const double *amps_im);

/* Moves the imaginary parts (host shapes as fdtd2d_batch_upload's; any pointer may be NULL); to_device != 0: host to
 * device, the image slots of Hz and Hzx taken from column 0. */
int fdtd2d_batch_transfer_hz_bloch(fdtd2d_batch_t *b, void *Hz_im, void *Ex_im, void *Ey_im, void *Hzx_im,
                                   int host_dtype, int to_device);

/* Moves the imaginary parts of the pole state (count x rows x cols each, as stored; any may be NULL).  FDTD2D_E_STATE
 * without the phase or without a pole. */
int fdtd2d_batch_transfer_hz_bloch_dispersion(fdtd2d_batch_t *b, void *jx_im, void *qx_im, void *jy_im, void *qy_im,
                                              int host_dtype, int to_device);

/* fdtd2d_batch_read_dft_window and fdtd2d_batch_read_probes of the imaginary part of Hz. */
int fdtd2d_batch_read_dft_window_hz_bloch(fdtd2d_batch_t *b, double *re, double *im);
int fdtd2d_batch_read_probes_hz_bloch(fdtd2d_batch_t *b, double *out, long long first, long long count_samples);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_HZ_BLOCH_H */
