/* fdtd2d_batch_bloch.h -- a Bloch phase for periodic batches, a companion of fdtd2d_batch_periodic.h.
 *
 * A Bloch batch is a periodic batch whose fields are complex and repeat as F(x + period) = F(x) * e^{i phi}, one phi per
 * member: oblique incidence on a grating, an angle sweep of a metasurface, a band diagram w(k) of a slab.  A sweep is B
 * copies of one unit cell that differ only in phi, stepped in one launch.
 *
 * Definition.  Every complex field is a real part and an imaginary part of the batch dtype T.  Member b has a rotation
 * rho_b = (c_b, s_b) of type T: the float64 cos(phi_b) and sin(phi_b) as given, rounded to T.  Every coefficient (ch,
 * ce, ca, cb, the row factors) is real, so the step of fdtd2d_batch_periodic.h acts on the real part and on the
 * imaginary part separately, operations and order unchanged.  The two parts meet at the seam only:
 *   the image column     Ez[:, C-1] = rho * Ez[:, 0], and likewise Ezx:
 *                            re' = c*re - s*im        im' = s*re + c*im
 *                        two products and one sum each, each rounded to T.  The H half-step at j = C-2 reads this value.
 *   the left neighbour   of column 0 in the E half-step is conj(rho) * Hy[i, C-2]:
 *                            re' = c*hr + s*hi        im' = c*hi - s*hr
 *   the fused build      writes these as explicit fma: re' = fma(c, re, -(s*im)), im' = fma(s, re, c*im), and
 *                        re' = fma(c, hr, s*hi), im' = fma(c, hi, -(s*hr)); the resident and the streamed path agree.
 *   the rectangle source takes complex amplitudes a[n] (float64 re, im) and a complex float64 weight w_b[j] per column
 *                        0..C-2 of each member (default 1):
 *                            Ez_re = (T)((double)Ez_re + (ar*wr - ai*wi))
 *                            Ez_im = (T)((double)Ez_im + (ar*wi + ai*wr))
 *                        (the fused build: fma(ar, wr, -(ai*wi)) and fma(ar, wi, ai*wr)).  With w_b[j] =
 *                        e^{i phi_b j/(C-1)} a line source across the period launches the obliquely travelling wave.
 *   the window DFT       is the real window DFT of fdtd2d_batch_monitor.h, once for the real part and once for the
 *                        imaginary part, same arithmetic and order; the complex transform is W(re) + i W(im).
 *   the probes           record both parts of Ez.
 * With c = 1, s = 0, real amplitudes and unit weights the real part equals a plain periodic batch value for value
 * (signed zeros aside) and the imaginary part is zero.
 *
 * Storage.  The image slot of Ez and Ezx holds the UNROTATED copy of column 0, on the device and in LDS: the thread that
 * owns an image cell recomputes column 0's update with its own value as the old one, so the induction and the two
 * barriers of the periodic kernels carry over.  rho is applied where the image is read (the Hy update at j = C-2, and
 * download), conj(rho) to Hy[i, C-2] in column 0's E update.  Upload, fdtd2d_batch_transfer_ezx and reset write the
 * image slot from column 0 as for any periodic batch.
 *
 * Capacity of the resident path: 11 arrays in LDS (Ez, Hx, Hy, Ezx twice, then cb, ch, ca), the 4R row factors, the
 * 2 (C-1) float64 source weights, the phasor table and, when they fit too, twice the window accumulators: at most
 * about 3700 float32 or 1850 float64 cells, so at most 4 cells per thread.
 *
 * Refused while a Bloch phase is set, before anything changes: a window or a probe touching column C-1 (FDTD2D_E_ARG,
 * naming the member for a probe: the rotation would have to be applied there too); the whole-grid fdtd2d_batch_set_dft
 * (use a window), fdtd2d_batch_set_point_sources and fdtd2d_batch_run_channels, fdtd2d_batch_hold_dft_window and
 * fdtd2d_batch_dft_window_product, fdtd2d_batch_probe_spectra and fdtd2d_batch_field_absmax (all FDTD2D_E_STATE).
 * Their complex counterparts, which an adjoint run of complex fields needs, are in fdtd2d_batch_bloch_adjoint.h.
 * fdtd2d_batch_set_conductivity, _set_conductivity_window, _set_eps_window, _set_pml, _set_option keep working. */
#ifndef FDTD2D_BATCH_BLOCH_H
#define FDTD2D_BATCH_BLOCH_H

#include "fdtd2d_batch_periodic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: 1 while a Bloch phase is set.  _RESIDENT, _RESIDENT_MAX_CELLS and _LDS_BYTES then report the
 * Bloch rule. */
#define FDTD2D_BATCH_INFO_BLOCH 16

/* cos_phi, sin_phi: count float64 values each, rounded to the batch dtype.  Needs periodic columns (FDTD2D_E_STATE
 * otherwise) and no whole-grid transform, point sources or held window (FDTD2D_E_STATE), no window or probe touching
 * column C-1 and finite values (FDTD2D_E_ARG).  The first call allocates the imaginary Ez, Hx, Hy and Ezx as zero, the
 * unit source weights and the imaginary parts of the monitors that are set; a later call changes the rotations alone.
 * NULL, NULL turns the phase off and frees them: the batch is a plain periodic one again, its real parts as they are.
 * fdtd2d_batch_set_periodic(b, 0) turns it off too.  fdtd2d_batch_reset zeroes both parts.  Synchronous. */
int fdtd2d_batch_set_bloch(fdtd2d_batch_t *b, const double *cos_phi, const double *sin_phi);

/* The source weights: wr, wi of shape (count, C-1), float64, finite; NULL, NULL restores ones.  Needs a Bloch phase. */
int fdtd2d_batch_set_bloch_source(fdtd2d_batch_t *b, const double *wr, const double *wi);

/* fdtd2d_batch_run with complex amplitudes: amps_re, amps_im (count x nsteps float64 each; amps_im NULL = zero; both
 * NULL = no source).  fdtd2d_batch_run and fdtd2d_batch_run_waveform on a Bloch batch are this call with a zero
 * imaginary part. */
int fdtd2d_batch_run_bloch(fdtd2d_batch_t *b, int nsteps, const double *amps_re, const double *amps_im);

/* Moves the imaginary parts (host shapes as fdtd2d_batch_upload's; any pointer may be NULL); to_device != 0: host to
 * device, the image slots of Ez and Ezx taken from column 0.  fdtd2d_batch_upload, _download and _transfer_ezx move the
 * real parts.  Every download delivers the image column of Ez and Ezx rotated by rho. */
int fdtd2d_batch_transfer_bloch(fdtd2d_batch_t *b, void *Ez_im, void *Hx_im, void *Hy_im, void *Ezx_im, int host_dtype,
                                int to_device);

/* fdtd2d_batch_read_dft_window and fdtd2d_batch_read_probes of the imaginary part of Ez. */
int fdtd2d_batch_read_dft_window_bloch(fdtd2d_batch_t *b, double *re, double *im);
int fdtd2d_batch_read_probes_bloch(fdtd2d_batch_t *b, double *out, long long first, long long count_samples);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_BLOCH_H */
