/* fdtd2d_batch_lattice.h -- doubly periodic Bloch batches, a companion of fdtd2d_batch_bloch.h.
 *
 * A lattice batch holds unit cells of a rectangular 2D lattice: the fields are complex and repeat along the rows and
 * along the columns, F(r + a_rows) = F(r) e^{i phi_rows} and F(r + a_cols) = F(r) e^{i phi_cols}, one pair of phases
 * per member.  The band structure w(k) of a photonic crystal along a path Gamma-X-M-Gamma is B copies of one unit cell
 * that differ only in (phi_rows, phi_cols), stepped in one launch.
 *
 * Definition.  The member shape is (R, C) and the period Qr = R-1 rows by Qc = C-1 columns: row R-1 is the image of
 * row 0 and column C-1 the image of column 0.  The host shapes are those of every batch: Ez (R, C), Hx (R, C-1),
 * Hy (R-1, C); row R-1 of Hx and column C-1 of Hy are never written.  Every field is a real part and an imaginary
 * part of the batch dtype T.  Member b has two rotations of type T, the float64 cos and sin as given, rounded to T:
 * rho_r = (cr, sr) across the row seam and rho_c = (cc, sc) across the column seam.  Every coefficient is real, so
 * each part takes the same real update; the parts meet at the seams only, through
 *       rho * (re, im):        re' = c*re - s*im        im' = s*re + c*im
 *       conj(rho) * (re, im):  re' = c*re + s*im        im' = c*im - s*re
 * two products and one sum each, each rounded to T (the fused build: fma(c, re, -(s*im)), fma(s, re, c*im) and
 * fma(c, re, s*im), fma(c, im, -(s*re)), as in fdtd2d_batch_bloch.h).  One step, in this order:
 *   H half-step      for 0 <= i <= R-2, 0 <= j <= C-2, per part, with ch = dt / (mu dx):
 *                        Hx[i,j] = Hx[i,j] - ch[i,j] * (Ez[i+1,j] - Ez[i,j])
 *                        Hy[i,j] = Hy[i,j] + ch[i,j] * (Ez[i,j+1] - Ez[i,j])
 *                    where Ez[R-1,j] is rho_r * Ez[0,j] and Ez[i,C-1] is rho_c * Ez[i,0] (the corner is never read);
 *                    the fused build evaluates fma(-ch, d, Hx) and fma(ch, d, Hy).
 *   E half-step      for 0 <= i <= R-2, 0 <= j <= C-2 (row 0 is updated: there is no PEC row), per part:
 *                        dhy = Hy[i,j] - Hy[i,j-1]      dhx = Hx[i,j] - Hx[i-1,j]
 *                        Ez[i,j] = ca[i,j] * Ez[i,j] + (dhy - dhx) * cb[i,j]
 *                    where Hy[i,-1] is conj(rho_c) * Hy[i,C-2] and Hx[-1,j] is conj(rho_r) * Hx[R-2,j]; ca and cb are
 *                    those of fdtd2d_batch_lossy.h (the fused build: fma(dhy - dhx, cb, ca * Ez)).
 *   rectangle source the Bloch one: complex amplitudes, the complex float64 weight per column 0..C-2 (default 1):
 *                        Ez_re = (T)((double)Ez_re + (ar*wr - ai*wi))     Ez_im = (T)((double)Ez_im + (ar*wi + ai*wr))
 *   images           Ez[i,C-1] = rho_c * Ez[i,0], Ez[R-1,j] = rho_r * Ez[0,j], and the corner
 *                    Ez[R-1,C-1] = rho_r * (rho_c * Ez[0,0]): the column rotation first, each rotation rounded to T.
 *   monitors         the window DFT and the probes of each part, as for a Bloch batch.
 * With rho_r = rho_c = (1, 0), real amplitudes and unit weights the imaginary part stays zero.
 *
 * There is no layer, no PEC row and no Ezx in this mode.  A conductivity may be non-zero anywhere in rows 0..R-2 and
 * columns 0..C-2: there is no margin, because there is no edge.  eps, mu and sigma at row R-1 or column C-1 are
 * accepted and never read.  fdtd2d_batch_set_eps_window keeps refusing a window that holds cell [0, 0].
 *
 * Storage.  As in fdtd2d_batch_bloch.h the image slots of Ez hold the UNROTATED copies of row 0 and of column 0 (the
 * corner: of cell (0, 0)), on the device and in LDS; the thread that owns an image cell recomputes its source cell's
 * update with its own value as the old one, so the images stay bit-identical to their source cells with two barriers
 * per step, and the streamed E kernel runs in place.  The rotations are applied where an image is read and on
 * download.  Upload and reset write the image slots from row 0 and column 0.
 *
 * Capacity of the resident path: 9 arrays in LDS (Ez, Hx, Hy twice, then cb, ch, ca), the 2 (C-1) float64 source
 * weights, the phasor table and, when they fit too, twice the window accumulators: at most about 4500 float32 or 2270
 * float64 cells.  FDTD2D_BATCH_INFO_RESIDENT, _RESIDENT_MAX_CELLS and _LDS_BYTES report this rule while the mode is on.
 *
 * Calls that serve a lattice batch as they serve a Bloch batch (fdtd2d_batch_bloch.h, fdtd2d_batch_bloch_adjoint.h):
 *   fdtd2d_batch_run_bloch                 complex amplitudes; fdtd2d_batch_run and fdtd2d_batch_run_waveform are this
 *                                          call with a zero imaginary part
 *   fdtd2d_batch_transfer_bloch            the imaginary parts; Ezx_im must be NULL (FDTD2D_E_STATE otherwise).  Upload
 *                                          (this call and fdtd2d_batch_upload) writes the images from row 0 and
 *                                          column 0; every download delivers the rotated images as defined above
 *   fdtd2d_batch_set_bloch_source          the source weights
 *   fdtd2d_batch_read_dft_window_bloch, fdtd2d_batch_read_probes_bloch     the imaginary part's monitors
 *   fdtd2d_batch_bloch_probe_spectra, fdtd2d_batch_bloch_field_absmax      these read stored data only (the latter
 *                                          over rows 0..R-2 and columns 0..C-2)
 * fdtd2d_batch_info(FDTD2D_BATCH_INFO_BLOCH) stays 0: it reports the phase of fdtd2d_batch_set_bloch.
 *
 * Refused while the mode is on (FDTD2D_E_STATE), before anything changes: fdtd2d_batch_set_pml with a layer (without
 * one it is accepted and changes nothing), fdtd2d_batch_transfer_ezx, fdtd2d_batch_set_bloch,
 * fdtd2d_batch_set_dispersion and _set_dispersion_window, fdtd2d_batch_set_dft, and every point-source, channel,
 * held-window and product call, real or Bloch (fdtd2d_batch_set_point_sources, _run_channels, _hold_dft_window,
 * _dft_window_product, _probe_spectra, _field_absmax, _set_bloch_point_sources, _run_bloch_channels, _hold_bloch_window,
 * _bloch_window_product).  Adjoint runs of lattice batches are not provided.  A window or a probe that touches row R-1
 * or column C-1 and a source rectangle that reaches row R-1 or column C-1 are refused with FDTD2D_E_ARG.
 * fdtd2d_batch_set_conductivity, _set_conductivity_window, _set_eps_window, _set_materials, _set_option and _reset keep
 * working. */
#ifndef FDTD2D_BATCH_LATTICE_H
#define FDTD2D_BATCH_LATTICE_H

#include "fdtd2d_batch_bloch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cos_r, sin_r, cos_c, sin_c: count float64 values each, rounded to the batch dtype: rho_r = (cos_r, sin_r) across the
 * row seam, rho_c = (cos_c, sin_c) across the column seam.  Needs periodic columns (fdtd2d_batch_set_periodic) and
 * materials.  The first call allocates the imaginary Ez, Hx and Hy as zero, the unit source weights and the imaginary
 * parts of the monitors that are set, and copies row 0 and column 0 of Ez over the image slots; a later call changes
 * the rotations alone.  All four NULL turns the mode off and frees them: the batch is a plain periodic one again (PEC
 * rows, no layer), its real parts as they are; that is refused (FDTD2D_E_ARG) while a conductivity is non-zero where a
 * periodic batch allows none.  fdtd2d_batch_set_periodic(b, 0) turns the mode off too.
 * Refused before anything changes.  FDTD2D_E_STATE: no periodic columns, no materials, a layer, a Bloch phase set with
 * fdtd2d_batch_set_bloch, a dispersive pole, the whole-grid transform, point sources, or a held window.  FDTD2D_E_ARG,
 * naming the member where there is one: some but not all pointers NULL; a non-finite value; a window or a probe that
 * touches row R-1 or column C-1; a source rectangle that reaches row R-1.  Synchronous. */
int fdtd2d_batch_set_lattice(fdtd2d_batch_t *b, const double *cos_r, const double *sin_r, const double *cos_c,
                             const double *sin_c);

/* 1 while the lattice mode is on, 0 otherwise; FDTD2D_E_ARG for NULL. */
int fdtd2d_batch_is_lattice(const fdtd2d_batch_t *b);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_LATTICE_H */
