/* fdtd2d_batch_hz_lattice.h -- the lattice mode of the Hz polarisation: doubly periodic Bloch batches with the electric
 * field in the plane, a companion of fdtd2d_batch_lattice.h and fdtd2d_batch_hz_bloch.h.
 *
 * An Hz lattice batch is a periodic batch in the Hz polarisation (fdtd2d_batch_set_polarization(b, FDTD2D_POL_HZ) on
 * periodic columns) whose every member is one unit cell of a rectangular lattice: its fields are complex and repeat as
 * F(x + a_r) = F(x) e^{i phi_r} down the rows and F(x + a_c) = F(x) e^{i phi_c} along the columns, one pair of phases
 * per member.  It gives the second band structure of a 2D photonic crystal, the one with E across the rods; with the
 * conductivity and the Drude-Lorentz pole of fdtd2d_batch_hz.h, which act on Ex and Ey, the bands of a metallic crystal
 * that no exchange of eps and mu on an Ez lattice batch can give.  It has no layer.
 *
 * Shapes.  The member shape is (R, C) and the period is R-1 by C-1.  Row R-1 of Hz is the image of row 0, column C-1 the
 * image of column 0 and the corner the image of (0, 0).  Host shapes are every batch's: Hz (R, C), Ex (R, C-1),
 * Ey (R-1, C).  Row R-1 of Ex and column C-1 of Ey are never written.
 *
 * Fields.  Hz, Ex, Ey and, with a pole, Jx, Qx, Jy, Qy are pairs (re, im) of the batch dtype T.  There is no Hzx and
 * there are no row factors.
 *
 * Rotations.  rho_r = (cr, sr) acts across the row seam and rho_c = (cc, sc) across the column seam: each the float64
 * cos and sin as given, rounded to T.  rho * (re, im) is re' = c*re - s*im, im' = s*re + c*im and conj(rho) * (re, im)
 * is re' = c*re + s*im, im' = c*im - s*re: two products and one sum each, each rounded to T; the fused build writes
 * them as fma(c, re, -(s*im)), fma(s, re, c*im), fma(c, re, s*im), fma(c, im, -(s*re)).  These are exactly the forms
 * of fdtd2d_batch_lattice.h.
 *
 * One step is the E half-step, the H half-step, then the source, as in fdtd2d_batch_hz.h.  Every cell is a material
 * cell.
 *   E half-step, 0 <= i <= R-2 and 0 <= j <= C-2, per part:
 *       dxi = Hz[i+1, j] - Hz[i, j]        dyj = Hz[i, j+1] - Hz[i, j]
 *     where Hz[R-1, j] is rho_r * (image slot) and Hz[i, C-1] is rho_c * (image slot), each formed first; the corner is
 *     never read.  The updates of Ex and Ey, with and without the pole, are the material-cell lines of fdtd2d_batch_hz.h
 *     unchanged:
 *       jx = a*Jx + (cj*Ex - ck*Qx);  Qx = Qx + jx;  Ex = ca*Ex + (dxi - jx)*cb;  Jx = jx
 *       jy = a*Jy + (cj*Ey - ck*Qy);  Qy = Qy + jy;  Ey = ca*Ey - (dyj + jy)*cb;  Jy = jy
 *     (without a pole jx = jy = 0 and no state), and so are their fused forms.
 *   H half-step, 0 <= i <= R-2 and 0 <= j <= C-2, per part; row 0 is updated, there is no fixed row in this mode:
 *       dey = Ey[i, j] - Ey[i, j-1]        dex = Ex[i, j] - Ex[i-1, j]
 *     where Ey[i, -1] = conj(rho_c) * Ey[i, C-2] and Ex[-1, j] = conj(rho_r) * Ex[R-2, j], each formed first;
 *       Hz = Hz - (dey - dex)*ch,
 *     with the fused form of fdtd2d_batch_hz.h.
 *   Source: that of fdtd2d_batch_hz_bloch.h.  Complex amplitudes a[n] and a complex float64 weight per column 0..C-2 are
 *     added to Hz through float64: Hz_re = (T)((double)Hz_re + (ar*wr - ai*wi)), Hz_im = (T)((double)Hz_im + (ar*wi +
 *     ai*wr)).
 *   Images: Hz[i, C-1] = rho_c * Hz[i, 0], Hz[R-1, j] = rho_r * Hz[0, j], the corner rho_r * (rho_c * Hz[0, 0]).  Ex, Ey
 *     and the pole state have no images.
 *   Monitors: the window DFT and the probes of each part of Hz, as in fdtd2d_batch_hz_bloch.h.
 *
 * Storage follows both parent headers.  The image slots of Hz hold the UNROTATED copies, on the device and in LDS: the
 * thread that owns an image cell recomputes its source cell's H update, including its source, with its own value as the
 * old one.  The rotations are applied where an image is read and on download.  Upload and reset write the image slots
 * from row 0 and column 0.
 *
 * Materials.  fdtd2d_batch_set_hz_conductivity and fdtd2d_batch_set_hz_dispersion may be non-zero anywhere in rows
 * 0..R-2 and columns 0..C-2 while the mode is on: there is no margin, because there is no edge.  They may be set before
 * or after the mode; set before, the periodic rule held them, which is a subset.
 *
 * Identities.
 *   (a) With both rotations (1, 0), real amplitudes and unit weights the imaginary parts stay zero.
 *   (b) Without a conductivity and without a pole a run is bit-identical, in the exact build, to the Ez lattice run of
 *       fdtd2d_batch_lattice.h with eps and mu exchanged: Hz = Ez, Ex = -Hx, Ey = -Hy.
 *   (c) With sigma = 0, wp2 = 0 and zero state a run is bit-identical to the run without a pole.
 *   (d) The transposed member with its two phases exchanged gives Hz^T, Ex = -Ey^T, Ey = -Ex^T and the state likewise,
 *       bit for bit in the exact build: every negation commutes with every rounding in the step.  This holds for unit
 *       source weights, which do not depend on the row.
 *   (e) Negating both phases conjugates every field.
 *
 * Capacity of the resident path: 9 arrays in LDS (Hz, Ex, Ey twice, then ch, cb, ca) and with a pole 18 (those, cj, and
 * Jx, Qx, Jy, Qy twice); behind them the 2 (C-1) float64 source weights, the phasor table and, when they fit too, twice
 * the window accumulators.  About 4500 float32 or 2270 float64 cells, and with a pole about 2270 float32 or 1130 float64
 * cells: a 32x32-cell unit cell with a metal stays resident in float64.
 *
 * The complex traffic goes through the entry points of fdtd2d_batch_hz_bloch.h, which serve this mode as they serve the
 * phase: fdtd2d_batch_run_hz_bloch (fdtd2d_batch_run and _run_waveform mean a zero imaginary part),
 * fdtd2d_batch_transfer_hz_bloch (Hzx_im must be NULL, else FDTD2D_E_STATE), fdtd2d_batch_transfer_hz_bloch_dispersion,
 * fdtd2d_batch_set_hz_bloch_source, fdtd2d_batch_read_dft_window_hz_bloch and fdtd2d_batch_read_probes_hz_bloch.
 * fdtd2d_batch_upload, _download and fdtd2d_batch_transfer_hz_dispersion move the real parts.  Every download delivers
 * the images rotated as defined.
 *
 * Refused while the mode is on, before anything changes (FDTD2D_E_STATE): fdtd2d_batch_set_pml with a layer and
 * fdtd2d_batch_transfer_ezx; fdtd2d_batch_set_hz_bloch; fdtd2d_batch_set_hz_flux_lines and
 * fdtd2d_batch_set_hz_bloch_flux_lines; fdtd2d_batch_set_dft, fdtd2d_batch_set_point_sources and
 * fdtd2d_batch_run_channels; fdtd2d_batch_set_polarization to Ez and fdtd2d_batch_set_periodic(b, 0); and everything the
 * Hz polarisation refuses anyway, fdtd2d_batch_set_lattice and every Ez Bloch or lattice entry point included
 * (fdtd2d_batch_is_lattice and FDTD2D_BATCH_INFO_BLOCH stay 0).  Windows, probes and source rectangles at the image row
 * or column are refused with FDTD2D_E_ARG.
 *
 * Not available: flux lines in this mode, point sources and channels, every adjoint, fdtd2d_batch_bloch_probe_spectra and
 * fdtd2d_batch_bloch_field_absmax for Hz batches, the window patchers, the single-grid engine of fdtd2d.h. */
#ifndef FDTD2D_BATCH_HZ_LATTICE_H
#define FDTD2D_BATCH_HZ_LATTICE_H

#include "fdtd2d_batch_hz_bloch.h"
#include "fdtd2d_batch_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: 1 while the mode of this header is on (FDTD2D_BATCH_INFO_BLOCH and FDTD2D_BATCH_INFO_HZ_BLOCH stay
 * 0).  _RESIDENT, _RESIDENT_MAX_CELLS and _LDS_BYTES then report the rule above.  The id is 25, the one behind
 * FDTD2D_BATCH_INFO_HZ_BLOCH, and is written relative to it. */
enum { FDTD2D_BATCH_INFO_HZ_LATTICE = FDTD2D_BATCH_INFO_HZ_BLOCH + 1 };

/* cos_r, sin_r, cos_c, sin_c: count float64 values each, rounded to the batch dtype.  Needs the Hz polarisation,
 * periodic columns and materials, and no layer, phase of fdtd2d_batch_set_hz_bloch, flux lines of either Hz header,
 * whole-grid transform or point sources (FDTD2D_E_STATE otherwise); all four pointers or none, finite values, no window
 * or probe touching row R-1 or column C-1 and no source rectangle reaching them (FDTD2D_E_ARG, naming the member where
 * there is one).  The first call allocates the imaginary Hz, Ex, Ey as zero, the imaginary Jx, Qx, Jy, Qy if a pole is
 * set, the imaginary parts of the monitors that are set and the unit source weights, and writes the image slots; a
 * later call changes the rotations alone and keeps fields, pole and monitors.  All four NULL turns the mode off and
 * frees them: the batch is a plain periodic Hz batch again, its real parts as they are; that is refused with
 * FDTD2D_E_ARG while sigma or wp2 is non-zero where a periodic Hz batch allows none.  Synchronous. */
int fdtd2d_batch_set_hz_lattice(fdtd2d_batch_t *b, const double *cos_r, const double *sin_r, const double *cos_c,
                                const double *sin_c);

/* 1 while the mode is on, else 0 */
int fdtd2d_batch_is_hz_lattice(const fdtd2d_batch_t *b);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_HZ_LATTICE_H */
