/* fdtd2d_batch_bloch_flux.h -- flux monitors for batches with a Bloch phase, a companion of fdtd2d_batch_flux.h and
 * fdtd2d_batch_bloch.h.
 *
 * A batch with periodic columns and a Bloch phase (fdtd2d_batch_set_bloch), with or without the pole of
 * fdtd2d_batch_set_bloch_dispersion, can carry the flux lines of fdtd2d_batch_flux.h on its complex fields: transmitted,
 * reflected and absorbed power against the angle of incidence, one k-point per member.  The lines never change the
 * fields, the window DFT or the probes, and a monitored resident run is still one launch, a streamed one still two
 * launches per step.
 *
 * Definitions.
 *   lines       Geometry, limits and sampling are those of fdtd2d_batch_flux.h for a batch with periodic columns: up to
 *               4 lines at up to 16 frequencies; row lines {0, row i, first column, count} at rows 1..R-2 within columns
 *               0..C-2; column lines {1, column j, first row, count} at columns 0..C-2 (the image column C-1 is refused);
 *               every `every`-th completed step n counted from the call, after the source of the step, t = n dt.
 *               The frequencies may have either sign: with complex fields omega and -omega are different spectra.
 *   sums        At a sampled step n every line cell adds, in float64 and with the one phasor exp(-i omega_k n dt), Ez
 *               and Ht of the real part and Ez and Ht of the imaginary part: two blocks of the layout of
 *               fdtd2d_batch_flux.h (Ez re[nfreq][cells], Ez im, Ht re, Ht im), one per part.
 *   Ht          row line:    Ht = 0.5 ((double)Hx[i-1,j] + (double)Hx[i,j])              on each part
 *               column line: Ht = 0.5 ((double)Hy[i,j-1] + (double)Hy[i,j])              on each part
 *               At column 0 the left neighbour lies across the seam.  It is the value the E half-step itself subtracts:
 *               conj(rho) Hy[i, C-2], re' = c hr + s hi, im' = c hi - s hr, evaluated in the batch dtype in the build's
 *               own form (fused multiply-adds in the fused build), then widened.  Rows 0 and R-1, which the step does not
 *               update, evaluate it the same way.
 *   spectra     E_k = Er_k + i Ei_k with Er_k, Ei_k the complex sums of the two parts; H_k likewise.
 *   flux        Per member, line and frequency: P = s dx sum_cells Re(E_k conj(H_k exp(+i omega_k dt / 2))), s = +1
 *               for a row line and -1 for a column line, cells in ascending order, no factor 1/2 and no normalisation;
 *               formed on the device by one launch (one workgroup per member, one thread per line and frequency).
 *
 * Scope.  FDTD2D_E_STATE without a Bloch phase, in the lattice mode, on a batch created with the Mur frame or without
 * periodic columns, while Bloch point sources or a held Bloch window are set, and without materials.  While Bloch lines
 * are set, turning the phase off, the lattice mode, switching periodic columns, fdtd2d_batch_set_bloch_point_sources,
 * fdtd2d_batch_run_bloch_channels and fdtd2d_batch_hold_bloch_window are refused with FDTD2D_E_STATE (the last two until
 * line sources are installed on the lines: fdtd2d_batch_bloch_flux_adjoint.h).  A new phase
 * keeps the lines and their sums, and so do fdtd2d_batch_set_bloch_dispersion and the removal of the pole: the batch
 * switches kernel family.  fdtd2d_batch_set_flux_lines keeps refusing a batch with a Bloch phase; the real lines'
 * fdtd2d_batch_read_flux_lines and fdtd2d_batch_flux refuse Bloch lines (FDTD2D_E_STATE).
 *
 * Ids.  FDTD2D_BATCH_INFO_FLUX_LINES reports the number of lines of either kind and FDTD2D_BATCH_INFO_FLUX_LDS their
 * placement; FDTD2D_BATCH_OPT_FLUX_LDS forces either kind's sums into global memory.  This header adds no id.
 *
 * Capacity.  The resident path holds the lines' phasor table, 16*nfreq bytes, behind the window's.  The 64*nfreq*cells
 * bytes of sums (both parts) live in LDS behind both window accumulators when they fit in the 160 KiB too, otherwise in
 * global memory.  Every sum takes the same float64 additions in the same order on every path, placement and launch
 * split. */
#ifndef FDTD2D_BATCH_BLOCH_FLUX_H
#define FDTD2D_BATCH_BLOCH_FLUX_H

#include "fdtd2d_batch_bloch.h"
#include "fdtd2d_batch_flux.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lines: nlines x {orientation (0 row, 1 column), index, first, count}; omega: count x nfreq.  nlines = 0 removes the
 * lines (the other arguments are then ignored).  The sums start at zero and the step count at this call.
 * FDTD2D_E_ARG, before any device work and with the previous lines left in place, as fdtd2d_batch_set_flux_lines
 * refuses its arguments; FDTD2D_E_STATE as under "Scope".  The new buffers are made before the old ones are released.
 * Synchronous. */
int fdtd2d_batch_set_bloch_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                      int every);
/* The raw sums of one part of the field (part 0: real, 1: imaginary), each count x nfreq x cells (cells: the lines'
 * counts together, lines concatenated in the order given): the transform of that part's Ez into ez_re, ez_im and of its
 * Ht (without the half-step factor) into ht_re, ht_im.  FDTD2D_E_ARG for another part, FDTD2D_E_STATE without Bloch
 * lines.  Synchronous. */
int fdtd2d_batch_read_bloch_flux_lines(fdtd2d_batch_t *b, int part, double *ez_re, double *ez_im, double *ht_re,
                                       double *ht_im);
/* out: count x nlines x nfreq float64, P as defined above.  FDTD2D_E_STATE without Bloch lines.  Synchronous. */
int fdtd2d_batch_bloch_flux(fdtd2d_batch_t *b, double *out);

/* fdtd2d_batch_reset zeroes the sums and restarts their count at step 0. */

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_BLOCH_FLUX_H */
