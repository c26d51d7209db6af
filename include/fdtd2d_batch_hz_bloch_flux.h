/* fdtd2d_batch_hz_bloch_flux.h -- flux monitors for periodic batches in the Hz polarisation with a Bloch phase, a
 * companion of fdtd2d_batch_hz_bloch.h, fdtd2d_batch_hz_flux.h and fdtd2d_batch_bloch_flux.h.
 *
 * An Hz Bloch batch (fdtd2d_batch_set_hz_bloch: complex Hz, Ex, Ey, one phase per member) can carry the flux lines of
 * fdtd2d_batch_flux.h, with or without fdtd2d_batch_set_hz_conductivity and fdtd2d_batch_set_hz_dispersion, on the
 * resident and the streamed path: the power through a line per k-point, hence T, R and A of a metal grating with the
 * electric field in the plane under oblique incidence, and its diffraction efficiencies.  The lines never change the
 * fields; a monitored resident run is still one launch, a streamed one still two launches per step.
 *
 * Lines.  The geometry, the limits (FDTD2D_BATCH_MAX_FLUX_LINES, FDTD2D_BATCH_MAX_FLUX_FREQS), `every`, the sampling rule,
 * the placement option and the reset rule are those of fdtd2d_batch_flux.h for a batch with periodic columns: row lines at
 * rows 1..R-2 within columns 0..C-2, column lines at columns 0..C-2; the image column C-1 is refused.  The frequencies may
 * have either sign: omega and -omega are different spectra of a complex field, as on the lines of
 * fdtd2d_batch_bloch_flux.h.
 *
 * Sums.  At a sampled step n, after the step's source and the image column, every line cell adds in float64, with the one
 * phasor exp(-i omega_k n dt) of fdtd2d_batch_flux.h:
 *     Hz and Et of the real part of the fields       (one block of the BatchFlux layout, in flux_acc)
 *     Hz and Et of the imaginary part                (a second block of the same layout, in flux_acc_im)
 * As in fdtd2d_batch_hz_flux.h the "Ez" arrays of a block hold the transform of Hz and its "Ht" arrays that of Et.  On
 * each part
 *     row line:     Et = 0.5 ((double)Ex[i-1,j] + (double)Ex[i,j])
 *     column line:  Et = 0.5 ((double)Ey[i,j-1] + (double)Ey[i,j])
 * At column 0 the left neighbour lies across the seam: it is the value the H half-step itself subtracts,
 *     batch_bloch_unrot(c, s, Ey_re[i,C-2], Ey_im[i,C-2]):   re' = c*er + s*ei,   im' = c*ei - s*er
 * evaluated in the batch dtype in the build's own form (the fused build: re' = fma(c, er, s*ei), im' = fma(c, ei,
 * -(s*er))), then widened.  It is evaluated the same way on rows 0 and R-1, where the step skips the update.  The slots
 * Ex[:,C-1] and Ey[R-1,:], which no update writes, are read as stored.  Ex and Ey are those of step n's E half-step.
 *
 * Spectra and flux.  H_k = Hr_k + i Hi_k with Hr_k, Hi_k the (complex) sums of the real and of the imaginary part, and
 * E_k likewise.  That E lives at (n - 1/2) dt, so per member, line and frequency
 *     P = s dx sum_cells Re(H_k conj(E_k exp(+i omega_k dt / 2))),   s = -1 on a row line, +1 on a column line,
 * the cells in ascending order: sum = 0.0; sum = sum + (hr*xr + hi*xi) with x = E_k (gc + i gs), xr = er*gc - ei*gs,
 * xi = er*gs + ei*gc.  No factor 1/2 and no normalisation.  One launch forms P, one workgroup per member and one thread
 * per line and frequency.  The half-step factor is applied there, never in the sums.
 *
 * Identities.
 *   (a) With c = 1, s = 0, real amplitudes and unit weights the real part's sums equal those of
 *       fdtd2d_batch_set_hz_flux_lines on the plain periodic Hz run, and the imaginary part's sums are zero.
 *   (b) Without a conductivity and without a pole the sums and P are bit-identical (exact build) to those of
 *       fdtd2d_batch_set_bloch_flux_lines on the Ez Bloch run with eps and mu exchanged: H_k = its E_k, E_k = -its H_k,
 *       P equal.
 *   (c) Every sum takes the same float64 additions in the same order on every path, placement and launch split.
 *
 * Scope.  The lines need the phase of fdtd2d_batch_set_hz_bloch (hence the Hz polarisation and periodic columns) and
 * materials: FDTD2D_E_STATE otherwise, before anything changes.  While they are set, turning the phase off is refused
 * (FDTD2D_E_STATE); a new phase, fdtd2d_batch_set_hz_conductivity and fdtd2d_batch_set_hz_dispersion, before or after the
 * lines, keep the lines and their sums: the batch only switches between the two kernel instances.  Everything the phase
 * refuses stays refused: fdtd2d_batch_set_hz_flux_lines under the phase, fdtd2d_batch_set_hz_bloch while such lines are
 * set, fdtd2d_batch_set_flux_lines and fdtd2d_batch_set_bloch_flux_lines on an Hz batch.  fdtd2d_batch_read_flux_lines,
 * fdtd2d_batch_flux and the reads of fdtd2d_batch_hz_flux.h and fdtd2d_batch_bloch_flux.h refuse these lines, naming this
 * header's call.  Not available: line sources and adjoints on these lines.
 *
 * The kernels.  A batch with these lines takes the kernels of kernels_batch_hz_bloch_flux.hpp: those of
 * fdtd2d_batch_hz_bloch.h step for step, plus the sums, taken in the H phase by the thread that owns the cell.
 *
 * Capacity.  The rule of fdtd2d_batch_hz_bloch.h stands (11 arrays, 20 with a pole, the row factors, the source weights,
 * the window's phasor table); the lines' phasor table, 16*nfreq bytes, sits behind the window's and counts in the rule.
 * The 64*nfreq*cells bytes of sums (both parts; cells: all lines together) live in LDS behind both window accumulators
 * when they fit in the 160 KiB too, otherwise in global memory.  No new info id: FDTD2D_BATCH_INFO_FLUX_LINES,
 * FDTD2D_BATCH_INFO_FLUX_LDS and FDTD2D_BATCH_OPT_FLUX_LDS of fdtd2d_batch_flux.h serve these lines, and
 * FDTD2D_BATCH_INFO_RESIDENT_MAX_CELLS and _LDS_BYTES count their table and sums. */
#ifndef FDTD2D_BATCH_HZ_BLOCH_FLUX_H
#define FDTD2D_BATCH_HZ_BLOCH_FLUX_H

#include "fdtd2d_batch_flux.h"
#include "fdtd2d_batch_hz_bloch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lines: nlines x {orientation (0 row, 1 column), index, first, count}; omega: count x nfreq, either sign.  nlines = 0
 * removes the lines (the other arguments are then ignored).  The sums of both parts start at zero and the step count at
 * this call.  FDTD2D_E_ARG, before any device work and with the previous lines left in place, for the arguments that
 * fdtd2d_batch_set_flux_lines refuses on a periodic batch.  The new buffers are made before the old ones are released.
 * FDTD2D_E_STATE as under "Scope".  Synchronous. */
int fdtd2d_batch_set_hz_bloch_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                         int every);
/* The raw sums of one part of the fields (part 0: real, 1: imaginary), each count x nfreq x cells (cells: the lines'
 * counts together, lines concatenated in the order given): the transform of Hz into hz_re, hz_im and that of Et (without
 * the half-step factor) into et_re, et_im.  FDTD2D_E_STATE without these lines, FDTD2D_E_ARG for another part.
 * Synchronous. */
int fdtd2d_batch_read_hz_bloch_flux_lines(fdtd2d_batch_t *b, int part, double *hz_re, double *hz_im, double *et_re,
                                          double *et_im);
/* out: count x nlines x nfreq float64, P as defined above, formed on the device by one launch from the sums of both
 * parts.  FDTD2D_E_STATE without these lines.  Synchronous. */
int fdtd2d_batch_hz_bloch_flux(fdtd2d_batch_t *b, double *out);

/* fdtd2d_batch_reset zeroes the sums of both parts and restarts their count at step 0. */

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_HZ_BLOCH_FLUX_H */
