/* fdtd2d_batch_hz_flux.h -- flux monitors for batched grids in the Hz polarisation, a companion of fdtd2d_batch_hz.h and
 * fdtd2d_batch_flux.h.
 *
 * A batch in the Hz polarisation (fdtd2d_batch_set_polarization) with a PML layer or with periodic columns can carry the
 * flux lines of fdtd2d_batch_flux.h, carried through the duality Hz = Ez, Ex = -Hx, Ey = -Hy: on the line cells the step
 * kernels accumulate the running Fourier transforms of Hz and of the tangential E centred on the same cells, and one
 * kernel forms the power that crosses each line per frequency.  They work with and without fdtd2d_batch_set_hz_conductivity
 * and fdtd2d_batch_set_hz_dispersion, on the resident and the streamed path.  The lines never change the fields, and a
 * monitored resident run is still one launch, a streamed one still two launches per step.
 *
 * The line geometry and its bounds, `every`, the sampling rule, the frequency table, the limits (FDTD2D_BATCH_MAX_FLUX_LINES,
 * FDTD2D_BATCH_MAX_FLUX_FREQS), the placement option and the reset rule are those of fdtd2d_batch_flux.h.  What differs:
 *   axes        Columns are x, rows are y: Ex += ce (Hz[i+1,j] - Hz[i,j]), Ey -= ce (Hz[i,j+1] - Hz[i,j]) and
 *               Hz -= ch (dEy - dEx).  Hence S_y = -Ex Hz and S_x = Ey Hz.
 *   sums        At a sampled step n, after the sources of that step and the image column, for every line cell and
 *               frequency k, in float64:
 *                   H_k += Hz exp(-i omega_k n dt)       Hz as stored, widened to double
 *                   E_k += Et exp(-i omega_k n dt)       the same phasor
 *               row line:    Et = 0.5 ((double)Ex[i-1,j] + (double)Ex[i,j])
 *               column line: Et = 0.5 ((double)Ey[i,j-1] + (double)Ey[i,j]); with periodic columns the left
 *               neighbour of column 0 is column C-2.  This is fdtd2d_batch_flux.h's Ht applied to the Hx slot (which
 *               holds Ex) and the Hy slot (which holds Ey); the slots Ex[:,C-1] and Ey[R-1,:], which no update writes,
 *               are read as they are stored.  Ex and Ey are those of step n's E half-step, the ones its H half-step reads.
 *   half step   That E lives at (n - 1/2) dt, so the physical spectrum is E_k exp(+i omega_k dt / 2).  The factor is
 *               applied where the flux is formed (fdtd2d_batch_hz_flux), never in the sums:
 *               fdtd2d_batch_read_hz_flux_lines returns them raw.
 *   flux        Per member, line and frequency: P = s dx sum_cells Re(H_k conj(E_k exp(+i omega_k dt / 2))), s = -1
 *               for a row line and +1 for a column line, cells in ascending order.  A row line still counts power
 *               towards increasing row and a column line towards increasing column.  No factor 1/2 and no
 *               normalisation: users take ratios.
 *
 * Identity.  With no conductivity and no pole, the sums and the flux are bit-identical (exact build) to those of
 * fdtd2d_batch_flux.h on the Ez run of the same batch with eps and mu exchanged: H_k = its E_k, E_k = -its H_k, P equal.
 *
 * Scope.  FDTD2D_E_STATE outside the Hz polarisation, without a layer or periodic columns, and without materials.  While
 * these lines are set, fdtd2d_batch_set_polarization to Ez, removing the layer of a batch without periodic columns and
 * switching periodic columns are refused with FDTD2D_E_STATE.  fdtd2d_batch_set_flux_lines,
 * fdtd2d_batch_set_bloch_flux_lines and fdtd2d_batch_set_flux_line_sources keep refusing a batch in the Hz polarisation,
 * and fdtd2d_batch_read_flux_lines and fdtd2d_batch_flux refuse these lines.
 *
 * The kernels.  A batch with these lines takes the kernels of kernels_batch_hz_flux.hpp: those of fdtd2d_batch_hz.h step
 * for step, plus the sums.  An Hz batch always holds coefficient arrays and ca, so its arrays do not change with the lines.
 *
 * Capacity.  The resident path holds the lines' phasor table, 16*nfreq bytes, behind the window's: arrays (7, or 12 with a
 * pole) + factors + tables <= 160 KiB is the capacity rule.  The 32*nfreq*cells bytes of sums (cells: all lines together)
 * live in LDS behind the window's accumulators when they fit too, otherwise in global memory.
 * FDTD2D_BATCH_INFO_FLUX_LINES, FDTD2D_BATCH_INFO_FLUX_LDS and FDTD2D_BATCH_OPT_FLUX_LDS of fdtd2d_batch_flux.h serve
 * these lines too, and FDTD2D_BATCH_INFO_RESIDENT_MAX_CELLS and _LDS_BYTES count their table and sums.  Every sum takes
 * the same float64 additions in the same order on every path and placement. */
#ifndef FDTD2D_BATCH_HZ_FLUX_H
#define FDTD2D_BATCH_HZ_FLUX_H

#include "fdtd2d_batch_flux.h"
#include "fdtd2d_batch_hz.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lines: nlines x {orientation (0 row, 1 column), index, first, count}; omega: count x nfreq.  nlines = 0 removes the
 * lines (the other arguments are then ignored).  The sums start at zero and the step count at this call.
 * FDTD2D_E_ARG, before any device work and with the previous lines left in place, for the arguments that
 * fdtd2d_batch_set_flux_lines refuses.  FDTD2D_E_STATE as under "Scope".  Synchronous. */
int fdtd2d_batch_set_hz_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                   int every);
/* The raw sums, each count x nfreq x cells (cells: the lines' counts together, lines concatenated in the order given):
 * H_k into hz_re, hz_im and E_k (without the half-step factor) into et_re, et_im.  FDTD2D_E_STATE without these lines.
 * Synchronous. */
int fdtd2d_batch_read_hz_flux_lines(fdtd2d_batch_t *b, double *hz_re, double *hz_im, double *et_re, double *et_im);
/* out: count x nlines x nfreq float64, P as defined above, formed on the device by one launch (one workgroup per
 * member, a fixed summation order).  FDTD2D_E_STATE without these lines.  Synchronous. */
int fdtd2d_batch_hz_flux(fdtd2d_batch_t *b, double *out);

/* fdtd2d_batch_reset zeroes the sums and restarts their count at step 0; fdtd2d_batch_upload, _set_materials,
 * _set_sources, _set_pml (with factors), _set_hz_conductivity and _set_hz_dispersion leave them alone. */

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_HZ_FLUX_H */
