/* fdtd2d_batch_flux.h -- flux monitors for batched grids, a companion of fdtd2d_batch_monitor.h.
 *
 * A batch with a PML layer or with periodic columns can carry up to 4 flux lines: straight runs of cells on which the
 * step kernels accumulate, at up to 16 frequencies per member, the running Fourier transforms of Ez and of the
 * tangential H centred on the same cells.  From them one kernel forms the power that crosses each line per frequency
 * (a Poynting flux), which is what transmitted, reflected and absorbed power are ratios of.  Like the other monitors
 * the lines never change the fields, and a monitored resident run is still one launch, a streamed one still two
 * launches per step.
 *
 * Definitions.
 *   axes        Columns are x, rows are y: Hx -= ch (Ez[i+1,j] - Ez[i,j]), Hy += ch (Ez[i,j+1] - Ez[i,j]) and
 *               Ez += ce (dHy - dHx).  Hence S_y = Ez Hx and S_x = -Ez Hy.
 *   lines       The same geometry for all members (like the window).  A row line is {0, row i, first column, count}
 *               and counts power towards increasing row; a column line is {1, column j, first row, count} and counts
 *               power towards increasing column.  Row lines: 1 <= i <= R-2.  Column lines: 1 <= j <= C-2, and
 *               0 <= j <= C-2 on a batch with periodic columns (the image column C-1 is refused; a row line may span
 *               the whole period, columns 0..C-2, and no further).  A line may cross the layer: its numbers there are
 *               the layer's own split fields', not a physical flux.
 *   sampling    The rule of fdtd2d_batch_set_dft_window: every `every`-th completed step n counted from the call,
 *               t = n dt.  The frequencies are the lines' own (count x nfreq, member-major), not the window's.
 *   sums        At a sampled step n, after the source of that step, for every line cell and frequency k, in float64:
 *                   E_k += Ez exp(-i omega_k n dt)       Ez as stored, widened to double
 *                   H_k += Ht exp(-i omega_k n dt)       the same phasor (the expression of the window's)
 *               row line:    Ht = 0.5 ((double)Hx[i-1,j] + (double)Hx[i,j])
 *               column line: Ht = 0.5 ((double)Hy[i,j-1] + (double)Hy[i,j]); with periodic columns the left
 *               neighbour of column 0 is column C-2.  H is the H of step n's H half-step, the one its E half-step reads.
 *   half step   That H lives at (n - 1/2) dt, so the physical spectrum is H_k exp(+i omega_k dt / 2).  The factor is
 *               applied where the flux is formed (fdtd2d_batch_flux), never in the sums: fdtd2d_batch_read_flux_lines
 *               returns them raw.
 *   flux        Per member, line and frequency: P = s dx sum_cells Re(E_k conj(H_k exp(+i omega_k dt / 2))), s = +1
 *               for a row line and -1 for a column line, cells in ascending order.  No factor 1/2 and no
 *               normalisation: users take ratios.
 *
 * Scope.  FDTD2D_E_STATE on a batch created with the Mur frame, on a NONE batch without a layer or periodic columns, on
 * a batch with a Bloch phase and in the lattice mode: those kernels carry no flux lines.  While lines are set, removing
 * the layer of a batch without periodic columns, switching periodic columns, and setting a Bloch phase or the lattice
 * mode are refused with FDTD2D_E_STATE.
 *
 * The kernels.  A batch with flux lines takes the flux kernels (kernels_batch_flux.hpp): the lossy PML, the periodic
 * and the two dispersive kernels step for step, plus the sums.  A lossless PML batch has no flux kernels of its own: it
 * runs the lossy ones with an all-zero conductivity (ca = 1, cb = ce), which are bit-identical to the lossless kernels
 * there.  So while lines are set such a batch holds coefficient arrays and ca, seven arrays per member in LDS instead of
 * four (uniform materials) or six: FDTD2D_BATCH_INFO_RESIDENT, _RESIDENT_MAX_CELLS and _LDS_BYTES describe it, and
 * FDTD2D_BATCH_INFO_LOSSY stays 0.  Removing the lines gives the lossless kernels back.
 *
 * Capacity.  The resident path holds the lines' phasor table, 16*nfreq bytes, behind the window's: arrays + tables
 * <= 160 KiB is the capacity rule.  The 32*nfreq*cells bytes of sums (cells: all lines together) live in LDS behind the
 * window's when they fit too, otherwise in global memory.  Every sum takes the same float64 additions in the same order
 * on every path and placement. */
#ifndef FDTD2D_BATCH_FLUX_H
#define FDTD2D_BATCH_FLUX_H

#include "fdtd2d_batch_dispersive_adjoint.h"   /* the id the lines' ids follow */
#include "fdtd2d_batch_monitor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDTD2D_BATCH_MAX_FLUX_LINES 4
#define FDTD2D_BATCH_MAX_FLUX_FREQS 16

/* fdtd2d_batch_info: the number of flux lines set; and 1 if their sums live in LDS on the resident path now (lines are
 * set, fdtd2d_batch_run takes the resident path, FDTD2D_BATCH_OPT_FLUX_LDS allows it and they fit), 0 otherwise.
 * The two ids after the last one taken (fdtd2d_batch_dispersive_adjoint.h's), written relative to it and as
 * enumerators like it: the companions' checks of their own ids scan every header for numbered ids and pin the largest. */
enum {
    FDTD2D_BATCH_INFO_FLUX_LINES = FDTD2D_BATCH_INFO_HELD_DISPERSIVE_WINDOW + 1,
    FDTD2D_BATCH_INFO_FLUX_LDS = FDTD2D_BATCH_INFO_HELD_DISPERSIVE_WINDOW + 2
};
/* fdtd2d_batch_set_option.  -1 (default): the sums in LDS by the rule above; 0: never (global memory).  Results never
 * depend on it. */
#define FDTD2D_BATCH_OPT_FLUX_LDS 3

/* lines: nlines x {orientation (0 row, 1 column), index, first, count}; omega: count x nfreq.  nlines = 0 removes the
 * lines (the other arguments are then ignored).  The sums start at zero and the step count at this call.
 * FDTD2D_E_ARG, before any device work and with the previous lines left in place, for nlines outside 0..4, nfreq
 * outside 1..16, lines or omega NULL, every < 1, an orientation other than 0 or 1, an index outside the bounds above, or
 * a line that is empty or runs off the grid (past column C-2 with periodic columns).  FDTD2D_E_STATE as under "Scope",
 * and without materials.  Synchronous. */
int fdtd2d_batch_set_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                int every);
/* The raw sums, each count x nfreq x cells (cells: the lines' counts together, lines concatenated in the order given):
 * E_k into ez_re, ez_im and H_k (without the half-step factor) into ht_re, ht_im.  FDTD2D_E_STATE without lines.
 * Synchronous. */
int fdtd2d_batch_read_flux_lines(fdtd2d_batch_t *b, double *ez_re, double *ez_im, double *ht_re, double *ht_im);
/* out: count x nlines x nfreq float64, P as defined above, formed on the device by one launch (one workgroup per
 * member, a fixed summation order).  FDTD2D_E_STATE without lines.  Synchronous. */
int fdtd2d_batch_flux(fdtd2d_batch_t *b, double *out);

/* fdtd2d_batch_reset zeroes the sums and restarts their count at step 0; fdtd2d_batch_upload, _set_materials,
 * _set_sources, _set_pml (with factors), _set_conductivity and _set_dispersion leave them alone. */

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_FLUX_H */
