/* fdtd2d_batch_flux_adjoint.h -- line sources for batched grids: the transpose of the flux monitor, a companion of
 * fdtd2d_batch_flux.h and fdtd2d_batch_adjoint.h.
 *
 * A flux line reads Ez and the tangential H centred on its cells.  Its transpose is a source on the same cells that
 * drives Ez and, with the same centring, the two H values the monitor averages.  That is what the adjoint of a flux
 * objective injects (fdtd2d_amd.batch_flux_gradient), and an electric and a magnetic sheet on one
 * line form a one-way source.  The sources live on the lines of fdtd2d_batch_set_flux_lines and are driven by the
 * channels of fdtd2d_batch_run_channels, like the point sources of fdtd2d_batch_adjoint.h.
 *
 * Definitions.
 *   entries     The lines' cells concatenated in the order the lines were given (the order of
 *               fdtd2d_batch_read_flux_lines): entry w of line k is cell `first + (w - offset_k)` of that line.  A cell
 *               that lies on two lines has two entries, one per line.
 *   weights     we, wh: count x cells x nchan float64, member-major, nchan <= 32.  Either may be NULL (no electric,
 *               no magnetic part).
 *   sums        In step n of a run with channels, for entry w (float64, one rounding per operation, no fused
 *               multiply-add):
 *                   s_e(w) = 0.0;  for c = 0 .. nchan-1:  s_e = s_e + we[w][c] * chan[c][n];     s_h(w) likewise with wh
 *   H part      BEFORE the H update of step n.  Every H value that the update writes (Hx[i][j] and Hy[i][j] with
 *               i <= R-2, j <= C-2) gathers
 *                   a = 0.0;  for line k = 0 .. nlines-1:
 *                       own cell (i, j) on line k:          a = a + 0.5 * s_h(its entry)
 *                       neighbour cell on line k:           a = a + 0.5 * s_h(its entry)
 *               where Hx counts row lines alone and its neighbour cell is (i+1, j), Hy counts column lines alone and
 *               its neighbour cell is (i, j+1), which is (i, 0) for j = C-2 with periodic columns.  These are exactly the
 *               two values the monitor averages for a cell: Hx[i-1][j], Hx[i][j] of a row line's cell and Hy[i][j-1],
 *               Hy[i][j] of a column line's (Hy[i][C-2] for column 0 of a periodic batch).  An H value with at least
 *               one such term becomes H = (T)((double)H + a), and the update of the step then reads it; the others
 *               are not touched.  Two lines that share an H value (a cell on two lines of one orientation, or parallel
 *               lines one cell apart) therefore combine in one float64 sum, lines ascending, own cell first, and one
 *               rounding to T.  Values that no update writes (Hx[:][C-1], Hy[R-1][:]) take nothing.
 *   E part      After the E half-step, the rectangle source and the point sources of step n, where the point sources
 *               add theirs: a cell on at least one line takes
 *                   a = 0.0;  for line k ascending that holds the cell:  a = a + s_e(its entry);   Ez = (T)((double)Ez + a)
 *               and the image column of a periodic batch repeats column 0.  The whole-grid DFT, the window DFT, the
 *               probes and the lines' own sums sample afterwards, so a monitor sees the step's injection.
 *
 * Scope.  FDTD2D_E_STATE without flux lines (which excludes the Mur frame, a Bloch phase and the lattice mode: those
 * batches carry no lines of this kind) and when point sources with another channel count are set;
 * fdtd2d_batch_set_point_sources refuses another channel count likewise while line sources are set.  Setting new flux
 * lines or removing them removes the line sources; fdtd2d_batch_reset keeps them.  fdtd2d_batch_run and _run_waveform
 * leave them silent; fdtd2d_batch_run_channels drives them, with or without point sources.
 *
 * The kernels.  While line sources are set the batch takes the kernels of kernels_batch_flux_adjoint.hpp: the flux
 * kernels step for step, plus the injection.  A batch without line sources launches exactly what it launched before.
 * The weights stay in global memory (they are read by the few threads that own a line cell or one of its H values, once
 * per step), so the capacity rule and the placement of the sums are those of fdtd2d_batch_flux.h. */
#ifndef FDTD2D_BATCH_FLUX_ADJOINT_H
#define FDTD2D_BATCH_FLUX_ADJOINT_H

#include "fdtd2d_batch_adjoint.h"
#include "fdtd2d_batch_flux.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: the channel count of the line sources (0 without them).  The id after fdtd2d_batch_flux.h's, an
 * enumerator like them. */
enum { FDTD2D_BATCH_INFO_FLUX_LINE_SOURCES = FDTD2D_BATCH_INFO_FLUX_LDS + 1 };

/* we, wh as above; both NULL (or nchan = 0) removes the sources.  FDTD2D_E_ARG for nchan outside 1..32 or a weight that
 * is not finite; FDTD2D_E_STATE as under "Scope".  A refused call leaves the previous sources in place.  Synchronous. */
int fdtd2d_batch_set_flux_line_sources(fdtd2d_batch_t *b, int nchan, const double *we, const double *wh);

/* Reads the installed weights back (count x cells x nchan each; an absent part reads as zeros).  FDTD2D_E_STATE without
 * line sources. */
int fdtd2d_batch_read_flux_line_sources(fdtd2d_batch_t *b, double *we, double *wh);

/* Forms the weights of the adjoint of a flux objective on the device, from the lines' current sums, and installs them
 * with nchan = 2 * nfreq (one launch; nfreq: the lines').  dJdP: count x nlines x nfreq.  solve: the inverse of the
 * 2 nfreq x 2 nfreq channel system, row-major, one for all members or count of them (solve_per_member != 0).  scale_e,
 * scale_h: count x cells, a real factor per entry (NULL: ones).  With E_k, H_k the raw sums of entry w on line l,
 * g_k = exp(+i omega_k dt / 2) and c_k = dJdP[l][k] * s_l * dx (s_l = +1 row line, -1 column line):
 *     te_k = scale_e[w] * c_k * conj(H_k g_k)        th_k = scale_h[w] * c_k * conj(E_k g_k)
 *     we[w][c] = sum_k solve[c][k] * Re te_k  then  + sum_k solve[c][nfreq + k] * Im te_k     (k ascending from 0.0)
 * and wh likewise from th.  FDTD2D_E_STATE without lines or with point sources of another channel
 * count; FDTD2D_E_ARG for a NULL dJdP or solve.  Synchronous. */
int fdtd2d_batch_flux_line_weights(fdtd2d_batch_t *b, const double *dJdP, const double *solve, int solve_per_member,
                                   const double *scale_e, const double *scale_h);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_FLUX_ADJOINT_H */
