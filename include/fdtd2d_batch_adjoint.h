/* fdtd2d_batch_adjoint.h -- what an adjoint run of batched grids needs, a companion of fdtd2d.h.
 *
 * Two device primitives beside the monitors of fdtd2d_batch_monitor.h:
 *   point sources with channels   up to 64 cells per member, each injecting a weighted sum of up to 32 shared time
 *                                 series (the mirror image of the probes), on every path;
 *   a held window and its product the window DFT of one run kept on the device and multiplied, cell by cell and
 *                                 frequency by frequency, with the window DFT of a later run.
 * With them the gradient of a probe-spectrum objective with respect to every cell's permittivity costs two runs
 * (fdtd2d_amd.batch_eps_gradient).
 * These entry points live in their own header because fdtd2d.h's batch section is a fixed surface. */
#ifndef FDTD2D_BATCH_ADJOINT_H
#define FDTD2D_BATCH_ADJOINT_H

#include "fdtd2d.h"
#include "fdtd2d_batch_monitor.h"

#ifdef __cplusplus
extern "C" {
#endif

/* point cells per member now (0 without point sources) */
#define FDTD2D_BATCH_INFO_POINT_SOURCES 12
/* 1 if a held copy of the window DFT exists (fdtd2d_batch_hold_dft_window), 0 otherwise */
#define FDTD2D_BATCH_INFO_HELD_WINDOW   13

#define FDTD2D_BATCH_MAX_POINT_SOURCES 64
#define FDTD2D_BATCH_MAX_CHANNELS      32

/* Point sources.  ncell <= 64 cells per member; cells is count x ncell x {row, col}, member-major (the layout of
 * fdtd2d_batch_set_probes); nchan <= 32 channels; weights is count x ncell x nchan float64.  ncell = 0 removes them
 * (the other arguments are then ignored).  FDTD2D_E_ARG before any device work for ncell outside 0..64, nchan outside
 * 1..32, a NULL array, a cell outside the grid, a cell listed twice in one member, or a weight that is not finite.
 * Synchronous.  Only fdtd2d_batch_run_channels applies them; fdtd2d_batch_run and _run_waveform ignore them.
 * On the resident path the ncell sums of a step wait in LDS: 8 * ncell bytes join the capacity rule,
 *   arrays (fdtd2d.h / fdtd2d_batch_pml.h) + 16 * nfreq + 8 * ncell <= 160 KiB,
 * and FDTD2D_BATCH_INFO_RESIDENT / _RESIDENT_MAX_CELLS / _LDS_BYTES describe it. */
int fdtd2d_batch_set_point_sources(fdtd2d_batch_t *b, int ncell, const int *cells, int nchan, const double *weights);

/* fdtd2d_batch_run (same amps, may be NULL) plus the point sources.  chan: nchan x nsteps float64 shared by all
 * members, or count x nchan x nsteps when chan_per_member is not 0.  After the E half-step and the rectangle source
 * of step n, every point cell of every member takes
 *     s = 0.0;  for c = 0 .. nchan-1:  s = s + w[c] * chan[c][n]     (float64, one rounding per operation)
 *     Ez = (T)((double)Ez + s)
 * and the whole-grid DFT, the window DFT and the probes sample afterwards.  A resident run is still one launch per
 * run (or per FDTD2D_BATCH_OPT_STEPS_PER_LAUNCH steps), a streamed one two launches per step.  FDTD2D_E_STATE
 * without point sources, FDTD2D_E_ARG for chan NULL. */
int fdtd2d_batch_run_channels(fdtd2d_batch_t *b, int nsteps, const double *amps, const double *chan,
                              int chan_per_member);

/* Copies the current window accumulators device-to-device into a held buffer.  The copy survives fdtd2d_batch_reset,
 * _set_sources, _set_point_sources and further runs; it is dropped when the window is removed or set again.
 * FDTD2D_E_STATE without a window. */
int fdtd2d_batch_hold_dft_window(fdtd2d_batch_t *b);

/* out[b][w] = sum over k of Re(coef[b][k] * held[b][k][w] * cur[b][k][w]); coef_re, coef_im: count x nfreq;
 * out: count x nrows x ncols float64.  One launch.  Operation order, in float64 with one rounding per operation:
 * for held h and current c',  tr = hr*cr' - hi*ci',  ti = hr*ci' + hi*cr',  term = coef_re*tr - coef_im*ti,  summed
 * over k ascending from 0.0.  FDTD2D_E_STATE without a window or without a held copy.  Synchronous. */
int fdtd2d_batch_dft_window_product(fdtd2d_batch_t *b, const double *coef_re, const double *coef_im, double *out);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_ADJOINT_H */
