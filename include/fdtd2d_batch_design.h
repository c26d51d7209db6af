/* fdtd2d_batch_design.h -- what a design loop on batched grids needs, a companion of fdtd2d.h.
 *
 * Three device primitives beside the monitors (fdtd2d_batch_monitor.h) and the adjoint primitives
 * (fdtd2d_batch_adjoint.h), so that an iteration of gradient descent moves only what it needs between host and device:
 *   probe spectra        the Fourier transform of the recorded probe traces, formed on the device after the run
 *                        (count x nprobe x nfreq values come back instead of count x nprobe x nsamples);
 *   field maxima         max |f| of one field per member (count values instead of three fields per member);
 *   a permittivity window  new eps for one window of every member (count x nrows x ncols values go up instead of the
 *                        full arrays), leaving the engine as fdtd2d_batch_set_materials with the updated arrays would.
 * fdtd2d_amd.AdjointSession keeps an engine standing on them.
 * These entry points live in their own header because fdtd2d.h's batch section and the other companions are fixed
 * surfaces.  They add no FDTD2D_BATCH_INFO_* / _OPT_* code (the next free ones are 14 / 3). */
#ifndef FDTD2D_BATCH_DESIGN_H
#define FDTD2D_BATCH_DESIGN_H

#include "fdtd2d.h"
#include "fdtd2d_batch_monitor.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Spectra of the probe traces.  Sample n of a probe was recorded after step s = (step at fdtd2d_batch_set_probes /
 * fdtd2d_batch_reset) + n + 1.  For every member b, probe p and frequency k (omega: count x nfreq, member-major):
 *     re = 0.0; im = 0.0
 *     for n = first .. first + count_samples - 1 ascending:
 *         t = (double)s * dt;  re = re + x[n] * cos(omega * t);  im = im + x[n] * (-sin(omega * t))
 * in float64 with one rounding per operation in the exact build: the phasor and the additions of the window DFT
 * (fdtd2d_batch_set_dft_window), in its order.  So with the window and the probes set at the same step, every = 1 and
 * the same omega, a probe's spectrum is bit-identical to the window's accumulators at the probe's cell.
 * re, im: count x nprobe x nfreq.  peak (count, may be NULL): the maximum over the member's probes and the samples of
 * the range of |x| (0.0 for an empty range).  nfreq 1..16, or 0 with re = im = NULL for the peak alone.
 * FDTD2D_E_STATE without probes; FDTD2D_E_ARG before any device work for nfreq outside 0..16, a NULL array that is
 * needed, a frequency that is not finite, or a range outside the samples recorded so far
 * (FDTD2D_BATCH_INFO_PROBE_SAMPLES).  One launch.  Synchronous.  Fields, traces and monitors are left as they are. */
int fdtd2d_batch_probe_spectra(fdtd2d_batch_t *b, int nfreq, const double *omega, long long first,
                               long long count_samples, double *re, double *im, double *peak);

/* out[b] = max |f| over member b's cells of one field (FDTD2D_FIELD_EZ, _HX or _HY; padding excluded), the engine's
 * values widened to float64.  A NaN in the field gives NaN.  One launch.  Synchronous. */
int fdtd2d_batch_field_absmax(fdtd2d_batch_t *b, int field, double *out);

/* Replaces the permittivity of the window [row0, row0 + nrows) x [col0, col0 + ncols) of every member;
 * eps: count x nrows x ncols of host_dtype.  Afterwards the engine is in the state that fdtd2d_batch_set_materials
 * with the full updated arrays would leave: a coefficient cell is dt / (x * dx) in the engine's type from the value
 * rounded to it, and fdtd2d_batch_courant reports the Courant number of the full updated member.  One upload of the
 * window and one launch over the window's cells.  FDTD2D_E_STATE without material arrays (uniform batches have none to
 * patch); FDTD2D_E_ARG before any device work for an empty window, one outside the grid, one that holds cell [0, 0]
 * (it sets the Mur factor and the PML grading), a NULL array, a bad host_dtype, or a value that is not positive and
 * finite in the engine's type.  Fields, monitors, sources and the PML are left as they are.  Synchronous. */
int fdtd2d_batch_set_eps_window(fdtd2d_batch_t *b, int row0, int col0, int nrows, int ncols, const void *eps,
                                int host_dtype);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_DESIGN_H */
