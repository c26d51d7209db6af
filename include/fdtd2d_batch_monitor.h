/* fdtd2d_batch_monitor.h -- monitors for batched grids, a companion of fdtd2d.h.
 *
 * Every member of a batch can carry a window DFT (up to 16 frequencies over one window of cells) and up to 64 point
 * probes, on every path (resident and streamed, Mur / NONE and PML), alongside the whole-grid fdtd2d_batch_set_dft.
 * Monitors never change the fields.  They are computed on the device inside the step kernels: a monitored resident
 * run is still one launch, a streamed one still two launches per step.
 * These entry points live in their own header because fdtd2d.h's batch section is a fixed surface. */
#ifndef FDTD2D_BATCH_MONITOR_H
#define FDTD2D_BATCH_MONITOR_H

#include "fdtd2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the window accumulators live in LDS on the resident path now (a window is set, fdtd2d_batch_run takes the
 * resident path, FDTD2D_BATCH_OPT_DFT_WINDOW_LDS allows it and they fit, see below); 0 otherwise */
#define FDTD2D_BATCH_INFO_DFT_WINDOW_LDS 10
/* samples recorded so far per probe: min(capacity, steps since fdtd2d_batch_set_probes / reset); 0 without probes */
#define FDTD2D_BATCH_INFO_PROBE_SAMPLES  11
/* -1 (default): window accumulators in LDS by the rule below; 0: never (global memory).  Results never depend on it. */
#define FDTD2D_BATCH_OPT_DFT_WINDOW_LDS  2

#define FDTD2D_BATCH_MAX_DFT_FREQS 16
#define FDTD2D_BATCH_MAX_PROBES    64

/* Window DFT.  One window [row0,row0+nrows) x [col0,col0+ncols), shared by all members.  nfreq <= 16 angular
 * frequencies per member: omega is count x nfreq, member-major.  After every `every`-th completed step n, counted
 * from this call, add Ez*exp(-i*omega_k*n*dt) in float64 to accumulator k of every window cell (the sampling rule
 * and the t = n*dt of fdtd2d_batch_set_dft).  nfreq = 0 removes the window (the other arguments are then ignored).
 * Accumulators start at zero.  FDTD2D_E_ARG before any device work for a window outside the grid or empty, nfreq
 * outside 0..16, omega NULL or every < 1.  Synchronous.
 * With a window the resident path also holds a phasor table of 16*nfreq bytes behind the member's arrays:
 * arrays (fdtd2d.h / fdtd2d_batch_pml.h) + 16*nfreq <= 160 KiB is the capacity rule, and
 * FDTD2D_BATCH_INFO_RESIDENT / _RESIDENT_MAX_CELLS / _LDS_BYTES describe it.  The 16*nfreq*nrows*ncols bytes of
 * accumulators join them in LDS when they fit too; otherwise they stay in global memory.  The sums are
 * bit-identical whatever the path and the placement. */
int fdtd2d_batch_set_dft_window(fdtd2d_batch_t *b, int row0, int col0, int nrows, int ncols,
                                int nfreq, const double *omega, int every);
/* re, im: each count x nfreq x nrows x ncols, row-major.  FDTD2D_E_STATE without a window.  Synchronous. */
int fdtd2d_batch_read_dft_window(fdtd2d_batch_t *b, double *re, double *im);

/* Probes.  nprobe <= 64 cells per member; cells is count x nprobe x {row, col}, member-major.  From now on, record
 * Ez after the source of every step, as float64, into `capacity` samples per probe.  Sample 0 is the first step
 * after this call.  Steps past capacity are not recorded.  nprobe = 0 removes the probes (the other arguments are
 * then ignored).  FDTD2D_E_ARG before any device work for nprobe outside 0..64, cells NULL, a cell outside the grid
 * or capacity < 1.  Synchronous. */
int fdtd2d_batch_set_probes(fdtd2d_batch_t *b, int nprobe, const int *cells, long long capacity);
/* out: count x nprobe x `count_samples` float64, samples [first, first + count_samples).  FDTD2D_E_STATE without
 * probes; FDTD2D_E_ARG for a range outside [0, capacity).  Synchronous. */
int fdtd2d_batch_read_probes(fdtd2d_batch_t *b, double *out, long long first, long long count_samples);

/* fdtd2d_batch_reset zeroes both monitors and restarts their count at step 0; fdtd2d_batch_upload, _set_materials,
 * _set_sources and _set_pml leave them alone. */

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_MONITOR_H */
