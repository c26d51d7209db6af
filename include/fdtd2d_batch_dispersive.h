/* fdtd2d_batch_dispersive.h -- dispersive (Drude-Lorentz) materials for batched grids, a companion of fdtd2d.h.
 *
 * One pole per member with a strength per cell.  Member b has a damping gamma_b >= 0 and a resonance omega0_b >= 0
 * (rad/s; omega0_b = 0 is a Drude pole), every cell a strength wp2[b,i,j] >= 0 (rad^2/s^2).  For a field ~ e^{-i w t}
 *     chi(w) = wp2 / (omega0^2 - w^2 - i gamma w),   P = EPS0 chi E,   eps(w) = eps[i,j] + EPS0 chi(w)
 * with EPS0 = 8.85418e-12, the library's vacuum constant.  A Lorentz pole of strength d_eps: wp2 = d_eps * omega0^2.
 *
 * State per cell, in the batch's type T, zero at first and after fdtd2d_batch_reset:
 *     Jh = dx times the polarisation current, at half steps (it carries the units of H)
 *     Q  = dx P / dt
 * Coefficients, formed in float64 and rounded once to T:
 *     g = gamma_b dt / 2;  a_b = (T)((1 - g)/(1 + g));  bq = dt/(1 + g);  ck_b = (T)(bq omega0_b^2 dt)
 *     cj[i,j] = (T)(dx bq EPS0 wp2[i,j])
 * cj does not depend on eps: fdtd2d_batch_set_materials and _set_eps_window do not re-form it.
 * A cell that takes the plain update of fdtd2d_batch_lossy.h (e = ca*e + (dhy - dhx)*cb) takes instead, in this order,
 *     jn = a*Jh + (cj*e - ck*Q)
 *     Q  = Q + jn
 *     e  = ca*e + ((dhy - dhx) - jn)*cb
 *     Jh = jn
 * every operation rounded to T (in the fused build jn = fma(a, Jh, fma(cj, e, -(ck*Q))) and
 * e = fma((dhy - dhx) - jn, cb, ca*e), written out so that every path contracts alike).  A batch without a conductivity
 * has ca = 1, cb = ce.  Cells that take no plain update (the layer, the PEC rows, the edge) leave Jh and Q untouched.
 * H, the layer's split update, sources, point sources, DFTs and probes are unchanged and keep their order.  With
 * wp2 = 0 everywhere and zero state jn is exactly 0 and a run is bit-identical to the same run without the pole.
 * It is a leapfrog of E, Q (whole steps) against H, Jh (half steps).
 *
 * wp2 may be non-zero exactly where a conductivity may be (fdtd2d_batch_lossy.h, fdtd2d_batch_periodic.h).  The pole
 * needs a batch that runs on the PML family: a FDTD2D_BOUNDARY_NONE batch with a layer (fdtd2d_batch_set_pml) or with
 * periodic columns (with or without a layer).  On a periodic batch the image column of Jh and Q repeats column 0.
 * While a pole is set every run takes the dispersive step kernels, the capacity rule of the resident path counts ten
 * arrays (Ez, Hx, Hy, Ezx, cb, ch, ca, Jh, Q, cj), and refused with FDTD2D_E_STATE are: fdtd2d_batch_set_bloch,
 * removing the layer of a non-periodic batch, turning periodic columns off without a layer,
 * fdtd2d_batch_hold_dft_window and fdtd2d_batch_dft_window_product (the adjoint of a dispersive medium is not part of
 * this header).  fdtd2d_batch_set_materials and _set_eps_window repeat the stability check below and refuse
 * (FDTD2D_E_ARG) leaving the batch as it was.
 * These entry points live in their own header because fdtd2d.h's batch section and the other companions are fixed
 * surfaces. */
#ifndef FDTD2D_BATCH_DISPERSIVE_H
#define FDTD2D_BATCH_DISPERSIVE_H

#include "fdtd2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: 1 while a pole is set */
#define FDTD2D_BATCH_INFO_DISPERSIVE 19

/* wp2: count x rows x cols of dtype (FDTD2D_F32 or _F64); gamma, omega0: count entries.  All three NULL removes the
 * pole, frees Jh, Q and cj and returns the batch to its other kernels.  Needs materials; a uniform-material batch gets
 * coefficient arrays, a batch without conductivity ca = 1 and cb = ce.  Allocates and zeroes Jh and Q on first use;
 * later calls keep the state.
 * FDTD2D_E_STATE, before anything changes: a Mur batch, a plain box without a layer, a batch with a Bloch phase.
 * FDTD2D_E_ARG, naming the member, before any device work: a wp2, gamma or omega0 that is negative or not finite; wp2
 * non-zero where it may not be; a cell with wp2 > 0 and
 *     dt^2 (omega0^2 + wp2 EPS0 / eps) + 8 dt^2 / (eps mu dx^2) > 4
 * (eps as the engine stores it, mu the member's smallest): a sufficient condition for the lossless scheme to stay
 * bounded.  Synchronous. */
int fdtd2d_batch_set_dispersion(fdtd2d_batch_t *b, const void *wp2, int dtype, const double *gamma,
                                const double *omega0);

/* New strengths for window = {row0, col0, nrows, ncols} of every member; wp2: count x nrows x ncols.  Afterwards the
 * batch is as fdtd2d_batch_set_dispersion with the full updated array would leave it.  FDTD2D_E_STATE without a pole
 * set; the FDTD2D_E_ARG refusals of fdtd2d_batch_set_dispersion, and for an empty window or one outside the grid.  One
 * upload of the window and one launch over its cells.  Synchronous. */
int fdtd2d_batch_set_dispersion_window(fdtd2d_batch_t *b, const int window[4], const void *wp2, int dtype);

/* Jh and Q (count x rows x cols each, as stored; either may be NULL), host <-> device: to_device != 0 uploads.  On a
 * periodic batch an upload overwrites the image column of both arrays with column 0.  FDTD2D_E_STATE without a pole
 * set. */
int fdtd2d_batch_transfer_dispersion(fdtd2d_batch_t *b, void *jh, void *q, int host_dtype, int to_device);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_DISPERSIVE_H */
