/* fdtd2d_batch_hz.h -- the Hz polarisation for batched grids, a companion of fdtd2d.h.
 *
 * Every other batch kernel advances Ez with Hx and Hy (the electric field along the invariant axis).  This header adds the
 * other polarisation, Hz with Ex and Ey (the electric field in the plane), for FDTD2D_BOUNDARY_NONE batches with a PML
 * layer (fdtd2d_batch_set_pml) or periodic columns (fdtd2d_batch_set_periodic), with an electric conductivity and one
 * Drude-Lorentz pole acting on Ex and Ey.
 *
 * Storage is the batch's own.  The Ez slot holds Hz at the same nodes, the Hx slot Ex, the Hy slot Ey, the Ezx slot Hzx
 * (the split part of Hz in the layer): fdtd2d_batch_upload / _download move (Hz, Ex, Ey) and fdtd2d_batch_transfer_pml
 * moves Hzx.  Ex and Ey are the physical fields, with no hidden sign.
 *
 * Materials.  eps[i,j] is the permittivity of both Ex[i,j] and Ey[i,j] (co-located, as mu[i,j] serves Hx[i,j] and
 * Hy[i,j] in the Ez polarisation); mu[i,j] belongs to Hz[i,j].  In the batch's type T
 *     ce = dt/(eps dx),   ch = dt/(mu dx)
 * and from sigma, as fdtd2d_batch_lossy.h forms them, s = sigma dt/(2 eps) in float64, ca = (T)((1 - s)/(1 + s)),
 * cb = ce * (T)(1/(1 + s)).  The pole has a, ck per member and cj per cell exactly as fdtd2d_batch_dispersive.h forms
 * them; cj is indexed like eps.  State per cell, zero at first and after fdtd2d_batch_reset: Jx, Qx (of Ex) and Jy, Qy (of
 * Ey).
 *
 * One step is the E half-step, the H half-step, then the sources.
 *
 * E half-step, for i <= R-2 and j <= C-2, with dxi = Hz[i+1,j] - Hz[i,j] and dyj = Hz[i,j+1] - Hz[i,j].
 * The material cells -- L <= i <= R-2-L and, on a batch without periodic columns, L <= j <= C-2-L (L the layer's cells,
 * 0 without a layer) -- take
 *     jx = a*Jx + (cj*Ex - ck*Qx);  Qx = Qx + jx;  Ex = ca*Ex + (dxi - jx)*cb;  Jx = jx
 *     jy = a*Jy + (cj*Ey - ck*Qy);  Qy = Qy + jy;  Ey = ca*Ey - (dyj + jy)*cb;  Jy = jy
 * every operation rounded to T (without a pole jx = jy = 0 and the state does not exist).  In the fused build
 *     jx = fma(a, Jx, fma(cj, Ex, -(ck*Qx))),  Ex = fma(dxi - jx, cb, ca*Ex),  Ey = fma(-(dyj + jy), cb, ca*Ey)
 * written out so that the resident and the streamed path contract alike.  All other cells take the layer's update
 *     Ex = ahr[i]*Ex + (bhr[i]*ce)*dxi,   Ey = ahc[j]*Ey - (bhc[j]*ce)*dyj
 * (fused: fma(bhr*ce, dxi, ahr*Ex) and fma(-(bhc*ce), dyj, ahc*Ey)) and leave the state untouched; on a periodic batch
 * the column factors are exactly 1 and Ey = Ey - ce*dyj.  The factors are those of fdtd2d_batch_set_pml: the "H" factors
 * (ahr, bhr, ahc, bhc: graded at the half cells) now serve E and the "E" factors (aer, ber, aec, bec) serve Hz.  On the
 * material cells the half-cell factors must be exactly (1, 1): the usual grading, whose half-cell depth is zero for
 * L <= i <= n-2-L, has them so.
 *
 * H half-step, for 1 <= i <= R-2 and 1 <= j <= C-2 (periodic: 0 <= j <= C-2, the left neighbour of column 0 being column
 * C-2), with dey = Ey[i,j] - Ey[i,j-1] and dex = Ex[i,j] - Ex[i-1,j].  Outside the layer (L <= i <= R-1-L and, without
 * periodic columns, L <= j <= C-1-L)
 *     Hz = Hz - (dey - dex)*ch                                  (fused: fma(-(dey - dex), ch, Hz))
 * and in the layer the split update mirrored
 *     x = aec*Hzx - (bec*ch)*dey;  y = aer*(Hz - Hzx) + (ber*ch)*dex;  Hzx = x;  Hz = x + y
 * (fused: fma(-(bec*ch), dey, aec*Hzx) and fma(ber*ch, dex, aer*(Hz - Hzx))).
 *
 * After the H half-step, in this order: the rectangle source and (fdtd2d_batch_run_channels) the point sources add to Hz;
 * the image column of a periodic batch is refreshed (Hz[:,C-1] = Hz[:,0], Hzx likewise); the whole-grid DFT, the window
 * DFT and the probes read Hz.  That is what the Ez kernels do with Ez.  Ex, Ey and the pole state have no image column:
 * the E half-step never touches column C-1.
 *
 * Identities.  With sigma = 0, wp2 = 0 and zero state a run is bit-identical to the run without a pole.  With nothing
 * set, a run is bit-identical (exact build) to the Ez run of the same batch with eps and mu exchanged: Hz = Ez,
 * Ex = -Hx, Ey = -Hy.
 *
 * sigma and wp2 may be non-zero on rows g <= i <= R-2-g, g = the margin of fdtd2d_batch_lossy.h (max(L, 6)), and on a
 * batch without periodic columns also only on columns g <= j <= C-2-g: the rule of the Ez polarisation less one row and
 * one column on the high side, because Ex[i,j] lives at i + 1/2.  Column C-1 of a periodic batch is never read.
 *
 * While the batch is in the Hz polarisation every run takes the kernels of this header; the capacity rule of the resident
 * path counts seven arrays (Hz, Ex, Ey, Hzx, ch, cb, ca) and with a pole twelve (those and cj, Jx, Qx, Jy, Qy).  A run
 * needs a layer or periodic columns (FDTD2D_E_STATE otherwise: a plain box has no Hz kernels).  Refused with
 * FDTD2D_E_STATE in the Hz polarisation: fdtd2d_batch_set_conductivity and _set_conductivity_window (in this polarisation
 * that sigma would be a magnetic loss), fdtd2d_batch_set_dispersion, _set_dispersion_window and
 * _transfer_dispersion, fdtd2d_batch_set_bloch, fdtd2d_batch_set_lattice, the flux lines of fdtd2d_batch_flux.h and
 * fdtd2d_batch_bloch_flux.h and their sources (this polarisation's own lines are fdtd2d_batch_hz_flux.h's), every hold of
 * a window and every window product.  This polarisation's own phase is fdtd2d_batch_hz_bloch.h's and its own lattice
 * mode fdtd2d_batch_hz_lattice.h's, each entered from a periodic batch in the Hz polarisation.
 * These entry points live in their own header because fdtd2d.h's batch section and the other companions are fixed
 * surfaces. */
#ifndef FDTD2D_BATCH_HZ_H
#define FDTD2D_BATCH_HZ_H

#include "fdtd2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDTD2D_POL_EZ 0
#define FDTD2D_POL_HZ 1

/* Switches the polarisation.  Needs a FDTD2D_BOUNDARY_NONE batch with real fields.  FDTD2D_E_STATE, changing nothing: a
 * Mur batch, a Bloch phase, the lattice mode, a conductivity or a pole of the polarisation being left, flux lines (and
 * with them line sources), a held window.  FDTD2D_E_ARG for another value.  A switch that changes the polarisation zeroes
 * the fields and the step counter, as fdtd2d_batch_reset does; one that does not is a no-op. */
int fdtd2d_batch_set_polarization(fdtd2d_batch_t *b, int polarization);

/* FDTD2D_POL_EZ or FDTD2D_POL_HZ (FDTD2D_E_ARG for NULL) */
int fdtd2d_batch_polarization(const fdtd2d_batch_t *b);

/* sigma: count x rows x cols of dtype, the conductivity seen by Ex[i,j] and Ey[i,j]; NULL removes it.  Needs the Hz
 * polarisation (FDTD2D_E_STATE) and materials.  FDTD2D_E_ARG, naming the member, before any device work: a sigma that is
 * negative or not finite, or non-zero where it may not be.  Synchronous. */
int fdtd2d_batch_set_hz_conductivity(fdtd2d_batch_t *b, const void *sigma, int dtype);

/* wp2: count x rows x cols of dtype; gamma, omega0: count entries.  All three NULL removes the pole, frees its arrays and
 * returns the batch to the seven-array kernels.  Allocates and zeroes Jx, Qx, Jy, Qy on first use; later calls keep the
 * state.  FDTD2D_E_STATE: not the Hz polarisation, or a batch without a layer and without periodic columns.
 * FDTD2D_E_ARG, naming the member, before any device work: the refusals of fdtd2d_batch_set_dispersion, its stability
 * check unchanged, with the allowed cells above.  Synchronous. */
int fdtd2d_batch_set_hz_dispersion(fdtd2d_batch_t *b, const void *wp2, int dtype, const double *gamma,
                                   const double *omega0);

/* Jx, Qx, Jy, Qy (count x rows x cols each, as stored; any may be NULL), host <-> device: to_device != 0 uploads.
 * FDTD2D_E_STATE without a pole of this header. */
int fdtd2d_batch_transfer_hz_dispersion(fdtd2d_batch_t *b, void *jx, void *qx, void *jy, void *qy, int host_dtype,
                                        int to_device);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_HZ_H */
