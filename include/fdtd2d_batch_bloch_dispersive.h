/* fdtd2d_batch_bloch_dispersive.h -- the Drude-Lorentz pole of fdtd2d_batch_dispersive.h for batches with complex
 * fields: a Bloch phase (fdtd2d_batch_bloch.h) or the lattice mode (fdtd2d_batch_lattice.h).  A companion of fdtd2d.h.
 *
 * A metal (or an absorption line) in a unit cell swept over the angle of incidence or along a band path: one pole per
 * member with a strength per cell, one k-point per member.  The pole, its parameters (wp2, gamma_b, omega0_b), its
 * coefficients (a_b, ck_b, cj[i,j], formed in float64 and rounded once to T) and its stability condition are those of
 * fdtd2d_batch_dispersive.h.  Every coefficient is real, so the pole acts on the real part and on the imaginary part of
 * the field separately; the parts still meet at the seams only.
 *
 * State per cell, in the batch's type T, zero at first and after fdtd2d_batch_reset: Jh and Q, a real and an imaginary
 * part each.
 *
 * Definition.  In every cell that takes the plain update e = ca*e + (dhy - dhx)*cb of the Bloch or the lattice kernels
 * (rows outside the layer and the PEC rows of a Bloch batch, every cell of a lattice period), each part (re, im) takes
 * instead, in this order,
 *     jn = a*Jh + (cj*e - ck*Q)
 *     Q  = Q + jn
 *     e  = ca*e + ((dhy - dhx) - jn)*cb
 *     Jh = jn
 * every operation rounded to T (in the fused build jn = fma(a, Jh, fma(cj, e, -(ck*Q))) and
 * e = fma((dhy - dhx) - jn, cb, ca*e), the forms of fdtd2d_batch_dispersive.h).  dhy and dhx are those of
 * fdtd2d_batch_bloch.h / fdtd2d_batch_lattice.h: the neighbours across a seam are already rotated by conj(rho).  Layer
 * rows, PEC rows, H, the rectangle source, the window DFT and the probes are untouched and keep their order.  With
 * wp2 = 0 everywhere and zero state a run is bit-identical to the same run without the pole.
 *
 * The image slots of Jh and Q (column C-1; in the lattice mode also row R-1 and the corner) hold the UNROTATED copies
 * of their source cells, as the slots of Ez do: the thread that owns an image cell recomputes its source cell's update
 * with its own old values, so the images stay bit-identical to their source cells with two barriers per step.
 *
 * wp2 may be non-zero exactly where a conductivity may be: on a Bloch batch everywhere but the margin on the rows
 * (fdtd2d_batch_periodic.h), on a lattice batch everywhere.  While this pole is set every run takes the kernels of
 * batch_bloch_dispersive.hip, the capacity rule of the resident path counts 16 arrays on a Bloch batch (its 11, Jh and
 * Q twice, cj) and 14 on a lattice batch (its 9 and those five), fdtd2d_batch_info reports
 * FDTD2D_BATCH_INFO_DISPERSIVE (19) as 1, and refused with FDTD2D_E_STATE, the batch unchanged, are:
 *     turning the phase or the mode off: fdtd2d_batch_set_bloch(NULL, NULL), fdtd2d_batch_set_periodic(0),
 *     fdtd2d_batch_set_lattice with NULLs;
 *     fdtd2d_batch_set_bloch_point_sources (with cells), fdtd2d_batch_run_bloch_channels,
 *     fdtd2d_batch_hold_bloch_window, fdtd2d_batch_bloch_window_product (the adjoint of a dispersive medium is not part
 *     of this header);
 *     the three entry points of fdtd2d_batch_dispersive.h, which keep refusing a batch with complex fields.
 * New rotations (fdtd2d_batch_set_bloch, fdtd2d_batch_set_lattice), fdtd2d_batch_set_pml and clearing the layer on a
 * Bloch batch, the conductivity calls, fdtd2d_batch_set_bloch_source, windows, probes, fdtd2d_batch_bloch_probe_spectra
 * and fdtd2d_batch_bloch_field_absmax keep working.  fdtd2d_batch_set_materials and _set_eps_window repeat the stability
 * check and refuse (FDTD2D_E_ARG) leaving the batch as it was.
 * These entry points live in their own header because fdtd2d.h's batch section and the other companions are fixed
 * surfaces. */
#ifndef FDTD2D_BATCH_BLOCH_DISPERSIVE_H
#define FDTD2D_BATCH_BLOCH_DISPERSIVE_H

#include "fdtd2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* wp2: count x rows x cols of dtype (FDTD2D_F32 or _F64); gamma, omega0: count entries; formed into a, ck and cj as
 * fdtd2d_batch_set_dispersion forms them.  All three NULL removes the pole, frees its arrays and returns the batch to
 * the Bloch or lattice kernels.  Allocates and zeroes Jh and Q (both parts) on first use; later calls keep the state.
 * FDTD2D_E_STATE, before anything changes: a batch with neither a Bloch phase nor the lattice mode (use
 * fdtd2d_batch_set_dispersion); a batch with Bloch point sources or a held Bloch window.
 * FDTD2D_E_ARG, naming the member, before any device work: a wp2, gamma or omega0 that is negative or not finite; wp2
 * non-zero where a conductivity may not be; a cell with wp2 > 0 and
 *     dt^2 (omega0^2 + wp2 EPS0 / eps) + 8 dt^2 / (eps mu dx^2) > 4
 * (eps as the engine stores it, mu the member's smallest).  Synchronous. */
int fdtd2d_batch_set_bloch_dispersion(fdtd2d_batch_t *b, const void *wp2, int dtype, const double *gamma,
                                      const double *omega0);

/* New strengths for window = {row0, col0, nrows, ncols} of every member; wp2: count x nrows x ncols.  Afterwards the
 * batch is as fdtd2d_batch_set_bloch_dispersion with the full updated array would leave it.  FDTD2D_E_STATE without
 * this pole set; the FDTD2D_E_ARG refusals above, and for an empty window or one outside the grid.  Synchronous. */
int fdtd2d_batch_set_bloch_dispersion_window(fdtd2d_batch_t *b, const int window[4], const void *wp2, int dtype);

/* The two parts of Jh and of Q (count x rows x cols each, any of them NULL), host <-> device: to_device != 0 uploads.
 * An upload writes the image slots from their source cells: column 0, and in the lattice mode also row 0 and cell
 * (0, 0).  A download delivers the images rotated, as Ez is delivered: column C-1 as rho * its slot (lattice: rho_c),
 * row R-1 as rho_r * its slot, the corner as rho_r * (rho_c * its slot); a rotation needs both parts of the slot, which
 * the library reads itself.  FDTD2D_E_STATE without this pole set. */
int fdtd2d_batch_transfer_bloch_dispersion(fdtd2d_batch_t *b, void *jh_re, void *jh_im, void *q_re, void *q_im,
                                           int host_dtype, int to_device);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_BLOCH_DISPERSIVE_H */
