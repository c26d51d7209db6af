/* fdtd2d_batch_lossy.h -- lossy materials for batched grids, a companion of fdtd2d.h.
 *
 * An electric conductivity sigma (S/m, >= 0 and finite) per cell of every member.  Per cell, formed when the
 * conductivity or the materials are set, with eps as the engine stores it (rounded to its type T first):
 *     s   = sigma * dt / (2 * eps)        in float64
 *     ca  = (T)((1 - s) / (1 + s))
 *     inv = (T)(1 / (1 + s))
 *     cb  = ce * inv                      in T, ce = dt / (eps * dx) as the batch holds it
 * The cells that take the reference's plain update take  e = ca * e + (dhy - dhx) * cb  instead (in the fused build
 * fma(dhy - dhx, cb, ca * e)).  H, the Mur frame, the PML branch, sources, point sources, DFTs and probes are unchanged
 * and keep their order.  With sigma = 0 everywhere ca = inv = 1 exactly, and a run is bit-identical to the same run
 * without conductivity.
 * sigma may be non-zero only on cells that take the plain update: not within 6 cells of an edge of a
 * FDTD2D_BOUNDARY_MUR5 batch or of a batch with a PML layer, not inside the layer, and not on the edge cells of a
 * plain FDTD2D_BOUNDARY_NONE batch.
 * While a conductivity is set every run takes the lossy step kernels (the point-source family with its monitors and
 * point sources silent when unset), the capacity rule of the resident path counts one array more, and
 * fdtd2d_batch_set_materials / _set_materials_uniform / _set_eps_window re-form ca and cb from the new permittivity.
 * The Courant check is untouched.
 * These entry points live in their own header because fdtd2d.h's batch section and the other companions are fixed
 * surfaces. */
#ifndef FDTD2D_BATCH_LOSSY_H
#define FDTD2D_BATCH_LOSSY_H

#include "fdtd2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: 1 while a conductivity is set */
#define FDTD2D_BATCH_INFO_LOSSY 14

/* sigma: count x rows x cols of dtype (FDTD2D_F32 or _F64); NULL removes the conductivity and returns the batch to
 * the other kernels.  Needs materials; a uniform-material batch gets coefficient arrays (there is no uniform lossy
 * kernel).  FDTD2D_E_ARG before any device work, naming the first offending member, for a value that is negative or
 * not finite or non-zero where it may not be.  One upload and one launch.  Synchronous. */
int fdtd2d_batch_set_conductivity(fdtd2d_batch_t *b, const void *sigma, int dtype);

/* New conductivity for window = {row0, col0, nrows, ncols} of every member; sigma: count x nrows x ncols.  Afterwards
 * the batch is as fdtd2d_batch_set_conductivity with the full updated array would leave it.  A batch without
 * conductivity starts from zero.  The refusals of fdtd2d_batch_set_conductivity, and FDTD2D_E_ARG for an empty window
 * or one outside the grid.  One upload of the window and one launch over its cells.  Synchronous. */
int fdtd2d_batch_set_conductivity_window(fdtd2d_batch_t *b, const int window[4], const void *sigma, int dtype);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_LOSSY_H */
