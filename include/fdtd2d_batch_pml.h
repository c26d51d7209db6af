/* fdtd2d_batch_pml.h -- the split-field PML for batched grids, a companion of fdtd2d.h.
 *
 * Every member of a batch created with FDTD2D_BOUNDARY_NONE can carry the Berenger layer of
 * fdtd2d_set_pml (definition: oracle/pml_numpy.py; the layer's outer edge is PEC, as NONE's is).
 * Each member is value-identical to an fdtd2d_t with FDTD2D_BOUNDARY_PML given the same factors.
 * These entry points live in their own header because fdtd2d.h's batch section is a fixed surface. */
#ifndef FDTD2D_BATCH_PML_H
#define FDTD2D_BATCH_PML_H

#include "fdtd2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* row_factors: count x 4*rows values {ahr, bhr, aer, ber}; col_factors: count x 4*cols values {ahc, bhc, aec,
 * bec}; member-major, in the batch's dtype (else FDTD2D_E_ARG), each member's as fdtd2d_set_pml takes them
 * (fdtd2d_amd.pml_profiles with s_max from the member's own Courant number).  layer_cells = L, shared by all
 * members: cells within L of an edge take the split update, the rest the reference's (main.py:21-27).
 * FDTD2D_E_ARG unless 1 <= L and 2L + 3 <= min(rows, cols); a batch created with MUR5 is FDTD2D_E_STATE.
 * Allocates Ezx (count x R x C) and sets it to zero (fdtd2d_batch_reset zeros it too).  Both pointers NULL
 * remove the layer and free Ezx (a plain NONE batch again); one NULL is FDTD2D_E_ARG.  Synchronous.
 * With a layer the resident path holds Ez, Hx, Hy, Ezx (+ ce, ch with material arrays) and the 4R + 4C factors:
 * arrays x roundup16(R*C*sizeof(T)) + roundup16(4R*sizeof(T)) + roundup16(4C*sizeof(T)) <= 160 KiB;
 * FDTD2D_BATCH_INFO_RESIDENT / _RESIDENT_MAX_CELLS / _LDS_BYTES describe that rule while the layer is on. */
int fdtd2d_batch_set_pml(fdtd2d_batch_t *b, const void *row_factors, const void *col_factors, int host_dtype,
                         int layer_cells);
/* count x R x C of Ezx, host <-> device (to_device != 0: upload); FDTD2D_E_STATE without a layer. */
int fdtd2d_batch_transfer_ezx(fdtd2d_batch_t *b, void *host, int host_dtype, int to_device);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_PML_H */
