/* fdtd2d_batch_periodic.h -- periodic columns for batched grids, a companion of fdtd2d.h.
 *
 * Every member becomes one period of a structure that repeats along its columns: gratings, metasurface unit cells,
 * photonic-crystal slabs.  Rows end in the split-field PML of fdtd2d_batch_set_pml, or in PEC without a layer.
 *
 * Grid.  The period is Q = cols - 1 cells; column cols - 1 is the image of column 0, so the complete state keeps the
 * host shapes Ez (R, C), Hx (R, C-1), Hy (R-1, C).  One step, with the row factors of fdtd2d_batch_set_pml (all
 * exactly 1 without a layer) and column factors that are exactly 1:
 *     Hx[i,j] = ahr[i]*Hx[i,j] - (bhr[i]*ch[i,j]) * (Ez[i+1,j] - Ez[i,j])          i <= R-2, j <= C-2
 *     Hy[i,j] =        Hy[i,j] +         ch[i,j]  * (Ez[i,j+1] - Ez[i,j])          (Hy[i,C-2] reads the image)
 *   for 1 <= i <= R-2 and 0 <= j <= C-2, with dhy = Hy[i,j] - Hy[i,(j-1) mod Q], dhx = Hx[i,j] - Hx[i-1,j]:
 *     rows inside the layer (i < L or i > R-1-L):
 *       ey = Ez[i,j] - Ezx[i,j];  Ezx[i,j] = Ezx[i,j] + ce[i,j]*dhy;  ey = aer[i]*ey - (ber[i]*ce[i,j])*dhx
 *       Ez[i,j] = Ezx[i,j] + ey
 *     other rows:  Ez[i,j] = ca[i,j]*Ez[i,j] + (dhy - dhx)*cb[i,j]     (fdtd2d_batch_lossy.h; ca = 1, cb = ce without
 *                                                                       a conductivity: the reference's update)
 *   rows 0 and R-1 are never updated (PEC).  Then the rectangle source, then the point sources, then
 *   Ez[:,C-1] = Ez[:,0] and Ezx[:,C-1] = Ezx[:,0], then the whole-grid DFT, the window DFT and the probes sample.
 * Multiplying by a factor that is exactly 1 changes no value, so this is oracle/pml_numpy.step's operation order.
 *
 * The image column is output only: source rectangles and point sources must lie in columns 0..C-2 (FDTD2D_E_ARG naming
 * the member); eps, mu and sigma at column C-1 are accepted and never read (the image takes column 0's coefficients);
 * fdtd2d_batch_upload and fdtd2d_batch_transfer_ezx overwrite the image column of Ez and Ezx with column 0; monitors may
 * sit anywhere.  A conductivity may be non-zero anywhere in columns 0..C-2 on rows outside the layer and at least 6
 * rows from the top and bottom edges.
 *
 * A periodic batch always runs on the periodic step kernels (the lossy PML family with its monitors and point sources
 * silent when unset); a uniform-material batch gets coefficient arrays.  The capacity rule of the resident path is the
 * lossy PML one (7 arrays and the factors).  A Bloch phase (complex fields, one phase per member) is the companion
 * fdtd2d_batch_bloch.h.  Not supported: the Mur frame, periodic rows, the single-grid engine. */
#ifndef FDTD2D_BATCH_PERIODIC_H
#define FDTD2D_BATCH_PERIODIC_H

#include "fdtd2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdtd2d_batch_info: 1 while the columns are periodic */
#define FDTD2D_BATCH_INFO_PERIODIC 15

/* on != 0: periodic columns; 0: the batch returns to its other kernels (a layer and a conductivity that were set stay).
 * Needs a FDTD2D_BOUNDARY_NONE batch (FDTD2D_E_STATE on a Mur batch).  Turning it on refuses (FDTD2D_E_ARG, naming the
 * member, nothing changed) a source rectangle that reaches column C-1, a layer whose column factors are not exactly 1
 * and a conductivity inside the row margin; it copies column 0 of Ez and Ezx over the image column.  Either way the
 * point sources are removed (set them again).  While on:
 *   fdtd2d_batch_set_pml            fits by rows alone (2 L + 3 <= rows) and refuses column factors that are not
 *                                   exactly 1; NULL, NULL removes the layer (PEC top and bottom)
 *   fdtd2d_batch_set_sources,
 *   fdtd2d_batch_set_point_sources  refuse cells in column C-1; a point source in column 0 takes one more entry of the
 *                                   FDTD2D_BATCH_MAX_POINT_SOURCES for its image
 *   fdtd2d_batch_set_conductivity,
 *   _set_conductivity_window        apply the row margin alone
 *   FDTD2D_BATCH_INFO_RESIDENT, _RESIDENT_MAX_CELLS, _LDS_BYTES report the periodic rule.
 * Synchronous. */
int fdtd2d_batch_set_periodic(fdtd2d_batch_t *b, int on);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_PERIODIC_H */
