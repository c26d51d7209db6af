/* fdtd2d_batch_bloch_flux_adjoint.h -- line sources on the flux lines of a Bloch batch: the transpose of the complex flux
 * monitor, a companion of fdtd2d_batch_bloch_flux.h, fdtd2d_batch_flux_adjoint.h and fdtd2d_batch_bloch_adjoint.h.
 *
 * The sources live on the lines of fdtd2d_batch_set_bloch_flux_lines and are driven by the real channels of
 * fdtd2d_batch_run_bloch_channels.  They are what the adjoint of an objective on fdtd2d_batch_bloch_flux injects
 * (fdtd2d_amd.batch_bloch_flux_gradient), and an electric and a magnetic sheet with a phase ramp
 * on one line form a one-way source at oblique incidence.
 *
 * Definitions.
 *   entries     As in fdtd2d_batch_flux_adjoint.h: the lines' cells concatenated in the order the lines were given.
 *   weights     Complex, as four float64 arrays we_re, we_im, wh_re, wh_im, each count x cells x nchan, member-major,
 *               nchan <= 32.  Any of them may be NULL: that part is absent.
 *   sums        In step n of a run with channels, for entry w and each of the four arrays (float64, one rounding per
 *               operation, no fused multiply-add):
 *                   s = 0.0;  for c = 0 .. nchan-1:  s = s + w[entry][c] * chan[c][n]
 *               The sum of an absent array is 0.0.  s_e = (s_e_re, s_e_im), s_h = (s_h_re, s_h_im).
 *   E part      After the E half-step and the rectangle source of step n, where the Bloch point sources would add
 *               theirs.  A cell on at least one line takes, per part p of the field whose array we_p is present,
 *                   a = 0.0;  for line k ascending that holds the cell:  a = a + s_e_p(its entry);
 *                   Ez_p = (T)((double)Ez_p + a)
 *               and the part whose array is absent takes nothing.  A cell in column 0 is also added to the image slot,
 *               unrotated, as Bloch point sources are: the image stays the bit-for-bit copy of column 0.  The window
 *               DFT, the probes and the lines' own sums sample afterwards.
 *   H part      BEFORE the H update of step n, and only while wh_re or wh_im is present.  Every H value that the
 *               update writes (Hx[i][j], Hy[i][j] with i <= R-2, j <= C-2) gathers, in the order of
 *               fdtd2d_batch_flux_adjoint.h (lines of its orientation ascending, own cell before neighbour cell),
 *                   a = (0.0, 0.0);  per term:  t = (0.5 * s_h_re, 0.5 * s_h_im) of the entry;
 *                                               the seam term alone: t = r t (below);
 *                                               a_re = a_re + t_re;  a_im = a_im + t_im
 *               and an H value with at least one term becomes H_re = (T)((double)H_re + a_re),
 *               H_im = (T)((double)H_im + a_im).  The two values of an entry are those the Bloch monitor averages:
 *               Hx[i-1][j], Hx[i][j] for a row line and Hy[i][j-1], Hy[i][j] for a column line.  Values that no update
 *               writes (Hy[R-1][:]) take nothing.
 *   the seam    For a column-line entry at column 0 the left neighbour is Hy[i][C-2] across the seam: its term (the
 *               neighbour term of Hy[i][C-2]) is r (0.5 s_h) with r = (c, s) the rotation the run steps with, (c, -s) in
 *               a run with conjugate != 0; c and s as stored in the batch dtype, widened:
 *                   re' = c*tr - s*ti      im' = c*ti + s*tr      (float64, four products, one difference, one sum)
 *
 * Why the seam term is this one.  fdtd2d_batch_bloch_adjoint.h shows that the transpose of the one-step operator is the
 * same operator with rho replaced by conj(rho), so the adjoint field is a Bloch run with the conjugated rotation.  The
 * monitor's read is linear too: for an entry at column 0 it takes 0.5 (conj(rho) Hy[i, C-2] + Hy[i, 0]), a complex
 * multiple of one H value.  The transpose of "multiply by the complex number z" under the plain, unconjugated pairing
 * the gradient product uses is again "multiply by z", so the transposed monitor deposits conj(rho) (0.5 s_h) into
 * Hy[i, C-2].  In the conjugated run the stepping rotation r is conj(rho): r (0.5 s_h) is exactly that deposit, with c
 * and s the very numbers the monitor used (negating s is exact).  In a forward run r = rho, and the term is the physical
 * magnetic sheet at column "-1": the sheet deposits 0.5 s_h into Hy[i, -1] = conj(rho) Hy[i, C-2], which in the stored
 * value Hy[i, C-2] = rho Hy[i, -1] is rho (0.5 s_h).
 *
 * Scope.  FDTD2D_E_STATE without Bloch lines (which excludes lattice, Mur and phase-less batches).  Setting or removing
 * the Bloch lines removes the line sources; fdtd2d_batch_reset, a new phase and fdtd2d_batch_set_bloch_dispersion or its
 * removal keep them.  Without line sources a batch with Bloch lines refuses fdtd2d_batch_run_bloch_channels and
 * fdtd2d_batch_hold_bloch_window as before; once line sources are installed (all-zero weights included) both are
 * accepted: fdtd2d_batch_run_bloch_channels drives the sources with either value of conjugate (with and without the
 * pole), fdtd2d_batch_run_bloch leaves them silent, and fdtd2d_batch_bloch_window_product works as on any Bloch batch.
 * fdtd2d_batch_hold_bloch_window keeps refusing a batch with the pole.  fdtd2d_batch_set_bloch_point_sources stays
 * refused while Bloch lines are set, fdtd2d_batch_set_bloch_flux_lines stays refused while a held window exists (set the
 * lines before the first hold), and fdtd2d_batch_set_flux_line_sources keeps refusing a Bloch batch.
 *
 * Ids.  FDTD2D_BATCH_INFO_FLUX_LINE_SOURCES reports the channel count of line sources of either kind.  This header adds
 * no id.
 *
 * The kernels.  While line sources are set the batch takes the kernels of kernels_batch_bloch_flux_adjoint.hpp: the
 * Bloch flux kernels step for step, plus the injection.  A batch without line sources launches exactly what it launched
 * before.  The weights stay in global memory, so LDS placement, the capacity rule and the phasor tables are those of
 * fdtd2d_batch_bloch_flux.h.  The fused build may contract the sums' multiply-adds. */
#ifndef FDTD2D_BATCH_BLOCH_FLUX_ADJOINT_H
#define FDTD2D_BATCH_BLOCH_FLUX_ADJOINT_H

#include "fdtd2d_batch_bloch_adjoint.h"
#include "fdtd2d_batch_bloch_flux.h"
#include "fdtd2d_batch_flux_adjoint.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The four arrays as above; all NULL (or nchan = 0) removes the sources.  FDTD2D_E_ARG for nchan outside 1..32 or a
 * weight that is not finite; FDTD2D_E_STATE as under "Scope".  A refused call leaves the previous sources in place.
 * Synchronous. */
int fdtd2d_batch_set_bloch_flux_line_sources(fdtd2d_batch_t *b, int nchan, const double *we_re, const double *we_im,
                                             const double *wh_re, const double *wh_im);

/* Reads the installed weights back (count x cells x nchan each; an absent part reads as zeros).  FDTD2D_E_STATE without
 * line sources on Bloch lines. */
int fdtd2d_batch_read_bloch_flux_line_sources(fdtd2d_batch_t *b, double *we_re, double *we_im, double *wh_re,
                                              double *wh_im);

/* The Bloch counterpart of fdtd2d_batch_flux_line_weights, with its arguments: forms the weights of the adjoint of a
 * flux objective on the device in one launch, from both parts' current sums, and installs them as real weights with
 * nchan = 2 * nfreq (we_re and wh_re; the imaginary arrays absent).  E_k, H_k are the raw sums of the complex field,
 * E = (ar_re - ai_im) + i (ar_im + ai_re) with ar / ai the sums of the real / imaginary part, H likewise; the targets
 * te_k, th_k and the weights are those of fdtd2d_batch_flux_line_weights.  A real series added to the real part carries
 * any complex spectrum at omega_k > 0; the rotated seam term supplies the rest.  FDTD2D_E_STATE without Bloch lines;
 * FDTD2D_E_ARG for a NULL dJdP or solve.  Synchronous. */
int fdtd2d_batch_bloch_flux_line_weights(fdtd2d_batch_t *b, const double *dJdP, const double *solve,
                                         int solve_per_member, const double *scale_e, const double *scale_h);

#ifdef __cplusplus
}
#endif
#endif /* FDTD2D_BATCH_BLOCH_FLUX_ADJOINT_H */
