// Doubly periodic Bloch batches (include/fdtd2d_batch_lattice.h): the unit cell of a rectangular lattice.  The pattern
// of kernels_batch_bloch.hpp with a second seam: every field is a pair (real part, imaginary part) of T, row R-1 is the
// image of row 0 and column C-1 the image of column 0, member b carries rho_r = (cr, sr) across the row seam and
// rho_c = (cc, sc) across the column seam.  There is no layer, no Ezx and no PEC row: every cell of rows 0..R-2 and
// columns 0..C-2 takes the plain (lossy) update, and the parts meet in four places only:
//   H, i = R-2: the lower neighbour of Ez is rho_r * the row image       H, j = C-2: the right one is rho_c * the column image
//   E, row 0:   the upper neighbour of Hx is conj(rho_r) * Hx[R-2, j]    E, column 0: the left one is conj(rho_c) * Hy[i, C-2]
// The image slots of Ez hold the UNROTATED copies of row 0 and of column 0 (the corner: of cell (0, 0)), in LDS and in
// global memory.  The thread that owns an image cell evaluates its source cell's update from that cell's operands with
// its own value as the old one: (i, C-1) recomputes (i, 0), (R-1, j) recomputes (0, j), the corner recomputes (0, 0).
// By induction every image stays bit-identical to its source cell, no thread reads an Ez that another thread writes in
// the E phase, two barriers per step suffice and the streamed E kernel stays in place and race-free.
//
// Neither seam costs a branch: both rotations are applied everywhere with the coefficients selected (c, s) on the seam
// and (1, 0) elsewhere (kernels_batch_bloch.hpp), and the wraps are selects on LDS indices.  The E phase has no branch
// at all but the source test: every thread updates.  LDS: Ez, Hx, Hy (real), Ez, Hx, Hy (imaginary), cb, ch, ca in
// separate arrays read with one index: consecutive lanes, consecutive words, apart from the seam lanes' words.
//
// Not here: the layer, the whole-grid DFT and the point sources (refused on the host while the mode is on).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_bloch.hpp"

namespace fdtd {

// the imaginary parts and what else a lattice batch adds to the periodic kernels' arguments
template <class T> struct BatchLattice {
    T *ez, *hx, *hy;          // imaginary parts, the layout of the real ones
    const T *rho_r, *rho_c;   // count x {c, s} each: across the row seam, across the column seam
    const double *w;          // count x {wr[C-1], wi[C-1]}: the source weight of columns 0..C-2
    const double *amps;       // imaginary amplitudes, amps[b * amp_stride + n] (the view's stride); nullptr = zero
    double *acc;              // the window DFT of the imaginary part (BatchMon::acc's layout)
    double *trace;            // the probe traces of the imaginary part (BatchMon::trace's layout)
};

// x - c * d: Hx without row factors.  The fused build writes the fma out (see batch_periodic_split).
template <class T> __device__ __forceinline__ T batch_lattice_hx(T x, T c, T d)
{
#ifdef FDTD2D_FUSED
    return batch_periodic_fma(-c, d, x);
#else
    return x - c * d;
#endif
}

// LDS of one resident member in bytes before the monitors: 9 arrays and the source weights
template <class T> __host__ __device__ __forceinline__ size_t batch_lattice_lds_bytes(int R, int C)
{
    return 9 * batch_lds_seg<T>(R * C) * sizeof(T) + 16 * (size_t)(C - 1);
}

// LDS = Ez, Hx, Hy (real), Ez, Hx, Hy (imaginary), cb, ch, ca, the source weights, then the phasor table and (lds_acc)
// the accumulators of the real and of the imaginary part.  Two barriers per step.
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_lattice(BatchView<T> v, BatchMon m,
                                                                               BatchLattice<T> la,
                                                                               const T *__restrict__ ca, int n0, int nt,
                                                                               long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_lattice_lds[];
    const int R = v.R, C = v.C;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_lattice_lds);
    T *shx = sez + seg, *shy = shx + seg;
    T *siz = shy + seg, *six = siz + seg, *siy = six + seg;
    T *scb = siy + seg, *sch = scb + seg, *sca = sch + seg;
    double *sw = reinterpret_cast<double *>(sez + 9 * seg);   // wr[C-1], wi[C-1]
    double *stab = sw + 2 * (C - 1);
    double *sacc = stab + 2 * m.nf, *sacci = sacc + 2 * (size_t)m.nf * m.window();
    BatchMon mi = m;                          // the monitors of the imaginary part: same window, phasors and cells
    mi.acc = la.acc;
    mi.trace = la.trace;
    const int di = nthr / C, dj = nthr % C, ti = tid / C, tj = tid % C;
    auto cells = [&](auto &&body) {   // the cell walk of k_batch_resident_pml
        int i = ti, j = tj;
        asm volatile("" : "+v"(i), "+v"(j));
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            if (i < R) body(q, i, j, i * C + j);
            j += dj;
            i += di;
            if (j >= C) {
                j -= C;
                ++i;
            }
        }
    };

    for (int b = blockIdx.x; b < v.B; b += gridDim.x) {
        const size_t base = (size_t)b * v.mstride;
        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            sez[l] = v.ez[g];
            shx[l] = v.hx[g];
            shy[l] = v.hy[g];
            siz[l] = la.ez[g];
            six[l] = la.hx[g];
            siy[l] = la.hy[g];
            scb[l] = v.ce[g];
            sch[l] = v.ch[g];
            sca[l] = ca[g];
        });
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = la.w[(size_t)b * 2 * (C - 1) + k];
        const T rrc = la.rho_r[2 * b], rrs = la.rho_r[2 * b + 1];
        const T rcc = la.rho_c[2 * b], rcs = la.rho_c[2 * b + 1];
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = la.amps && src.r1 > src.r0 ? la.amps + (size_t)b * v.amp_stride : nullptr;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const BatchMonMember moni = batch_mon_begin(mi, b, sacci, tid, nthr);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const bool cseam = j == C - 2;            // the right neighbour is the column image: rho_c * column 0
                const bool rseam = i == R - 2;            // the lower neighbour is the row image: rho_r * row 0
                const T kcc = cseam ? rcc : (T)1, kcs = cseam ? rcs : (T)0;
                const T krc = rseam ? rrc : (T)1, krs = rseam ? rrs : (T)0;
                T nr, ni, dr, dq;
                batch_bloch_rot(kcc, kcs, sez[l + 1], siz[l + 1], nr, ni);
                batch_bloch_rot(krc, krs, sez[l + C], siz[l + C], dr, dq);
                const T cc = sch[l];
                const T er = sez[l], ei = siz[l];
                shx[l] = batch_lattice_hx(shx[l], cc, dr - er);
                shy[l] = batch_periodic_plain(shy[l], cc, nr - er);
                six[l] = batch_lattice_hx(six[l], cc, dq - ei);
                siy[l] = batch_periodic_plain(siy[l], cc, ni - ei);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step);
            cells([&](int, int i, int j, int l) {
                T er = sez[l], ei = siz[l];
                const int ic = i == R - 1 ? 0 : i, jc = j == C - 1 ? 0 : j;    // the cell whose update this is
                const int lc = ic * C + jc;
                const bool cwrap = jc == 0, rwrap = ic == 0;    // its left / upper neighbour is across a seam
                const int lw = cwrap ? lc + (C - 2) : lc - 1;
                const int lu = rwrap ? lc + (R - 2) * C : lc - C;
                const T kcc = cwrap ? rcc : (T)1, kcs = cwrap ? rcs : (T)0;
                const T krc = rwrap ? rrc : (T)1, krs = rwrap ? rrs : (T)0;
                T wr, wi, ur, ui;
                batch_bloch_unrot(kcc, kcs, shy[lw], siy[lw], wr, wi);
                batch_bloch_unrot(krc, krs, shx[lu], six[lu], ur, ui);
                const T cc = scb[lc], a = sca[lc];
                const T dhyr = shy[lc] - wr, dhxr = shx[lc] - ur;
                const T dhyi = siy[lc] - wi, dhxi = six[lc] - ui;
                er = batch_lossy_e(er, dhyr - dhxr, a, cc);
                ei = batch_lossy_e(ei, dhyi - dhxi, a, cc);
                if (src.covers(ic, jc)) {                     // an image takes its source cell's source
                    double dr, dq;
                    batch_bloch_source(ar, ai, sw[jc], sw[C - 1 + jc], dr, dq);
                    er = (T)((double)er + dr);
                    ei = (T)((double)ei + dq);
                }
                sez[l] = er;
                siz[l] = ei;
                if (sampled) {
                    // two copies of the adds, so that the LDS one uses LDS instructions, not flat ones
                    const int w = m.window_cell(i, j);
                    if (w >= 0 && m.lds_acc) {
                        m.add(sacc, stab, w, (double)er);
                        m.add(sacci, stab, w, (double)ei);
                    } else if (w >= 0) {
                        m.add(mon.acc, stab, w, (double)er);
                        m.add(moni.acc, stab, w, (double)ei);
                    }
                }
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, sez, step);
            batch_mon_probes(mi, moni, b, siz, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = sez[l];
            la.ez[g] = siz[l];
            if (i > R - 2 || j > C - 2) return;       // row R-1 of Hx and column C-1 of Hy are never written
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
            la.hx[g] = six[l];
            la.hy[g] = siy[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        batch_mon_end(mi, b, sacci, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed path: H (which also writes the phasors of the step), then E in place, with the arithmetic of the resident
// kernel above
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_lattice(BatchView<T> v, BatchMon m, BatchLattice<T> la, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    const bool cseam = j == C - 2, rseam = i == R - 2;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T kcc = cseam ? la.rho_c[2 * b] : (T)1, kcs = cseam ? la.rho_c[2 * b + 1] : (T)0;
        const T krc = rseam ? la.rho_r[2 * b] : (T)1, krs = rseam ? la.rho_r[2 * b + 1] : (T)0;
        T nr, ni, dr, dq;
        batch_bloch_rot(kcc, kcs, v.ez[o + 1], la.ez[o + 1], nr, ni);
        batch_bloch_rot(krc, krs, v.ez[o + v.pitch], la.ez[o + v.pitch], dr, dq);
        const T cc = v.ch[o];
        const T er = v.ez[o], ei = la.ez[o];
        v.hx[o] = batch_lattice_hx(v.hx[o], cc, dr - er);
        v.hy[o] = batch_periodic_plain(v.hy[o], cc, nr - er);
        la.hx[o] = batch_lattice_hx(la.hx[o], cc, dq - ei);
        la.hy[o] = batch_periodic_plain(la.hy[o], cc, ni - ei);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_batch_e_lattice(BatchView<T> v, BatchMon m, BatchLattice<T> la,
                                                         const T *__restrict__ ca, int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    const int ic = i == R - 1 ? 0 : i, jc = j == C - 1 ? 0 : j;
    const bool cwrap = jc == 0, rwrap = ic == 0;
    BatchMon mi = m;
    mi.acc = la.acc;
    mi.trace = la.trace;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t mb = (size_t)b * v.mstride;
        const size_t o = mb + (size_t)i * (size_t)v.pitch + (size_t)j;
        const size_t oc = mb + (size_t)ic * (size_t)v.pitch + (size_t)jc;
        const size_t ow = cwrap ? oc + (size_t)(C - 2) : oc - 1;
        const size_t ou = rwrap ? oc + (size_t)(R - 2) * (size_t)v.pitch : oc - (size_t)v.pitch;
        const T kcc = cwrap ? la.rho_c[2 * b] : (T)1, kcs = cwrap ? la.rho_c[2 * b + 1] : (T)0;
        const T krc = rwrap ? la.rho_r[2 * b] : (T)1, krs = rwrap ? la.rho_r[2 * b + 1] : (T)0;
        T er = v.ez[o], ei = la.ez[o];
        T wr, wi, ur, ui;
        batch_bloch_unrot(kcc, kcs, v.hy[ow], la.hy[ow], wr, wi);
        batch_bloch_unrot(krc, krs, v.hx[ou], la.hx[ou], ur, ui);
        const T cc = v.ce[oc], a = ca[oc];
        const T dhyr = v.hy[oc] - wr, dhxr = v.hx[oc] - ur;
        const T dhyi = la.hy[oc] - wi, dhxi = la.hx[oc] - ui;
        er = batch_lossy_e(er, dhyr - dhxr, a, cc);
        ei = batch_lossy_e(ei, dhyi - dhxi, a, cc);
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(ic, jc)) {
            const double *w = la.w + (size_t)b * 2 * (C - 1);
            const double ai = la.amps ? la.amps[(size_t)b * v.amp_stride + n] : 0.0;
            double dr, dq;
            batch_bloch_source(src.amps[n], ai, w[jc], w[C - 1 + jc], dr, dq);
            er = (T)((double)er + dr);
            ei = (T)((double)ei + dq);
        }
        v.ez[o] = er;
        la.ez[o] = ei;
        batch_mon_cell(m, b, t, i, j, step, (double)er);
        batch_mon_cell(mi, b, t, i, j, step, (double)ei);
    }
}

// host stubs of the kernels above (batch_lattice.hip): resident [MAXC 4, 5] (5: float32 members above 4096 cells,
// nullptr for float64, whose capacity ends below 4 cells per thread)
struct BatchLatticeKernels {
    const void *resident[2];
    const void *h, *e;
};
template <class T> const BatchLatticeKernels &batch_lattice_kernels();

}  // namespace fdtd
