// The lattice mode of the Hz polarisation (include/fdtd2d_batch_hz_lattice.h): the unit cell of a rectangular lattice
// with Hz, Ex, Ey, a conductivity and one Drude-Lorentz pole on the in-plane E.  The two seams of
// kernels_batch_lattice.hpp around the Hz step of kernels_batch_hz_bloch.hpp: every field is a pair (real part,
// imaginary part) of T, row R-1 of Hz is the image of row 0 and column C-1 the image of column 0, member b carries
// rho_r = (cr, sr) across the row seam and rho_c = (cc, sc) across the column seam.  There is no layer, no Hzx and no
// fixed row: every cell of rows 0..R-2 and columns 0..C-2 is a material cell (batch_hz_e with mat = true,
// batch_hz_plain), and the parts meet in four places only:
//   E, i = R-2: the lower neighbour of Hz is rho_r * the row image       E, j = C-2: the right one is rho_c * the column image
//   H, row 0:   the upper neighbour of Ex is conj(rho_r) * Ex[R-2, j]    H, column 0: the left one is conj(rho_c) * Ey[i, C-2]
// The image slots of Hz hold the UNROTATED copies of row 0 and of column 0 (the corner: of cell (0, 0)), in LDS and in
// global memory.  The thread that owns an image cell evaluates its source cell's H update, source included, from that
// cell's operands with its own value as the old one: (i, C-1) recomputes (i, 0), (R-1, j) recomputes (0, j), the corner
// recomputes (0, 0).  By induction every image stays bit-identical to its source cell, no thread reads an Hz that another
// thread writes in the H phase, two barriers per step suffice and the streamed pair stays in place and race-free.  Ex, Ey
// and the pole state have no image: the E phase never touches row R-1 or column C-1 and reads and writes them at the
// thread's own cell index alone.
//
// Neither seam costs a branch: both rotations are applied everywhere with the coefficients selected (c, s) on the seam
// and (1, 0) elsewhere, and the wraps are selects on LDS indices.
//
// LDS of the resident kernel: Hz, Ex, Ey (real), Hz, Ex, Ey (imaginary), ch, cb, ca -- 9 arrays -- and with a pole cj,
// Jx, Qx, Jy, Qy (real), Jx, Qx, Jy, Qy (imaginary) behind them -- 18 arrays; then the source weights (2 (C-1) float64),
// the phasor table and (lds_acc) the accumulators of both parts.
//
// Not here: the layer, the whole-grid DFT, the point sources and the flux lines (refused on the host while the mode is on).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_hz_bloch.hpp"
#include "kernels_batch_lattice.hpp"

namespace fdtd {

// `la` carries the imaginary parts in the slots of the real ones (ez: Hz, hx: Ex, hy: Ey).  Two barriers per step.
template <class T, bool POLE, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_hz_lattice(BatchView<T> v, BatchMon m,
                                                                                  BatchLattice<T> la,
                                                                                  BatchHzBlochDisp<T> d,
                                                                                  const T *__restrict__ ca, int n0, int nt,
                                                                                  long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_hz_lattice_lds[];
    const int R = v.R, C = v.C;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *shz = reinterpret_cast<T *>(batch_hz_lattice_lds);
    T *sex = shz + seg, *sey = sex + seg;
    T *siz = sey + seg, *six = siz + seg, *siy = six + seg;
    T *sch = siy + seg, *scb = sch + seg, *sca = scb + seg;
    T *scj = sca + seg, *sjx = scj + seg, *sqx = sjx + seg, *sjy = sqx + seg, *sqy = sjy + seg;   // POLE alone
    T *sjxi = sqy + seg, *sqxi = sjxi + seg, *sjyi = sqxi + seg, *sqyi = sjyi + seg;              // POLE alone
    double *sw = reinterpret_cast<double *>(shz + (POLE ? 18 : 9) * seg);   // wr[C-1], wi[C-1]
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
            shz[l] = v.ez[g];
            sex[l] = v.hx[g];
            sey[l] = v.hy[g];
            siz[l] = la.ez[g];
            six[l] = la.hx[g];
            siy[l] = la.hy[g];
            sch[l] = v.ch[g];
            scb[l] = v.ce[g];
            sca[l] = ca[g];
            if constexpr (POLE) {
                scj[l] = d.cj[g];
                sjx[l] = d.jx[g];
                sqx[l] = d.qx[g];
                sjy[l] = d.jy[g];
                sqy[l] = d.qy[g];
                sjxi[l] = d.jxi[g];
                sqxi[l] = d.qxi[g];
                sjyi[l] = d.jyi[g];
                sqyi[l] = d.qyi[g];
            }
        });
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = la.w[(size_t)b * 2 * (C - 1) + k];
        const T rrc = la.rho_r[2 * b], rrs = la.rho_r[2 * b + 1];
        const T rcc = la.rho_c[2 * b], rcs = la.rho_c[2 * b + 1];
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = la.amps && src.r1 > src.r0 ? la.amps + (size_t)b * v.amp_stride : nullptr;
        T da = T(0), dck = T(0);
        if constexpr (POLE) {
            da = d.a[b];
            dck = d.ck[b];
        }
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const BatchMonMember moni = batch_mon_begin(mi, b, sacci, tid, nthr);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {   // the E half-step
                if (i > R - 2 || j > C - 2) return;
                const bool cseam = j == C - 2;            // the right neighbour is the column image: rho_c * column 0
                const bool rseam = i == R - 2;            // the lower neighbour is the row image: rho_r * row 0
                const T kcc = cseam ? rcc : (T)1, kcs = cseam ? rcs : (T)0;
                const T krc = rseam ? rrc : (T)1, krs = rseam ? rrs : (T)0;
                T nr, ni, ur, ui;
                batch_bloch_rot(kcc, kcs, shz[l + 1], siz[l + 1], nr, ni);
                batch_bloch_rot(krc, krs, shz[l + C], siz[l + C], ur, ui);
                const T hr = shz[l], hi = siz[l];
                const T dxr = ur - hr, dyr = nr - hr;
                const T dxi = ui - hi, dyi = ni - hi;
                const T a = sca[l], cb = scb[l];
                T exr = sex[l], eyr = sey[l], exi = six[l], eyi = siy[l];
                if constexpr (POLE) {
                    const T cj = scj[l];
                    batch_hz_e<T, true, true>(exr, eyr, dxr, dyr, true, a, cb, T(1), T(1), T(1), T(1), da, dck, cj,
                                              sjx[l], sqx[l], sjy[l], sqy[l]);
                    batch_hz_e<T, true, true>(exi, eyi, dxi, dyi, true, a, cb, T(1), T(1), T(1), T(1), da, dck, cj,
                                              sjxi[l], sqxi[l], sjyi[l], sqyi[l]);
                } else {
                    T z = T(0);
                    batch_hz_e<T, true, false>(exr, eyr, dxr, dyr, true, a, cb, T(1), T(1), T(1), T(1), da, dck, z, z, z,
                                               z, z);
                    batch_hz_e<T, true, false>(exi, eyi, dxi, dyi, true, a, cb, T(1), T(1), T(1), T(1), da, dck, z, z, z,
                                               z, z);
                }
                sex[l] = exr;
                sey[l] = eyr;
                six[l] = exi;
                siy[l] = eyi;
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step);
            cells([&](int, int i, int j, int l) {   // the H half-step, the source, the monitors
                T hr = shz[l], hi = siz[l];
                const int ic = i == R - 1 ? 0 : i, jc = j == C - 1 ? 0 : j;    // the cell whose update this is
                const int lc = ic * C + jc;
                const bool cwrap = jc == 0, rwrap = ic == 0;    // its left / upper neighbour is across a seam
                const int lw = cwrap ? lc + (C - 2) : lc - 1;
                const int lu = rwrap ? lc + (R - 2) * C : lc - C;
                const T kcc = cwrap ? rcc : (T)1, kcs = cwrap ? rcs : (T)0;
                const T krc = rwrap ? rrc : (T)1, krs = rwrap ? rrs : (T)0;
                T wr, wi, ur, ui;
                batch_bloch_unrot(kcc, kcs, sey[lw], siy[lw], wr, wi);
                batch_bloch_unrot(krc, krs, sex[lu], six[lu], ur, ui);
                const T cc = sch[lc];
                const T deyr = sey[lc] - wr, dexr = sex[lc] - ur;
                const T deyi = siy[lc] - wi, dexi = six[lc] - ui;
                hr = batch_hz_plain(hr, deyr - dexr, cc);
                hi = batch_hz_plain(hi, deyi - dexi, cc);
                if (src.covers(ic, jc)) {                     // an image takes its source cell's source
                    double dr, dq;
                    batch_bloch_source(ar, ai, sw[jc], sw[C - 1 + jc], dr, dq);
                    hr = (T)((double)hr + dr);
                    hi = (T)((double)hi + dq);
                }
                shz[l] = hr;
                siz[l] = hi;
                if (sampled) {
                    // two copies of the adds, so that the LDS one uses LDS instructions, not flat ones
                    const int w = m.window_cell(i, j);
                    if (w >= 0 && m.lds_acc) {
                        m.add(sacc, stab, w, (double)hr);
                        m.add(sacci, stab, w, (double)hi);
                    } else if (w >= 0) {
                        m.add(mon.acc, stab, w, (double)hr);
                        m.add(moni.acc, stab, w, (double)hi);
                    }
                }
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, shz, step);
            batch_mon_probes(mi, moni, b, siz, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = shz[l];
            la.ez[g] = siz[l];
            if (i > R - 2 || j > C - 2) return;       // row R-1 and column C-1 of Ex, Ey and the state are never written
            v.hx[g] = sex[l];
            v.hy[g] = sey[l];
            la.hx[g] = six[l];
            la.hy[g] = siy[l];
            if constexpr (POLE) {
                d.jx[g] = sjx[l];
                d.qx[g] = sqx[l];
                d.jy[g] = sjy[l];
                d.qy[g] = sqy[l];
                d.jxi[g] = sjxi[l];
                d.qxi[g] = sqxi[l];
                d.jyi[g] = sjyi[l];
                d.qyi[g] = sqyi[l];
            }
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        batch_mon_end(mi, b, sacci, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed path, first launch of a step: the E half-step of both parts in place (it also writes the phasors of the step),
// with the arithmetic of the resident kernel above
template <class T, bool POLE>
__global__ __launch_bounds__(256) void k_batch_e_hz_lattice(BatchView<T> v, BatchMon m, BatchLattice<T> la,
                                                            BatchHzBlochDisp<T> d, const T *__restrict__ ca,
                                                            long long step)
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
        T nr, ni, ur, ui;
        batch_bloch_rot(kcc, kcs, v.ez[o + 1], la.ez[o + 1], nr, ni);
        batch_bloch_rot(krc, krs, v.ez[o + v.pitch], la.ez[o + v.pitch], ur, ui);
        const T hr = v.ez[o], hi = la.ez[o];
        const T dxr = ur - hr, dyr = nr - hr;
        const T dxi = ui - hi, dyi = ni - hi;
        const T a = ca[o], cb = v.ce[o];
        T exr = v.hx[o], eyr = v.hy[o], exi = la.hx[o], eyi = la.hy[o];
        if constexpr (POLE) {
            const T da = d.a[b], dck = d.ck[b], cj = d.cj[o];
            T jx = d.jx[o], qx = d.qx[o], jy = d.jy[o], qy = d.qy[o];
            T jxi = d.jxi[o], qxi = d.qxi[o], jyi = d.jyi[o], qyi = d.qyi[o];
            batch_hz_e<T, true, true>(exr, eyr, dxr, dyr, true, a, cb, T(1), T(1), T(1), T(1), da, dck, cj, jx, qx, jy, qy);
            batch_hz_e<T, true, true>(exi, eyi, dxi, dyi, true, a, cb, T(1), T(1), T(1), T(1), da, dck, cj, jxi, qxi, jyi,
                                      qyi);
            d.jx[o] = jx;
            d.qx[o] = qx;
            d.jy[o] = jy;
            d.qy[o] = qy;
            d.jxi[o] = jxi;
            d.qxi[o] = qxi;
            d.jyi[o] = jyi;
            d.qyi[o] = qyi;
        } else {
            T z = T(0);
            batch_hz_e<T, true, false>(exr, eyr, dxr, dyr, true, a, cb, T(1), T(1), T(1), T(1), z, z, z, z, z, z, z);
            batch_hz_e<T, true, false>(exi, eyi, dxi, dyi, true, a, cb, T(1), T(1), T(1), T(1), z, z, z, z, z, z, z);
        }
        v.hx[o] = exr;
        v.hy[o] = eyr;
        la.hx[o] = exi;
        la.hy[o] = eyi;
    }
}

// second launch: the H half-step of both parts in place, the source, the images and the monitors on Hz
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_hz_lattice(BatchView<T> v, BatchMon m, BatchLattice<T> la, int n,
                                                            long long step)
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
        T hr = v.ez[o], hi = la.ez[o];
        T wr, wi, ur, ui;
        batch_bloch_unrot(kcc, kcs, v.hy[ow], la.hy[ow], wr, wi);
        batch_bloch_unrot(krc, krs, v.hx[ou], la.hx[ou], ur, ui);
        const T cc = v.ch[oc];
        const T deyr = v.hy[oc] - wr, dexr = v.hx[oc] - ur;
        const T deyi = la.hy[oc] - wi, dexi = la.hx[oc] - ui;
        hr = batch_hz_plain(hr, deyr - dexr, cc);
        hi = batch_hz_plain(hi, deyi - dexi, cc);
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(ic, jc)) {
            const double *w = la.w + (size_t)b * 2 * (C - 1);
            const double ai = la.amps ? la.amps[(size_t)b * v.amp_stride + n] : 0.0;
            double dr, dq;
            batch_bloch_source(src.amps[n], ai, w[jc], w[C - 1 + jc], dr, dq);
            hr = (T)((double)hr + dr);
            hi = (T)((double)hi + dq);
        }
        v.ez[o] = hr;
        la.ez[o] = hi;
        batch_mon_cell(m, b, t, i, j, step, (double)hr);
        batch_mon_cell(mi, b, t, i, j, step, (double)hi);
    }
}

// host stubs of the kernels above (batch_hz_lattice.hip): resident [pole][MAXC 4, 5] (5: float32 members without a pole
// above 4096 cells; nullptr for float64 and with a pole, whose capacities end below 4 cells per thread)
struct BatchHzLatticeKernels {
    const void *resident[2][2];
    const void *e[2];
    const void *h;
};
template <class T> const BatchHzLatticeKernels &batch_hz_lattice_kernels();

}  // namespace fdtd
