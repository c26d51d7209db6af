// A Bloch phase for the Hz polarisation of periodic batches (include/fdtd2d_batch_hz_bloch.h): the periodic kernels of
// kernels_batch_hz.hpp with every field a pair (real part, imaginary part) of T and the seam rotated by the member's
// rho = (c, s), as kernels_batch_bloch.hpp does for the Ez polarisation.  Every coefficient is real, so each part takes
// the Hz step unchanged (batch_hz_e, batch_hz_split, batch_hz_plain); the parts meet in two places only:
//   E half-step, j = C-2: the right neighbour of Hz is rho * image (re' = c*re - s*im, im' = s*re + c*im)
//   H half-step, column 0 (and the image thread's copy of that update): the left neighbour of Ey is conj(rho) * Ey[i, C-2]
//               (re' = c*er + s*ei, im' = c*ei - s*er)
// The image slot of Hz and Hzx holds the UNROTATED copy of column 0 (in LDS and in global memory): the image thread
// evaluates column 0's update from column 0's operands, its own value as the old one and column 0's source weight, so
// the image stays bit-identical to column 0, with two barriers per step, and the streamed kernels stay in place and
// race-free.  Ex, Ey and the pole state (Jx, Qx, Jy, Qy, both parts) have no image: the E half-step never touches column
// C-1, and the state is read and written at the thread's own cell index alone.
//
// The seam costs no branch: rho is applied everywhere with the coefficients selected (c, s) on the seam and (1, 0)
// elsewhere.  The pair of a cell is read with one LDS index from two arrays (not interleaved).
//
// LDS of the resident kernel: Hz, Ex, Ey, Hzx (real), Hz, Ex, Ey, Hzx (imaginary), ch, cb, ca -- 11 arrays -- and with a
// pole cj, Jx, Qx, Jy, Qy (real), Jx, Qx, Jy, Qy (imaginary) behind them -- 20 arrays; then the row factors (4R), the
// source weights (2 (C-1) float64), the phasor table and (lds_acc) the accumulators of both parts.
//
// Not here: the whole-grid DFT, the point sources and the flux lines (refused on the host while the phase is set).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_bloch.hpp"
#include "kernels_batch_hz.hpp"

namespace fdtd {

// the pole of an Hz Bloch batch: both parts of Jx, Qx, Jy, Qy, cj in the fields' padded layout, a and ck per member
template <class T> struct BatchHzBlochDisp {
    T *jx, *qx, *jy, *qy;          // real parts
    T *jxi, *qxi, *jyi, *qyi;      // imaginary parts
    const T *cj, *a, *ck;
};

// k_batch_resident_hz<T, true, POLE, MAXC> with complex fields.  `bl` carries the imaginary parts in the slots of the
// real ones (ez: Hz, hx: Ex, hy: Ey, ezx: Hzx).  Two barriers per step.
template <class T, bool POLE, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_hz_bloch(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                                BatchBloch<T> bl, BatchHzBlochDisp<T> d,
                                                                                const T *__restrict__ ca, int n0, int nt,
                                                                                long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_hz_bloch_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *shz = reinterpret_cast<T *>(batch_hz_bloch_lds);
    T *sex = shz + seg, *sey = sex + seg, *shzx = sey + seg;
    T *siz = shzx + seg, *six = siz + seg, *siy = six + seg, *sizx = siy + seg;
    T *sch = sizx + seg, *scb = sch + seg, *sca = scb + seg;
    T *scj = sca + seg, *sjx = scj + seg, *sqx = sjx + seg, *sjy = sqx + seg, *sqy = sjy + seg;   // POLE alone
    T *sjxi = sqy + seg, *sqxi = sjxi + seg, *sjyi = sqxi + seg, *sqyi = sjyi + seg;              // POLE alone
    T *sfr = shz + (POLE ? 20 : 11) * seg;    // ahr[R], bhr[R], aer[R], ber[R]
    double *sw = reinterpret_cast<double *>(sfr + batch_lds_seg<T>(4 * R));   // wr[C-1], wi[C-1]
    double *stab = sw + 2 * (C - 1);
    double *sacc = stab + 2 * m.nf, *sacci = sacc + 2 * (size_t)m.nf * m.window();
    BatchMon mi = m;                          // the monitors of the imaginary part: same window, phasors and cells
    mi.acc = bl.acc;
    mi.trace = bl.trace;
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
            shzx[l] = p.ezx[g];
            siz[l] = bl.ez[g];
            six[l] = bl.hx[g];
            siy[l] = bl.hy[g];
            sizx[l] = bl.ezx[g];
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
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = bl.w[(size_t)b * 2 * (C - 1) + k];
        const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = bl.amps && src.r1 > src.r0 ? bl.amps + (size_t)b * v.amp_stride : nullptr;
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
                const bool seam = j == C - 2;             // the right neighbour is the image: rho * column 0
                const T kc = seam ? rc : (T)1, ks = seam ? rs : (T)0;
                T nr, ni;
                batch_bloch_rot(kc, ks, shz[l + 1], siz[l + 1], nr, ni);
                const T hr = shz[l], hi = siz[l];
                const T dxr = shz[l + C] - hr, dyr = nr - hr;
                const T dxi = siz[l + C] - hi, dyi = ni - hi;
                const bool mat = i >= L && i <= R - 2 - L;
                const T a = sca[l], cb = scb[l], fa = sfr[i], fb = sfr[R + i];
                T exr = sex[l], eyr = sey[l], exi = six[l], eyi = siy[l];
                if constexpr (POLE) {
                    const T cj = scj[l];
                    batch_hz_e<T, true, true>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, sjx[l],
                                              sqx[l], sjy[l], sqy[l]);
                    batch_hz_e<T, true, true>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, sjxi[l],
                                              sqxi[l], sjyi[l], sqyi[l]);
                } else {
                    T z = T(0);
                    batch_hz_e<T, true, false>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), da, dck, z, z, z, z, z);
                    batch_hz_e<T, true, false>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), da, dck, z, z, z, z, z);
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
                const bool image = j == C - 1;
                const int lc = image ? l - (C - 1) : l;       // the cell whose update this is
                const int lw = j == 0 ? l + (C - 2) : l - 1;  // its left neighbour, cyclically
                if (i >= 1 && i <= R - 2) {
                    const bool wrap = j == 0 || image;        // that neighbour is across the seam: conj(rho) * Ey
                    const T kc = wrap ? rc : (T)1, ks = wrap ? rs : (T)0;
                    T wr, wi;
                    batch_bloch_unrot(kc, ks, sey[lw], siy[lw], wr, wi);
                    const T cc = sch[lc];
                    const T deyr = sey[lc] - wr, dexr = sex[lc] - sex[lc - C];
                    const T deyi = siy[lc] - wi, dexi = six[lc] - six[lc - C];
                    if (i < L || i > R - 1 - L) {
                        const T fa = sfr[2 * R + i], fb = sfr[3 * R + i];
                        const T xr = shzx[l], xi = sizx[l];
                        const T xnr = batch_periodic_plain(xr, cc, -deyr);
                        const T ynr = batch_hz_split(hr - xr, fa, fb, cc, dexr);
                        const T xni = batch_periodic_plain(xi, cc, -deyi);
                        const T yni = batch_hz_split(hi - xi, fa, fb, cc, dexi);
                        shzx[l] = xnr;
                        sizx[l] = xni;
                        hr = xnr + ynr;
                        hi = xni + yni;
                    } else {
                        hr = batch_hz_plain(hr, deyr - dexr, cc);
                        hi = batch_hz_plain(hi, deyi - dexi, cc);
                    }
                }
                const int js = image ? 0 : j;                 // the image takes column 0's source
                if (src.covers(i, js)) {
                    double dr, dq;
                    batch_bloch_source(ar, ai, sw[js], sw[C - 1 + js], dr, dq);
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
            v.hx[g] = sex[l];
            v.hy[g] = sey[l];
            p.ezx[g] = shzx[l];
            bl.ez[g] = siz[l];
            bl.hx[g] = six[l];
            bl.hy[g] = siy[l];
            bl.ezx[g] = sizx[l];
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

// streamed path, first launch of a step: the E half-step of both parts in place (it also writes the phasors of the step)
template <class T, bool POLE>
__global__ __launch_bounds__(256) void k_batch_e_hz_bloch(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                          BatchHzBlochDisp<T> d, const T *__restrict__ ca, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    const bool seam = j == C - 2;
    const bool mat = i >= L && i <= R - 2 - L;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T kc = seam ? bl.rho[2 * b] : (T)1, ks = seam ? bl.rho[2 * b + 1] : (T)0;
        T nr, ni;
        batch_bloch_rot(kc, ks, v.ez[o + 1], bl.ez[o + 1], nr, ni);
        const T hr = v.ez[o], hi = bl.ez[o];
        const T dxr = v.ez[o + v.pitch] - hr, dyr = nr - hr;
        const T dxi = bl.ez[o + v.pitch] - hi, dyi = ni - hi;
        const T a = ca[o], cb = v.ce[o], fa = fr[i], fb = fr[R + i];
        T exr = v.hx[o], eyr = v.hy[o], exi = bl.hx[o], eyi = bl.hy[o];
        if constexpr (POLE) {
            const T da = d.a[b], dck = d.ck[b], cj = d.cj[o];
            T jx = d.jx[o], qx = d.qx[o], jy = d.jy[o], qy = d.qy[o];
            T jxi = d.jxi[o], qxi = d.qxi[o], jyi = d.jyi[o], qyi = d.qyi[o];
            batch_hz_e<T, true, true>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, jx, qx, jy, qy);
            batch_hz_e<T, true, true>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, jxi, qxi, jyi, qyi);
            if (mat) {
                d.jx[o] = jx;
                d.qx[o] = qx;
                d.jy[o] = jy;
                d.qy[o] = qy;
                d.jxi[o] = jxi;
                d.qxi[o] = qxi;
                d.jyi[o] = jyi;
                d.qyi[o] = qyi;
            }
        } else {
            T z = T(0);
            batch_hz_e<T, true, false>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), z, z, z, z, z, z, z);
            batch_hz_e<T, true, false>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), z, z, z, z, z, z, z);
        }
        v.hx[o] = exr;
        v.hy[o] = eyr;
        bl.hx[o] = exi;
        bl.hy[o] = eyi;
    }
}

// second launch: the H half-step of both parts in place, the source, the image column and the monitors on Hz
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_hz_bloch(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                          int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    const bool image = j == C - 1;
    const bool wrap = j == 0 || image;
    const bool interior = i >= 1 && i <= R - 2;
    const bool layer = i < L || i > R - 1 - L;
    const int js = image ? 0 : j;
    BatchMon mi = m;
    mi.acc = bl.acc;
    mi.trace = bl.trace;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const size_t oc = image ? o - (size_t)(C - 1) : o;
        const size_t ow = j == 0 ? o + (size_t)(C - 2) : o - 1;
        T hr = v.ez[o], hi = bl.ez[o];
        if (interior) {
            const T kc = wrap ? bl.rho[2 * b] : (T)1, ks = wrap ? bl.rho[2 * b + 1] : (T)0;
            T wr, wi;
            batch_bloch_unrot(kc, ks, v.hy[ow], bl.hy[ow], wr, wi);
            const T cc = v.ch[oc];
            const T deyr = v.hy[oc] - wr, dexr = v.hx[oc] - v.hx[oc - v.pitch];
            const T deyi = bl.hy[oc] - wi, dexi = bl.hx[oc] - bl.hx[oc - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R;
                const T fa = fr[2 * R + i], fb = fr[3 * R + i];
                const T xr = p.ezx[o], xi = bl.ezx[o];
                const T xnr = batch_periodic_plain(xr, cc, -deyr);
                const T ynr = batch_hz_split(hr - xr, fa, fb, cc, dexr);
                const T xni = batch_periodic_plain(xi, cc, -deyi);
                const T yni = batch_hz_split(hi - xi, fa, fb, cc, dexi);
                p.ezx[o] = xnr;
                bl.ezx[o] = xni;
                hr = xnr + ynr;
                hi = xni + yni;
            } else {
                hr = batch_hz_plain(hr, deyr - dexr, cc);
                hi = batch_hz_plain(hi, deyi - dexi, cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, js)) {
            const double *w = bl.w + (size_t)b * 2 * (C - 1);
            const double ai = bl.amps ? bl.amps[(size_t)b * v.amp_stride + n] : 0.0;
            double dr, dq;
            batch_bloch_source(src.amps[n], ai, w[js], w[C - 1 + js], dr, dq);
            hr = (T)((double)hr + dr);
            hi = (T)((double)hi + dq);
        }
        v.ez[o] = hr;
        bl.ez[o] = hi;
        batch_mon_cell(m, b, t, i, j, step, (double)hr);
        batch_mon_cell(mi, b, t, i, j, step, (double)hi);
    }
}

// host stubs of the kernels above (batch_hz_bloch.hip): [pole].  MAXC = 4 serves both: eleven arrays leave room for about
// 3700 float32 cells, twenty for about 1900
struct BatchHzBlochKernels {
    const void *resident[2];
    const void *e[2];
    const void *h;
};
template <class T> const BatchHzBlochKernels &batch_hz_bloch_kernels();

}  // namespace fdtd
