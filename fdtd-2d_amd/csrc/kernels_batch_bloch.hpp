// A Bloch phase for the periodic batch kernels (include/fdtd2d_batch_bloch.h): copies of k_batch_resident_periodic,
// k_batch_h_periodic and k_batch_e_periodic with every field a pair (real part, imaginary part) of T and the seam
// rotated by the member's rho = (c, s).  Every coefficient is real, so each part takes the periodic step unchanged;
// the parts meet in two places only:
//   H, j = C-2: the right neighbour of Ez is rho * image (re' = c*re - s*im, im' = s*re + c*im)
//   E, column 0 (and the image thread's copy of that update): the left neighbour of Hy is conj(rho) * Hy[i, C-2]
//               (re' = c*hr + s*hi, im' = c*hi - s*hr)
// The image slot of Ez and Ezx holds the UNROTATED copy of column 0 (in LDS and in global memory), so the periodic
// kernels' induction carries over: the image thread evaluates column 0's update from column 0's operands, its own value
// as the old one and column 0's source weight, the image stays bit-identical to column 0, two barriers per step, and
// the streamed E kernel stays in place and race-free.
//
// The seam costs no branch: rho is applied everywhere with the coefficients selected (c, s) on the seam and (1, 0)
// elsewhere; 1*x - 0*y and fma(1, x, -(0*y)) return x (a signed zero aside).  A wave diverges only on the two column
// tests of the periodic kernel.  The pair of a cell is read with one LDS index from two arrays (not interleaved), which
// keeps the periodic kernel's access pattern: consecutive lanes, consecutive words, apart from column 0's word.
//
// Not here: the whole-grid DFT and the point sources (refused on the host while a Bloch phase is set).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_periodic.hpp"

namespace fdtd {

// the imaginary parts and what else a Bloch batch adds to the periodic kernels' arguments
template <class T> struct BatchBloch {
    T *ez, *hx, *hy, *ezx;    // imaginary parts, the layout of the real ones
    const T *rho;             // count x {c, s}
    const double *w;          // count x {wr[C-1], wi[C-1]}: the source weight of columns 0..C-2
    const double *amps;       // imaginary amplitudes, amps[b * amp_stride + n] (the view's stride); nullptr = zero
    double *acc;              // the window DFT of the imaginary part (BatchMon::acc's layout)
    double *trace;            // the probe traces of the imaginary part (BatchMon::trace's layout)
};

// rho * (re, im): two products and one sum each.  The fused build writes the fma out (see batch_periodic_split).
template <class T> __device__ __forceinline__ void batch_bloch_rot(T c, T s, T re, T im, T &ore, T &oim)
{
#ifdef FDTD2D_FUSED
    ore = batch_periodic_fma(c, re, -(s * im));
    oim = batch_periodic_fma(s, re, c * im);
#else
    ore = c * re - s * im;
    oim = s * re + c * im;
#endif
}
// conj(rho) * (re, im)
template <class T> __device__ __forceinline__ void batch_bloch_unrot(T c, T s, T re, T im, T &ore, T &oim)
{
#ifdef FDTD2D_FUSED
    ore = batch_periodic_fma(c, re, s * im);
    oim = batch_periodic_fma(c, im, -(s * re));
#else
    ore = c * re + s * im;
    oim = c * im - s * re;
#endif
}
// a * w in float64: what the rectangle source adds to the two parts
__device__ __forceinline__ void batch_bloch_source(double ar, double ai, double wr, double wi, double &dr, double &di)
{
#ifdef FDTD2D_FUSED
    dr = __builtin_fma(ar, wr, -(ai * wi));
    di = __builtin_fma(ar, wi, ai * wr);
#else
    dr = ar * wr - ai * wi;
    di = ar * wi + ai * wr;
#endif
}

// LDS of one resident member in bytes before the monitors: 11 arrays, the row factors, the source weights
template <class T> __host__ __device__ __forceinline__ size_t batch_bloch_lds_bytes(int R, int C)
{
    return (11 * batch_lds_seg<T>(R * C) + batch_lds_seg<T>(4 * R)) * sizeof(T) + 16 * (size_t)(C - 1);
}

// k_batch_resident_periodic with complex fields: LDS = Ez, Hx, Hy, Ezx (real), Ez, Hx, Hy, Ezx (imaginary), cb, ch, ca,
// the row factors, the source weights, then the phasor table and (lds_acc) the accumulators of the real and of the
// imaginary part.  Two barriers per step.
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_bloch(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                             BatchBloch<T> bl,
                                                                             const T *__restrict__ ca, int n0, int nt,
                                                                             long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_bloch_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_bloch_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg;
    T *siz = sezx + seg, *six = siz + seg, *siy = six + seg, *sizx = siy + seg;
    T *scb = sizx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sfr = sez + 11 * seg;                  // ahr[R], bhr[R], aer[R], ber[R]
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
            sez[l] = v.ez[g];
            shx[l] = v.hx[g];
            shy[l] = v.hy[g];
            sezx[l] = p.ezx[g];
            siz[l] = bl.ez[g];
            six[l] = bl.hx[g];
            siy[l] = bl.hy[g];
            sizx[l] = bl.ezx[g];
            scb[l] = v.ce[g];
            sch[l] = v.ch[g];
            sca[l] = ca[g];
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = bl.w[(size_t)b * 2 * (C - 1) + k];
        const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = bl.amps && src.r1 > src.r0 ? bl.amps + (size_t)b * v.amp_stride : nullptr;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const BatchMonMember moni = batch_mon_begin(mi, b, sacci, tid, nthr);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const bool seam = j == C - 2;             // the right neighbour is the image: rho * column 0
                const T kc = seam ? rc : (T)1, ks = seam ? rs : (T)0;
                T nr, ni;
                batch_bloch_rot(kc, ks, sez[l + 1], siz[l + 1], nr, ni);
                const T cc = sch[l], fa = sfr[i], fb = sfr[R + i];
                const T er = sez[l], ei = siz[l];
                shx[l] = batch_periodic_split(shx[l], fa, fb, cc, sez[l + C] - er);
                shy[l] = batch_periodic_plain(shy[l], cc, nr - er);
                six[l] = batch_periodic_split(six[l], fa, fb, cc, siz[l + C] - ei);
                siy[l] = batch_periodic_plain(siy[l], cc, ni - ei);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step);
            cells([&](int, int i, int j, int l) {
                T er = sez[l], ei = siz[l];
                const bool image = j == C - 1;
                const int lc = image ? l - (C - 1) : l;       // the cell whose update this is
                const int lw = j == 0 ? l + (C - 2) : l - 1;  // its left neighbour, cyclically
                if (i >= 1 && i <= R - 2) {
                    const bool wrap = j == 0 || image;        // that neighbour is across the seam: conj(rho) * Hy
                    const T kc = wrap ? rc : (T)1, ks = wrap ? rs : (T)0;
                    T wr, wi;
                    batch_bloch_unrot(kc, ks, shy[lw], siy[lw], wr, wi);
                    const T cc = scb[lc];
                    const T dhyr = shy[lc] - wr, dhxr = shx[lc] - shx[lc - C];
                    const T dhyi = siy[lc] - wi, dhxi = six[lc] - six[lc - C];
                    if (i < L || i > R - 1 - L) {
                        const T fa = sfr[2 * R + i], fb = sfr[3 * R + i];
                        const T xr = sezx[l], xi = sizx[l];
                        const T exr = batch_periodic_plain(xr, cc, dhyr);
                        const T eyr = batch_periodic_split(er - xr, fa, fb, cc, dhxr);
                        const T exi = batch_periodic_plain(xi, cc, dhyi);
                        const T eyi = batch_periodic_split(ei - xi, fa, fb, cc, dhxi);
                        sezx[l] = exr;
                        sizx[l] = exi;
                        er = exr + eyr;
                        ei = exi + eyi;
                    } else {
                        const T a = sca[lc];
                        er = batch_lossy_e(er, dhyr - dhxr, a, cc);
                        ei = batch_lossy_e(ei, dhyi - dhxi, a, cc);
                    }
                }
                const int js = image ? 0 : j;                 // the image takes column 0's source
                if (src.covers(i, js)) {
                    double dr, dq;
                    batch_bloch_source(ar, ai, sw[js], sw[C - 1 + js], dr, dq);
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
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
            p.ezx[g] = sezx[l];
            bl.ez[g] = siz[l];
            bl.hx[g] = six[l];
            bl.hy[g] = siy[l];
            bl.ezx[g] = sizx[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        batch_mon_end(mi, b, sacci, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed path: k_batch_h_periodic (which also writes the phasors of the step) and k_batch_e_periodic, in place, with
// the arithmetic of the resident kernel above
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_bloch(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                       long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    const bool seam = j == C - 2;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T kc = seam ? bl.rho[2 * b] : (T)1, ks = seam ? bl.rho[2 * b + 1] : (T)0;
        T nr, ni;
        batch_bloch_rot(kc, ks, v.ez[o + 1], bl.ez[o + 1], nr, ni);
        const T cc = v.ch[o], fa = fr[i], fb = fr[R + i];
        const T er = v.ez[o], ei = bl.ez[o];
        v.hx[o] = batch_periodic_split(v.hx[o], fa, fb, cc, v.ez[o + v.pitch] - er);
        v.hy[o] = batch_periodic_plain(v.hy[o], cc, nr - er);
        bl.hx[o] = batch_periodic_split(bl.hx[o], fa, fb, cc, bl.ez[o + v.pitch] - ei);
        bl.hy[o] = batch_periodic_plain(bl.hy[o], cc, ni - ei);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_batch_e_bloch(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                       const T *__restrict__ ca, int n, long long step)
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
        T er = v.ez[o], ei = bl.ez[o];
        if (interior) {
            const T kc = wrap ? bl.rho[2 * b] : (T)1, ks = wrap ? bl.rho[2 * b + 1] : (T)0;
            T wr, wi;
            batch_bloch_unrot(kc, ks, v.hy[ow], bl.hy[ow], wr, wi);
            const T cc = v.ce[oc];
            const T dhyr = v.hy[oc] - wr, dhxr = v.hx[oc] - v.hx[oc - v.pitch];
            const T dhyi = bl.hy[oc] - wi, dhxi = bl.hx[oc] - bl.hx[oc - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R;
                const T fa = fr[2 * R + i], fb = fr[3 * R + i];
                const T xr = p.ezx[o], xi = bl.ezx[o];
                const T exr = batch_periodic_plain(xr, cc, dhyr);
                const T eyr = batch_periodic_split(er - xr, fa, fb, cc, dhxr);
                const T exi = batch_periodic_plain(xi, cc, dhyi);
                const T eyi = batch_periodic_split(ei - xi, fa, fb, cc, dhxi);
                p.ezx[o] = exr;
                bl.ezx[o] = exi;
                er = exr + eyr;
                ei = exi + eyi;
            } else {
                const T a = ca[oc];
                er = batch_lossy_e(er, dhyr - dhxr, a, cc);
                ei = batch_lossy_e(ei, dhyi - dhxi, a, cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, js)) {
            const double *w = bl.w + (size_t)b * 2 * (C - 1);
            const double ai = bl.amps ? bl.amps[(size_t)b * v.amp_stride + n] : 0.0;
            double dr, dq;
            batch_bloch_source(src.amps[n], ai, w[js], w[C - 1 + js], dr, dq);
            er = (T)((double)er + dr);
            ei = (T)((double)ei + dq);
        }
        v.ez[o] = er;
        bl.ez[o] = ei;
        batch_mon_cell(m, b, t, i, j, step, (double)er);
        batch_mon_cell(mi, b, t, i, j, step, (double)ei);
    }
}

// host stubs of the kernels above (batch_bloch.hip)
struct BatchBlochKernels {
    const void *resident, *h, *e;
};
template <class T> const BatchBlochKernels &batch_bloch_kernels();

}  // namespace fdtd
