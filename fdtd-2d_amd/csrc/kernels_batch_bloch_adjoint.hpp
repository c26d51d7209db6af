// Point sources with channels for the Bloch batch kernels, and the product of two complex windows
// (include/fdtd2d_batch_bloch_adjoint.h).  The three kernels below are k_batch_resident_bloch, k_batch_h_bloch and
// k_batch_e_bloch, step for step, plus the point sources of kernels_batch_adjoint.hpp; they are copies so that the Bloch
// kernels keep their code and registers.  They are instantiated in batch_bloch_adjoint.hip, beside the product kernel.
//
// A point cell takes its float64 sum in the REAL part alone, behind the rectangle source: Ez_re = (T)((double)Ez_re + s).
// The imaginary part takes nothing; the seam carries the real series into it.  A point cell in column 0 is listed a
// second time at its image cell with the same weights (as for any periodic batch), and the image thread adds the same
// sum: the image slot stays the bit-identical, unrotated copy of column 0.
//
// The conjugate rotation (c, -s) of an adjoint run costs no kernel code: the library passes a second table in bl.rho.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_adjoint.hpp"
#include "kernels_batch_bloch.hpp"

namespace fdtd {

// k_batch_resident_bloch with the point sources: LDS = the 11 arrays, the row factors, the source weights, then the phasor
// table, the nc sums of the step and (lds_acc) the accumulators of the real and of the imaginary part.  Two barriers
// per step: the one after H publishes the sums with the phasors.
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_bloch_pts(BatchView<T> v, BatchPml<T> p,
                                                                                 BatchMon m, BatchBloch<T> bl, BatchPts P,
                                                                                 const T *__restrict__ ca, int n0, int nt,
                                                                                 long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_bloch_pts_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_bloch_pts_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg;
    T *siz = sezx + seg, *six = siz + seg, *siy = six + seg, *sizx = siy + seg;
    T *scb = sizx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sfr = sez + 11 * seg;                  // ahr[R], bhr[R], aer[R], ber[R]
    double *sw = reinterpret_cast<double *>(sfr + batch_lds_seg<T>(4 * R));   // wr[C-1], wi[C-1]
    double *stab = sw + 2 * (C - 1), *ssum = stab + 2 * m.nf;
    double *sacc = ssum + P.nc, *sacci = sacc + 2 * (size_t)m.nf * m.window();
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
        const int pts = batch_pts_begin(P, b, tid);
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
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step);
            cells([&](int q, int i, int j, int l) {
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
                if (pts >> q & 1) er = (T)((double)er + ssum[batch_pts_entry(pts, q)]);   // the real part alone
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

// streamed path: k_batch_h_bloch, whose block (0, y) also writes the sums of the run's step n, and k_batch_e_bloch, which
// adds them behind the rectangle source.  Two launches per step, as without point sources.
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_bloch_pts(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                           BatchPts P, int n, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    batch_pts_table(P, v.B, n);
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
__global__ __launch_bounds__(256) void k_batch_e_bloch_pts(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                           BatchPts P, const T *__restrict__ ca, int n, long long step)
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
        er = batch_pts_cell(P, b, t, er);     // the real part alone
        v.ez[o] = er;
        bl.ez[o] = ei;
        batch_mon_cell(m, b, t, i, j, step, (double)er);
        batch_mon_cell(mi, b, t, i, j, step, (double)ei);
    }
}

// host stubs of the kernels above, in BatchBlochKernels' layout, and the complex product's launch
// (batch_bloch_adjoint.hip)
template <class T> const BatchBlochKernels &batch_bloch_pts_kernels();
void batch_bloch_window_product_launch(const double *held_re, const double *held_im, const double *cur_re,
                                       const double *cur_im, const double *coef, double *out, int B, int nf, size_t W,
                                       hipStream_t stream);

}  // namespace fdtd
