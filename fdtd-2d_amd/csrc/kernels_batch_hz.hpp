// The Hz polarisation of PML and periodic batches (include/fdtd2d_batch_hz.h): Hz with Ex and Ey, the electric field in
// the plane, with an electric conductivity and one Drude-Lorentz pole on Ex and Ey.
// Storage is the batch's own: the Ez slot holds Hz, the Hx slot Ex, the Hy slot Ey, the Ezx slot Hzx.  A step is the E
// half-step (the phase in which the Ez kernels advance Hx and Hy), the H half-step (the phase in which they advance Ez),
// then the sources, the image column and the monitors, which see Hz where the Ez kernels see Ez.  What is new is that
// the conductivity and the pole sit in the FIRST phase, on the two edge fields, where the Ez kernels have nothing:
//     jx = a*Jx + (cj*Ex - ck*Qx);  Qx = Qx + jx;  Ex = ca*Ex + (dxi - jx)*cb;  Jx = jx
//     jy = a*Jy + (cj*Ey - ck*Qy);  Qy = Qy + jy;  Ey = ca*Ey - (dyj + jy)*cb;  Jy = jy
// on the material cells; every other cell of the phase takes the layer's update with cb read as ce (sigma is zero there,
// so cb = ce exactly).  The second phase is the split update of Hz mirrored, with ch.
// The kernels are separate kernels (instantiated in batch_hz.hip, reached through batch_hz_kernels()) so that every
// existing one keeps its code and registers.  One kernel serves both boundaries (PER) and both material sets (POLE).
//
// LDS of the resident kernel: Hz, Ex, Ey, Hzx, ch, cb, ca, and with a pole cj, Jx, Qx, Jy, Qy behind them; then the
// factors (4R + 4C slots; a periodic batch never reads the column ones), the phasor table, the point-source sums and the
// window accumulators.  Seven or twelve arrays.  Coefficients and state are read and written at the thread's own cell
// index alone, in the first phase, which already owns Ex[l] and Ey[l]: no new barrier, and no thread reads an Ex, Ey, J
// or Q that another thread writes in that phase.
//
// The periodic image: the thread that owns (i, C-1) recomputes column 0's Hz update in the second phase from column 0's
// Ex, Ey and ch and its own Hz / Hzx as the old values, exactly as k_batch_resident_periodic does for Ez.  Ex, Ey and the
// pole state have no image: the first phase never touches column C-1, and Ey[i, C-2] reads the image of Hz, which the
// second phase of the step before has refreshed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_dispersive.hpp"

namespace fdtd {

// the pole of an Hz batch: Jx, Qx, Jy, Qy, cj in the fields' padded layout, a and ck per member
template <class T> struct BatchHzDisp {
    T *jx, *qx, *jy, *qy;
    const T *cj, *a, *ck;
};

// a * x + (b * c) * d: Ex with the row factors, and the y-part of Hz in the layer.  One rounding per operation in the
// exact build; the fma written out in the fused one (as in batch_periodic_split, its mirror) so that every path
// contracts alike
template <class T> __device__ __forceinline__ T batch_hz_split(T x, T a, T b, T c, T d)
{
#ifdef FDTD2D_FUSED
    return batch_periodic_fma(b * c, d, a * x);
#else
    return a * x + (b * c) * d;
#endif
}
// h - curl * ch: Hz outside the layer
template <class T> __device__ __forceinline__ T batch_hz_plain(T h, T curl, T ch)
{
#ifdef FDTD2D_FUSED
    return batch_periodic_fma(-curl, ch, h);
#else
    return h - curl * ch;
#endif
}

// The first phase of one cell (i <= R-2, j <= C-2): Ex and Ey from the differences of Hz.  `mat`: a material cell.
// jx, qx, jy, qy: the cell's pole state by reference (LDS slots, or registers that the caller stores); POLE alone.
template <class T, bool PER, bool POLE>
__device__ __forceinline__ void batch_hz_e(T &ex, T &ey, T dxi, T dyj, bool mat, T ca, T cb, T ahr, T bhr, T ahc, T bhc,
                                           T da, T dck, T cj, T &jx, T &qx, T &jy, T &qy)
{
    if (mat) {
        if constexpr (POLE) {
            const T nx = batch_disp_j(da, jx, cj, ex, dck, qx);
            qx = qx + nx;
            ex = batch_lossy_e(ex, dxi - nx, ca, cb);
            jx = nx;
            const T ny = batch_disp_j(da, jy, cj, ey, dck, qy);
            qy = qy + ny;
            ey = batch_lossy_e(ey, -(dyj + ny), ca, cb);
            jy = ny;
        } else {
            ex = batch_lossy_e(ex, dxi, ca, cb);
            ey = batch_lossy_e(ey, -dyj, ca, cb);
        }
    } else {
        ex = batch_hz_split(ex, ahr, bhr, cb, dxi);
        if constexpr (PER) ey = batch_periodic_plain(ey, cb, -dyj);   // the column factors are exactly 1
        else ey = batch_periodic_split(ey, ahc, bhc, cb, dyj);
    }
}

// k_batch_resident_pml_lossy / k_batch_resident_periodic in the Hz polarisation
template <class T, bool PER, bool POLE, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_hz(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                          BatchPts P, BatchHzDisp<T> d,
                                                                          const T *__restrict__ ca, int n0, int nt,
                                                                          long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_hz_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *shz = reinterpret_cast<T *>(batch_hz_lds);
    T *sex = shz + seg, *sey = sex + seg, *shzx = sey + seg, *sch = shzx + seg, *scb = sch + seg, *sca = scb + seg;
    T *scj = sca + seg, *sjx = scj + seg, *sqx = sjx + seg, *sjy = sqx + seg, *sqy = sjy + seg;   // POLE alone
    T *sfr = shz + (POLE ? 12 : 7) * seg;     // ahr[R], bhr[R], aer[R], ber[R]
    T *sfc = sfr + batch_lds_seg<T>(4 * R);   // ahc[C], bhc[C], aec[C], bec[C] (PER: exactly 1, never read)
    double *stab = reinterpret_cast<double *>(sfc + batch_lds_seg<T>(4 * C)), *ssum = stab + 2 * m.nf;
    double *sacc = ssum + P.nc;
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
            sch[l] = v.ch[g];
            scb[l] = v.ce[g];
            sca[l] = ca[g];
            if constexpr (POLE) {
                scj[l] = d.cj[g];
                sjx[l] = d.jx[g];
                sqx[l] = d.qx[g];
                sjy[l] = d.jy[g];
                sqy[l] = d.qy[g];
            }
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        if constexpr (!PER)
            for (int k = tid; k < 4 * C; k += nthr) sfc[k] = p.colf[(size_t)b * 4 * C + k];
        BatchSource<T> src;
        src.load(v, b);
        T da = T(0), dck = T(0);
        if constexpr (POLE) {
            da = d.a[b];
            dck = d.ck[b];
        }
        const double omega = v.dft ? v.omega[b] : 0.0;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const int pts = batch_pts_begin(P, b, tid);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {   // the E half-step
                if (i > R - 2 || j > C - 2) return;
                const T h = shz[l];
                const T dxi = shz[l + C] - h, dyj = shz[l + 1] - h;
                const bool mat = i >= L && i <= R - 2 - L && (PER || (j >= L && j <= C - 2 - L));
                T ex = sex[l], ey = sey[l];
                if constexpr (POLE) {
                    batch_hz_e<T, PER, true>(ex, ey, dxi, dyj, mat, sca[l], scb[l], sfr[i], sfr[R + i],
                                             PER ? T(1) : sfc[j], PER ? T(1) : sfc[C + j], da, dck, scj[l], sjx[l],
                                             sqx[l], sjy[l], sqy[l]);
                } else {
                    T z = T(0);
                    batch_hz_e<T, PER, false>(ex, ey, dxi, dyj, mat, sca[l], scb[l], sfr[i], sfr[R + i],
                                              PER ? T(1) : sfc[j], PER ? T(1) : sfc[C + j], da, dck, z, z, z, z, z);
                }
                sex[l] = ex;
                sey[l] = ey;
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step);
            const bool sampled = m.sampled(step);
            cells([&](int q, int i, int j, int l) {   // the H half-step, the sources, the monitors
                T h = shz[l];
                const bool image = PER && j == C - 1;
                const int lc = image ? l - (C - 1) : l;              // the cell whose update this is
                const int lw = PER && j == 0 ? l + (C - 2) : l - 1;  // its left neighbour (PER: cyclically)
                if (i >= 1 && i <= R - 2 && (PER || (j >= 1 && j <= C - 2))) {
                    const T cc = sch[lc];
                    const T dey = sey[lc] - sey[lw], dex = sex[lc] - sex[lc - C];
                    if (i < L || i > R - 1 - L || (!PER && (j < L || j > C - 1 - L))) {
                        const T x = shzx[l];
                        T y = h - x;
                        T xn;
                        if constexpr (PER) xn = batch_periodic_plain(x, cc, -dey);
                        else xn = batch_periodic_split(x, sfc[2 * C + j], sfc[3 * C + j], cc, dey);
                        y = batch_hz_split(y, sfr[2 * R + i], sfr[3 * R + i], cc, dex);
                        shzx[l] = xn;
                        h = xn + y;
                    } else {
                        h = batch_hz_plain(h, dey - dex, cc);
                    }
                }
                if (src.covers(i, image ? 0 : j)) h = (T)((double)h + amp);
                if (pts >> q & 1) h = (T)((double)h + ssum[batch_pts_entry(pts, q)]);
                shz[l] = h;
                if (ph.on) {
                    double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)l;
                    dd[0] += (double)h * ph.c;
                    dd[R * C] += (double)h * ph.s;
                }
                if (sampled) {
                    // two copies of the adds, so that the LDS one uses LDS instructions, not flat ones
                    const int w = m.window_cell(i, j);
                    if (w >= 0 && m.lds_acc) m.add(sacc, stab, w, (double)h);
                    else if (w >= 0) m.add(mon.acc, stab, w, (double)h);
                }
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, shz, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = shz[l];
            v.hx[g] = sex[l];
            v.hy[g] = sey[l];
            p.ezx[g] = shzx[l];
            if constexpr (POLE) {
                d.jx[g] = sjx[l];
                d.qx[g] = sqx[l];
                d.jy[g] = sjy[l];
                d.qy[g] = sqy[l];
            }
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed path, first launch of a step: the E half-step in place (it also writes the phasors and the point-source sums
// of the step, as the Ez paths' H launch does)
template <class T, bool PER, bool POLE>
__global__ __launch_bounds__(256) void k_batch_e_hz(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                    BatchHzDisp<T> d, const T *__restrict__ ca, int n, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    batch_pts_table(P, v.B, n);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    const bool mat = i >= L && i <= R - 2 - L && (PER || (j >= L && j <= C - 2 - L));
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R, *fc = p.colf + (size_t)b * 4 * C;
        const T h = v.ez[o];
        const T dxi = v.ez[o + v.pitch] - h, dyj = v.ez[o + 1] - h;
        T ex = v.hx[o], ey = v.hy[o];
        const T ahc = PER ? T(1) : fc[j], bhc = PER ? T(1) : fc[C + j];
        if constexpr (POLE) {
            T jx = d.jx[o], qx = d.qx[o], jy = d.jy[o], qy = d.qy[o];
            batch_hz_e<T, PER, true>(ex, ey, dxi, dyj, mat, ca[o], v.ce[o], fr[i], fr[R + i], ahc, bhc, d.a[b], d.ck[b],
                                     d.cj[o], jx, qx, jy, qy);
            if (mat) {
                d.jx[o] = jx;
                d.qx[o] = qx;
                d.jy[o] = jy;
                d.qy[o] = qy;
            }
        } else {
            T z = T(0);
            batch_hz_e<T, PER, false>(ex, ey, dxi, dyj, mat, ca[o], v.ce[o], fr[i], fr[R + i], ahc, bhc, z, z, z, z, z,
                                      z, z);
        }
        v.hx[o] = ex;
        v.hy[o] = ey;
    }
}

// second launch: the H half-step in place, the sources, the image column and the monitors on Hz
template <class T, bool PER>
__global__ __launch_bounds__(256) void k_batch_h_hz(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P, int n,
                                                    long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    const bool image = PER && j == C - 1;
    const bool interior = i >= 1 && i <= R - 2 && (PER || (j >= 1 && j <= C - 2));
    const bool layer = i < L || i > R - 1 - L || (!PER && (j < L || j > C - 1 - L));
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const size_t oc = image ? o - (size_t)(C - 1) : o;
        const size_t ow = PER && j == 0 ? o + (size_t)(C - 2) : o - 1;
        T h = v.ez[o];
        if (interior) {
            const T cc = v.ch[oc];
            const T dey = v.hy[oc] - v.hy[ow], dex = v.hx[oc] - v.hx[oc - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R, *fc = p.colf + (size_t)b * 4 * C;
                const T x = p.ezx[o];
                T y = h - x;
                T xn;
                if constexpr (PER) xn = batch_periodic_plain(x, cc, -dey);
                else xn = batch_periodic_split(x, fc[2 * C + j], fc[3 * C + j], cc, dey);
                y = batch_hz_split(y, fr[2 * R + i], fr[3 * R + i], cc, dex);
                p.ezx[o] = xn;
                h = xn + y;
            } else {
                h = batch_hz_plain(h, dey - dex, cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, image ? 0 : j)) h = (T)((double)h + src.amps[n]);
        h = batch_pts_cell(P, b, t, h);
        v.ez[o] = h;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)t;
            dd[0] += (double)h * ph.c;
            dd[R * C] += (double)h * ph.s;
        }
        batch_mon_cell(m, b, t, i, j, step, (double)h);
    }
}

// host stubs of the kernels above (batch_hz.hip): [periodic][pole], the resident ones also [MAXC 4, 8] (only a float32
// member without a pole has more than 4 cells per thread: seven arrays of 4 B leave room for about 5800 cells)
struct BatchHzKernels {
    const void *resident[2][2][2];
    const void *e[2][2];
    const void *h[2];
};
template <class T> const BatchHzKernels &batch_hz_kernels();

}  // namespace fdtd
