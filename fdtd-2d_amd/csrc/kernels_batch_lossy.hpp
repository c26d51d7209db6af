// Lossy materials for the batched kernels (include/fdtd2d_batch_lossy.h): an electric conductivity per cell.
// With s = sigma dt / (2 eps), ca = (1 - s)/(1 + s) and cb = ce / (1 + s), the cells that take the reference's plain
// update take e = ca * e + (dhy - dhx) * cb instead; H, the Mur frame, the PML branch, the sources and the monitors are
// those of the point-source kernels (kernels_batch_adjoint.hpp), step for step.  The conductivity is zero in the frame
// and the layer, where ca = 1 and cb = ce exactly, so the frame rules and the PML branch read cb as their ce.
// The kernels below are separate kernels (instantiated in batch_lossy.hip, reached through batch_lossy_kernels()) so
// that every existing one keeps its code and registers.  There is no uniform-material instance, and the streamed H
// launches are the point-source ones themselves: H does not see the conductivity.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_adjoint.hpp"

namespace fdtd {

// ca * e + curl * cb: two roundings apart in the exact build, fma(curl, cb, ca * e) in the fused one
template <class T> __device__ __forceinline__ T batch_lossy_e(T e, T curl, T ca, T cb)
{
#ifdef FDTD2D_FUSED
    if constexpr (sizeof(T) == 4) return __builtin_fmaf(curl, cb, ca * e);
    else return __builtin_fma(curl, cb, ca * e);
#else
    return ca * e + curl * cb;
#endif
}

// Stage A (MurRules::a) with the lossy update, over MurRules' accessor with ce(i, j) = cb, and ca in the same layout
// (at: the accessor's index of a cell).  Only the cells outside the 5-cell frame take it: a frame cell's rule reads
// stage A up to row / column 5 (and R - 6 / C - 6), where the conductivity is zero, ca = 1 and cb = ce, so there
// MurRules itself, reading cb as its ce, gives the lossy value bit for bit.
template <class T, class Acc>
__device__ __forceinline__ T batch_lossy_a(const Acc &m, const T *ca, size_t at, int i, int j)
{
    const T e = m.p(i, j);
    if (i < 1 || i > m.R - 2 || j < 1 || j > m.C - 2) return e;
    return batch_lossy_e(e, (m.hy(i, j) - m.hy(i, j - 1)) - (m.hx(i, j) - m.hx(i - 1, j)), ca[at], m.ce(i, j));
}
__device__ __forceinline__ bool batch_in_frame(int i, int j, int R, int C)
{
    return i < 5 || i >= R - 5 || j < 5 || j >= C - 5;
}

// ---- the kernels: v.ce holds cb, ca is its companion in the same layout ------------------------------------------
// k_batch_resident_mon_pts with the lossy update: LDS = Ez, Hx, Hy, cb, ch, ca, then the phasor table, the nc sums of
// the step and (lds_acc) the accumulators.  ca sits behind ch so that every array before it keeps its offset; it is
// read at the thread's own cell index like the others (neighbouring lanes, neighbouring banks).
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_lossy(BatchView<T> v, BatchMon m, BatchPts P,
                                                                             const T *__restrict__ ca, int n0, int nt,
                                                                             long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_lossy_lds[];
    const int R = v.R, C = v.C;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_lossy_lds);
    T *shx = sez + seg, *shy = shx + seg, *scb = shy + seg, *sch = scb + seg, *sca = sch + seg;
    double *stab = reinterpret_cast<double *>(sez + 6 * seg), *ssum = stab + 2 * m.nf;
    double *sacc = ssum + P.nc;
    const int di = nthr / C, dj = nthr % C, ti = tid / C, tj = tid % C;
    auto cells = [&](auto &&body) {   // the cell walk of k_batch_resident
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
    const LdsAcc<T, true> acc{sez, shx, shy, scb, T(0), R, C};

    for (int b = blockIdx.x; b < v.B; b += gridDim.x) {
        const size_t base = (size_t)b * v.mstride;
        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            sez[l] = v.ez[g];
            shx[l] = v.hx[g];
            shy[l] = v.hy[g];
            scb[l] = v.ce[g];
            sch[l] = v.ch[g];
            sca[l] = ca[g];
        });
        const MurRules<T, LdsAcc<T, true>> f{acc, v.kmur[b]};
        BatchSource<T> src;
        src.load(v, b);
        const double omega = v.dft ? v.omega[b] : 0.0;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const int pts = batch_pts_begin(P, b, tid);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const T e = sez[l];
                const T cc = sch[l];
                shx[l] = shx[l] - cc * (sez[l + C] - e);
                shy[l] = shy[l] + cc * (sez[l + 1] - e);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            T out[MAXC];
            cells([&](int q, int i, int j, int l) {
                out[q] = v.mur && batch_in_frame(i, j, R, C) ? f.d(i, j) : batch_lossy_a(acc, sca, (size_t)l, i, j);
            });
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step);
            const bool sampled = m.sampled(step);
            cells([&](int q, int i, int j, int l) {
                T e = out[q];
                if (src.covers(i, j)) e = (T)((double)e + amp);
                if (pts >> q & 1) e = (T)((double)e + ssum[batch_pts_entry(pts, q)]);
                sez[l] = e;
                if (ph.on) {
                    double *d = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)l;
                    d[0] += (double)e * ph.c;
                    d[R * C] += (double)e * ph.s;
                }
                if (sampled) {
                    // two copies of the adds, so that the LDS one uses LDS instructions, not flat ones
                    const int w = m.window_cell(i, j);
                    if (w >= 0 && m.lds_acc) m.add(sacc, stab, w, (double)e);
                    else if (w >= 0) m.add(mon.acc, stab, w, (double)e);
                }
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, sez, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = sez[l];
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// k_batch_resident_pml_mon_pts with the lossy update: LDS = Ez, Hx, Hy, Ezx, cb, ch, ca, the factors, then the phasor
// table, the nc sums of the step and (lds_acc) the accumulators.
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_pml_lossy(BatchView<T> v, BatchPml<T> p,
                                                                                 BatchMon m, BatchPts P,
                                                                                 const T *__restrict__ ca, int n0,
                                                                                 int nt, long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_lossy_pml_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_lossy_pml_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *scb = sezx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sfr = sez + 7 * seg;                   // ahr[R], bhr[R], aer[R], ber[R]
    T *sfc = sfr + batch_lds_seg<T>(4 * R);   // ahc[C], bhc[C], aec[C], bec[C]
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
            sez[l] = v.ez[g];
            shx[l] = v.hx[g];
            shy[l] = v.hy[g];
            sezx[l] = p.ezx[g];
            scb[l] = v.ce[g];
            sch[l] = v.ch[g];
            sca[l] = ca[g];
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        for (int k = tid; k < 4 * C; k += nthr) sfc[k] = p.colf[(size_t)b * 4 * C + k];
        BatchSource<T> src;
        src.load(v, b);
        const double omega = v.dft ? v.omega[b] : 0.0;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const int pts = batch_pts_begin(P, b, tid);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const T e = sez[l];
                const T cc = sch[l];
                shx[l] = sfr[i] * shx[l] - (sfr[R + i] * cc) * (sez[l + C] - e);
                shy[l] = sfc[j] * shy[l] + (sfc[C + j] * cc) * (sez[l + 1] - e);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step);
            const bool sampled = m.sampled(step);
            cells([&](int q, int i, int j, int l) {
                T e = sez[l];
                if (i >= 1 && i <= R - 2 && j >= 1 && j <= C - 2) {
                    const T cc = scb[l];
                    const T dhy = shy[l] - shy[l - 1], dhx = shx[l] - shx[l - C];
                    if (i < L || i > R - 1 - L || j < L || j > C - 1 - L) {
                        const T x = sezx[l];
                        T ey = e - x;
                        const T ex = sfc[2 * C + j] * x + (sfc[3 * C + j] * cc) * dhy;
                        ey = sfr[2 * R + i] * ey - (sfr[3 * R + i] * cc) * dhx;
                        sezx[l] = ex;
                        e = ex + ey;
                    } else {
                        e = batch_lossy_e(e, dhy - dhx, sca[l], cc);
                    }
                }
                if (src.covers(i, j)) e = (T)((double)e + amp);
                if (pts >> q & 1) e = (T)((double)e + ssum[batch_pts_entry(pts, q)]);
                sez[l] = e;
                if (ph.on) {
                    double *d = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)l;
                    d[0] += (double)e * ph.c;
                    d[R * C] += (double)e * ph.s;
                }
                if (sampled) {
                    // two copies of the adds, so that the LDS one uses LDS instructions, not flat ones
                    const int w = m.window_cell(i, j);
                    if (w >= 0 && m.lds_acc) m.add(sacc, stab, w, (double)e);
                    else if (w >= 0) m.add(mon.acc, stab, w, (double)e);
                }
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, sez, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = sez[l];
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
            p.ezx[g] = sezx[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed path: k_batch_e_mon_pts and k_batch_e_pml_mon_pts with the lossy update, behind the H launches of
// k_batch_h_mon_pts / k_batch_h_pml_mon_pts (which also write the phasors and the sums of the step)
template <class T>
__global__ __launch_bounds__(256) void k_batch_e_lossy(BatchView<T> v, BatchMon m, BatchPts P,
                                                       const T *__restrict__ ca, T *__restrict__ ez_new, int n,
                                                       long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int i = t / v.C, j = t % v.C;
    const Geom g{v.R, v.C, 0, v.pitch};
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t base = (size_t)b * v.mstride;
        const FrameCtx<T, true> f{{v.ez + base, v.hx + base, v.hy + base, v.ce + base, T(0), g, v.R, v.C}, v.kmur[b]};
        T e = v.mur && batch_in_frame(i, j, v.R, v.C) ? f.d(i, j) : batch_lossy_a(f.m, ca + base, at(g, i, j), i, j);
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, j)) e = (T)((double)e + src.amps[n]);
        e = batch_pts_cell(P, b, t, e);
        ez_new[base + at(g, i, j)] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *d = v.dft + (size_t)b * 2 * (size_t)(v.R * v.C) + (size_t)t;
            d[0] += (double)e * ph.c;
            d[v.R * v.C] += (double)e * ph.s;
        }
        batch_mon_cell(m, b, t, i, j, step, (double)e);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_batch_e_pml_lossy(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                           const T *__restrict__ ca, int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    const bool interior = i >= 1 && i <= R - 2 && j >= 1 && j <= C - 2;
    const bool layer = i < L || i > R - 1 - L || j < L || j > C - 1 - L;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        T e = v.ez[o];
        if (interior) {
            const T cc = v.ce[o];
            const T dhy = v.hy[o] - v.hy[o - 1], dhx = v.hx[o] - v.hx[o - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R, *fc = p.colf + (size_t)b * 4 * C;
                const T x = p.ezx[o];
                T ey = e - x;
                const T ex = fc[2 * C + j] * x + (fc[3 * C + j] * cc) * dhy;
                ey = fr[2 * R + i] * ey - (fr[3 * R + i] * cc) * dhx;
                p.ezx[o] = ex;
                e = ex + ey;
            } else {
                e = batch_lossy_e(e, dhy - dhx, ca[o], cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, j)) e = (T)((double)e + src.amps[n]);
        e = batch_pts_cell(P, b, t, e);
        v.ez[o] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *d = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)t;
            d[0] += (double)e * ph.c;
            d[R * C] += (double)e * ph.s;
        }
        batch_mon_cell(m, b, t, i, j, step, (double)e);
    }
}

// the lossy coefficients of a window (twin of k_batch_eps_window): w holds count x nr x nc conductivities, then as
// many permittivities as the engine stores them, both float64.  s = sigma dt / (2 eps) in float64;
// ca = (T)((1 - s)/(1 + s)), cb = ce * (T)(1/(1 + s)) with ce as the batch holds it.
template <class T>
__global__ __launch_bounds__(256) void k_batch_sigma_window(T *__restrict__ ca, T *__restrict__ cb,
                                                            const T *__restrict__ ce, const double *__restrict__ w,
                                                            int B, int r0, int c0, int nr, int nc, long long pitch,
                                                            size_t mstride, double dt)
{
    const size_t W = (size_t)nr * nc, n = (size_t)B * W;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const size_t b = t / W;
        const int r = (int)(t - b * W), wi = r / nc, wj = r - wi * nc;
        const double s = w[t] * dt / (2.0 * w[n + t]);
        const size_t g = b * mstride + (size_t)(r0 + wi) * pitch + (c0 + wj);
        ca[g] = (T)((1.0 - s) / (1.0 + s));
        cb[g] = ce[g] * (T)(1.0 / (1.0 + s));
    }
}

// host stubs of the kernels above (batch_lossy.hip): [MAXC 4, 8, 16]
struct BatchLossyKernels {
    const void *resident[3], *resident_pml[3];
    const void *e, *e_pml;
};
template <class T> const BatchLossyKernels &batch_lossy_kernels();
void batch_sigma_window_launch(void *ca, void *cb, const void *ce, const double *w, bool dtype_f64, int B, int r0,
                               int c0, int nr, int nc, long long pitch, size_t mstride, double dt, hipStream_t stream);

}  // namespace fdtd
