// Point sources with channels for the batched kernels (include/fdtd2d_batch_adjoint.h).  The kernels below are the
// monitored kernels of kernels_batch_monitor.hpp, step for step, plus the point sources; they are separate kernels so
// that the monitored ones keep their code and registers, as those are separate from the unmonitored ones.  They are
// instantiated in batch_adjoint.hip, beside the window product kernel, and reached through batch_pts_kernels().
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_monitor.hpp"

namespace fdtd {

// ---- point sources with channels (include/fdtd2d_batch_adjoint.h) -------------------------------------------------
// The mirror image of the probes: cell p of member b takes sum_c w[p][c] * chan[c][n] after the rectangle source of
// step n.  The sums are formed once per (member, cell, step), where the phasors are: by lanes of a resident
// workgroup's last wave into an LDS table during the H phase, or by block (0, y) of the streamed H launch into a
// count x nc table.
struct BatchPts {
    const int *cells;         // count x nc cells, row * C + col (streamed path)
    const int *own;           // count x nc, ascending per member: owner thread * 16 + slot of the resident cell walk
    const double *w;          // count x nchan x nc weights (channel-major: neighbouring lanes read neighbours)
    const double *chan;       // chan[b * chan_mstride + c * chan_stride + n] for the run's step n
    double *tab;              // streamed path: count x nc sums of the step being completed
    long long chan_mstride, chan_stride;
    int nc, nchan;
};

// s = 0.0; s = s + w[c] * a[c] for c ascending, in float64.  Not inlined (like batch_mon_phasor): the channel loop
// would otherwise share the resident step loop's registers and spill.
static __device__ __attribute__((noinline)) double batch_pts_dot(const double *w, const double *a, int nchan,
                                                                 size_t wstride, size_t astride)
{
    double s = 0.0;
#pragma unroll 2   // two channels' loads in flight; the adds keep their order
    for (int c = 0; c < nchan; ++c) s = s + w[(size_t)c * wstride] * a[(size_t)c * astride];
    return s;
}
static __device__ __forceinline__ double batch_pts_sum(const BatchPts &P, int b, int p, long long n)
{
    return batch_pts_dot(P.w + (size_t)b * P.nchan * P.nc + p, P.chan + (size_t)b * (size_t)P.chan_mstride + (size_t)n,
                         P.nchan, (size_t)P.nc, (size_t)P.chan_stride);
}

// resident path, in the H phase of the run's step n: lane p of the last wave forms cell p's sum; the barrier after H
// publishes the table.  The lane is made opaque so that its weight address is formed per step instead of being hoisted
// out of the step loop and held (which spills in the double-precision 16-slot instances).
static __device__ __forceinline__ void batch_pts_sums(const BatchPts &P, int b, int lane, double *ssum, long long n)
{
    asm volatile("" : "+v"(lane));
    if (lane >= 0 && lane < P.nc) ssum[lane] = batch_pts_sum(P, b, lane, n);
}

// resident path: which slots of this thread's cell walk are point cells (bit q of the low half), and the table entry
// of the lowest one (the high half); the table is sorted by (thread, slot), so the others follow it.  Worked out once
// per member, and kept in one register: the double-precision 16-slot instances have none to spare.
static __device__ __forceinline__ int batch_pts_begin(const BatchPts &P, int b, int tid)
{
    int s = 0;
    for (int p = 0; p < P.nc; ++p) {
        const int o = P.own[(size_t)b * P.nc + p];
        if ((o >> 4) == tid) {
            if (!s) s = p << 16;
            s |= 1 << (o & 15);
        }
    }
    return s;
}
// the table entry of slot q (a point cell of this thread)
static __device__ __forceinline__ int batch_pts_entry(int s, int q) { return (s >> 16) + __popc(s & ((1 << q) - 1)); }

// streamed path, in the H launch of the run's step n: block (0, y) writes the sums of its members for the E launch
static __device__ __forceinline__ void batch_pts_table(const BatchPts &P, int B, int n)
{
    const int p = threadIdx.x;
    if (blockIdx.x != 0 || p >= P.nc) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) P.tab[(size_t)b * P.nc + p] = batch_pts_sum(P, b, p, n);
}

// streamed path, in the E launch: member b's Ez e at cell t after the rectangle source (the probes' search)
template <class T> static __device__ __forceinline__ T batch_pts_cell(const BatchPts &P, int b, int t, T e)
{
    const unsigned lo = blockIdx.x * blockDim.x;
    for (int p = 0; p < P.nc; ++p) {
        const int c = P.cells[(size_t)b * P.nc + p];
        if ((unsigned)c - lo < blockDim.x) {
            if (c == t) e = (T)((double)e + P.tab[(size_t)b * P.nc + p]);
        }
    }
    return e;
}

// ---- the kernels ---------------------------------------------------------------------------------------------
// k_batch_resident_mon with the point sources: LDS = Ez, Hx, Hy (+ ce, ch), then the phasor table, the nc sums of the
// step and (lds_acc) the accumulators.
template <class T, bool ARR, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_mon_pts(BatchView<T> v, BatchMon m, BatchPts P,
                                                                               int n0, int nt, long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_mon_lds[];
    const int R = v.R, C = v.C;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_mon_lds);
    T *shx = sez + seg, *shy = shx + seg, *sce = shy + seg, *sch = sce + seg;
    double *stab = reinterpret_cast<double *>(sez + (ARR ? 5 : 3) * seg), *ssum = stab + 2 * m.nf;
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
    const LdsAcc<T, ARR> acc{sez, shx, shy, sce, v.ce_u, R, C};

    for (int b = blockIdx.x; b < v.B; b += gridDim.x) {
        const size_t base = (size_t)b * v.mstride;
        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            sez[l] = v.ez[g];
            shx[l] = v.hx[g];
            shy[l] = v.hy[g];
            if (ARR) {
                sce[l] = v.ce[g];
                sch[l] = v.ch[g];
            }
        });
        const MurRules<T, LdsAcc<T, ARR>> f{acc, v.kmur[b]};
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
                const T cc = ARR ? sch[l] : v.ch_u;
                shx[l] = shx[l] - cc * (sez[l + C] - e);
                shy[l] = shy[l] + cc * (sez[l + 1] - e);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            T out[MAXC];
            cells([&](int q, int i, int j, int) { out[q] = v.mur ? f.d(i, j) : f.a(i, j); });
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

// k_batch_resident_pml_mon with the point sources: LDS = Ez, Hx, Hy, Ezx (+ ce, ch), the factors, then the phasor
// table, the nc sums of the step and (lds_acc) the accumulators.
template <class T, bool ARR, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_pml_mon_pts(BatchView<T> v, BatchPml<T> p,
                                                                                   BatchMon m, BatchPts P, int n0,
                                                                                   int nt, long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_mon_pml_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_mon_pml_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *sce = sezx + seg, *sch = sce + seg;
    T *sfr = sez + (ARR ? 6 : 4) * seg;       // ahr[R], bhr[R], aer[R], ber[R]
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
            if (ARR) {
                sce[l] = v.ce[g];
                sch[l] = v.ch[g];
            }
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
                const T cc = ARR ? sch[l] : v.ch_u;
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
                    const T cc = ARR ? sce[l] : v.ce_u;
                    const T dhy = shy[l] - shy[l - 1], dhx = shx[l] - shx[l - C];
                    if (i < L || i > R - 1 - L || j < L || j > C - 1 - L) {
                        const T x = sezx[l];
                        T ey = e - x;
                        const T ex = sfc[2 * C + j] * x + (sfc[3 * C + j] * cc) * dhy;
                        ey = sfr[2 * R + i] * ey - (sfr[3 * R + i] * cc) * dhx;
                        sezx[l] = ex;
                        e = ex + ey;
                    } else {
                        e = e + (dhy - dhx) * cc;
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

// streamed path: the H launches also write the sums of the run's step n; the E launches add them behind the rectangle
// source.  Two launches per step, as without point sources.
template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_h_mon_pts(BatchView<T> v, BatchMon m, BatchPts P, int n, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    batch_pts_table(P, v.B, n);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int i = t / v.C, j = t % v.C;
    if (i > v.R - 2 || j > v.C - 2) return;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T e = v.ez[o];
        const T cc = ARR ? v.ch[o] : v.ch_u;
        v.hx[o] = v.hx[o] - cc * (v.ez[o + v.pitch] - e);
        v.hy[o] = v.hy[o] + cc * (v.ez[o + 1] - e);
    }
}

template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_e_mon_pts(BatchView<T> v, BatchMon m, BatchPts P,
                                                         T *__restrict__ ez_new, int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int i = t / v.C, j = t % v.C;
    const Geom g{v.R, v.C, 0, v.pitch};
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t base = (size_t)b * v.mstride;
        const FrameCtx<T, ARR> f{{v.ez + base, v.hx + base, v.hy + base, ARR ? v.ce + base : nullptr, v.ce_u, g,
                                  v.R, v.C},
                                 v.kmur[b]};
        T e = v.mur ? f.d(i, j) : f.a(i, j);
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

template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_h_pml_mon_pts(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                             int n, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    batch_pts_table(P, v.B, n);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R, *fc = p.colf + (size_t)b * 4 * C;
        const T e = v.ez[o];
        const T cc = ARR ? v.ch[o] : v.ch_u;
        v.hx[o] = fr[i] * v.hx[o] - (fr[R + i] * cc) * (v.ez[o + v.pitch] - e);
        v.hy[o] = fc[j] * v.hy[o] + (fc[C + j] * cc) * (v.ez[o + 1] - e);
    }
}

template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_e_pml_mon_pts(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                             int n, long long step)
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
            const T cc = ARR ? v.ce[o] : v.ce_u;
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
                e = e + (dhy - dhx) * cc;
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

// host stubs of the kernels above, in BatchMonKernels' layout, and the product kernel's launch (batch_adjoint.hip)
template <class T> const BatchMonKernels &batch_pts_kernels();
void batch_window_product_launch(const double *held, const double *cur, const double *coef, double *out, int B, int nf,
                                 size_t W, hipStream_t stream);
// the same for ncoef = 1..3 coefficient sets with a scale per member and set (fdtd2d_batch_dispersive_adjoint.h)
void batch_window_product_multi_launch(const double *held, const double *cur, const double *coef, const double *scale,
                                       double *out, int B, int nf, size_t W, int ncoef, hipStream_t stream);

}  // namespace fdtd
