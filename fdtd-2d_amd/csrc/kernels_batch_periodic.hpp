// Periodic columns for the batched kernels (include/fdtd2d_batch_periodic.h): the lossy PML kernels of
// kernels_batch_lossy.hpp with the column difference of the E half-step taken cyclically over the period Q = C - 1.
// Column C - 1 is the image of column 0.  H is the PML kernels' own: Hy[i, C-2] reads the image, which supplies the
// wrap.  The layer is one of rows alone; the column factors are exactly 1 (the host refuses anything else), and x * 1
// is exact, so they are left out of the arithmetic without changing a value (the carve keeps their 4C slots: the
// capacity rule is the lossy PML one).
//
// The image without a third barrier: the thread that owns (i, C-1) evaluates column 0's update in the same E phase,
// from column 0's H operands and coefficients and its own Ez / Ezx as the old value, and applies column 0's source
// test (the host lists a column-0 point source a second time at the image cell, with the same weights, so its sum is
// the same float64).  By induction the image stays bit-identical to column 0, and no thread reads an Ez or Ezx that
// another thread writes in that phase, in LDS or in the in-place streamed kernel.
//
// The wrap is two selects on LDS indices, not branches: lc = l - (C-1) on the image (column 0's cell), and the left
// neighbour lw = l + (C-2) in column 0, l - 1 elsewhere (on the image l - 1 is (i, C-2), column 0's left neighbour).
// Banks: a 32-lane group reads Hy[lw] at 32 consecutive words except for a lane in column 0, whose word (i, C-2) is the
// one the image lane of the same row reads (a broadcast when both are in the group, one extra LDS cycle otherwise).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_lossy.hpp"

namespace fdtd {

// The multiply-add pairs of a step.  One rounding per operation in the exact build; in the fused build the fma is
// written out, as in batch_lossy_e: -ffp-contract=fast could contract either product of a * x - (b * c) * d, and a
// different choice in the resident and the streamed kernel would make the result depend on the path.
template <class T> __device__ __forceinline__ T batch_periodic_fma(T a, T b, T c)
{
    if constexpr (sizeof(T) == 4) return __builtin_fmaf(a, b, c);
    else return __builtin_fma(a, b, c);
}
// a * x - (b * c) * d: Hx with the row factors, and the y-part of Ez in the layer
template <class T> __device__ __forceinline__ T batch_periodic_split(T x, T a, T b, T c, T d)
{
#ifdef FDTD2D_FUSED
    return batch_periodic_fma(-(b * c), d, a * x);
#else
    return a * x - (b * c) * d;
#endif
}
// x + c * d: Hy, and the x-part of Ez in the layer (the column factors are exactly 1)
template <class T> __device__ __forceinline__ T batch_periodic_plain(T x, T c, T d)
{
#ifdef FDTD2D_FUSED
    return batch_periodic_fma(c, d, x);
#else
    return x + c * d;
#endif
}

// k_batch_resident_pml_lossy with periodic columns: LDS = Ez, Hx, Hy, Ezx, cb, ch, ca, the factors, then the phasor
// table, the nc sums of the step and (lds_acc) the accumulators.  Two barriers per step.
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_periodic(BatchView<T> v, BatchPml<T> p,
                                                                                BatchMon m, BatchPts P,
                                                                                const T *__restrict__ ca, int n0, int nt,
                                                                                long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_periodic_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_periodic_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *scb = sezx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sfr = sez + 7 * seg;                   // ahr[R], bhr[R], aer[R], ber[R]
    T *sfc = sfr + batch_lds_seg<T>(4 * R);   // the column factors' slots (all exactly 1, never read)
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
                shx[l] = batch_periodic_split(shx[l], sfr[i], sfr[R + i], cc, sez[l + C] - e);
                shy[l] = batch_periodic_plain(shy[l], cc, sez[l + 1] - e);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step);
            const bool sampled = m.sampled(step);
            cells([&](int q, int i, int j, int l) {
                T e = sez[l];
                const bool image = j == C - 1;
                const int lc = image ? l - (C - 1) : l;       // the cell whose update this is
                const int lw = j == 0 ? l + (C - 2) : l - 1;  // its left neighbour, cyclically
                if (i >= 1 && i <= R - 2) {
                    const T cc = scb[lc];
                    const T dhy = shy[lc] - shy[lw], dhx = shx[lc] - shx[lc - C];
                    if (i < L || i > R - 1 - L) {
                        const T x = sezx[l];
                        T ey = e - x;
                        const T ex = batch_periodic_plain(x, cc, dhy);
                        ey = batch_periodic_split(ey, sfr[2 * R + i], sfr[3 * R + i], cc, dhx);
                        sezx[l] = ex;
                        e = ex + ey;
                    } else {
                        e = batch_lossy_e(e, dhy - dhx, sca[lc], cc);
                    }
                }
                if (src.covers(i, image ? 0 : j)) e = (T)((double)e + amp);
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

// streamed path: k_batch_h_pml_mon_pts (which also writes the phasors and the sums of the step) with the arithmetic of
// the resident kernel above, then k_batch_e_pml_lossy with periodic columns, in place
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_periodic(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P, int n,
                                                          long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    batch_pts_table(P, v.B, n);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T e = v.ez[o];
        const T cc = v.ch[o];
        v.hx[o] = batch_periodic_split(v.hx[o], fr[i], fr[R + i], cc, v.ez[o + v.pitch] - e);
        v.hy[o] = batch_periodic_plain(v.hy[o], cc, v.ez[o + 1] - e);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_batch_e_periodic(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                          const T *__restrict__ ca, int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    const bool image = j == C - 1;
    const bool interior = i >= 1 && i <= R - 2;
    const bool layer = i < L || i > R - 1 - L;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const size_t oc = image ? o - (size_t)(C - 1) : o;
        const size_t ow = j == 0 ? o + (size_t)(C - 2) : o - 1;
        T e = v.ez[o];
        if (interior) {
            const T cc = v.ce[oc];
            const T dhy = v.hy[oc] - v.hy[ow], dhx = v.hx[oc] - v.hx[oc - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R;
                const T x = p.ezx[o];
                T ey = e - x;
                const T ex = batch_periodic_plain(x, cc, dhy);
                ey = batch_periodic_split(ey, fr[2 * R + i], fr[3 * R + i], cc, dhx);
                p.ezx[o] = ex;
                e = ex + ey;
            } else {
                e = batch_lossy_e(e, dhy - dhx, ca[oc], cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, image ? 0 : j)) e = (T)((double)e + src.amps[n]);
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

// host stubs of the kernels above (batch_periodic.hip): [MAXC 4, 8, 16]
struct BatchPeriodicKernels {
    const void *resident[3];
    const void *h, *e;
};
template <class T> const BatchPeriodicKernels &batch_periodic_kernels();

}  // namespace fdtd
