// Batched kernels with the split-field PML (fdtd2d_batch_set_pml): every member carries the Berenger layer of
// Engine(boundary="pml") with its own factor arrays, operation for operation as oracle/pml_numpy.step and
// k_update_h_pml / k_update_e_pml (kernels_pml.hpp).  Separate from kernels_batch.hpp so that the Mur kernels
// keep their code and register use.
//
// A new Ez reads only its own Ez / Ezx and H, never a neighbour's Ez, so E is updated in place:
//   k_batch_resident_pml  one workgroup per member (grid-stride over members): Ez, Hx, Hy, Ezx (+ ce, ch with
//                         material arrays) and the member's 4R + 4C factors in LDS; two barriers per step
//                         (after H: E reads the neighbours' H; after E + source + DFT: the next H reads the
//                         neighbours' Ez).
//   k_batch_h_pml/_e_pml  one launch per half-step for the whole batch; Ez and Ezx in place.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_batch.hpp"

namespace fdtd {

template <class T> struct BatchPml {
    T *ezx;                   // the x-part of Ez, same layout as Ez (zero outside the layer)
    const T *rowf;            // per member 4R: ahr, bhr, aer, ber
    const T *colf;            // per member 4C: ahc, bhc, aec, bec
    int L;                    // layer depth in cells, shared by all members
};

// LDS of one resident member: `arrays` field arrays of R*C, then the 4R row and 4C column factors
template <class T> __host__ __device__ __forceinline__ size_t batch_pml_lds_elems(int arrays, int R, int C)
{
    return (size_t)arrays * batch_lds_seg<T>(R * C) + batch_lds_seg<T>(4 * R) + batch_lds_seg<T>(4 * C);
}

// Thread t owns cells t, t + nthr, ... (row-major over R x C), at most MAXC of them.
// Dynamic LDS: Ez, Hx, Hy, Ezx (+ ce, ch with material arrays), batch_lds_seg<T>(R*C) elements each, then the
// factors (batch_pml_lds_elems).
template <class T, bool ARR, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_pml(BatchView<T> v, BatchPml<T> p, int n0,
                                                                           int nt, long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_pml_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_pml_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *sce = sezx + seg, *sch = sce + seg;
    T *sfr = sez + (ARR ? 6 : 4) * seg;       // ahr[R], bhr[R], aer[R], ber[R]
    T *sfc = sfr + batch_lds_seg<T>(4 * R);   // ahc[C], bhc[C], aec[C], bec[C]
    const int di = nthr / C, dj = nthr % C, ti = tid / C, tj = tid % C;
    // the cell walk of k_batch_resident, opaque at every phase so that neighbour addresses and factor loads are
    // recomputed per step instead of being hoisted out of the step loop (which spills)
    auto cells = [&](auto &&body) {
        int i = ti, j = tj;
        asm volatile("" : "+v"(i), "+v"(j));
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            if (i < R) body(i, j, i * C + j);
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
        cells([&](int i, int j, int l) {
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
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            // H half-step, PML form at every cell (the factors are exactly 1 outside the layer)
            cells([&](int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const T e = sez[l];
                const T cc = ARR ? sch[l] : v.ch_u;
                shx[l] = sfr[i] * shx[l] - (sfr[R + i] * cc) * (sez[l + C] - e);
                shy[l] = sfc[j] * shy[l] + (sfc[C + j] * cc) * (sez[l + 1] - e);
            });
            __syncthreads();
            // E half-step in place: split update inside the layer, main.py:21-27 elsewhere; edge cells stay (PEC)
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step_base + s + 1);
            cells([&](int i, int j, int l) {
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
                sez[l] = e;
                if (ph.on) {
                    double *d = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)l;
                    d[0] += (double)e * ph.c;
                    d[R * C] += (double)e * ph.s;
                }
            });
            __syncthreads();
        }

        cells([&](int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = sez[l];
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
            p.ezx[g] = sezx[l];
        });
        __syncthreads();   // the next member's loads overwrite these arrays
    }
}

// ---- streamed path: one launch per half-step for the whole batch ----------------------------------------
// grid (ceil(R*C / 256), min(B, 65535)); member b = blockIdx.y, blockIdx.y + gridDim.y, ...
template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_h_pml(BatchView<T> v, BatchPml<T> p)
{
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

// E half-step of every cell in place, then the source and the DFT sample of step `step` (the step this launch
// completes); n = its index into the amplitudes.
template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_e_pml(BatchView<T> v, BatchPml<T> p, int n, long long step)
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
        v.ez[o] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *d = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)t;
            d[0] += (double)e * ph.c;
            d[R * C] += (double)e * ph.s;
        }
    }
}

}  // namespace fdtd
