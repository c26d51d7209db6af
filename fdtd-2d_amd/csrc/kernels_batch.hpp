// Batched kernels for gfx950: B independent members of one shape (fdtd2d_batch_*), each with its own
// materials, Mur factor, source rectangle, amplitudes and DFT frequency, stepped together.
//
// Storage: every field holds B members back to back, each rows x pitch elements (pitch a multiple of
// 64 elements, as in Geom); member b's element (i, j) lives at b * rows * pitch + i * pitch + j.
// Hx's column C-1, Hy's row R-1 and the padding columns are permanent zeros.
//
// Arithmetic is the reference's, cell for cell, in T with one rounding per operation (the same
// expressions as k_update_h / k_update_e / MurRules / k_add_point), so every member is
// value-identical to a single Engine run on it.
//
// Two paths:
//   k_batch_resident  one workgroup per member (grid-stride over members): the member's fields (and its
//                     coefficient arrays) are loaded into LDS once, up to nt steps run inside the launch,
//                     and the fields are written back once.  Three workgroup barriers per step: after the
//                     H half-step (E reads H), after the E values are computed into registers (the stores
//                     overwrite the P values neighbours read), after the stores (the next H reads Ez).
//   k_batch_h/_e      one launch per half-step for the whole batch, for members that do not fit in LDS;
//                     the member comes from blockIdx.y, the frame through the global-memory MurRules
//                     accessor, Ez ping-pongs between two buffer sets.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_step.hpp"
#include "mur_rules.hpp"

namespace fdtd {

// LDS a workgroup may declare on gfx950 (160 KiB per CU, all of it for one workgroup)
constexpr size_t BATCH_LDS_LIMIT = 163840;
constexpr int BATCH_RES_THREADS = 1024;   // most threads of a resident workgroup

// elements of one LDS array of `cells` elements, rounded up to 16 bytes (every carve offset 16-B aligned)
template <class T> __host__ __device__ __forceinline__ size_t batch_lds_seg(int cells)
{
    return ((size_t)cells * sizeof(T) + 15) / 16 * 16 / sizeof(T);
}

template <class T> struct BatchView {
    T *ez, *hx, *hy;          // current fields
    const T *ce, *ch;         // coefficient arrays (nullptr with uniform materials)
    T ce_u, ch_u;             // uniform coefficients
    const T *kmur;            // Mur factor per member (main.py:30-31 from the member's own [0,0] cell)
    int B, R, C;
    int mur;                  // 1: 5-px Mur frame + corner rule, 0: frame cells keep their stage-A value
    long long pitch;          // elements per stored row
    size_t mstride;           // elements per member = R * pitch
    const int *rect;          // 4 per member: row, col, nrows, ncols (0 x 0 = no source)
    const double *amps;       // amps[b * amp_stride + n] for the launch's step n; nullptr = no source
    long long amp_stride;
    double *dft;              // per member: re[R*C] then im[R*C] (row-major, no padding); nullptr = off
    const double *omega;      // one angular frequency per member
    int every;                // sample after the steps s with (s - dft_step0) % every == 0
    long long dft_step0;
    double dt;
};

// the source of step n for member b at cell (i, j): (T)((double)Ez + amp) like k_add_point
template <class T> struct BatchSource {
    int r0, c0, r1, c1;       // rectangle [r0, r1) x [c0, c1), empty when there is none
    const double *amps;       // this member's amplitudes, indexed by the launch's step
    __device__ __forceinline__ void load(const BatchView<T> &v, int b)
    {
        const int *r = v.rect + 4 * b;
        r0 = r[0]; c0 = r[1]; r1 = r0 + r[2]; c1 = c0 + r[3];
        amps = v.amps ? v.amps + (size_t)b * v.amp_stride : nullptr;
        if (!amps) r1 = r0;
    }
    __device__ __forceinline__ bool covers(int i, int j) const { return i >= r0 && i < r1 && j >= c0 && j < c1; }
};

// phasor exp(-i omega t) of a sampled step, t = step * dt (as fdtd2d_set_dft's host phasors)
struct BatchPhasor {
    double c, s;
    bool on;
};
template <class T>
__device__ __forceinline__ BatchPhasor batch_phasor(const BatchView<T> &v, double omega, long long step)
{
    BatchPhasor p{0.0, 0.0, false};
    if (v.dft && (step - v.dft_step0) % v.every == 0) {
        const double t = (double)step * v.dt;
        p.c = cos(omega * t);
        p.s = -sin(omega * t);
        p.on = true;
    }
    return p;
}

// ---- resident path ------------------------------------------------------------------------------------
// LDS accessor of MurRules: a member's arrays as rows of C elements
template <class T, bool ARR> struct LdsAcc {
    const T *P, *x, *y, *c;
    T ce_u;
    int R, C;
    __device__ __forceinline__ T p(int i, int j) const { return P[i * C + j]; }
    __device__ __forceinline__ T hx(int i, int j) const { return x[i * C + j]; }
    __device__ __forceinline__ T hy(int i, int j) const { return y[i * C + j]; }
    __device__ __forceinline__ T ce(int i, int j) const { return ARR ? c[i * C + j] : ce_u; }
};

// Thread t owns cells t, t + nthr, t + 2 nthr, ... (row-major over R x C), at most MAXC of them; the
// new Ez of its cells waits in registers between the second and third barrier of a step.
// Dynamic LDS: Ez, Hx, Hy (+ ce, ch with material arrays), batch_lds_seg<T>(R*C) elements each.
template <class T, bool ARR, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident(BatchView<T> v, int n0, int nt,
                                                                       long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_lds[];
    const int R = v.R, C = v.C;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_lds);
    T *shx = sez + seg, *shy = shx + seg, *sce = shy + seg, *sch = sce + seg;
    const int di = nthr / C, dj = nthr % C, ti = tid / C, tj = tid % C;
    // walks the thread's cells: body(q, i, j, l) for every owned cell (l = i * C + j).  The indices are
    // made opaque at every walk so that the neighbour addresses of the inlined MurRules branches are
    // recomputed per step instead of being hoisted out of the step loop and held (which spills).
    auto cells = [&](auto &&body) {
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
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            // H half-step (main.py:66-76): a cell's Hx, Hy depend on Ez only, so they are updated in place
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const T e = sez[l];
                const T cc = ARR ? sch[l] : v.ch_u;
                shx[l] = shx[l] - cc * (sez[l + C] - e);
                shy[l] = shy[l] + cc * (sez[l + 1] - e);
            });
            __syncthreads();
            // E half-step (main.py:12-63): every new value is a pure function of P and the new H
            T out[MAXC];
            cells([&](int q, int i, int j, int) { out[q] = v.mur ? f.d(i, j) : f.a(i, j); });
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step_base + s + 1);
            cells([&](int q, int i, int j, int l) {
                T e = out[q];
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

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = sez[l];
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
        });
        __syncthreads();   // the next member's loads overwrite these arrays
    }
}

// ---- streamed path: one launch per half-step for the whole batch ----------------------------------------
// grid (ceil(R*C / 256), min(B, 65535)); member b = blockIdx.y, blockIdx.y + gridDim.y, ...
template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_h(BatchView<T> v)
{
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

// E half-step from v.ez (= P) into ez_new, then the source and the DFT sample of step `step` (the step this
// launch completes); n = its index into the amplitudes.
template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_e(BatchView<T> v, T *__restrict__ ez_new, int n, long long step)
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
        ez_new[base + at(g, i, j)] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *d = v.dft + (size_t)b * 2 * (size_t)(v.R * v.C) + (size_t)t;
            d[0] += (double)e * ph.c;
            d[v.R * v.C] += (double)e * ph.s;
        }
    }
}

}  // namespace fdtd
