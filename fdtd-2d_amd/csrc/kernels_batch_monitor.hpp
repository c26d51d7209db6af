// Monitors of the batched kernels (include/fdtd2d_batch_monitor.h): a window DFT at up to 16 frequencies per member
// and up to 64 point probes per member.  The monitored kernels below are the kernels of kernels_batch.hpp and
// kernels_batch_pml.hpp, step for step, plus the monitors; they are separate kernels so that the unmonitored ones keep
// their code and registers.  They are instantiated in batch_monitor.hip and reached through batch_mon_kernels().
//
// Phasors are evaluated once per (member, frequency, sampled step) with batch_phasor's expression: by lanes of the
// last wave of a resident workgroup into an LDS table during the H phase, or by block (0, y) of the streamed H launch
// into a count x nf table that the E launch of the same step reads.  Every accumulator takes the same float64
// additions in the same order on every path and placement, so the results never depend on them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch.hpp"
#include "kernels_batch_pml.hpp"

namespace fdtd {

constexpr int BATCH_MON_MAX_FREQ = 16;
constexpr int BATCH_MON_MAX_PROBES = 64;

struct BatchMon {
    // window DFT (nf = 0: none): [r0, r0 + nr) x [c0, c0 + nc), shared by all members
    double *acc;              // per member 2 * nf * nr * nc: re[nf][window], then im[nf][window] (global memory)
    const double *omega;      // count x nf, member-major
    double *ph;               // streamed path: count x nf x {cos, -sin} of the step being completed
    int r0, c0, nr, nc, nf, every;
    long long step0;          // samples the steps s with (s - step0) % every == 0, t = s * dt
    int lds_acc;              // resident path: the member's accumulators live in LDS behind the phasor table
    // probes (np = 0: none)
    const int *cells;         // count x np cells, row * C + col
    double *trace;            // [member][probe][cap] float64
    int np;
    long long cap, pstep0;    // step s is sample s - 1 - pstep0, recorded while < cap

    __device__ __forceinline__ size_t window() const { return (size_t)nr * (size_t)nc; }
    __device__ __forceinline__ bool sampled(long long step) const { return nf > 0 && (step - step0) % every == 0; }
    // index of cell (i, j) in the window, -1 outside it
    __device__ __forceinline__ int window_cell(int i, int j) const
    {
        const int wi = i - r0, wj = j - c0;
        return (unsigned)wi < (unsigned)nr && (unsigned)wj < (unsigned)nc ? wi * nc + wj : -1;
    }
    // accumulators of window cell w += e * phasor k (tab: nf x {cos, -sin}), as the whole-grid DFT adds
    __device__ __forceinline__ void add(double *a, const double *tab, int w, double e) const
    {
        const size_t W = window();
        for (int k = 0; k < nf; ++k) {
            a[(size_t)k * W + w] += e * tab[2 * k];
            a[(size_t)(nf + k) * W + w] += e * tab[2 * k + 1];
        }
    }
    __device__ __forceinline__ double *member_acc(int b) const { return acc + (size_t)b * 2 * nf * window(); }
    // Ez of completed step `step` at member b's probe p
    __device__ __forceinline__ void record(int b, int p, long long step, double e) const
    {
        const long long n = step - 1 - pstep0;
        if (n >= 0 && n < cap) trace[((size_t)b * np + p) * (size_t)cap + (size_t)n] = e;
    }
};

// exp(-i omega t) of step `step`, t = step * dt: the expression of batch_phasor.  Not inlined: the float64 sin / cos
// (with their large-argument reduction) would otherwise share the resident step loop's registers and spill.
static __device__ __attribute__((noinline)) void batch_mon_phasor(double *out, double omega, long long step, double dt)
{
    const double t = (double)step * dt;
    out[0] = cos(omega * t);
    out[1] = -sin(omega * t);
}

// ---- resident path: one member of a workgroup --------------------------------------------------------------
// Lane k of the last wave evaluates frequency k's phasor and records probe k.  The LDS behind the member's arrays
// holds the phasor table (2 nf doubles) and, with lds_acc, the member's accumulators.
struct BatchMonMember {
    double *acc;              // the member's accumulators in global memory (the LDS copy is sacc with lds_acc)
    double omega;             // lane k < nf: omega_k
    int cell;                 // lane p < np: probe p's cell
    int lane;                 // the thread's lane in the last wave (< 0 in the others)
};

// at the start of member b, before the barrier that precedes its first step
__device__ __forceinline__ BatchMonMember batch_mon_begin(const BatchMon &m, int b, double *sacc, int tid, int nthr)
{
    BatchMonMember s{nullptr, 0.0, 0, tid - (nthr - 64)};
    if (m.nf) {
        double *g = m.member_acc(b);
        s.acc = g;
        if (m.lds_acc) {
            const size_t n = 2 * (size_t)m.nf * m.window();
            for (size_t k = tid; k < n; k += nthr) sacc[k] = g[k];
        }
        if (s.lane >= 0 && s.lane < m.nf) s.omega = m.omega[(size_t)b * m.nf + s.lane];
    }
    if (s.lane >= 0 && s.lane < m.np) s.cell = m.cells[(size_t)b * m.np + s.lane];
    return s;
}

// in the H phase of step `step`: the phasor table, published by the barrier after H
__device__ __forceinline__ void batch_mon_phasors(const BatchMon &m, const BatchMonMember &s, double *stab,
                                                  long long step, double dt)
{
    if (s.lane >= 0 && s.lane < m.nf && m.sampled(step)) batch_mon_phasor(stab + 2 * s.lane, s.omega, step, dt);
}

// after the last barrier of step `step`: the probes read the member's final Ez of the step (the next writes to Ez
// come after the next step's first barrier)
template <class T>
__device__ __forceinline__ void batch_mon_probes(const BatchMon &m, const BatchMonMember &s, int b, const T *sez,
                                                 long long step)
{
    if (s.lane >= 0 && s.lane < m.np) m.record(b, s.lane, step, (double)sez[s.cell]);
}

// at the end of member b, before the barrier after which the next member's loads overwrite LDS
__device__ __forceinline__ void batch_mon_end(const BatchMon &m, int b, const double *sacc, int tid, int nthr)
{
    if (m.nf && m.lds_acc) {
        double *g = m.member_acc(b);
        const size_t n = 2 * (size_t)m.nf * m.window();
        for (size_t k = tid; k < n; k += nthr) g[k] = sacc[k];
    }
}

// ---- streamed path ------------------------------------------------------------------------------------------
// in the H launch of step `step`: block (0, y) writes the phasors of its members for the E launch
__device__ __forceinline__ void batch_mon_phasor_table(const BatchMon &m, int B, long long step, double dt)
{
    const int k = threadIdx.x;
    if (blockIdx.x != 0 || k >= m.nf || !m.sampled(step)) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y)
        batch_mon_phasor(m.ph + ((size_t)b * m.nf + k) * 2, m.omega[(size_t)b * m.nf + k], step, dt);
}

// in the E launch of step `step`: member b's new Ez e at cell t = (i, j) of this block's range
__device__ __forceinline__ void batch_mon_cell(const BatchMon &m, int b, int t, int i, int j, long long step, double e)
{
    if (m.sampled(step)) {
        const int w = m.window_cell(i, j);
        if (w >= 0) m.add(m.member_acc(b), m.ph + (size_t)b * 2 * m.nf, w, e);
    }
    // which probes fall in this block's cells: one uniform compare per probe, then a compare in the hit's wave only
    const unsigned lo = blockIdx.x * blockDim.x;
    for (int p = 0; p < m.np; ++p) {
        const int c = m.cells[(size_t)b * m.np + p];
        if ((unsigned)c - lo < blockDim.x) {
            if (c == t) m.record(b, p, step, e);
        }
    }
}

// ---- the monitored kernels -----------------------------------------------------------------------------------
// k_batch_resident with the monitors: LDS = Ez, Hx, Hy (+ ce, ch), then the phasor table and (lds_acc) the
// accumulators.  The window adds happen where the new Ez is stored (after the second barrier).
template <class T, bool ARR, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_mon(BatchView<T> v, BatchMon m, int n0, int nt,
                                                                           long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_mon_lds[];
    const int R = v.R, C = v.C;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_mon_lds);
    T *shx = sez + seg, *shy = shx + seg, *sce = shy + seg, *sch = sce + seg;
    double *stab = reinterpret_cast<double *>(sez + (ARR ? 5 : 3) * seg), *sacc = stab + 2 * m.nf;
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

// k_batch_resident_pml with the monitors: LDS = Ez, Hx, Hy, Ezx (+ ce, ch), the factors, then the phasor table and
// (lds_acc) the accumulators.  The window adds happen in the E phase, where the new Ez is stored.
template <class T, bool ARR, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_pml_mon(BatchView<T> v, BatchPml<T> p,
                                                                               BatchMon m, int n0, int nt,
                                                                               long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_mon_pml_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_mon_pml_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *sce = sezx + seg, *sch = sce + seg;
    T *sfr = sez + (ARR ? 6 : 4) * seg;       // ahr[R], bhr[R], aer[R], ber[R]
    T *sfc = sfr + batch_lds_seg<T>(4 * R);   // ahc[C], bhc[C], aec[C], bec[C]
    double *stab = reinterpret_cast<double *>(sfc + batch_lds_seg<T>(4 * C)), *sacc = stab + 2 * m.nf;
    const int di = nthr / C, dj = nthr % C, ti = tid / C, tj = tid % C;
    auto cells = [&](auto &&body) {   // the cell walk of k_batch_resident_pml
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
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const T e = sez[l];
                const T cc = ARR ? sch[l] : v.ch_u;
                shx[l] = sfr[i] * shx[l] - (sfr[R + i] * cc) * (sez[l + C] - e);
                shy[l] = sfc[j] * shy[l] + (sfc[C + j] * cc) * (sez[l + 1] - e);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step);
            const bool sampled = m.sampled(step);
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

        cells([&](int i, int j, int l) {
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

// streamed path: the H launches of step `step` also write its phasor table; the E launches add the window and record
// the probes.  Two launches per step, as without monitors.
template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_h_mon(BatchView<T> v, BatchMon m, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
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
__global__ __launch_bounds__(256) void k_batch_e_mon(BatchView<T> v, BatchMon m, T *__restrict__ ez_new, int n,
                                                     long long step)
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
        batch_mon_cell(m, b, t, i, j, step, (double)e);
    }
}

template <class T, bool ARR>
__global__ __launch_bounds__(256) void k_batch_h_pml_mon(BatchView<T> v, BatchPml<T> p, BatchMon m, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
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
__global__ __launch_bounds__(256) void k_batch_e_pml_mon(BatchView<T> v, BatchPml<T> p, BatchMon m, int n,
                                                         long long step)
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
        batch_mon_cell(m, b, t, i, j, step, (double)e);
    }
}

// host stubs of the monitored kernels (instantiated in batch_monitor.hip): [ARR][MAXC 4, 8, 16] and [ARR]
struct BatchMonKernels {
    const void *resident[2][3], *resident_pml[2][3];
    const void *h[2], *e[2], *h_pml[2], *e_pml[2];
};
template <class T> const BatchMonKernels &batch_mon_kernels();

}  // namespace fdtd
