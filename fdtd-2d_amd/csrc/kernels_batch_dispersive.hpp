// Dispersive (Drude-Lorentz) materials for the batched kernels (include/fdtd2d_batch_dispersive.h): one pole per
// member, a strength per cell.  The cells that take the plain update of kernels_batch_lossy.hpp take
//     jn = a * Jh + (cj * e - ck * Q);  Q = Q + jn;  e = ca * e + ((dhy - dhx) - jn) * cb;  Jh = jn
// instead, with Jh, Q (state) and cj (coefficient) per cell and a, ck per member.  Everything else is the lossy PML
// kernel's (k_batch_resident_pml_lossy, k_batch_e_pml_lossy) or the periodic one's (k_batch_resident_periodic,
// k_batch_e_periodic), step for step: H, the layer's split update, the sources and the monitors do not see the pole,
// and the streamed H launches are those kernels' own.
// The kernels below are separate kernels (instantiated in batch_dispersive.hip, reached through
// batch_dispersive_kernels()) so that every existing one keeps its code and registers.
//
// LDS of the resident kernels: Ez, Hx, Hy, Ezx, cb, ch, ca, then Jh, Q, cj behind them, so that every earlier array
// keeps its offset; then the factors, the phasor table, the point-source sums and the window accumulators.  Ten arrays:
// under 4096 float32 or 2048 float64 cells per member, so a workgroup always has at least a quarter as many threads as
// cells and 4 cells per thread is the only instance.  Jh, Q and cj are read and written at the thread's own cell index
// alone (neighbouring lanes, neighbouring banks), in the E phase that already owns the cell: no new barrier.
//
// The periodic image: the thread that owns (i, C-1) recomputes column 0's update.  Column 0's thread writes its Jh and Q
// in the same phase, so the image thread reads its own slots of Jh and Q as the old values (and cj of column 0, like
// cb and ca).  By the induction that keeps the image of Ez bit-identical to column 0 the image slots of Jh and Q stay
// bit-identical to column 0's; the host writes them from column 0 wherever it writes the state.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_periodic.hpp"

namespace fdtd {

// the pole of a batch: Jh, Q, cj in the fields' padded layout, a and ck per member
template <class T> struct BatchDisp {
    T *jh, *q;
    const T *cj, *a, *ck;
};

// a * Jh + (cj * e - ck * Q): one rounding per operation in the exact build; in the fused build the two fma are written
// out (as in batch_lossy_e and batch_periodic_split) so that the resident and the streamed kernel cannot contract
// differently
template <class T> __device__ __forceinline__ T batch_disp_j(T a, T jh, T cj, T e, T ck, T q)
{
#ifdef FDTD2D_FUSED
    return batch_periodic_fma(a, jh, batch_periodic_fma(cj, e, -(ck * q)));
#else
    return a * jh + (cj * e - ck * q);
#endif
}

// k_batch_resident_pml_lossy with the pole
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_pml_dispersive(BatchView<T> v, BatchPml<T> p,
                                                                                      BatchMon m, BatchPts P,
                                                                                      BatchDisp<T> d,
                                                                                      const T *__restrict__ ca, int n0,
                                                                                      int nt, long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_disp_pml_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_disp_pml_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *scb = sezx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sjh = sca + seg, *sq = sjh + seg, *scj = sq + seg;
    T *sfr = sez + 10 * seg;                  // ahr[R], bhr[R], aer[R], ber[R]
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
            sjh[l] = d.jh[g];
            sq[l] = d.q[g];
            scj[l] = d.cj[g];
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        for (int k = tid; k < 4 * C; k += nthr) sfc[k] = p.colf[(size_t)b * 4 * C + k];
        BatchSource<T> src;
        src.load(v, b);
        const T da = d.a[b], dck = d.ck[b];
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
                        const T jn = batch_disp_j(da, sjh[l], scj[l], e, dck, sq[l]);
                        sq[l] = sq[l] + jn;
                        e = batch_lossy_e(e, (dhy - dhx) - jn, sca[l], cc);
                        sjh[l] = jn;
                    }
                }
                if (src.covers(i, j)) e = (T)((double)e + amp);
                if (pts >> q & 1) e = (T)((double)e + ssum[batch_pts_entry(pts, q)]);
                sez[l] = e;
                if (ph.on) {
                    double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)l;
                    dd[0] += (double)e * ph.c;
                    dd[R * C] += (double)e * ph.s;
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
            d.jh[g] = sjh[l];
            d.q[g] = sq[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// k_batch_resident_periodic with the pole; the image thread takes its own slots of Jh and Q as the old values
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_periodic_dispersive(BatchView<T> v, BatchPml<T> p,
                                                                                           BatchMon m, BatchPts P,
                                                                                           BatchDisp<T> d,
                                                                                           const T *__restrict__ ca,
                                                                                           int n0, int nt,
                                                                                           long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_disp_periodic_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_disp_periodic_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *scb = sezx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sjh = sca + seg, *sq = sjh + seg, *scj = sq + seg;
    T *sfr = sez + 10 * seg;                  // ahr[R], bhr[R], aer[R], ber[R]
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
            sjh[l] = d.jh[g];
            sq[l] = d.q[g];
            scj[l] = d.cj[g];
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        BatchSource<T> src;
        src.load(v, b);
        const T da = d.a[b], dck = d.ck[b];
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
                        // Jh and Q at l, never lc: column 0's thread writes its own in this phase
                        const T jn = batch_disp_j(da, sjh[l], scj[lc], e, dck, sq[l]);
                        sq[l] = sq[l] + jn;
                        e = batch_lossy_e(e, (dhy - dhx) - jn, sca[lc], cc);
                        sjh[l] = jn;
                    }
                }
                if (src.covers(i, image ? 0 : j)) e = (T)((double)e + amp);
                if (pts >> q & 1) e = (T)((double)e + ssum[batch_pts_entry(pts, q)]);
                sez[l] = e;
                if (ph.on) {
                    double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)l;
                    dd[0] += (double)e * ph.c;
                    dd[R * C] += (double)e * ph.s;
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
            d.jh[g] = sjh[l];
            d.q[g] = sq[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed path: k_batch_e_pml_lossy and k_batch_e_periodic with the pole, in place, behind the H launches of
// k_batch_h_pml_mon_pts / k_batch_h_periodic (H does not see the pole)
template <class T>
__global__ __launch_bounds__(256) void k_batch_e_pml_dispersive(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                                BatchDisp<T> d, const T *__restrict__ ca, int n,
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
                const T qo = d.q[o];
                const T jn = batch_disp_j(d.a[b], d.jh[o], d.cj[o], e, d.ck[b], qo);
                d.q[o] = qo + jn;
                e = batch_lossy_e(e, (dhy - dhx) - jn, ca[o], cc);
                d.jh[o] = jn;
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, j)) e = (T)((double)e + src.amps[n]);
        e = batch_pts_cell(P, b, t, e);
        v.ez[o] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)t;
            dd[0] += (double)e * ph.c;
            dd[R * C] += (double)e * ph.s;
        }
        batch_mon_cell(m, b, t, i, j, step, (double)e);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_batch_e_periodic_dispersive(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                     BatchPts P, BatchDisp<T> d,
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
                // Jh and Q at o, never oc: column 0's thread writes its own in this launch
                const T qo = d.q[o];
                const T jn = batch_disp_j(d.a[b], d.jh[o], d.cj[oc], e, d.ck[b], qo);
                d.q[o] = qo + jn;
                e = batch_lossy_e(e, (dhy - dhx) - jn, ca[oc], cc);
                d.jh[o] = jn;
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, image ? 0 : j)) e = (T)((double)e + src.amps[n]);
        e = batch_pts_cell(P, b, t, e);
        v.ez[o] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)t;
            dd[0] += (double)e * ph.c;
            dd[R * C] += (double)e * ph.s;
        }
        batch_mon_cell(m, b, t, i, j, step, (double)e);
    }
}

// cj of a window (twin of k_batch_sigma_window): w holds count x nr x nc strengths in float64, bq[b] = dt / (1 + g_b);
// cj = (T)(dx * bq * EPS0 * wp2) with the products taken left to right in float64
template <class T>
__global__ __launch_bounds__(256) void k_batch_wp2_window(T *__restrict__ cj, const double *__restrict__ w,
                                                          const double *__restrict__ bq, int B, int r0, int c0, int nr,
                                                          int nc, long long pitch, size_t mstride, double dx, double eps0)
{
    const size_t W = (size_t)nr * nc, n = (size_t)B * W;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const size_t b = t / W;
        const int r = (int)(t - b * W), wi = r / nc, wj = r - wi * nc;
        const size_t g = b * mstride + (size_t)(r0 + wi) * pitch + (c0 + wj);
        cj[g] = (T)(((dx * bq[b]) * eps0) * w[t]);
    }
}

// host stubs of the kernels above (batch_dispersive.hip): 4 cells per thread alone
struct BatchDispersiveKernels {
    const void *resident_pml, *resident_periodic;
    const void *e_pml, *e_periodic;
};
template <class T> const BatchDispersiveKernels &batch_dispersive_kernels();
void batch_wp2_window_launch(void *cj, const double *w, const double *bq, bool dtype_f64, int B, int r0, int c0, int nr,
                             int nc, long long pitch, size_t mstride, double dx, double eps0, hipStream_t stream);

}  // namespace fdtd
