// Line sources of the batched kernels (include/fdtd2d_batch_flux_adjoint.h): the transpose of the flux monitor.  Every
// entry of the lines' concatenated cells adds a weighted sum of the run's channels to Ez and, halved, to the two H values
// the monitor averages for that cell.  The kernels below are the flux kernels (kernels_batch_flux.hpp), step for step,
// plus the injection; they are separate kernels (instantiated in batch_flux_adjoint.hip, reached through
// batch_flux_src_kernels()) so that the flux kernels keep their code and registers.
//
// Placement.  The weights (count x cells x nchan float64, twice) stay in global memory: they would not fit in LDS beside
// a member, and only the threads that own a line cell (E part) or one of its two H values (H part) read them, once per
// step.  Such a thread forms its own sums in batch_fluxsrc_gather (never inlined, so neither the channel loop nor the
// lines' geometry share the step loop's registers): no table, no barrier and no LDS of their own.  An H value gathers
// the terms of every entry that touches it in a fixed order (lines ascending, own cell before the neighbour cell), so
// lines that share an H value need no atomics and every path adds the same float64 numbers in the same order.  Which of
// a thread's cells take anything is worked out once per launch into two masks; the step loop tests a bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_flux.hpp"

namespace fdtd {

struct BatchFluxSrc {
    const double *we, *wh;    // count x cells x nchan, entry-major (nullptr: no electric / no magnetic part)
    const double *chan;       // chan[b * chan_mstride + c * chan_stride + n] for the run's step n
    const int *geom;          // the lines once more, in global memory for batch_fluxsrc_gather: line k at 5 k as
                              // {orientation, index, first, count, offset}, then the number of lines at 20
    long long chan_mstride, chan_stride;
    int nchan, cells;
};
constexpr int BATCH_FLUXSRC_GEOM = 5 * BATCH_FLUX_MAX_LINES + 1;

// The sums of one cell or one H value, out of line and fed by plain pointers alone: the step loops call it from a branch
// few threads take, and inlined it would hold the lines' geometry in the loops' registers (the 16-cell instances have
// none to spare).  w, chan: the member's weights and its channels at the run's step.
//   mode 0, the E part of cell (i, j):  a = 0.0; lines ascending that hold it: a = a + s(entry)
//   mode 1 (Hx, row lines) and 2 (Hy, column lines), the H part of H value (i, j):  a = 0.0; lines of that orientation
//   ascending, the own cell (i, j) before the neighbour cell (i2, j2): a = a + 0.5 * s(entry)
// with s(entry) = 0.0; s = s + w[entry][c] * chan[c] for c ascending.
static __device__ __attribute__((noinline)) double batch_fluxsrc_gather(const int *__restrict__ geom,
                                                                        const double *__restrict__ w,
                                                                        const double *__restrict__ chan, int nchan,
                                                                        size_t chan_stride, int mode, int i, int j, int i2,
                                                                        int j2)
{
    double a = 0.0;
    const int nl = geom[5 * BATCH_FLUX_MAX_LINES];
    for (int k = 0; k < nl; ++k) {
        const int col = geom[5 * k], index = geom[5 * k + 1], first = geom[5 * k + 2], count = geom[5 * k + 3];
        if (mode && (col != 0) != (mode == 2)) continue;
        for (int t = 0; t < (mode ? 2 : 1); ++t) {
            const int ci = t ? i2 : i, cj = t ? j2 : j;
            const int c = (col ? ci : cj) - first;
            if ((col ? cj : ci) != index || (unsigned)c >= (unsigned)count) continue;
            const double *we = w + (size_t)(geom[5 * k + 4] + c) * (size_t)nchan;
            double s = 0.0;
            for (int q = 0; q < nchan; ++q) s = s + we[q] * chan[(size_t)q * chan_stride];
            a = a + (mode ? 0.5 * s : s);
        }
    }
    return a;
}

// the neighbour cell that shares H value (i, j) with cell (i, j): (i + 1, j) for Hx, (i, j + 1) for Hy, cyclically with
// periodic columns (Hy[i][C-2] is the left neighbour of column 0)
template <bool PER> static __device__ __forceinline__ int batch_fluxsrc_next_col(int j, int C)
{
    return PER && j == C - 2 ? 0 : j + 1;
}

// the E part of cell (i, j) of member b in the run's step n
static __device__ __forceinline__ double batch_fluxsrc_e(const BatchFluxSrc &S, int b, int i, int j, long long n)
{
    return batch_fluxsrc_gather(S.geom, S.we + (size_t)b * (size_t)S.cells * (size_t)S.nchan,
                                S.chan + (size_t)b * (size_t)S.chan_mstride + (size_t)n, S.nchan, (size_t)S.chan_stride,
                                0, i, j, i, j);
}

// the H part of Hx[i][j] (hy false) or Hy[i][j] (hy true) of member b in the run's step n
template <bool PER>
static __device__ __forceinline__ double batch_fluxsrc_h(const BatchFluxSrc &S, int b, int i, int j, int C, bool hy,
                                                         long long n)
{
    return batch_fluxsrc_gather(S.geom, S.wh + (size_t)b * (size_t)S.cells * (size_t)S.nchan,
                                S.chan + (size_t)b * (size_t)S.chan_mstride + (size_t)n, S.nchan, (size_t)S.chan_stride,
                                hy ? 2 : 1, i, j, hy ? i : i + 1, hy ? batch_fluxsrc_next_col<PER>(j, C) : j);
}

// which of Hx[i][j] (bit 0) and Hy[i][j] (bit 1) take an H part: a row line holds (i, j) or (i + 1, j); a column line
// holds (i, j) or its right neighbour
template <bool PER> static __device__ __forceinline__ unsigned batch_fluxsrc_hbits(const BatchFlux &f, int i, int j, int C)
{
    unsigned cols = 0;
#pragma unroll
    for (int k = 0; k < BATCH_FLUX_MAX_LINES; ++k)
        if (k < f.nl && f.orient[k] != 0) cols |= 1u << k;
    const unsigned own = batch_flux_lines_of(f, i, j);
    const unsigned hx = (own | batch_flux_lines_of(f, i + 1, j)) & ~cols;
    const unsigned hy = (own | batch_flux_lines_of(f, i, batch_fluxsrc_next_col<PER>(j, C))) & cols;
    return (hx ? 1u : 0u) | (hy ? 2u : 0u);
}

// ---- resident path ---------------------------------------------------------------------------------------------
// k_batch_resident_flux with the line sources; the LDS layout is that kernel's.
template <class T, int MAXC, bool PER, bool DISP>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_flux_src(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                                BatchPts P, BatchDisp<T> d, BatchFlux f,
                                                                                BatchFluxSrc S, const T *__restrict__ ca,
                                                                                int n0, int nt, long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_flux_src_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_flux_src_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg, *scb = sezx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sjh = sca + seg, *sq = sjh + seg, *scj = sq + seg;   // with a pole alone
    T *sfr = sez + (DISP ? 10 : 7) * seg;     // ahr[R], bhr[R], aer[R], ber[R]
    T *sfc = sfr + batch_lds_seg<T>(4 * R);   // ahc[C], bhc[C], aec[C], bec[C] (periodic: all exactly 1, never read)
    double *stab = reinterpret_cast<double *>(sfc + batch_lds_seg<T>(4 * C)), *ftab = stab + 2 * m.nf;
    double *ssum = ftab + 2 * f.nff;
    double *sacc = ssum + P.nc;
    double *sfacc = sacc + (m.lds_acc ? 2 * (size_t)m.nf * m.window() : 0);
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

    // nibble q of fmask: the lines that hold cell q of this thread's walk; an image cell carries column 0's lines (it
    // repeats that cell's E part and takes no sums).  Bits 2q, 2q + 1 of hmask: Hx, Hy of cell q take an H part.
    unsigned long long fmask = 0;
    unsigned hmask = 0;
    cells([&](int q, int i, int j, int) {
        fmask |= (unsigned long long)batch_flux_lines_of(f, i, PER && j == C - 1 ? 0 : j) << (4 * q);
        if (S.wh && i <= R - 2 && j <= C - 2) hmask |= batch_fluxsrc_hbits<PER>(f, i, j, C) << (2 * q);
    });

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
            if constexpr (DISP) {
                sjh[l] = d.jh[g];
                sq[l] = d.q[g];
                scj[l] = d.cj[g];
            }
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        if constexpr (!PER)
            for (int k = tid; k < 4 * C; k += nthr) sfc[k] = p.colf[(size_t)b * 4 * C + k];
        BatchSource<T> src;
        src.load(v, b);
        [[maybe_unused]] T da = T(0), dck = T(0);
        if constexpr (DISP) {
            da = d.a[b];
            dck = d.ck[b];
        }
        const double omega = v.dft ? v.omega[b] : 0.0;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        double *const facc = f.member_acc(b);
        if (f.lds_acc) {
            const size_t n = f.member_size();
            for (size_t k = tid; k < n; k += nthr) sfacc[k] = facc[k];
        }
        const int flane = mon.lane - m.nf;
        const double fomega = flane >= 0 && flane < f.nff ? f.omega[(size_t)b * f.nff + flane] : 0.0;
        const int pts = batch_pts_begin(P, b, tid);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int q, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const unsigned hb = hmask >> (2 * q) & 3u;
                if (hb) {   // the H part, before the update
                    if (hb & 1u) shx[l] = (T)((double)shx[l] + batch_fluxsrc_h<PER>(S, b, i, j, C, false, n0 + s));
                    if (hb & 2u) shy[l] = (T)((double)shy[l] + batch_fluxsrc_h<PER>(S, b, i, j, C, true, n0 + s));
                }
                const T e = sez[l];
                const T cc = sch[l];
                if constexpr (PER) {
                    shx[l] = batch_periodic_split(shx[l], sfr[i], sfr[R + i], cc, sez[l + C] - e);
                    shy[l] = batch_periodic_plain(shy[l], cc, sez[l + 1] - e);
                } else {
                    shx[l] = sfr[i] * shx[l] - (sfr[R + i] * cc) * (sez[l + C] - e);
                    shy[l] = sfc[j] * shy[l] + (sfc[C + j] * cc) * (sez[l + 1] - e);
                }
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            if (flane >= 0 && flane < f.nff && f.sampled(step))
                batch_mon_phasor(ftab + 2 * flane, fomega, step, v.dt);
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step);
            const bool sampled = m.sampled(step), fsampled = f.sampled(step);
            cells([&](int q, int i, int j, int l) {
                T e = sez[l];
                const bool image = PER && j == C - 1;
                const int lc = image ? l - (C - 1) : l;              // the cell whose update this is
                const int lw = PER && j == 0 ? l + (C - 2) : l - 1;  // its left neighbour (cyclically with PER)
                if (i >= 1 && i <= R - 2 && (PER || (j >= 1 && j <= C - 2))) {
                    const T cc = scb[lc];
                    const T dhy = shy[lc] - shy[lw], dhx = shx[lc] - shx[lc - C];
                    if (i < L || i > R - 1 - L || (!PER && (j < L || j > C - 1 - L))) {
                        const T x = sezx[l];
                        T ey = e - x;
                        T ex;
                        if constexpr (PER) {
                            ex = batch_periodic_plain(x, cc, dhy);
                            ey = batch_periodic_split(ey, sfr[2 * R + i], sfr[3 * R + i], cc, dhx);
                        } else {
                            ex = sfc[2 * C + j] * x + (sfc[3 * C + j] * cc) * dhy;
                            ey = sfr[2 * R + i] * ey - (sfr[3 * R + i] * cc) * dhx;
                        }
                        sezx[l] = ex;
                        e = ex + ey;
                    } else if constexpr (DISP) {
                        // Jh and Q at l, never lc: column 0's thread writes its own in this phase
                        const T jn = batch_disp_j(da, sjh[l], scj[lc], e, dck, sq[l]);
                        sq[l] = sq[l] + jn;
                        e = batch_lossy_e(e, (dhy - dhx) - jn, sca[lc], cc);
                        sjh[l] = jn;
                    } else {
                        e = batch_lossy_e(e, dhy - dhx, sca[lc], cc);
                    }
                }
                if (src.covers(i, image ? 0 : j)) e = (T)((double)e + amp);
                if (pts >> q & 1) e = (T)((double)e + ssum[batch_pts_entry(pts, q)]);
                const unsigned on = (unsigned)(fmask >> (4 * q)) & 15u;
                if (S.we && on) e = (T)((double)e + batch_fluxsrc_e(S, b, i, image ? 0 : j, n0 + s));
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
                if (fsampled && on && !image) {
                    // H is not written in this phase.  l is the cell itself; a row line has i >= 1 and a column line
                    // j >= 1 (or the cyclic neighbour), so both reads stay inside
                    auto ht = [&](bool col) {
                        return col ? 0.5 * ((double)shy[lw] + (double)shy[l]) : 0.5 * ((double)shx[l - C] + (double)shx[l]);
                    };
                    if (f.lds_acc) batch_flux_cell(f, on, sfacc, ftab, i, j, (double)e, ht);
                    else batch_flux_cell(f, on, facc, ftab, i, j, (double)e, ht);
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
            if constexpr (DISP) {
                d.jh[g] = sjh[l];
                d.q[g] = sq[l];
            }
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        if (f.lds_acc) {
            const size_t n = f.member_size();
            for (size_t k = tid; k < n; k += nthr) facc[k] = sfacc[k];
        }
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// ---- streamed path ---------------------------------------------------------------------------------------------
// k_batch_h_flux with the H part, before the update of the thread's own two values
template <class T, bool PER>
__global__ __launch_bounds__(256) void k_batch_h_flux_src(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                          BatchFlux f, BatchFluxSrc S, int n, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    {
        const int k = (int)threadIdx.x - m.nf;
        if (blockIdx.x == 0 && k >= 0 && k < f.nff && f.sampled(step))
            for (int b = blockIdx.y; b < v.B; b += gridDim.y)
                batch_mon_phasor(f.ph + ((size_t)b * f.nff + k) * 2, f.omega[(size_t)b * f.nff + k], step, v.dt);
    }
    batch_pts_table(P, v.B, n);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    const unsigned hb = S.wh ? batch_fluxsrc_hbits<PER>(f, i, j, C) : 0u;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T e = v.ez[o];
        const T cc = v.ch[o];
        T hx = v.hx[o], hy = v.hy[o];
        if (hb & 1u) hx = (T)((double)hx + batch_fluxsrc_h<PER>(S, b, i, j, C, false, n));
        if (hb & 2u) hy = (T)((double)hy + batch_fluxsrc_h<PER>(S, b, i, j, C, true, n));
        if constexpr (PER) {
            v.hx[o] = batch_periodic_split(hx, fr[i], fr[R + i], cc, v.ez[o + v.pitch] - e);
            v.hy[o] = batch_periodic_plain(hy, cc, v.ez[o + 1] - e);
        } else {
            const T *fc = p.colf + (size_t)b * 4 * C;
            v.hx[o] = fr[i] * hx - (fr[R + i] * cc) * (v.ez[o + v.pitch] - e);
            v.hy[o] = fc[j] * hy + (fc[C + j] * cc) * (v.ez[o + 1] - e);
        }
    }
}

// k_batch_e_flux with the E part behind the point sources
template <class T, bool PER, bool DISP>
__global__ __launch_bounds__(256) void k_batch_e_flux_src(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                          BatchDisp<T> d, BatchFlux f, BatchFluxSrc S,
                                                          const T *__restrict__ ca, int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    const bool image = PER && j == C - 1;
    const bool interior = i >= 1 && i <= R - 2 && (PER || (j >= 1 && j <= C - 2));
    const bool layer = i < L || i > R - 1 - L || (!PER && (j < L || j > C - 1 - L));
    const unsigned on = batch_flux_lines_of(f, i, image ? 0 : j);   // an image cell repeats column 0's E part
    const bool fsampled = on && !image && f.sampled(step);
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const size_t oc = image ? o - (size_t)(C - 1) : o;
        const size_t ow = PER && j == 0 ? o + (size_t)(C - 2) : o - 1;
        T e = v.ez[o];
        if (interior) {
            const T cc = v.ce[oc];
            const T dhy = v.hy[oc] - v.hy[ow], dhx = v.hx[oc] - v.hx[oc - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R;
                const T x = p.ezx[o];
                T ey = e - x;
                T ex;
                if constexpr (PER) {
                    ex = batch_periodic_plain(x, cc, dhy);
                    ey = batch_periodic_split(ey, fr[2 * R + i], fr[3 * R + i], cc, dhx);
                } else {
                    const T *fc = p.colf + (size_t)b * 4 * C;
                    ex = fc[2 * C + j] * x + (fc[3 * C + j] * cc) * dhy;
                    ey = fr[2 * R + i] * ey - (fr[3 * R + i] * cc) * dhx;
                }
                p.ezx[o] = ex;
                e = ex + ey;
            } else if constexpr (DISP) {
                // Jh and Q at o, never oc: column 0's thread writes its own in this launch
                const T qo = d.q[o];
                const T jn = batch_disp_j(d.a[b], d.jh[o], d.cj[oc], e, d.ck[b], qo);
                d.q[o] = qo + jn;
                e = batch_lossy_e(e, (dhy - dhx) - jn, ca[oc], cc);
                d.jh[o] = jn;
            } else {
                e = batch_lossy_e(e, dhy - dhx, ca[oc], cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, image ? 0 : j)) e = (T)((double)e + src.amps[n]);
        e = batch_pts_cell(P, b, t, e);
        if (S.we && on) e = (T)((double)e + batch_fluxsrc_e(S, b, i, image ? 0 : j, n));
        v.ez[o] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)t;
            dd[0] += (double)e * ph.c;
            dd[R * C] += (double)e * ph.s;
        }
        batch_mon_cell(m, b, t, i, j, step, (double)e);
        if (fsampled) {
            // a line never holds row 0, and column 0 only with PER: the reads stay inside the member
            auto ht = [&](bool col) {
                return col ? 0.5 * ((double)v.hy[ow] + (double)v.hy[o])
                           : 0.5 * ((double)v.hx[o - (size_t)v.pitch] + (double)v.hx[o]);
            };
            batch_flux_cell(f, on, f.member_acc(b), f.ph + (size_t)b * 2 * f.nff, i, j, (double)e, ht);
        }
    }
}

// host stubs of the kernels above, in BatchFluxKernels' layout (batch_flux_adjoint.hip)
template <class T> const BatchFluxKernels &batch_flux_src_kernels();

// what k_batch_flux_line_weights reads and writes (fdtd2d_batch_flux_line_weights)
struct BatchFluxWeights {
    const double *dJdP;               // count x nl x nff
    const double *solve;              // 2 nff x 2 nff row-major, at solve + b * solve_mstride
    const double *scale_e, *scale_h;  // count x cells (nullptr: ones)
    double *we, *wh;                  // count x cells x 2 nff
    long long solve_mstride;
};
void batch_flux_line_weights_launch(const BatchFlux &f, const BatchFluxWeights &W, int B, double dt, double dx,
                                    hipStream_t stream);

}  // namespace fdtd
