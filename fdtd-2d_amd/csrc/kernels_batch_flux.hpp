// Flux lines of the batched kernels (include/fdtd2d_batch_flux.h): up to 4 runs of cells on which the running Fourier
// transforms of Ez and of the tangential H centred on the same cells are accumulated at up to 16 frequencies per member.
// The kernels below are the lossy PML kernels (kernels_batch_lossy.hpp), the periodic ones (kernels_batch_periodic.hpp)
// and the two dispersive ones (kernels_batch_dispersive.hpp), step for step, plus the sums; one body per path with the
// family as a template argument, every arithmetic expression the family's own.  They are separate kernels (instantiated
// in batch_flux.hip, reached through batch_flux_kernels()) so that every existing one keeps its code and registers.
//
// The E phase already reads what a line needs: shx[l] and shx[l - C] for a row line, shy[l] and its left neighbour for a
// column line, and H is not written in that phase.  So the sums are taken where the window's are, by the thread that
// owns the cell once its new Ez is final, with no barrier of their own.
//
// Phasors: lanes nf .. nf + nff - 1 of a resident workgroup's last wave write them behind the window's during the H
// phase; on the streamed path block (0, y) of the H launch writes a count x nff table.  Every sum takes the same float64
// additions in the same order on every path and placement.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_dispersive.hpp"

namespace fdtd {

constexpr int BATCH_FLUX_MAX_LINES = 4;
constexpr int BATCH_FLUX_MAX_FREQ = 16;

struct BatchFlux {
    double *acc;              // per member 4 * nff * cells: Ez re[nff][cells], Ez im, Ht re, Ht im (global memory)
    const double *omega;      // count x nff, member-major
    double *ph;               // streamed path: count x nff x {cos, -sin} of the step being completed
    long long step0;          // samples the steps s with (s - step0) % every == 0, t = s * dt
    int nl, nff, every;       // nl = 0: no lines
    int cells;                // the lines' counts together
    int lds_acc;              // resident path: the member's sums live in LDS behind the window's
    // line k: orient 0 = row `index`, columns [first, first + count); 1 = column `index`, rows [first, first + count);
    // its cells start at `offset` in the concatenation
    int orient[BATCH_FLUX_MAX_LINES], index[BATCH_FLUX_MAX_LINES], first[BATCH_FLUX_MAX_LINES],
        count[BATCH_FLUX_MAX_LINES], offset[BATCH_FLUX_MAX_LINES];

    __device__ __forceinline__ bool sampled(long long step) const { return nl > 0 && (step - step0) % every == 0; }
    __device__ __forceinline__ size_t member_size() const { return 4 * (size_t)nff * (size_t)cells; }
    __device__ __forceinline__ double *member_acc(int b) const { return acc + (size_t)b * member_size(); }
};

// which lines hold cell (i, j): bit k for line k.  The geometry is the batch's, so a thread works this out once per
// launch for each of its cells and the step loop tests a bit.
__device__ __forceinline__ unsigned batch_flux_lines_of(const BatchFlux &f, int i, int j)
{
    unsigned on = 0;
#pragma unroll
    for (int k = 0; k < BATCH_FLUX_MAX_LINES; ++k) {
        if (k >= f.nl) continue;
        const bool col = f.orient[k] != 0;
        const int c = (col ? i : j) - f.first[k];
        if ((col ? j : i) == f.index[k] && (unsigned)c < (unsigned)f.count[k]) on |= 1u << k;
    }
    return on;
}

// the sums of cell (i, j), whose new Ez is e, on the lines `on` that hold it (batch_flux_lines_of; tab: nff x
// {cos, -sin}).  ht(column line?) gives the tangential H centred on the cell.
template <class HT>
__device__ __forceinline__ void batch_flux_cell(const BatchFlux &f, unsigned on, double *a, const double *tab, int i,
                                                int j, double e, HT &&ht)
{
    const size_t W = (size_t)f.cells;
#pragma unroll
    for (int k = 0; k < BATCH_FLUX_MAX_LINES; ++k) {
        if (!(on >> k & 1)) continue;
        const bool col = f.orient[k] != 0;
        const int c = (col ? i : j) - f.first[k];
        const double h = ht(col);
        const size_t w = (size_t)(f.offset[k] + c);
        for (int q = 0; q < f.nff; ++q) {
            const double pc = tab[2 * q], ps = tab[2 * q + 1];
            a[(size_t)q * W + w] += e * pc;
            a[(size_t)(f.nff + q) * W + w] += e * ps;
            a[(size_t)(2 * f.nff + q) * W + w] += h * pc;
            a[(size_t)(3 * f.nff + q) * W + w] += h * ps;
        }
    }
}

// ---- resident path ---------------------------------------------------------------------------------------------
// LDS = Ez, Hx, Hy, Ezx, cb, ch, ca (+ Jh, Q, cj with a pole), the factors, then the phasor table (the window's nf
// entries, then the lines' nff), the nc sums of the step, the window's accumulators (m.lds_acc) and the lines' (f.lds_acc).
// PER: periodic columns (k_batch_resident_periodic[_dispersive]), otherwise the PML box (k_batch_resident_pml_lossy /
// _dispersive); DISP: the pole.
template <class T, int MAXC, bool PER, bool DISP>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_flux(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                            BatchPts P, BatchDisp<T> d, BatchFlux f,
                                                                            const T *__restrict__ ca, int n0, int nt,
                                                                            long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_flux_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_flux_lds);
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

    unsigned long long fmask = 0;     // nibble q: the lines that hold cell q of this thread's walk
    cells([&](int q, int i, int j, int) { fmask |= (unsigned long long)batch_flux_lines_of(f, i, j) << (4 * q); });

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
        // the lines' sums and the lane's frequency (lanes nf .. nf + nff - 1 of the last wave)
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
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
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
                const unsigned on = (unsigned)(fmask >> (4 * q)) & 15u;
                if (fsampled && on) {
                    // H is not written in this phase.  A line never holds an image cell, so l is the cell itself; a row
                    // line has i >= 1 and a column line j >= 1 (or the cyclic neighbour), so both reads stay inside
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
// k_batch_h_pml_mon_pts<T, true> / k_batch_h_periodic, which also write the lines' phasors of the step: threads
// nf .. nf + nff - 1 of block (0, y), for its members
template <class T, bool PER>
__global__ __launch_bounds__(256) void k_batch_h_flux(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P, BatchFlux f,
                                                      int n, long long step)
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
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T e = v.ez[o];
        const T cc = v.ch[o];
        if constexpr (PER) {
            v.hx[o] = batch_periodic_split(v.hx[o], fr[i], fr[R + i], cc, v.ez[o + v.pitch] - e);
            v.hy[o] = batch_periodic_plain(v.hy[o], cc, v.ez[o + 1] - e);
        } else {
            const T *fc = p.colf + (size_t)b * 4 * C;
            v.hx[o] = fr[i] * v.hx[o] - (fr[R + i] * cc) * (v.ez[o + v.pitch] - e);
            v.hy[o] = fc[j] * v.hy[o] + (fc[C + j] * cc) * (v.ez[o + 1] - e);
        }
    }
}

// k_batch_e_pml_lossy / k_batch_e_periodic / k_batch_e_pml_dispersive / k_batch_e_periodic_dispersive with the lines, in
// place: H is read-only in this launch
template <class T, bool PER, bool DISP>
__global__ __launch_bounds__(256) void k_batch_e_flux(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                      BatchDisp<T> d, BatchFlux f, const T *__restrict__ ca, int n,
                                                      long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    const bool image = PER && j == C - 1;
    const bool interior = i >= 1 && i <= R - 2 && (PER || (j >= 1 && j <= C - 2));
    const bool layer = i < L || i > R - 1 - L || (!PER && (j < L || j > C - 1 - L));
    const unsigned on = batch_flux_lines_of(f, i, j);
    const bool fsampled = on && f.sampled(step);
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
        v.ez[o] = e;
        const BatchPhasor ph = batch_phasor(v, v.dft ? v.omega[b] : 0.0, step);
        if (ph.on) {
            double *dd = v.dft + (size_t)b * 2 * (size_t)(R * C) + (size_t)t;
            dd[0] += (double)e * ph.c;
            dd[R * C] += (double)e * ph.s;
        }
        batch_mon_cell(m, b, t, i, j, step, (double)e);
        if (fsampled) {
            // a line never holds an image cell or row 0, and column 0 only with PER: the reads stay inside the member
            auto ht = [&](bool col) {
                return col ? 0.5 * ((double)v.hy[ow] + (double)v.hy[o])
                           : 0.5 * ((double)v.hx[o - (size_t)v.pitch] + (double)v.hx[o]);
            };
            batch_flux_cell(f, on, f.member_acc(b), f.ph + (size_t)b * 2 * f.nff, i, j, (double)e, ht);
        }
    }
}

// host stubs of the kernels above (batch_flux.hip).  resident[PER][MAXC 4, 8, 16], resident_disp[PER] (4 cells per
// thread alone, like the dispersive kernels), h[PER], e[PER][DISP]
struct BatchFluxKernels {
    const void *resident[2][3], *resident_disp[2];
    const void *h[2], *e[2][2];
};
template <class T> const BatchFluxKernels &batch_flux_kernels();
// the launch of k_batch_flux (batch_flux.hip): P of every member, line and frequency into out (count x nl x nff)
void batch_flux_launch(const BatchFlux &f, double *out, int B, double dt, double dx, hipStream_t stream);

}  // namespace fdtd
