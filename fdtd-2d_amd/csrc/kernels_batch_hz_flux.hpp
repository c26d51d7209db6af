// Flux lines of a batch in the Hz polarisation (include/fdtd2d_batch_hz_flux.h): the lines of fdtd2d_batch_flux.h carried
// through the duality Hz = Ez, Ex = -Hx, Ey = -Hy.  On the line cells the running Fourier transforms of Hz and of the
// tangential E centred on the same cells are accumulated: Et = 0.5 (Ex[i-1,j] + Ex[i,j]) on a row line and
// 0.5 (Ey[i,j-1] + Ey[i,j]) on a column line, which is the Ez kernels' Ht expression applied to the Hx slot (it holds Ex)
// and the Hy slot (it holds Ey).  The sums keep the layout of BatchFlux: the batch's "Ez" arrays hold the transform of Hz,
// its "Ht" arrays that of Et.
// The kernels below are those of kernels_batch_hz.hpp step for step, plus the sums.  They are separate kernels
// (instantiated in batch_hz_flux.hip, reached through batch_hz_flux_kernels()) so that every existing one keeps its code
// and registers.
//
// The H half-step already reads what a line needs: sex[l] and sex[l - C] for a row line, sey[l] and its left neighbour for
// a column line, and Ex, Ey are not written in that phase.  So the sums are taken where the window's are, by the thread
// that owns the cell once its new Hz is final, with no barrier of their own; the thread that owns the image column takes
// none (a line never holds an image cell).
//
// Phasors: lanes nf .. nf + nff - 1 of a resident workgroup's last wave write them behind the window's during the E
// half-step; on the streamed path block (0, y) of the E launch writes a count x nff table.  Every sum takes the same
// float64 additions in the same order on every path and placement.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_flux.hpp"
#include "kernels_batch_hz.hpp"

namespace fdtd {

// k_batch_resident_hz with the lines.  LDS: the arrays and factors of k_batch_resident_hz, then the phasor table (the
// window's nf entries, then the lines' nff), the nc sums of the step, the window's accumulators (m.lds_acc) and the lines'
// (f.lds_acc).
template <class T, bool PER, bool POLE, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_hz_flux(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                               BatchPts P, BatchHzDisp<T> d, BatchFlux f,
                                                                               const T *__restrict__ ca, int n0, int nt,
                                                                               long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_hz_flux_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *shz = reinterpret_cast<T *>(batch_hz_flux_lds);
    T *sex = shz + seg, *sey = sex + seg, *shzx = sey + seg, *sch = shzx + seg, *scb = sch + seg, *sca = scb + seg;
    T *scj = sca + seg, *sjx = scj + seg, *sqx = sjx + seg, *sjy = sqx + seg, *sqy = sjy + seg;   // POLE alone
    T *sfr = shz + (POLE ? 12 : 7) * seg;     // ahr[R], bhr[R], aer[R], ber[R]
    T *sfc = sfr + batch_lds_seg<T>(4 * R);   // ahc[C], bhc[C], aec[C], bec[C] (PER: exactly 1, never read)
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

    unsigned fmask = 0;               // nibble q: the lines that hold cell q of this thread's walk (MAXC <= 8)
    cells([&](int q, int i, int j, int) { fmask |= batch_flux_lines_of(f, i, j) << (4 * q); });

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
            if (flane >= 0 && flane < f.nff && f.sampled(step))
                batch_mon_phasor(ftab + 2 * flane, fomega, step, v.dt);
            batch_pts_sums(P, b, mon.lane, ssum, n0 + s);
            __syncthreads();
            const double amp = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const BatchPhasor ph = batch_phasor(v, omega, step);
            const bool sampled = m.sampled(step), fsampled = f.sampled(step);
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
                const unsigned on = (fmask >> (4 * q)) & 15u;
                if (fsampled && on) {
                    // Ex and Ey are not written in this phase.  A line never holds an image cell, so l is the cell
                    // itself; a row line has i >= 1 and a column line j >= 1 (or the cyclic neighbour), so both reads
                    // stay inside the member
                    auto et = [&](bool col) {
                        return col ? 0.5 * ((double)sey[lw] + (double)sey[l]) : 0.5 * ((double)sex[l - C] + (double)sex[l]);
                    };
                    if (f.lds_acc) batch_flux_cell(f, on, sfacc, ftab, i, j, (double)h, et);
                    else batch_flux_cell(f, on, facc, ftab, i, j, (double)h, et);
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
        if (f.lds_acc) {
            const size_t n = f.member_size();
            for (size_t k = tid; k < n; k += nthr) facc[k] = sfacc[k];
        }
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed path, first launch of a step: k_batch_e_hz, which also writes the lines' phasors of the step: threads
// nf .. nf + nff - 1 of block (0, y), for its members
template <class T, bool PER, bool POLE>
__global__ __launch_bounds__(256) void k_batch_e_hz_flux(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                         BatchHzDisp<T> d, BatchFlux f, const T *__restrict__ ca, int n,
                                                         long long step)
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

// second launch: k_batch_h_hz with the lines, in place: Ex and Ey are read-only in this launch
template <class T, bool PER>
__global__ __launch_bounds__(256) void k_batch_h_hz_flux(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchPts P,
                                                         BatchFlux f, int n, long long step)
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
        if (fsampled) {
            // a line never holds an image cell or row 0, and column 0 only with PER: the reads stay inside the member
            auto et = [&](bool col) {
                return col ? 0.5 * ((double)v.hy[ow] + (double)v.hy[o])
                           : 0.5 * ((double)v.hx[o - (size_t)v.pitch] + (double)v.hx[o]);
            };
            batch_flux_cell(f, on, f.member_acc(b), f.ph + (size_t)b * 2 * f.nff, i, j, (double)h, et);
        }
    }
}

// host stubs of the kernels above (batch_hz_flux.hip): [periodic][pole], the resident ones also [MAXC 4, 8] (with a pole
// 4 alone, as in BatchHzKernels)
struct BatchHzFluxKernels {
    const void *resident[2][2][2];
    const void *e[2][2];
    const void *h[2];
};
template <class T> const BatchHzFluxKernels &batch_hz_flux_kernels();
// the launch of k_batch_hz_flux (batch_hz_flux.hip): P of every member, line and frequency into out (count x nl x nff)
void batch_hz_flux_launch(const BatchFlux &f, double *out, int B, double dt, double dx, hipStream_t stream);

}  // namespace fdtd
