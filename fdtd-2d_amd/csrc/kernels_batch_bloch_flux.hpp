// Flux lines of a Bloch batch (include/fdtd2d_batch_bloch_flux.h): the lines of kernels_batch_flux.hpp on complex fields.
// The kernels below are the Bloch kernels (kernels_batch_bloch.hpp) and, with DISP, the Bloch kernels with the pole
// (kernels_batch_bloch_dispersive.hpp), step for step, plus the sums; every arithmetic expression of the step is the
// family's own.  They are separate kernels (instantiated in batch_bloch_flux.hip, reached through
// batch_bloch_flux_kernels()) so that every existing one keeps its code and registers.
//
// The sums.  Each part of the field (real, imaginary) is a real field with the sums of kernels_batch_flux.hpp: a block
// `Ez re[nff][cells], Ez im, Ht re, Ht im` per member and part, the real part's in BatchFlux::acc and the imaginary
// part's in a second array of the same layout (as BatchBloch::acc sits next to BatchMon::acc).  batch_flux_cell is
// called once per part with the same phasor table.  The sums are taken in the E phase by the thread that owns the cell,
// once both parts of its new Ez are final; H is not written in that phase, so they add no barrier.
//
// The seam.  A column line at column 0 needs Hy of the cell to its left, which lies across the seam: the value the E
// half-step itself subtracts, batch_bloch_unrot(c, s, Hy_re[i, C-2], Hy_im[i, C-2]) in T (the fused build's fma form
// there), then widened.  It is recomputed on the line cell alone, so that the step's own (wr, wi) do not stay live over
// the source and the window, and it is evaluated the same way on rows 0 and R-1, where the step skips the update.
//
// Phasors: lanes nf .. nf + nff - 1 of a resident workgroup's last wave write them behind the window's during the H
// phase; on the streamed path block (0, y) of the H launch writes a count x nff table.  Every sum takes the same float64
// additions in the same order on every path, placement and launch split.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_bloch_dispersive.hpp"
#include "kernels_batch_flux.hpp"

namespace fdtd {

// the tangential H of both parts, centred on cell l = (i, j) of a line: hx / hy index the cell itself, hxu the cell above,
// hyw the cell to the left (cyclically), whose value is rotated back across the seam when j == 0
template <class T>
__device__ __forceinline__ void batch_bloch_flux_ht(bool col, bool seam, T rc, T rs, T hxr_u, T hxr, T hxi_u, T hxi,
                                                    T hyr_w, T hyr, T hyi_w, T hyi, double &htr, double &hti)
{
    if (!col) {
        htr = 0.5 * ((double)hxr_u + (double)hxr);
        hti = 0.5 * ((double)hxi_u + (double)hxi);
        return;
    }
    T lr = hyr_w, li = hyi_w;
    if (seam) batch_bloch_unrot(rc, rs, hyr_w, hyi_w, lr, li);
    htr = 0.5 * ((double)lr + (double)hyr);
    hti = 0.5 * ((double)li + (double)hyi);
}

// ---- resident path ---------------------------------------------------------------------------------------------
// LDS = the family's arrays (11, or 16 with the pole), the row factors, the source weights, then the phasor table (the
// window's nf entries, then the lines' nff), the window's accumulators of both parts (m.lds_acc) and the lines' sums of
// both parts (f.lds_acc).  4 cells per thread, like the kernels this copies.
template <class T, bool DISP>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_bloch_flux(
    BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl, BatchBlochDisp<T> d, BatchFlux f, double *facc_im,
    const T *__restrict__ ca, int n0, int nt, long long step_base)
{
    constexpr int MAXC = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_bloch_flux_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_bloch_flux_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg;
    T *siz = sezx + seg, *six = siz + seg, *siy = six + seg, *sizx = siy + seg;
    T *scb = sizx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sjh = sca + seg, *sq = sjh + seg, *sjhi = sq + seg, *sqi = sjhi + seg, *scj = sqi + seg;   // with a pole alone
    T *sfr = sez + (DISP ? 16 : 11) * seg;    // ahr[R], bhr[R], aer[R], ber[R]
    double *sw = reinterpret_cast<double *>(sfr + batch_lds_seg<T>(4 * R));   // wr[C-1], wi[C-1]
    double *stab = sw + 2 * (C - 1), *ftab = stab + 2 * m.nf;
    double *sacc = ftab + 2 * f.nff, *sacci = sacc + 2 * (size_t)m.nf * m.window();
    double *sfacc = sacc + (m.lds_acc ? 4 * (size_t)m.nf * m.window() : 0), *sfacci = sfacc + f.member_size();
    BatchMon mi = m;                          // the monitors of the imaginary part: same window, phasors and cells
    mi.acc = bl.acc;
    mi.trace = bl.trace;
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

    unsigned fmask = 0;               // nibble q: the lines that hold cell q of this thread's walk
    cells([&](int q, int i, int j, int) { fmask |= batch_flux_lines_of(f, i, j) << (4 * q); });

    for (int b = blockIdx.x; b < v.B; b += gridDim.x) {
        const size_t base = (size_t)b * v.mstride;
        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            sez[l] = v.ez[g];
            shx[l] = v.hx[g];
            shy[l] = v.hy[g];
            sezx[l] = p.ezx[g];
            siz[l] = bl.ez[g];
            six[l] = bl.hx[g];
            siy[l] = bl.hy[g];
            sizx[l] = bl.ezx[g];
            scb[l] = v.ce[g];
            sch[l] = v.ch[g];
            sca[l] = ca[g];
            if constexpr (DISP) {
                sjh[l] = d.jh[g];
                sq[l] = d.q[g];
                sjhi[l] = d.jh_i[g];
                sqi[l] = d.q_i[g];
                scj[l] = d.cj[g];
            }
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = bl.w[(size_t)b * 2 * (C - 1) + k];
        const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
        [[maybe_unused]] T da = T(0), dck = T(0);
        if constexpr (DISP) {
            da = d.a[b];
            dck = d.ck[b];
        }
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = bl.amps && src.r1 > src.r0 ? bl.amps + (size_t)b * v.amp_stride : nullptr;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const BatchMonMember moni = batch_mon_begin(mi, b, sacci, tid, nthr);
        // the lines' sums of both parts and the lane's frequency (lanes nf .. nf + nff - 1 of the last wave)
        double *const facc = f.member_acc(b), *const facci = facc_im + (size_t)b * f.member_size();
        if (f.lds_acc) {
            const size_t n = f.member_size();
            for (size_t k = tid; k < n; k += nthr) {
                sfacc[k] = facc[k];
                sfacci[k] = facci[k];
            }
        }
        const int flane = mon.lane - m.nf;
        const double fomega = flane >= 0 && flane < f.nff ? f.omega[(size_t)b * f.nff + flane] : 0.0;
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const bool seam = j == C - 2;             // the right neighbour is the image: rho * column 0
                const T kc = seam ? rc : (T)1, ks = seam ? rs : (T)0;
                T nr, ni;
                batch_bloch_rot(kc, ks, sez[l + 1], siz[l + 1], nr, ni);
                const T cc = sch[l], fa = sfr[i], fb = sfr[R + i];
                const T er = sez[l], ei = siz[l];
                shx[l] = batch_periodic_split(shx[l], fa, fb, cc, sez[l + C] - er);
                shy[l] = batch_periodic_plain(shy[l], cc, nr - er);
                six[l] = batch_periodic_split(six[l], fa, fb, cc, siz[l + C] - ei);
                siy[l] = batch_periodic_plain(siy[l], cc, ni - ei);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            if (flane >= 0 && flane < f.nff && f.sampled(step))
                batch_mon_phasor(ftab + 2 * flane, fomega, step, v.dt);
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step), fsampled = f.sampled(step);
            cells([&](int q, int i, int j, int l) {
                T er = sez[l], ei = siz[l];
                const bool image = j == C - 1;
                const int lc = image ? l - (C - 1) : l;       // the cell whose update this is
                const int lw = j == 0 ? l + (C - 2) : l - 1;  // its left neighbour, cyclically
                if (i >= 1 && i <= R - 2) {
                    const bool wrap = j == 0 || image;        // that neighbour is across the seam: conj(rho) * Hy
                    const T kc = wrap ? rc : (T)1, ks = wrap ? rs : (T)0;
                    T wr, wi;
                    batch_bloch_unrot(kc, ks, shy[lw], siy[lw], wr, wi);
                    const T cc = scb[lc];
                    const T dhyr = shy[lc] - wr, dhxr = shx[lc] - shx[lc - C];
                    const T dhyi = siy[lc] - wi, dhxi = six[lc] - six[lc - C];
                    if (i < L || i > R - 1 - L) {
                        const T fa = sfr[2 * R + i], fb = sfr[3 * R + i];
                        const T xr = sezx[l], xi = sizx[l];
                        const T exr = batch_periodic_plain(xr, cc, dhyr);
                        const T eyr = batch_periodic_split(er - xr, fa, fb, cc, dhxr);
                        const T exi = batch_periodic_plain(xi, cc, dhyi);
                        const T eyi = batch_periodic_split(ei - xi, fa, fb, cc, dhxi);
                        sezx[l] = exr;
                        sizx[l] = exi;
                        er = exr + eyr;
                        ei = exi + eyi;
                    } else if constexpr (DISP) {
                        // Jh and Q at l, never lc: column 0's thread writes its own in this phase
                        const T a = sca[lc], cj = scj[lc];
                        const T jr = batch_disp_j(da, sjh[l], cj, er, dck, sq[l]);
                        const T ji = batch_disp_j(da, sjhi[l], cj, ei, dck, sqi[l]);
                        sq[l] = sq[l] + jr;
                        sqi[l] = sqi[l] + ji;
                        er = batch_lossy_e(er, (dhyr - dhxr) - jr, a, cc);
                        ei = batch_lossy_e(ei, (dhyi - dhxi) - ji, a, cc);
                        sjh[l] = jr;
                        sjhi[l] = ji;
                    } else {
                        const T a = sca[lc];
                        er = batch_lossy_e(er, dhyr - dhxr, a, cc);
                        ei = batch_lossy_e(ei, dhyi - dhxi, a, cc);
                    }
                }
                const int js = image ? 0 : j;                 // the image takes column 0's source
                if (src.covers(i, js)) {
                    double dr, dq;
                    batch_bloch_source(ar, ai, sw[js], sw[C - 1 + js], dr, dq);
                    er = (T)((double)er + dr);
                    ei = (T)((double)ei + dq);
                }
                sez[l] = er;
                siz[l] = ei;
                if (sampled) {
                    // two copies of the adds, so that the LDS one uses LDS instructions, not flat ones
                    const int w = m.window_cell(i, j);
                    if (w >= 0 && m.lds_acc) {
                        m.add(sacc, stab, w, (double)er);
                        m.add(sacci, stab, w, (double)ei);
                    } else if (w >= 0) {
                        m.add(mon.acc, stab, w, (double)er);
                        m.add(moni.acc, stab, w, (double)ei);
                    }
                }
                const unsigned on = (fmask >> (4 * q)) & 15u;
                if (fsampled && on) {
                    // H is not written in this phase.  A line never holds an image cell, so l is the cell itself; a row
                    // line has i >= 1 and a column line reads its cyclic neighbour lw, so every read stays inside
                    auto ht = [&](bool col, double &htr, double &hti) {
                        const int lu = col ? l : l - C;       // a column line never reads the row above
                        batch_bloch_flux_ht(col, j == 0, rc, rs, shx[lu], shx[l], six[lu], six[l], shy[lw], shy[l],
                                            siy[lw], siy[l], htr, hti);
                    };
                    auto htr = [&](bool col) {
                        double a, c;
                        ht(col, a, c);
                        return a;
                    };
                    auto hti = [&](bool col) {
                        double a, c;
                        ht(col, a, c);
                        return c;
                    };
                    if (f.lds_acc) {
                        batch_flux_cell(f, on, sfacc, ftab, i, j, (double)er, htr);
                        batch_flux_cell(f, on, sfacci, ftab, i, j, (double)ei, hti);
                    } else {
                        batch_flux_cell(f, on, facc, ftab, i, j, (double)er, htr);
                        batch_flux_cell(f, on, facci, ftab, i, j, (double)ei, hti);
                    }
                }
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, sez, step);
            batch_mon_probes(mi, moni, b, siz, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = sez[l];
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
            p.ezx[g] = sezx[l];
            bl.ez[g] = siz[l];
            bl.hx[g] = six[l];
            bl.hy[g] = siy[l];
            bl.ezx[g] = sizx[l];
            if constexpr (DISP) {
                d.jh[g] = sjh[l];
                d.q[g] = sq[l];
                d.jh_i[g] = sjhi[l];
                d.q_i[g] = sqi[l];
            }
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        batch_mon_end(mi, b, sacci, tid, nthr);
        if (f.lds_acc) {
            const size_t n = f.member_size();
            for (size_t k = tid; k < n; k += nthr) {
                facc[k] = sfacc[k];
                facci[k] = sfacci[k];
            }
        }
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// ---- streamed path ---------------------------------------------------------------------------------------------
// k_batch_h_bloch, which also writes the lines' phasors of the step: threads nf .. nf + nff - 1 of block (0, y), for its
// members
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_bloch_flux(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                            BatchFlux f, long long step)
{
    batch_mon_phasor_table(m, v.B, step, v.dt);
    {
        const int k = (int)threadIdx.x - m.nf;
        if (blockIdx.x == 0 && k >= 0 && k < f.nff && f.sampled(step))
            for (int b = blockIdx.y; b < v.B; b += gridDim.y)
                batch_mon_phasor(f.ph + ((size_t)b * f.nff + k) * 2, f.omega[(size_t)b * f.nff + k], step, v.dt);
    }
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    const bool seam = j == C - 2;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T kc = seam ? bl.rho[2 * b] : (T)1, ks = seam ? bl.rho[2 * b + 1] : (T)0;
        T nr, ni;
        batch_bloch_rot(kc, ks, v.ez[o + 1], bl.ez[o + 1], nr, ni);
        const T cc = v.ch[o], fa = fr[i], fb = fr[R + i];
        const T er = v.ez[o], ei = bl.ez[o];
        v.hx[o] = batch_periodic_split(v.hx[o], fa, fb, cc, v.ez[o + v.pitch] - er);
        v.hy[o] = batch_periodic_plain(v.hy[o], cc, nr - er);
        bl.hx[o] = batch_periodic_split(bl.hx[o], fa, fb, cc, bl.ez[o + v.pitch] - ei);
        bl.hy[o] = batch_periodic_plain(bl.hy[o], cc, ni - ei);
    }
}

// k_batch_e_bloch / k_batch_e_bloch_dispersive with the lines, in place: H is read-only in this launch
template <class T, bool DISP>
__global__ __launch_bounds__(256) void k_batch_e_bloch_flux(BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl,
                                                            BatchBlochDisp<T> d, BatchFlux f, double *facc_im,
                                                            const T *__restrict__ ca, int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    const bool image = j == C - 1;
    const bool wrap = j == 0 || image;
    const bool interior = i >= 1 && i <= R - 2;
    const bool layer = i < L || i > R - 1 - L;
    const int js = image ? 0 : j;
    const unsigned on = batch_flux_lines_of(f, i, j);
    const bool fsampled = on && f.sampled(step);
    BatchMon mi = m;
    mi.acc = bl.acc;
    mi.trace = bl.trace;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const size_t oc = image ? o - (size_t)(C - 1) : o;
        const size_t ow = j == 0 ? o + (size_t)(C - 2) : o - 1;
        T er = v.ez[o], ei = bl.ez[o];
        if (interior) {
            const T kc = wrap ? bl.rho[2 * b] : (T)1, ks = wrap ? bl.rho[2 * b + 1] : (T)0;
            T wr, wi;
            batch_bloch_unrot(kc, ks, v.hy[ow], bl.hy[ow], wr, wi);
            const T cc = v.ce[oc];
            const T dhyr = v.hy[oc] - wr, dhxr = v.hx[oc] - v.hx[oc - v.pitch];
            const T dhyi = bl.hy[oc] - wi, dhxi = bl.hx[oc] - bl.hx[oc - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R;
                const T fa = fr[2 * R + i], fb = fr[3 * R + i];
                const T xr = p.ezx[o], xi = bl.ezx[o];
                const T exr = batch_periodic_plain(xr, cc, dhyr);
                const T eyr = batch_periodic_split(er - xr, fa, fb, cc, dhxr);
                const T exi = batch_periodic_plain(xi, cc, dhyi);
                const T eyi = batch_periodic_split(ei - xi, fa, fb, cc, dhxi);
                p.ezx[o] = exr;
                bl.ezx[o] = exi;
                er = exr + eyr;
                ei = exi + eyi;
            } else if constexpr (DISP) {
                // Jh and Q at o, never oc: column 0's thread writes its own in this launch
                const T a = ca[oc], cj = d.cj[oc], da = d.a[b], dck = d.ck[b];
                const T qr = d.q[o], qi = d.q_i[o];
                const T jr = batch_disp_j(da, d.jh[o], cj, er, dck, qr);
                const T ji = batch_disp_j(da, d.jh_i[o], cj, ei, dck, qi);
                d.q[o] = qr + jr;
                d.q_i[o] = qi + ji;
                er = batch_lossy_e(er, (dhyr - dhxr) - jr, a, cc);
                ei = batch_lossy_e(ei, (dhyi - dhxi) - ji, a, cc);
                d.jh[o] = jr;
                d.jh_i[o] = ji;
            } else {
                const T a = ca[oc];
                er = batch_lossy_e(er, dhyr - dhxr, a, cc);
                ei = batch_lossy_e(ei, dhyi - dhxi, a, cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, js)) {
            const double *w = bl.w + (size_t)b * 2 * (C - 1);
            const double ai = bl.amps ? bl.amps[(size_t)b * v.amp_stride + n] : 0.0;
            double dr, dq;
            batch_bloch_source(src.amps[n], ai, w[js], w[C - 1 + js], dr, dq);
            er = (T)((double)er + dr);
            ei = (T)((double)ei + dq);
        }
        v.ez[o] = er;
        bl.ez[o] = ei;
        batch_mon_cell(m, b, t, i, j, step, (double)er);
        batch_mon_cell(mi, b, t, i, j, step, (double)ei);
        if (fsampled) {
            // a line never holds an image cell or (a row line) row 0: the reads stay inside the member
            const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
            auto ht = [&](bool col, double &htr, double &hti) {
                const size_t ou = col ? o : o - (size_t)v.pitch;   // a column line never reads the row above
                batch_bloch_flux_ht(col, j == 0, rc, rs, v.hx[ou], v.hx[o], bl.hx[ou], bl.hx[o], v.hy[ow], v.hy[o],
                                    bl.hy[ow], bl.hy[o], htr, hti);
            };
            auto htr = [&](bool col) {
                double a, c;
                ht(col, a, c);
                return a;
            };
            auto hti = [&](bool col) {
                double a, c;
                ht(col, a, c);
                return c;
            };
            const double *tab = f.ph + (size_t)b * 2 * f.nff;
            batch_flux_cell(f, on, f.member_acc(b), tab, i, j, (double)er, htr);
            batch_flux_cell(f, on, facc_im + (size_t)b * f.member_size(), tab, i, j, (double)ei, hti);
        }
    }
}

// host stubs of the kernels above (batch_bloch_flux.hip): [DISP]
struct BatchBlochFluxKernels {
    const void *resident[2], *h, *e[2];
};
template <class T> const BatchBlochFluxKernels &batch_bloch_flux_kernels();
// the launch of k_batch_bloch_flux (batch_bloch_flux.hip): P of every member, line and frequency into out (count x nl x
// nff), from the sums of both parts
void batch_bloch_flux_launch(const BatchFlux &f, const double *facc_im, double *out, int B, double dt, double dx,
                             hipStream_t stream);

}  // namespace fdtd
