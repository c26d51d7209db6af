// Flux lines of an Hz Bloch batch (include/fdtd2d_batch_hz_bloch_flux.h): the lines of kernels_batch_hz_flux.hpp on the
// complex fields of kernels_batch_hz_bloch.hpp.  The kernels below are the Hz Bloch kernels step for step, plus the sums;
// every arithmetic expression of the step is that family's own.  They are separate kernels (instantiated in
// batch_hz_bloch_flux.hip, reached through batch_hz_bloch_flux_kernels()) so that every existing one keeps its code and
// registers.
//
// The sums.  Each part of the fields (real, imaginary) is a real field with the sums of kernels_batch_hz_flux.hpp: a block
// `Hz re[nff][cells], Hz im, Et re, Et im` per member and part, the real part's in BatchFlux::acc and the imaginary
// part's in a second array of the same layout, as in kernels_batch_bloch_flux.hpp.  batch_flux_cell is called once per
// part with the same phasor table.  The sums are taken in the H phase, where kernels_batch_hz_flux.hpp takes them: by the
// thread that owns the cell, once both parts of its new Hz are final.  Ex and Ey are not written in that phase, so they
// add no barrier; the thread that owns the image column takes none (a line never holds an image cell).
//
// The seam.  A column line at column 0 needs Ey of the cell to its left, which lies across the seam: the value the H
// half-step itself subtracts, batch_bloch_unrot(c, s, Ey_re[i, C-2], Ey_im[i, C-2]) in T (the fused build's fma form
// there), then widened.  batch_bloch_flux_ht recomputes it on the line cell alone, so that the step's own (wr, wi) do not
// stay live over the source and the window, and evaluates it the same way on rows 0 and R-1, where the step skips the
// update.  It is the Ez lines' Ht expression applied to the Hx slot (it holds Ex) and the Hy slot (it holds Ey).
//
// Phasors: lanes nf .. nf + nff - 1 of a resident workgroup's last wave write them behind the window's during the E
// half-step; on the streamed path block (0, y) of the E launch writes a count x nff table.  Every sum takes the same
// float64 additions in the same order on every path, placement and launch split.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_bloch_flux.hpp"
#include "kernels_batch_hz_bloch.hpp"

namespace fdtd {

// ---- resident path ---------------------------------------------------------------------------------------------
// k_batch_resident_hz_bloch<T, POLE, 4> with the lines.  LDS = the family's arrays (11, or 20 with the pole), the row
// factors, the source weights, then the phasor table (the window's nf entries, then the lines' nff), the window's
// accumulators of both parts (m.lds_acc) and the lines' sums of both parts (f.lds_acc).  Two barriers per step.
template <class T, bool POLE>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_hz_bloch_flux(
    BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl, BatchHzBlochDisp<T> d, BatchFlux f, double *facc_im,
    const T *__restrict__ ca, int n0, int nt, long long step_base)
{
    constexpr int MAXC = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_hz_bloch_flux_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *shz = reinterpret_cast<T *>(batch_hz_bloch_flux_lds);
    T *sex = shz + seg, *sey = sex + seg, *shzx = sey + seg;
    T *siz = shzx + seg, *six = siz + seg, *siy = six + seg, *sizx = siy + seg;
    T *sch = sizx + seg, *scb = sch + seg, *sca = scb + seg;
    T *scj = sca + seg, *sjx = scj + seg, *sqx = sjx + seg, *sjy = sqx + seg, *sqy = sjy + seg;   // POLE alone
    T *sjxi = sqy + seg, *sqxi = sjxi + seg, *sjyi = sqxi + seg, *sqyi = sjyi + seg;              // POLE alone
    T *sfr = shz + (POLE ? 20 : 11) * seg;    // ahr[R], bhr[R], aer[R], ber[R]
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
            shz[l] = v.ez[g];
            sex[l] = v.hx[g];
            sey[l] = v.hy[g];
            shzx[l] = p.ezx[g];
            siz[l] = bl.ez[g];
            six[l] = bl.hx[g];
            siy[l] = bl.hy[g];
            sizx[l] = bl.ezx[g];
            sch[l] = v.ch[g];
            scb[l] = v.ce[g];
            sca[l] = ca[g];
            if constexpr (POLE) {
                scj[l] = d.cj[g];
                sjx[l] = d.jx[g];
                sqx[l] = d.qx[g];
                sjy[l] = d.jy[g];
                sqy[l] = d.qy[g];
                sjxi[l] = d.jxi[g];
                sqxi[l] = d.qxi[g];
                sjyi[l] = d.jyi[g];
                sqyi[l] = d.qyi[g];
            }
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = bl.w[(size_t)b * 2 * (C - 1) + k];
        const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = bl.amps && src.r1 > src.r0 ? bl.amps + (size_t)b * v.amp_stride : nullptr;
        T da = T(0), dck = T(0);
        if constexpr (POLE) {
            da = d.a[b];
            dck = d.ck[b];
        }
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
            cells([&](int, int i, int j, int l) {   // the E half-step
                if (i > R - 2 || j > C - 2) return;
                const bool seam = j == C - 2;             // the right neighbour is the image: rho * column 0
                const T kc = seam ? rc : (T)1, ks = seam ? rs : (T)0;
                T nr, ni;
                batch_bloch_rot(kc, ks, shz[l + 1], siz[l + 1], nr, ni);
                const T hr = shz[l], hi = siz[l];
                const T dxr = shz[l + C] - hr, dyr = nr - hr;
                const T dxi = siz[l + C] - hi, dyi = ni - hi;
                const bool mat = i >= L && i <= R - 2 - L;
                const T a = sca[l], cb = scb[l], fa = sfr[i], fb = sfr[R + i];
                T exr = sex[l], eyr = sey[l], exi = six[l], eyi = siy[l];
                if constexpr (POLE) {
                    const T cj = scj[l];
                    batch_hz_e<T, true, true>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, sjx[l],
                                              sqx[l], sjy[l], sqy[l]);
                    batch_hz_e<T, true, true>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, sjxi[l],
                                              sqxi[l], sjyi[l], sqyi[l]);
                } else {
                    T z = T(0);
                    batch_hz_e<T, true, false>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), da, dck, z, z, z, z, z);
                    batch_hz_e<T, true, false>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), da, dck, z, z, z, z, z);
                }
                sex[l] = exr;
                sey[l] = eyr;
                six[l] = exi;
                siy[l] = eyi;
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            if (flane >= 0 && flane < f.nff && f.sampled(step))
                batch_mon_phasor(ftab + 2 * flane, fomega, step, v.dt);
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step), fsampled = f.sampled(step);
            cells([&](int q, int i, int j, int l) {   // the H half-step, the source, the monitors
                T hr = shz[l], hi = siz[l];
                const bool image = j == C - 1;
                const int lc = image ? l - (C - 1) : l;       // the cell whose update this is
                const int lw = j == 0 ? l + (C - 2) : l - 1;  // its left neighbour, cyclically
                if (i >= 1 && i <= R - 2) {
                    const bool wrap = j == 0 || image;        // that neighbour is across the seam: conj(rho) * Ey
                    const T kc = wrap ? rc : (T)1, ks = wrap ? rs : (T)0;
                    T wr, wi;
                    batch_bloch_unrot(kc, ks, sey[lw], siy[lw], wr, wi);
                    const T cc = sch[lc];
                    const T deyr = sey[lc] - wr, dexr = sex[lc] - sex[lc - C];
                    const T deyi = siy[lc] - wi, dexi = six[lc] - six[lc - C];
                    if (i < L || i > R - 1 - L) {
                        const T fa = sfr[2 * R + i], fb = sfr[3 * R + i];
                        const T xr = shzx[l], xi = sizx[l];
                        const T xnr = batch_periodic_plain(xr, cc, -deyr);
                        const T ynr = batch_hz_split(hr - xr, fa, fb, cc, dexr);
                        const T xni = batch_periodic_plain(xi, cc, -deyi);
                        const T yni = batch_hz_split(hi - xi, fa, fb, cc, dexi);
                        shzx[l] = xnr;
                        sizx[l] = xni;
                        hr = xnr + ynr;
                        hi = xni + yni;
                    } else {
                        hr = batch_hz_plain(hr, deyr - dexr, cc);
                        hi = batch_hz_plain(hi, deyi - dexi, cc);
                    }
                }
                const int js = image ? 0 : j;                 // the image takes column 0's source
                if (src.covers(i, js)) {
                    double dr, dq;
                    batch_bloch_source(ar, ai, sw[js], sw[C - 1 + js], dr, dq);
                    hr = (T)((double)hr + dr);
                    hi = (T)((double)hi + dq);
                }
                shz[l] = hr;
                siz[l] = hi;
                if (sampled) {
                    // two copies of the adds, so that the LDS one uses LDS instructions, not flat ones
                    const int w = m.window_cell(i, j);
                    if (w >= 0 && m.lds_acc) {
                        m.add(sacc, stab, w, (double)hr);
                        m.add(sacci, stab, w, (double)hi);
                    } else if (w >= 0) {
                        m.add(mon.acc, stab, w, (double)hr);
                        m.add(moni.acc, stab, w, (double)hi);
                    }
                }
                const unsigned on = (fmask >> (4 * q)) & 15u;
                if (fsampled && on) {
                    // Ex and Ey are not written in this phase.  A line never holds an image cell, so l is the cell
                    // itself; a row line has i >= 1 and a column line reads its cyclic neighbour lw, so every read stays
                    // inside the member
                    auto et = [&](bool col, double &etr, double &eti) {
                        const int lu = col ? l : l - C;       // a column line never reads the row above
                        batch_bloch_flux_ht(col, j == 0, rc, rs, sex[lu], sex[l], six[lu], six[l], sey[lw], sey[l],
                                            siy[lw], siy[l], etr, eti);
                    };
                    auto etr = [&](bool col) {
                        double a, c;
                        et(col, a, c);
                        return a;
                    };
                    auto eti = [&](bool col) {
                        double a, c;
                        et(col, a, c);
                        return c;
                    };
                    if (f.lds_acc) {
                        batch_flux_cell(f, on, sfacc, ftab, i, j, (double)hr, etr);
                        batch_flux_cell(f, on, sfacci, ftab, i, j, (double)hi, eti);
                    } else {
                        batch_flux_cell(f, on, facc, ftab, i, j, (double)hr, etr);
                        batch_flux_cell(f, on, facci, ftab, i, j, (double)hi, eti);
                    }
                }
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, shz, step);
            batch_mon_probes(mi, moni, b, siz, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = shz[l];
            v.hx[g] = sex[l];
            v.hy[g] = sey[l];
            p.ezx[g] = shzx[l];
            bl.ez[g] = siz[l];
            bl.hx[g] = six[l];
            bl.hy[g] = siy[l];
            bl.ezx[g] = sizx[l];
            if constexpr (POLE) {
                d.jx[g] = sjx[l];
                d.qx[g] = sqx[l];
                d.jy[g] = sjy[l];
                d.qy[g] = sqy[l];
                d.jxi[g] = sjxi[l];
                d.qxi[g] = sqxi[l];
                d.jyi[g] = sjyi[l];
                d.qyi[g] = sqyi[l];
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
// k_batch_e_hz_bloch, which also writes the lines' phasors of the step: threads nf .. nf + nff - 1 of block (0, y), for
// its members
template <class T, bool POLE>
__global__ __launch_bounds__(256) void k_batch_e_hz_bloch_flux(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                               BatchBloch<T> bl, BatchHzBlochDisp<T> d, BatchFlux f,
                                                               const T *__restrict__ ca, long long step)
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
    const int R = v.R, C = v.C, L = p.L, i = t / C, j = t % C;
    if (i > R - 2 || j > C - 2) return;
    const bool seam = j == C - 2;
    const bool mat = i >= L && i <= R - 2 - L;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T kc = seam ? bl.rho[2 * b] : (T)1, ks = seam ? bl.rho[2 * b + 1] : (T)0;
        T nr, ni;
        batch_bloch_rot(kc, ks, v.ez[o + 1], bl.ez[o + 1], nr, ni);
        const T hr = v.ez[o], hi = bl.ez[o];
        const T dxr = v.ez[o + v.pitch] - hr, dyr = nr - hr;
        const T dxi = bl.ez[o + v.pitch] - hi, dyi = ni - hi;
        const T a = ca[o], cb = v.ce[o], fa = fr[i], fb = fr[R + i];
        T exr = v.hx[o], eyr = v.hy[o], exi = bl.hx[o], eyi = bl.hy[o];
        if constexpr (POLE) {
            const T da = d.a[b], dck = d.ck[b], cj = d.cj[o];
            T jx = d.jx[o], qx = d.qx[o], jy = d.jy[o], qy = d.qy[o];
            T jxi = d.jxi[o], qxi = d.qxi[o], jyi = d.jyi[o], qyi = d.qyi[o];
            batch_hz_e<T, true, true>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, jx, qx, jy, qy);
            batch_hz_e<T, true, true>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), da, dck, cj, jxi, qxi, jyi, qyi);
            if (mat) {
                d.jx[o] = jx;
                d.qx[o] = qx;
                d.jy[o] = jy;
                d.qy[o] = qy;
                d.jxi[o] = jxi;
                d.qxi[o] = qxi;
                d.jyi[o] = jyi;
                d.qyi[o] = qyi;
            }
        } else {
            T z = T(0);
            batch_hz_e<T, true, false>(exr, eyr, dxr, dyr, mat, a, cb, fa, fb, T(1), T(1), z, z, z, z, z, z, z);
            batch_hz_e<T, true, false>(exi, eyi, dxi, dyi, mat, a, cb, fa, fb, T(1), T(1), z, z, z, z, z, z, z);
        }
        v.hx[o] = exr;
        v.hy[o] = eyr;
        bl.hx[o] = exi;
        bl.hy[o] = eyi;
    }
}

// k_batch_h_hz_bloch with the lines, in place: Ex and Ey are read-only in this launch
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_hz_bloch_flux(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                               BatchBloch<T> bl, BatchFlux f, double *facc_im, int n,
                                                               long long step)
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
        T hr = v.ez[o], hi = bl.ez[o];
        if (interior) {
            const T kc = wrap ? bl.rho[2 * b] : (T)1, ks = wrap ? bl.rho[2 * b + 1] : (T)0;
            T wr, wi;
            batch_bloch_unrot(kc, ks, v.hy[ow], bl.hy[ow], wr, wi);
            const T cc = v.ch[oc];
            const T deyr = v.hy[oc] - wr, dexr = v.hx[oc] - v.hx[oc - v.pitch];
            const T deyi = bl.hy[oc] - wi, dexi = bl.hx[oc] - bl.hx[oc - v.pitch];
            if (layer) {
                const T *fr = p.rowf + (size_t)b * 4 * R;
                const T fa = fr[2 * R + i], fb = fr[3 * R + i];
                const T xr = p.ezx[o], xi = bl.ezx[o];
                const T xnr = batch_periodic_plain(xr, cc, -deyr);
                const T ynr = batch_hz_split(hr - xr, fa, fb, cc, dexr);
                const T xni = batch_periodic_plain(xi, cc, -deyi);
                const T yni = batch_hz_split(hi - xi, fa, fb, cc, dexi);
                p.ezx[o] = xnr;
                bl.ezx[o] = xni;
                hr = xnr + ynr;
                hi = xni + yni;
            } else {
                hr = batch_hz_plain(hr, deyr - dexr, cc);
                hi = batch_hz_plain(hi, deyi - dexi, cc);
            }
        }
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(i, js)) {
            const double *w = bl.w + (size_t)b * 2 * (C - 1);
            const double ai = bl.amps ? bl.amps[(size_t)b * v.amp_stride + n] : 0.0;
            double dr, dq;
            batch_bloch_source(src.amps[n], ai, w[js], w[C - 1 + js], dr, dq);
            hr = (T)((double)hr + dr);
            hi = (T)((double)hi + dq);
        }
        v.ez[o] = hr;
        bl.ez[o] = hi;
        batch_mon_cell(m, b, t, i, j, step, (double)hr);
        batch_mon_cell(mi, b, t, i, j, step, (double)hi);
        if (fsampled) {
            // a line never holds an image cell or (a row line) row 0: the reads stay inside the member
            const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
            auto et = [&](bool col, double &etr, double &eti) {
                const size_t ou = col ? o : o - (size_t)v.pitch;   // a column line never reads the row above
                batch_bloch_flux_ht(col, j == 0, rc, rs, v.hx[ou], v.hx[o], bl.hx[ou], bl.hx[o], v.hy[ow], v.hy[o],
                                    bl.hy[ow], bl.hy[o], etr, eti);
            };
            auto etr = [&](bool col) {
                double a, c;
                et(col, a, c);
                return a;
            };
            auto eti = [&](bool col) {
                double a, c;
                et(col, a, c);
                return c;
            };
            const double *tab = f.ph + (size_t)b * 2 * f.nff;
            batch_flux_cell(f, on, f.member_acc(b), tab, i, j, (double)hr, etr);
            batch_flux_cell(f, on, facc_im + (size_t)b * f.member_size(), tab, i, j, (double)hi, eti);
        }
    }
}

// host stubs of the kernels above (batch_hz_bloch_flux.hip): [pole]
struct BatchHzBlochFluxKernels {
    const void *resident[2];
    const void *e[2];
    const void *h;
};
template <class T> const BatchHzBlochFluxKernels &batch_hz_bloch_flux_kernels();
// the launch of k_batch_hz_bloch_flux (batch_hz_bloch_flux.hip): P of every member, line and frequency into out (count x
// nl x nff), from the sums of both parts
void batch_hz_bloch_flux_launch(const BatchFlux &f, const double *facc_im, double *out, int B, double dt, double dx,
                                hipStream_t stream);

}  // namespace fdtd
