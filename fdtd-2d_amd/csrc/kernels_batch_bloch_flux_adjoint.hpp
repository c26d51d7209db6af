// Line sources on the flux lines of a Bloch batch (include/fdtd2d_batch_bloch_flux_adjoint.h): the transpose of the
// complex monitor.  The kernels below are the Bloch flux kernels (kernels_batch_bloch_flux.hpp), step for step, plus the
// injection of kernels_batch_flux_adjoint.hpp on both parts of the field; they are separate kernels (instantiated in
// batch_bloch_flux_adjoint.hip, reached through batch_bloch_flux_src_kernels()) so that every existing one keeps its code
// and registers.
//
// Placement is that of kernels_batch_flux_adjoint.hpp.  The weights (count x cells x nchan float64, up to four arrays)
// stay in global memory; the threads that own a line cell (E part) or one of its two H values (H part) form their sums in
// batch_bfluxsrc_gather, never inlined, so neither the channel loop nor the lines' geometry share the step loop's
// registers: no table, no barrier and no LDS of their own.  An H value gathers the terms of every entry that touches it
// in a fixed order (lines ascending, own cell before the neighbour cell).  Which of a thread's cells take anything is
// worked out once per launch into one mask; the step loop tests a bit.
//
// The seam.  Hy[i][C-2] is the left neighbour of column 0 across the seam; the monitor reads it as conj(rho) Hy[i][C-2].
// The neighbour term of a column-0 entry is therefore rotated by the rotation the launch steps with (bl.rho: (c, s), or
// (c, -s) in a conjugated run), widened from the batch dtype: re' = c tr - s ti, im' = c ti + s tr in float64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_bloch_flux.hpp"
#include "kernels_batch_flux_adjoint.hpp"

namespace fdtd {

struct BatchBlochFluxSrc {
    const double *we_re, *we_im, *wh_re, *wh_im;   // count x cells x nchan, entry-major (nullptr: that part is absent)
    const double *chan;       // chan[b * chan_mstride + c * chan_stride + n] for the run's step n
    const int *geom;          // BatchFluxSrc::geom
    long long chan_mstride, chan_stride;
    int nchan, cells;
};

struct BatchBlochPair {
    double re, im;
};

// batch_fluxsrc_gather on both parts: w_re, w_im the member's weights of one kind (either may be nullptr: its sums are
// 0.0), chan its channels at the run's step.  Per term, s_re = 0.0; s_re = s_re + w_re[entry][c] * chan[c] for c
// ascending, s_im likewise; (tr, ti) = (s_re, s_im) in mode 0 and (0.5 s_re, 0.5 s_im) in modes 1 and 2; with seam, the
// neighbour term is rotated: (c tr - s ti, c ti + s tr); then a_re = a_re + tr, a_im = a_im + ti.
static __device__ __attribute__((noinline)) BatchBlochPair batch_bfluxsrc_gather(
    const int *__restrict__ geom, const double *__restrict__ w_re, const double *__restrict__ w_im,
    const double *__restrict__ chan, int nchan, size_t chan_stride, int mode, int i, int j, int i2, int j2, bool seam,
    double rc, double rs)
{
    BatchBlochPair a{0.0, 0.0};
    const int nl = geom[5 * BATCH_FLUX_MAX_LINES];
    for (int k = 0; k < nl; ++k) {
        const int col = geom[5 * k], index = geom[5 * k + 1], first = geom[5 * k + 2], count = geom[5 * k + 3];
        if (mode && (col != 0) != (mode == 2)) continue;
        for (int t = 0; t < (mode ? 2 : 1); ++t) {
            const int ci = t ? i2 : i, cj = t ? j2 : j;
            const int c = (col ? ci : cj) - first;
            if ((col ? cj : ci) != index || (unsigned)c >= (unsigned)count) continue;
            const size_t o = (size_t)(geom[5 * k + 4] + c) * (size_t)nchan;
            double sr = 0.0, si = 0.0;
            if (w_re)
                for (int q = 0; q < nchan; ++q) sr = sr + w_re[o + q] * chan[(size_t)q * chan_stride];
            if (w_im)
                for (int q = 0; q < nchan; ++q) si = si + w_im[o + q] * chan[(size_t)q * chan_stride];
            double tr = mode ? 0.5 * sr : sr, ti = mode ? 0.5 * si : si;
            if (t && seam) {
                const double pr = rc * tr, qr = rs * ti, pi = rc * ti, qi = rs * tr;
                tr = pr - qr;
                ti = pi + qi;
            }
            a.re = a.re + tr;
            a.im = a.im + ti;
        }
    }
    return a;
}

// the E part of cell (i, j) of member b in the run's step n
static __device__ __forceinline__ BatchBlochPair batch_bfluxsrc_e(const BatchBlochFluxSrc &S, int b, int i, int j,
                                                                  long long n)
{
    const size_t m = (size_t)b * (size_t)S.cells * (size_t)S.nchan;
    return batch_bfluxsrc_gather(S.geom, S.we_re ? S.we_re + m : nullptr, S.we_im ? S.we_im + m : nullptr,
                                 S.chan + (size_t)b * (size_t)S.chan_mstride + (size_t)n, S.nchan, (size_t)S.chan_stride,
                                 0, i, j, i, j, false, 1.0, 0.0);
}

// the H part of Hx[i][j] (hy false) or Hy[i][j] (hy true) of member b in the run's step n; (rc, rs): the launch's rotation
static __device__ __forceinline__ BatchBlochPair batch_bfluxsrc_h(const BatchBlochFluxSrc &S, int b, int i, int j, int C,
                                                                  bool hy, long long n, double rc, double rs)
{
    const size_t m = (size_t)b * (size_t)S.cells * (size_t)S.nchan;
    return batch_bfluxsrc_gather(S.geom, S.wh_re ? S.wh_re + m : nullptr, S.wh_im ? S.wh_im + m : nullptr,
                                 S.chan + (size_t)b * (size_t)S.chan_mstride + (size_t)n, S.nchan, (size_t)S.chan_stride,
                                 hy ? 2 : 1, i, j, hy ? i : i + 1, hy ? batch_fluxsrc_next_col<true>(j, C) : j,
                                 hy && j == C - 2, rc, rs);
}

// ---- resident path ---------------------------------------------------------------------------------------------
// k_batch_resident_bloch_flux with the line sources; the LDS layout is that kernel's.
template <class T, bool DISP>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_bloch_flux_src(
    BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl, BatchBlochDisp<T> d, BatchFlux f, double *facc_im,
    BatchBlochFluxSrc S, const T *__restrict__ ca, int n0, int nt, long long step_base)
{
    constexpr int MAXC = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_bloch_flux_src_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_bloch_flux_src_lds);
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

    // nibble q of the low half: the lines that hold cell q of this thread's walk; an image cell carries column 0's lines
    // (it repeats that cell's E part and takes no sums).  Bits 16 + 2q, 17 + 2q: Hx, Hy of cell q take an H part.
    const bool have_e = S.we_re || S.we_im, have_h = S.wh_re || S.wh_im;
    unsigned fmask = 0;
    cells([&](int q, int i, int j, int) {
        fmask |= batch_flux_lines_of(f, i, j == C - 1 ? 0 : j) << (4 * q);
        if (have_h && i <= R - 2 && j <= C - 2) fmask |= batch_fluxsrc_hbits<true>(f, i, j, C) << (16 + 2 * q);
    });

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
            cells([&](int q, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const unsigned hb = fmask >> (16 + 2 * q) & 3u;
                if (hb) {   // the H part of both parts of the field, before the update
                    if (hb & 1u) {
                        const BatchBlochPair a = batch_bfluxsrc_h(S, b, i, j, C, false, n0 + s, (double)rc, (double)rs);
                        shx[l] = (T)((double)shx[l] + a.re);
                        six[l] = (T)((double)six[l] + a.im);
                    }
                    if (hb & 2u) {
                        const BatchBlochPair a = batch_bfluxsrc_h(S, b, i, j, C, true, n0 + s, (double)rc, (double)rs);
                        shy[l] = (T)((double)shy[l] + a.re);
                        siy[l] = (T)((double)siy[l] + a.im);
                    }
                }
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
                const unsigned on = (fmask >> (4 * q)) & 15u;
                if (have_e && on) {                           // the E part; the image slot repeats column 0's, unrotated
                    const BatchBlochPair a = batch_bfluxsrc_e(S, b, i, js, n0 + s);
                    if (S.we_re) er = (T)((double)er + a.re);
                    if (S.we_im) ei = (T)((double)ei + a.im);
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
                if (fsampled && on && !image) {
                    // H is not written in this phase.  l is the cell itself; a row line has i >= 1 and a column line
                    // reads its cyclic neighbour lw, so every read stays inside
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
// k_batch_h_bloch_flux with the H part, before the update of the thread's own two values (of each part)
template <class T>
__global__ __launch_bounds__(256) void k_batch_h_bloch_flux_src(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                BatchBloch<T> bl, BatchFlux f, BatchBlochFluxSrc S, int n,
                                                                long long step)
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
    const unsigned hb = S.wh_re || S.wh_im ? batch_fluxsrc_hbits<true>(f, i, j, C) : 0u;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t o = (size_t)b * v.mstride + (size_t)i * (size_t)v.pitch + (size_t)j;
        const T *fr = p.rowf + (size_t)b * 4 * R;
        const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
        const T kc = seam ? rc : (T)1, ks = seam ? rs : (T)0;
        T nr, ni;
        batch_bloch_rot(kc, ks, v.ez[o + 1], bl.ez[o + 1], nr, ni);
        const T cc = v.ch[o], fa = fr[i], fb = fr[R + i];
        const T er = v.ez[o], ei = bl.ez[o];
        T hxr = v.hx[o], hyr = v.hy[o], hxi = bl.hx[o], hyi = bl.hy[o];
        if (hb & 1u) {
            const BatchBlochPair a = batch_bfluxsrc_h(S, b, i, j, C, false, n, (double)rc, (double)rs);
            hxr = (T)((double)hxr + a.re);
            hxi = (T)((double)hxi + a.im);
        }
        if (hb & 2u) {
            const BatchBlochPair a = batch_bfluxsrc_h(S, b, i, j, C, true, n, (double)rc, (double)rs);
            hyr = (T)((double)hyr + a.re);
            hyi = (T)((double)hyi + a.im);
        }
        v.hx[o] = batch_periodic_split(hxr, fa, fb, cc, v.ez[o + v.pitch] - er);
        v.hy[o] = batch_periodic_plain(hyr, cc, nr - er);
        bl.hx[o] = batch_periodic_split(hxi, fa, fb, cc, bl.ez[o + v.pitch] - ei);
        bl.hy[o] = batch_periodic_plain(hyi, cc, ni - ei);
    }
}

// k_batch_e_bloch_flux with the E part behind the rectangle source
template <class T, bool DISP>
__global__ __launch_bounds__(256) void k_batch_e_bloch_flux_src(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                BatchBloch<T> bl, BatchBlochDisp<T> d, BatchFlux f,
                                                                double *facc_im, BatchBlochFluxSrc S,
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
    const unsigned on = batch_flux_lines_of(f, i, js);   // an image cell repeats column 0's E part
    const bool fsampled = on && !image && f.sampled(step);
    const bool have_e = S.we_re || S.we_im;
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
        if (have_e && on) {
            const BatchBlochPair a = batch_bfluxsrc_e(S, b, i, js, n);
            if (S.we_re) er = (T)((double)er + a.re);
            if (S.we_im) ei = (T)((double)ei + a.im);
        }
        v.ez[o] = er;
        bl.ez[o] = ei;
        batch_mon_cell(m, b, t, i, j, step, (double)er);
        batch_mon_cell(mi, b, t, i, j, step, (double)ei);
        if (fsampled) {
            // a line never holds (a row line) row 0, and the image takes no sums: the reads stay inside the member
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

// host stubs of the kernels above, in BatchBlochFluxKernels' layout (batch_bloch_flux_adjoint.hip)
template <class T> const BatchBlochFluxKernels &batch_bloch_flux_src_kernels();

// what k_batch_bloch_flux_line_weights reads and writes (fdtd2d_batch_bloch_flux_line_weights): BatchFluxWeights, whose
// we and wh become the real parts' weights
void batch_bloch_flux_line_weights_launch(const BatchFlux &f, const double *facc_im, const BatchFluxWeights &W, int B,
                                          double dt, double dx, hipStream_t stream);

}  // namespace fdtd
