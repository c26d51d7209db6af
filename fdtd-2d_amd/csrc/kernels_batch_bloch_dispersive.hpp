// The Drude-Lorentz pole for batches with complex fields (include/fdtd2d_batch_bloch_dispersive.h): copies of the Bloch
// kernels (kernels_batch_bloch.hpp) and of the lattice kernels (kernels_batch_lattice.hpp) with the pole block of
// kernels_batch_dispersive.hpp in the E phase.  Every pole coefficient is real, so each part (real, imaginary) of a cell
// that takes the plain update takes
//     jn = a * Jh + (cj * e - ck * Q);  Q = Q + jn;  e = ca * e + ((dhy - dhx) - jn) * cb;  Jh = jn
// with its own Jh and Q; dhy and dhx are the Bloch / lattice kernel's, the seam neighbours already rotated by conj(rho).
// H, the layer's split update, the source and the monitors do not see the pole, and the streamed H launches are the
// families' own (k_batch_h_bloch, k_batch_h_lattice).  The kernels below are separate kernels (instantiated in
// batch_bloch_dispersive.hip, reached through batch_bloch_dispersive_kernels()) so that every existing one keeps its code
// and registers.
//
// LDS of the resident kernels: the family's arrays (11 Bloch, 9 lattice), then Jh, Q (real), Jh, Q (imaginary) and cj
// behind them, so that every earlier array keeps its offset; then what the family keeps behind its arrays.  16 and 14
// arrays: under 2560 / 2926 float32 cells per member, so a workgroup always has at least a quarter as many threads as
// cells and 4 cells per thread is the only instance.  The four state arrays are read and written at the thread's own
// cell index alone (consecutive lanes, consecutive words), cj at the index of the cell whose update it is (like cb and
// ca), in the E phase that already owns the cell: no new barrier.
//
// The images: the thread that owns an image cell recomputes its source cell's update with its own slots of Jh and Q as
// the old values, as it does for Ez.  By the same induction the image slots of Jh and Q stay bit-identical to their
// source cells (unrotated copies); the host writes them from the source cells wherever it writes the state and rotates
// them on download.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_dispersive.hpp"
#include "kernels_batch_lattice.hpp"

namespace fdtd {

// the pole of a batch with complex fields: Jh, Q (real and imaginary parts) and cj in the fields' padded layout, a and
// ck per member
template <class T> struct BatchBlochDisp {
    T *jh, *q, *jh_i, *q_i;
    const T *cj, *a, *ck;
};

// k_batch_resident_bloch with the pole
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_bloch_dispersive(
    BatchView<T> v, BatchPml<T> p, BatchMon m, BatchBloch<T> bl, BatchBlochDisp<T> d, const T *__restrict__ ca, int n0,
    int nt, long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_bloch_disp_lds[];
    const int R = v.R, C = v.C, L = p.L;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_bloch_disp_lds);
    T *shx = sez + seg, *shy = shx + seg, *sezx = shy + seg;
    T *siz = sezx + seg, *six = siz + seg, *siy = six + seg, *sizx = siy + seg;
    T *scb = sizx + seg, *sch = scb + seg, *sca = sch + seg;
    T *sjh = sca + seg, *sq = sjh + seg, *sjhi = sq + seg, *sqi = sjhi + seg, *scj = sqi + seg;
    T *sfr = sez + 16 * seg;                  // ahr[R], bhr[R], aer[R], ber[R]
    double *sw = reinterpret_cast<double *>(sfr + batch_lds_seg<T>(4 * R));   // wr[C-1], wi[C-1]
    double *stab = sw + 2 * (C - 1);
    double *sacc = stab + 2 * m.nf, *sacci = sacc + 2 * (size_t)m.nf * m.window();
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
            sjh[l] = d.jh[g];
            sq[l] = d.q[g];
            sjhi[l] = d.jh_i[g];
            sqi[l] = d.q_i[g];
            scj[l] = d.cj[g];
        });
        for (int k = tid; k < 4 * R; k += nthr) sfr[k] = p.rowf[(size_t)b * 4 * R + k];
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = bl.w[(size_t)b * 2 * (C - 1) + k];
        const T rc = bl.rho[2 * b], rs = bl.rho[2 * b + 1];
        const T da = d.a[b], dck = d.ck[b];
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = bl.amps && src.r1 > src.r0 ? bl.amps + (size_t)b * v.amp_stride : nullptr;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const BatchMonMember moni = batch_mon_begin(mi, b, sacci, tid, nthr);
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
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step);
            cells([&](int, int i, int j, int l) {
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
                    } else {
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
            d.jh[g] = sjh[l];
            d.q[g] = sq[l];
            d.jh_i[g] = sjhi[l];
            d.q_i[g] = sqi[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        batch_mon_end(mi, b, sacci, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed E of a Bloch batch with the pole, in place, behind k_batch_h_bloch
template <class T>
__global__ __launch_bounds__(256) void k_batch_e_bloch_dispersive(BatchView<T> v, BatchPml<T> p, BatchMon m,
                                                                  BatchBloch<T> bl, BatchBlochDisp<T> d,
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
            } else {
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
    }
}

// k_batch_resident_lattice with the pole
template <class T, int MAXC>
__global__ __launch_bounds__(BATCH_RES_THREADS) void k_batch_resident_lattice_dispersive(
    BatchView<T> v, BatchMon m, BatchLattice<T> la, BatchBlochDisp<T> d, const T *__restrict__ ca, int n0, int nt,
    long long step_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char batch_lattice_disp_lds[];
    const int R = v.R, C = v.C;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const size_t seg = batch_lds_seg<T>(R * C);
    T *sez = reinterpret_cast<T *>(batch_lattice_disp_lds);
    T *shx = sez + seg, *shy = shx + seg;
    T *siz = shy + seg, *six = siz + seg, *siy = six + seg;
    T *scb = siy + seg, *sch = scb + seg, *sca = sch + seg;
    T *sjh = sca + seg, *sq = sjh + seg, *sjhi = sq + seg, *sqi = sjhi + seg, *scj = sqi + seg;
    double *sw = reinterpret_cast<double *>(sez + 14 * seg);  // wr[C-1], wi[C-1]
    double *stab = sw + 2 * (C - 1);
    double *sacc = stab + 2 * m.nf, *sacci = sacc + 2 * (size_t)m.nf * m.window();
    BatchMon mi = m;                          // the monitors of the imaginary part: same window, phasors and cells
    mi.acc = la.acc;
    mi.trace = la.trace;
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
            siz[l] = la.ez[g];
            six[l] = la.hx[g];
            siy[l] = la.hy[g];
            scb[l] = v.ce[g];
            sch[l] = v.ch[g];
            sca[l] = ca[g];
            sjh[l] = d.jh[g];
            sq[l] = d.q[g];
            sjhi[l] = d.jh_i[g];
            sqi[l] = d.q_i[g];
            scj[l] = d.cj[g];
        });
        for (int k = tid; k < 2 * (C - 1); k += nthr) sw[k] = la.w[(size_t)b * 2 * (C - 1) + k];
        const T rrc = la.rho_r[2 * b], rrs = la.rho_r[2 * b + 1];
        const T rcc = la.rho_c[2 * b], rcs = la.rho_c[2 * b + 1];
        const T da = d.a[b], dck = d.ck[b];
        BatchSource<T> src;
        src.load(v, b);
        const double *ampi = la.amps && src.r1 > src.r0 ? la.amps + (size_t)b * v.amp_stride : nullptr;
        const BatchMonMember mon = batch_mon_begin(m, b, sacc, tid, nthr);
        const BatchMonMember moni = batch_mon_begin(mi, b, sacci, tid, nthr);
        __syncthreads();

        for (int s = 0; s < nt; ++s) {
            const long long step = step_base + s + 1;
            cells([&](int, int i, int j, int l) {
                if (i > R - 2 || j > C - 2) return;
                const bool cseam = j == C - 2;            // the right neighbour is the column image: rho_c * column 0
                const bool rseam = i == R - 2;            // the lower neighbour is the row image: rho_r * row 0
                const T kcc = cseam ? rcc : (T)1, kcs = cseam ? rcs : (T)0;
                const T krc = rseam ? rrc : (T)1, krs = rseam ? rrs : (T)0;
                T nr, ni, dr, dq;
                batch_bloch_rot(kcc, kcs, sez[l + 1], siz[l + 1], nr, ni);
                batch_bloch_rot(krc, krs, sez[l + C], siz[l + C], dr, dq);
                const T cc = sch[l];
                const T er = sez[l], ei = siz[l];
                shx[l] = batch_lattice_hx(shx[l], cc, dr - er);
                shy[l] = batch_periodic_plain(shy[l], cc, nr - er);
                six[l] = batch_lattice_hx(six[l], cc, dq - ei);
                siy[l] = batch_periodic_plain(siy[l], cc, ni - ei);
            });
            batch_mon_phasors(m, mon, stab, step, v.dt);
            __syncthreads();
            const double ar = src.r1 > src.r0 ? src.amps[n0 + s] : 0.0;
            const double ai = ampi ? ampi[n0 + s] : 0.0;
            const bool sampled = m.sampled(step);
            cells([&](int, int i, int j, int l) {
                T er = sez[l], ei = siz[l];
                const int ic = i == R - 1 ? 0 : i, jc = j == C - 1 ? 0 : j;    // the cell whose update this is
                const int lc = ic * C + jc;
                const bool cwrap = jc == 0, rwrap = ic == 0;    // its left / upper neighbour is across a seam
                const int lw = cwrap ? lc + (C - 2) : lc - 1;
                const int lu = rwrap ? lc + (R - 2) * C : lc - C;
                const T kcc = cwrap ? rcc : (T)1, kcs = cwrap ? rcs : (T)0;
                const T krc = rwrap ? rrc : (T)1, krs = rwrap ? rrs : (T)0;
                T wr, wi, ur, ui;
                batch_bloch_unrot(kcc, kcs, shy[lw], siy[lw], wr, wi);
                batch_bloch_unrot(krc, krs, shx[lu], six[lu], ur, ui);
                const T cc = scb[lc], a = sca[lc];
                const T dhyr = shy[lc] - wr, dhxr = shx[lc] - ur;
                const T dhyi = siy[lc] - wi, dhxi = six[lc] - ui;
                // Jh and Q at l, never lc: the source cell's thread writes its own in this phase
                const T cj = scj[lc];
                const T jr = batch_disp_j(da, sjh[l], cj, er, dck, sq[l]);
                const T ji = batch_disp_j(da, sjhi[l], cj, ei, dck, sqi[l]);
                sq[l] = sq[l] + jr;
                sqi[l] = sqi[l] + ji;
                er = batch_lossy_e(er, (dhyr - dhxr) - jr, a, cc);
                ei = batch_lossy_e(ei, (dhyi - dhxi) - ji, a, cc);
                sjh[l] = jr;
                sjhi[l] = ji;
                if (src.covers(ic, jc)) {                     // an image takes its source cell's source
                    double dr, dq;
                    batch_bloch_source(ar, ai, sw[jc], sw[C - 1 + jc], dr, dq);
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
            });
            __syncthreads();
            batch_mon_probes(m, mon, b, sez, step);
            batch_mon_probes(mi, moni, b, siz, step);
        }

        cells([&](int, int i, int j, int l) {
            const size_t g = base + (size_t)i * (size_t)v.pitch + (size_t)j;
            v.ez[g] = sez[l];
            la.ez[g] = siz[l];
            d.jh[g] = sjh[l];
            d.q[g] = sq[l];
            d.jh_i[g] = sjhi[l];
            d.q_i[g] = sqi[l];
            if (i > R - 2 || j > C - 2) return;       // row R-1 of Hx and column C-1 of Hy are never written
            v.hx[g] = shx[l];
            v.hy[g] = shy[l];
            la.hx[g] = six[l];
            la.hy[g] = siy[l];
        });
        batch_mon_end(m, b, sacc, tid, nthr);
        batch_mon_end(mi, b, sacci, tid, nthr);
        __syncthreads();   // the next member's loads overwrite LDS
    }
}

// streamed E of a lattice batch with the pole, in place, behind k_batch_h_lattice
template <class T>
__global__ __launch_bounds__(256) void k_batch_e_lattice_dispersive(BatchView<T> v, BatchMon m, BatchLattice<T> la,
                                                                    BatchBlochDisp<T> d, const T *__restrict__ ca,
                                                                    int n, long long step)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= v.R * v.C) return;
    const int R = v.R, C = v.C, i = t / C, j = t % C;
    const int ic = i == R - 1 ? 0 : i, jc = j == C - 1 ? 0 : j;
    const bool cwrap = jc == 0, rwrap = ic == 0;
    BatchMon mi = m;
    mi.acc = la.acc;
    mi.trace = la.trace;
    for (int b = blockIdx.y; b < v.B; b += gridDim.y) {
        const size_t mb = (size_t)b * v.mstride;
        const size_t o = mb + (size_t)i * (size_t)v.pitch + (size_t)j;
        const size_t oc = mb + (size_t)ic * (size_t)v.pitch + (size_t)jc;
        const size_t ow = cwrap ? oc + (size_t)(C - 2) : oc - 1;
        const size_t ou = rwrap ? oc + (size_t)(R - 2) * (size_t)v.pitch : oc - (size_t)v.pitch;
        const T kcc = cwrap ? la.rho_c[2 * b] : (T)1, kcs = cwrap ? la.rho_c[2 * b + 1] : (T)0;
        const T krc = rwrap ? la.rho_r[2 * b] : (T)1, krs = rwrap ? la.rho_r[2 * b + 1] : (T)0;
        T er = v.ez[o], ei = la.ez[o];
        T wr, wi, ur, ui;
        batch_bloch_unrot(kcc, kcs, v.hy[ow], la.hy[ow], wr, wi);
        batch_bloch_unrot(krc, krs, v.hx[ou], la.hx[ou], ur, ui);
        const T cc = v.ce[oc], a = ca[oc];
        const T dhyr = v.hy[oc] - wr, dhxr = v.hx[oc] - ur;
        const T dhyi = la.hy[oc] - wi, dhxi = la.hx[oc] - ui;
        // Jh and Q at o, never oc: the source cell's thread writes its own in this launch
        const T cj = d.cj[oc], da = d.a[b], dck = d.ck[b];
        const T qr = d.q[o], qi = d.q_i[o];
        const T jr = batch_disp_j(da, d.jh[o], cj, er, dck, qr);
        const T ji = batch_disp_j(da, d.jh_i[o], cj, ei, dck, qi);
        d.q[o] = qr + jr;
        d.q_i[o] = qi + ji;
        er = batch_lossy_e(er, (dhyr - dhxr) - jr, a, cc);
        ei = batch_lossy_e(ei, (dhyi - dhxi) - ji, a, cc);
        d.jh[o] = jr;
        d.jh_i[o] = ji;
        BatchSource<T> src;
        src.load(v, b);
        if (src.covers(ic, jc)) {
            const double *w = la.w + (size_t)b * 2 * (C - 1);
            const double ai = la.amps ? la.amps[(size_t)b * v.amp_stride + n] : 0.0;
            double dr, dq;
            batch_bloch_source(src.amps[n], ai, w[jc], w[C - 1 + jc], dr, dq);
            er = (T)((double)er + dr);
            ei = (T)((double)ei + dq);
        }
        v.ez[o] = er;
        la.ez[o] = ei;
        batch_mon_cell(m, b, t, i, j, step, (double)er);
        batch_mon_cell(mi, b, t, i, j, step, (double)ei);
    }
}

// host stubs of the kernels above (batch_bloch_dispersive.hip): 4 cells per thread alone
struct BatchBlochDispersiveKernels {
    const void *resident_bloch, *resident_lattice;
    const void *e_bloch, *e_lattice;
};
template <class T> const BatchBlochDispersiveKernels &batch_bloch_dispersive_kernels();

}  // namespace fdtd
