// Active window of the single-grid engine: host-side bookkeeping of where the fields can be non-zero.
// Plain C++ (no HIP), so that it builds and is tested on the host (tests/test_active_window_cpu.py).
//
// A run from rest touches few cells: one leapfrog step spreads the support of (Ez, Hx, Hy) by one cell in each
// direction, a little faster inside the 5-cell Mur frame.  The engine keeps two rectangles per handle, as half-open
// row and column ranges:
//
//   support      every cell of the CURRENT buffer set (Ez, Hx, Hy) outside it is zero
//   dirty_other  every cell of the OTHER buffer set (the next pass's target) outside it is zero
//
// A committed pass of n steps only has to write  W = grow(support U source, n) U dirty_other:  outside W the new
// state is zero and the target already holds zeros.  (+0 and -0 are not told apart: a cell the dense sweep would
// compute as -0 may stay +0.)
//
// Transitions (the engine calls them at the places named):
//
//   reset()                 both empty                     zero_fields memsets both sets (create ends with it)
//   invalidate()            both full                      upload, transfer_ezx to device, halo_unpack, pass_rows /
//                                                          pass_commit, device_ptr handed out
//   commit_pass(src, n)     support = grow(support U src, n), dirty_other = old support (it becomes the other set)
//   half_step()             support = grow(support, 1); dirty_other = dirty_other U old support
//                                                          the single-step kernels: they stay dense; Ez and H change
//                                                          sets separately there, and an H half-step alone already
//                                                          reaches one cell out, so EACH half-step grows by one
//   add_source(src)         support = support U src        fdtd2d_add_point
//   uncommitted()           dirty_other = full             trial launches of the tuner, warm launches of prepare_run:
//                                                          ping-pong trials leave many-step evolutions behind
//   copied_to_other()       dirty_other = dirty_other U support     fdtd2d_measure_copy copies the current set over
//
// grow(w, n) and its margin.  Away from the frame a cell at step s+1 depends on cells at most one away at step s
// (H from E: Hx[i,j] <- Ez[i+1,j], Hy[i,j] <- Ez[i,j+1]; stage A of mur_rules.hpp: Ez[i,j] <- Hy[i,j-1], Hx[i-1,j]).
// Inside the frame the rules look INWARD only, and further:
//   stage B (columns j < 5):     b(i,j) <- p(i,j+1), a(i,j+1) <- Ez[i,j+2], Ez[i+-1,j+1]          2 columns inward
//   stage C (rows i < 5):        c(i,j) <- p(i+1,j), b(i+1,j) <- Ez[i+2,j], Ez[i+1,j+-1]          2 rows inward,
//                                along the frame (5 <= j < C-5) still one column per step
//   stage D (5 x 5 corners):     d(i,j) <- c(i,j+1), c(i+1,j) <- b(i+1,j+1), b(i+2,j) <- a(i+1,j+2), a(i+2,j+1)
//                                <- Ez up to 3 rows / 3 columns inward, for j + 1 < 5 only; else as stage B / C
// so a frame cell with index j < 5 (counted from its edge) reads at most index min(j + 3, 6): it can turn non-zero in
// one step only if the support comes within index 6 of that edge.  Plain growth has then brought the bound to index
// <= 5.  Hence MARGIN = 6: a side of the grown rectangle that lies fewer than 6 cells from a grid edge snaps to the
// edge.  Growing n steps at once is the same as n single steps: once a bound is below 6 it snaps, and above it nothing
// in the frame is reached.  (The mirror cases at the bottom / right are symmetric.  The host check fails with 5.)
#pragma once
#include <algorithm>

namespace fdtd_aw {

constexpr int MARGIN = 6;

struct Rect {
    int r0 = 0, r1 = 0, c0 = 0, c1 = 0;      // rows [r0, r1), columns [c0, c1)
    bool empty() const { return r0 >= r1 || c0 >= c1; }
    long long cells() const { return empty() ? 0 : (long long)(r1 - r0) * (c1 - c0); }
    bool contains(int i, int j) const { return i >= r0 && i < r1 && j >= c0 && j < c1; }
    bool covers(const Rect &o) const { return o.empty() || (!empty() && o.r0 >= r0 && o.r1 <= r1 && o.c0 >= c0 && o.c1 <= c1); }
};

inline Rect unite(const Rect &a, const Rect &b)
{
    if (a.empty()) return b.empty() ? Rect{} : b;
    if (b.empty()) return a;
    return Rect{std::min(a.r0, b.r0), std::max(a.r1, b.r1), std::min(a.c0, b.c0), std::max(a.c1, b.c1)};
}

// w extended by n cells on every side, clipped to the R x C grid; a side closer than MARGIN to the edge snaps to it
inline Rect grow(const Rect &w, int n, int R, int C)
{
    if (w.empty()) return Rect{};
    auto lo = [](int v, int n_) { const int x = v - n_; return x < MARGIN ? 0 : x; };
    auto hi = [](int v, int n_, int N) { const long long x = (long long)v + n_; return x > N - MARGIN ? N : (int)x; };
    return Rect{lo(w.r0, n), hi(w.r1, n, R), lo(w.c0, n), hi(w.c1, n, C)};
}

struct ActiveWindow {
    int R = 0, C = 0;
    bool tracking = false;       // false: both rectangles stay full (slabs, PML engines)
    Rect support, dirty_other;

    Rect full() const { return Rect{0, R, 0, C}; }
    void init(int rows, int cols, bool track)
    {
        R = rows;
        C = cols;
        tracking = track;
        support = dirty_other = full();
    }
    void reset()
    {
        if (tracking) support = dirty_other = Rect{};
    }
    void invalidate() { support = dirty_other = full(); }
    void uncommitted() { dirty_other = full(); }
    void copied_to_other() { dirty_other = unite(dirty_other, support); }
    void add_source(const Rect &src) { support = unite(support, clip(src)); }
    void half_step()
    {
        const Rect old = support;
        support = grow(old, 1, R, C);
        dirty_other = unite(dirty_other, old);
    }
    void commit_pass(const Rect &src, int nsteps)
    {
        const Rect old = support;
        support = grow(unite(old, clip(src)), nsteps, R, C);
        dirty_other = old;
    }
    // what a committed pass of nsteps steps has to write
    Rect window(const Rect &src, int nsteps) const
    {
        return unite(grow(unite(support, clip(src)), nsteps, R, C), dirty_other);
    }
    Rect clip(const Rect &s) const
    {
        if (s.empty()) return Rect{};
        return Rect{std::max(s.r0, 0), std::min(s.r1, R), std::max(s.c0, 0), std::min(s.c1, C)};
    }
};

// Strips and rows of a restricted launch.  The pass cuts the columns into strips that WRITE [s OW, (s + 1) OW)
// (strip 0 and the last one are the edge strips; the last one is shifted left to end at the grid's edge) and the rows
// [lo, hi) between the top / bottom zones of depth zo into bands; a band reads nt rows beyond its own.
// Strip s of a pass writes columns [s ow, (s + 1) ow) and loads hc more on either side: does it HOLD columns of
// [c0, c1)?  The one definition shared by restrict_launch below (in closed form), by the launch order of
// launch_pass_impl (strips that hold source columns get bands of their own) and by the host check.
inline bool strip_holds(int s, int ow, int hc, int c0, int c1)
{
    return c1 + hc > s * ow && c0 - hc < (s + 1) * ow;
}

struct Launch {
    int band_lo = 0, band_hi = 0;    // rows of the bulk
    bool ztop = false, zbot = false; // zone tiles (all columns) of that side
    int strip_first = 1, n_inner = 0;
    bool edges = false;              // both edge strips
};

// w: the window (non-empty); src: the source rectangle, whose columns the launched strips must hold (empty: no source);
// ow: columns a strip writes; hc: its overlap per side.  [lo, hi): pass_geometry's bulk rows of the whole grid (lo = zo, hi = R - zo).
inline Launch restrict_launch(const Rect &w, const Rect &src, int R, int C, int nt, int lo, int hi, int ow, int hc, int nstrips)
{
    Launch L;
    const int zo = lo;
    // rows: within zone depth + pass length of the top / bottom the side snaps to the edge and takes its zone tiles
    L.ztop = w.r0 < zo + nt;
    L.zbot = w.r1 > R - zo - nt;
    L.band_lo = L.ztop ? lo : std::min(w.r0, hi);
    L.band_hi = L.zbot ? hi : std::max(w.r1, lo);
    L.band_hi = std::max(L.band_hi, L.band_lo);
    // columns: the strips whose written columns meet the window -- or hold source columns (they get bands of their own
    // in the launch order, which counts them among the inner run).  Widening the run by hc on either side of the source
    // is strip_holds() in closed form: s holds [c0, c1) iff (c0 - hc) / ow <= s <= (c1 + hc - 1) / ow.
    int c0 = w.c0, c1 = w.c1;
    if (!src.empty()) {
        c0 = std::min(c0, src.c0 - hc);
        c1 = std::max(c1, src.c1 + hc);
    }
    c0 = std::max(c0, 0);
    c1 = std::min(c1, C);
    if (nstrips <= 2) {
        L.edges = true;
        L.strip_first = 1;
        L.n_inner = 0;
        return L;
    }
    // the first strip, the last one, and the strip beside the left-shifted last one
    L.edges = c0 < ow || c1 > (nstrips - 2) * ow;
    const int sa = std::max(1, c0 / ow), sb = std::min(nstrips - 2, (c1 - 1) / ow);
    L.strip_first = sa;
    L.n_inner = std::max(0, sb - sa + 1);
    if (L.n_inner == 0) L.strip_first = 1;
    return L;
}

}  // namespace fdtd_aw
