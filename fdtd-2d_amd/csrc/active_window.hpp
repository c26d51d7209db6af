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

// Diagonal bounds beside a rectangle: every cell (i, j) of the set has  s0 <= i + j <= s1  and  d0 <= i - j <= d1
// (closed).  Rectangle and bounds together are an octagon.
//
// Why they hold.  Away from the frame, ONE leapfrog step moves the joint support of (Ez, Hx, Hy) by at most one cell
// in L1 distance, not merely one cell per axis:
//   Hx'[i,j] <- Hx[i,j], Ez[i+1,j], Ez[i,j]          Hy'[i,j] <- Hy[i,j], Ez[i,j+1], Ez[i,j]
//   Ez'[i,j] <- Ez[i,j], Hy'[i,j], Hy'[i,j-1], Hx'[i,j], Hx'[i-1,j]
//            <- Ez, Hx, Hy at (i,j), Ez[i,j+1], Ez[i+1,j], Hy[i,j-1], Ez[i,j-1], Hx[i-1,j], Ez[i-1,j]
// every cell read differs from (i, j) in ONE index by one.  (The new H rows read by Ez' never reach a diagonal
// neighbour: Hy'[i,j-1] reads Ez[i,j], not Ez[i,j-2] or Ez[i+1,j-1].)  So i + j and i - j each move by at most one per
// step, and by at most one per half-step of the single-step kernels.  The support of a source rectangle after n steps
// is the rectangle grown by n with its corners cut at 45 degrees: about half of a point source's window holds zeros.
//
// Where they hold.  The argument is the interior stencil's.  The frame rules of mur_rules.hpp read up to 3 cells
// inward, diagonally too (stage D), so the bounds are kept only while no frame rule can have had a non-zero input:
// while the rectangle they stand beside has no side within MARGIN of a grid edge (a snapped side lies at distance 0).
// By the derivation above a frame cell turns non-zero only in a step whose grown rectangle snaps, and then the bounds
// of that same grown rectangle are already dropped.  Dropped means unbounded, and `support` never gets them back
// before reset(): its sides only ever move outward.
//
// Transitions, beside the rectangles' table above:
//   reset                 empty                            invalidate, uncommitted     unbounded
//   add_source, unite     hull: min / max of each bound    commit_pass(src, n)         hull with the source, then -+ n
//   half_step             -+ 1                             copied_to_other             dirty_other: unbounded
//   dirty_other           takes the old support's bounds on commit_pass, their hull with its own on half_step
struct Oct {
    static constexpr int BIG = 1 << 29;
    int s0 = BIG, s1 = -BIG, d0 = BIG, d1 = -BIG;        // default: empty
    static Oct unbounded() { return Oct{-BIG, BIG, -BIG, BIG}; }
    static Oct of(const Rect &r)
    {
        if (r.empty()) return Oct{};
        return Oct{r.r0 + r.c0, r.r1 - 1 + r.c1 - 1, r.r0 - (r.c1 - 1), r.r1 - 1 - r.c0};
    }
    bool empty() const { return s0 > s1 || d0 > d1; }
    bool bounded() const { return s0 > -BIG || s1 < BIG || d0 > -BIG || d1 < BIG; }
    bool contains(int i, int j) const { return i + j >= s0 && i + j <= s1 && i - j >= d0 && i - j <= d1; }
    // does the rectangle of cells [ra, rb) x [ca, cb) (non-empty) meet the four half-planes?  The test of strip_of_block.
    bool meets(int ra, int rb, int ca, int cb) const
    {
        return rb - 1 + cb - 1 >= s0 && ra + ca <= s1 && rb - 1 - ca >= d0 && ra - (cb - 1) <= d1;
    }
};

inline Oct hull(const Oct &a, const Oct &b)
{
    return Oct{std::min(a.s0, b.s0), std::max(a.s1, b.s1), std::min(a.d0, b.d0), std::max(a.d1, b.d1)};
}

inline Oct grow(const Oct &o, int n)
{
    if (o.empty()) return o;
    auto lo = [&](int v) { return v <= -Oct::BIG ? -Oct::BIG : std::max(v - n, -Oct::BIG); };
    auto hi = [&](int v) { return v >= Oct::BIG ? Oct::BIG : std::min(v + n, Oct::BIG); };
    return Oct{lo(o.s0), hi(o.s1), lo(o.d0), hi(o.d1)};
}

struct ActiveWindow {
    int R = 0, C = 0;
    bool tracking = false;       // false: both rectangles stay full (slabs, PML engines)
    Rect support, dirty_other;
    Oct support_oct = Oct::unbounded(), dirty_oct = Oct::unbounded();      // diagonal bounds of the two rectangles
    bool oct_lost = true;        // a side of `support` has come within MARGIN of an edge since reset(): unbounded from then on

    Rect full() const { return Rect{0, R, 0, C}; }
    // a rectangle beside which diagonal bounds may stand
    bool clear_of_frame(const Rect &r) const
    {
        return r.empty() || (r.r0 >= MARGIN && r.r1 <= R - MARGIN && r.c0 >= MARGIN && r.c1 <= C - MARGIN);
    }
    void check_oct()
    {
        if (!clear_of_frame(support)) oct_lost = true;
        if (oct_lost) support_oct = Oct::unbounded();
        if (!clear_of_frame(dirty_other)) dirty_oct = Oct::unbounded();
    }
    void init(int rows, int cols, bool track)
    {
        R = rows;
        C = cols;
        tracking = track;
        support = dirty_other = full();
        support_oct = dirty_oct = Oct::unbounded();
        oct_lost = true;
    }
    void reset()
    {
        if (!tracking) return;
        support = dirty_other = Rect{};
        support_oct = dirty_oct = Oct{};
        oct_lost = false;
    }
    void invalidate()
    {
        support = dirty_other = full();
        support_oct = dirty_oct = Oct::unbounded();
        oct_lost = true;
    }
    void uncommitted()
    {
        dirty_other = full();
        dirty_oct = Oct::unbounded();
    }
    void copied_to_other()
    {
        dirty_other = unite(dirty_other, support);
        dirty_oct = Oct::unbounded();     // (a measuring tool's copy: the next pass writes its whole rectangle)
    }
    void add_source(const Rect &src)
    {
        support = unite(support, clip(src));
        support_oct = hull(support_oct, Oct::of(clip(src)));
        check_oct();
    }
    void half_step()
    {
        const Rect old = support;
        const Oct old_oct = support_oct;
        support = grow(old, 1, R, C);
        support_oct = grow(old_oct, 1);
        dirty_other = unite(dirty_other, old);
        dirty_oct = hull(dirty_oct, old_oct);
        check_oct();
    }
    void commit_pass(const Rect &src, int nsteps)
    {
        const Rect old = support;
        const Oct old_oct = support_oct;
        support = grow(unite(old, clip(src)), nsteps, R, C);
        support_oct = grow(hull(old_oct, Oct::of(clip(src))), nsteps);
        dirty_other = old;
        dirty_oct = old_oct;
        check_oct();
    }
    // what a committed pass of nsteps steps has to write
    Rect window(const Rect &src, int nsteps) const
    {
        return unite(grow(unite(support, clip(src)), nsteps, R, C), dirty_other);
    }
    // ... and the diagonal bounds of that: the hull of the grown support's and dirty_other's.  Cells of window() outside
    // them are zero in the new state and zero in the target already.
    Oct window_oct(const Rect &src, int nsteps) const
    {
        const Rect grown = grow(unite(support, clip(src)), nsteps, R, C);
        if (oct_lost || !clear_of_frame(grown) || !clear_of_frame(dirty_other)) return Oct::unbounded();
        return hull(grow(hull(support_oct, Oct::of(clip(src))), nsteps), dirty_oct);
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
    Oct oct = Oct::unbounded();      // diagonal bounds of the window (the caller's, from window_oct): tasks outside do nothing
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
