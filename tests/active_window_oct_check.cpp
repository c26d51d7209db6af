// Host check of the diagonal bounds in csrc/active_window.hpp (built and run by tests/test_active_window_oct_cpu.py
// with the address and undefined-behaviour sanitizers), in the manner of tests/active_window_check.cpp.
//
// Boolean "may be non-zero" maps of the two buffer sets are propagated with the exact dependency pattern of a leapfrog
// step -- H from E, stages A-D of mur_rules.hpp, the source -- and after EVERY transition every non-zero cell of the
// current set must lie inside `support` AND inside `support_oct`, every non-zero cell of the other set inside
// `dirty_other` and `dirty_oct`.  A committed pass writes only the cells inside window() and window_oct(): everywhere
// else the new state must be zero and the target must hold zeros already (per cell, which is stricter than the per-task
// test of strip_of_block).  As soon as a cell of the 5-cell frame is non-zero the bounds of that set must be unbounded,
// and the pass in which the first one turns non-zero must already have run without bounds.
//
// Cases: point, patch and line sources (the bounds touched to within the one cell by which commit_pass over-grows a
// source, and exactly after add_point); two sources in turn; half-steps; add_point; a copy and an uncommitted launch;
// supports approaching each of the four edges in passes of 1, 2 and 3 steps; random sequences.
// argv[3] = 1 checks against a copy of the bounds TIGHTENED by one cell instead: the program must then fail.
#include "../fdtd-2d_amd/csrc/active_window.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using fdtd_aw::Oct;
using fdtd_aw::Rect;
typedef std::vector<unsigned char> Map;

static int R, C;
static int failures = 0;
static int tighten = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (failures++ < 20) {                         \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

// the bounds under test: the header's, or (the mutation) each bounded side moved inward by one
static Oct used(const Oct &o)
{
    if (!tighten || o.empty()) return o;
    Oct t = o;
    if (t.s0 > -Oct::BIG) t.s0 += 1;
    if (t.s1 < Oct::BIG) t.s1 -= 1;
    if (t.d0 > -Oct::BIG) t.d0 += 1;
    if (t.d1 < Oct::BIG) t.d1 -= 1;
    return t;
}

struct Fields {
    Map ez, hx, hy;
    void fill(unsigned char v)
    {
        ez.assign((size_t)R * C, v);
        hx.assign((size_t)R * C, v);
        hy.assign((size_t)R * C, v);
    }
};

static inline bool at(const Map &m, int i, int j) { return m[(size_t)i * C + j] != 0; }

// Ez after the E half-step as a function of P (Ez before) and the updated H: mur_rules.hpp with "is non-zero" for values
struct Rules {
    const Map &P, &X, &Y;
    bool p(int i, int j) const { return at(P, i, j); }
    bool a(int i, int j) const
    {
        const bool e = p(i, j);
        if (i < 1 || i > R - 2 || j < 1 || j > C - 2) return e;
        return e || at(Y, i, j) || at(Y, i, j - 1) || at(X, i, j) || at(X, i - 1, j);
    }
    bool b(int i, int j) const
    {
        if (i >= 1 && i <= R - 2) {
            if (j < 5) return p(i, j + 1) || a(i, j + 1) || p(i, j);
            if (j >= C - 5) return p(i, j - 1) || a(i, j - 1) || p(i, j);
        }
        return a(i, j);
    }
    bool c(int i, int j) const
    {
        if (j >= 1 && j <= C - 2) {
            if (i < 5) return p(i + 1, j) || b(i + 1, j) || p(i, j);
            if (i >= R - 5) return p(i - 1, j) || b(i - 1, j) || p(i, j);
        }
        return b(i, j);
    }
    bool d(int i, int j) const
    {
        const bool top = i < 5, bot = i >= R - 5, lef = j < 5, rig = j >= C - 5;
        if (top && lef) return c(i, j + 1) || c(i + 1, j);
        if (top && rig) return c(i, j - 1) || c(i + 1, j);
        if (bot && lef) return c(i - 1, j) || c(i, j + 1);
        if (bot && rig) return c(i - 1, j) || c(i, j - 1);
        return c(i, j);
    }
};

static void step_h(const Map &ez, Map &hx, Map &hy)
{
    for (int i = 0; i <= R - 2; ++i)
        for (int j = 0; j <= C - 2; ++j) {
            const size_t o = (size_t)i * C + j;
            hx[o] = hx[o] || at(ez, i, j) || at(ez, i + 1, j);
            hy[o] = hy[o] || at(ez, i, j) || at(ez, i, j + 1);
        }
}

static void step_e(const Map &ez, const Map &hx, const Map &hy, Map &out)
{
    const Rules r{ez, hx, hy};
    out.assign((size_t)R * C, 0);
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < C; ++j) out[(size_t)i * C + j] = r.d(i, j);
}

static void add_src(Map &ez, const Rect &s)
{
    for (int i = s.r0; i < s.r1; ++i)
        for (int j = s.c0; j < s.c1; ++j) ez[(size_t)i * C + j] = 1;
}

static bool in_frame(int i, int j) { return i < 5 || i >= R - 5 || j < 5 || j >= C - 5; }

struct Sim {
    Fields set[2];
    int cur = 0, hcur = 0;
    fdtd_aw::ActiveWindow aw;

    void start()
    {
        set[0].fill(0);
        set[1].fill(0);
        cur = hcur = 0;
        aw.init(R, C, true);
        aw.reset();
    }

    void inside(const Map &m, const Rect &w, const Oct &o, const char *what, const char *name)
    {
        const Oct t = used(o);
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < C; ++j)
                if (at(m, i, j) && !(w.contains(i, j) && t.contains(i, j))) {
                    CHECK(false, "%s: %s (%d,%d) outside [%d,%d)x[%d,%d) / sum [%d,%d] diff [%d,%d]", what, name, i, j, w.r0, w.r1,
                          w.c0, w.c1, t.s0, t.s1, t.d0, t.d1);
                    return;
                }
    }

    void check(const char *what)
    {
        inside(set[cur].ez, aw.support, aw.support_oct, what, "Ez");
        inside(set[hcur].hx, aw.support, aw.support_oct, what, "Hx");
        inside(set[hcur].hy, aw.support, aw.support_oct, what, "Hy");
        inside(set[cur ^ 1].ez, aw.dirty_other, aw.dirty_oct, what, "other Ez");
        inside(set[hcur ^ 1].hx, aw.dirty_other, aw.dirty_oct, what, "other Hx");
        inside(set[hcur ^ 1].hy, aw.dirty_other, aw.dirty_oct, what, "other Hy");
        // the frame: a non-zero cell there and the bounds are gone
        if (frame_lit()) CHECK(!aw.support_oct.bounded(), "%s: a frame cell is non-zero and the bounds still stand", what);
    }
    bool frame_lit() const
    {
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < C; ++j)
                if (in_frame(i, j) && (at(set[cur].ez, i, j) || at(set[hcur].hx, i, j) || at(set[hcur].hy, i, j))) return true;
        return false;
    }

    // the bounds are TOUCHED: some non-zero cell of the current set lies on each bounded side, or `slack` cells inside it
    // (1 for the source of a run: commit_pass grows it by n, and its first injection has spread n - 1 cells by then)
    void check_touched(const char *what, int slack)
    {
        const Oct &o = aw.support_oct;
        if (!o.bounded() || o.empty()) return;
        int s0 = 1 << 30, s1 = -(1 << 30), d0 = 1 << 30, d1 = -(1 << 30);
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < C; ++j)
                if (at(set[cur].ez, i, j) || at(set[hcur].hx, i, j) || at(set[hcur].hy, i, j)) {
                    s0 = std::min(s0, i + j), s1 = std::max(s1, i + j);
                    d0 = std::min(d0, i - j), d1 = std::max(d1, i - j);
                }
        CHECK(s0 >= o.s0 && s0 <= o.s0 + slack && s1 <= o.s1 && s1 >= o.s1 - slack && d0 >= o.d0 && d0 <= o.d0 + slack && d1 <= o.d1 &&
                  d1 >= o.d1 - slack,
              "%s: maps span sum [%d,%d] diff [%d,%d], bounds [%d,%d] [%d,%d]", what,
              s0, s1, d0, d1, o.s0, o.s1, o.d0, o.d1);
    }

    // a committed pass of n steps that writes only the cells inside the window's rectangle and diagonal bounds
    void pass(const Rect &src, int n, bool dense = false)
    {
        const Rect W = aw.window(src, n);
        const Oct O = used(aw.window_oct(src, n));
        const bool lit_before = frame_lit();
        Map ez = set[cur].ez, hx = set[hcur].hx, hy = set[hcur].hy, tmp;
        for (int s = 0; s < n; ++s) {
            step_h(ez, hx, hy);
            step_e(ez, hx, hy, tmp);
            ez.swap(tmp);
            if (!src.empty()) add_src(ez, src);
        }
        Fields &te = set[cur ^ 1], &th = set[hcur ^ 1];
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < C; ++j) {
                const size_t o = (size_t)i * C + j;
                if (dense || (W.contains(i, j) && O.contains(i, j))) {
                    te.ez[o] = ez[o], th.hx[o] = hx[o], th.hy[o] = hy[o];
                } else {
                    CHECK(!ez[o] && !hx[o] && !hy[o], "pass of %d: new state (%d,%d) outside the octagon", n, i, j);
                    CHECK(!te.ez[o] && !th.hx[o] && !th.hy[o], "pass of %d: target holds (%d,%d) outside the octagon", n, i, j);
                }
            }
        cur ^= 1;
        hcur ^= 1;
        aw.commit_pass(src, n);
        check("pass");
        // the pass in which the first frame cell turns non-zero already runs without bounds
        if (!lit_before && frame_lit()) CHECK(!O.bounded(), "pass of %d: a frame cell turned non-zero in a pass that still had bounds", n);
    }
    void half_h()
    {
        step_h(set[cur].ez, set[hcur].hx, set[hcur].hy);
        aw.half_step();
        check("update_h");
    }
    void half_e()
    {
        step_e(set[cur].ez, set[hcur].hx, set[hcur].hy, set[cur ^ 1].ez);
        cur ^= 1;
        aw.half_step();
        check("update_e");
    }
    void point(const Rect &src)
    {
        add_src(set[cur].ez, src);
        aw.add_source(src);
        check("add_point");
    }
    void trial()
    {
        set[cur ^ 1].ez.assign((size_t)R * C, 1);
        set[hcur ^ 1].hx.assign((size_t)R * C, 1);
        set[hcur ^ 1].hy.assign((size_t)R * C, 1);
        aw.uncommitted();
        check("uncommitted");
    }
    void copy()
    {
        set[cur ^ 1].ez = set[cur].ez;
        set[hcur ^ 1].hx = set[hcur].hx;
        set[hcur ^ 1].hy = set[hcur].hy;
        aw.copied_to_other();
        check("copy");
    }
};

static void fixed_cases()
{
    R = 120, C = 140;
    const Rect pt{60, 61, 70, 71}, patch{55, 58, 60, 65}, hline{60, 61, 50, 90}, vline{40, 80, 70, 71};
    for (const Rect &src : {pt, patch, hline, vline}) {
        Sim s;
        s.start();
        s.pass(src, 16);
        s.check_touched("source, 16 steps", 1);
        CHECK(s.aw.support_oct.bounded(), "an interior source must leave bounds");
        const Oct o = s.aw.support_oct, q = Oct::of(src);
        CHECK(o.s0 == q.s0 - 16 && o.s1 == q.s1 + 16 && o.d0 == q.d0 - 16 && o.d1 == q.d1 + 16, "bounds of a source after 16 steps");
        s.pass(src, 8);
        s.pass(Rect{}, 4);
        s.check_touched("source, 28 steps", 1);
        // the corners of the rectangle are outside: that is what the octagon is for
        CHECK(!s.aw.support_oct.contains(s.aw.support.r0, s.aw.support.c0), "the rectangle's corner lies inside the bounds");
    }
    {   // two sources in turn: the hull
        Sim s;
        s.start();
        s.pass(Rect{30, 31, 40, 41}, 8);
        s.pass(Rect{80, 81, 100, 101}, 8);
        s.check_touched("two sources", 1);
        const Oct o = s.aw.support_oct;
        CHECK(o.s0 == 70 - 16 && o.s1 == 180 + 8 && o.d0 == -20 - 8 && o.d1 == -10 + 16, "hull of two sources: sum [%d,%d] diff [%d,%d]", o.s0,
              o.s1, o.d0, o.d1);
        s.pass(Rect{}, 16);
        s.check_touched("two sources, 16 more", 1);
    }
    {   // half-steps and add_point
        Sim s;
        s.start();
        s.point(pt);
        CHECK(s.aw.support_oct.s0 == 130 && s.aw.support_oct.s1 == 130 && s.aw.support_oct.d0 == -10 && s.aw.support_oct.d1 == -10, "add_point");
        for (int k = 0; k < 6; ++k) {
            s.half_h();
            s.half_e();
        }
        CHECK(s.aw.support_oct.s1 == 130 + 12 && s.aw.support_oct.d0 == -10 - 12, "each half-step grows the bounds by one");
        s.point(Rect{70, 71, 90, 91});
        s.pass(Rect{}, 8);
        s.pass(pt, 8);
    }
    {   // a point, then passes without a source: the bounds are exact (this is where a bound tightened by one fails)
        Sim s;
        s.start();
        s.point(pt);
        s.pass(Rect{}, 4);
        s.pass(Rect{}, 8);
        s.check_touched("a point, then passes without a source", 0);
        CHECK(s.aw.support_oct.s0 == 130 - 12 && s.aw.support_oct.d1 == -10 + 12, "a point after 12 steps");
    }
    {   // a copy, then an uncommitted launch: unbounded afterwards, and the committed passes start again from the rectangle
        Sim s;
        s.start();
        s.pass(pt, 8);
        s.pass(pt, 8);
        CHECK(s.aw.window_oct(pt, 8).bounded(), "two committed passes: bounded");
        s.copy();
        CHECK(!s.aw.dirty_oct.bounded() && !s.aw.window_oct(pt, 8).bounded() && s.aw.support_oct.bounded(), "a copy: the target unbounded");
        s.pass(pt, 8);
        CHECK(s.aw.window_oct(pt, 8).bounded(), "the pass after a copy: bounded again");
        s.trial();
        CHECK(!s.aw.dirty_oct.bounded() && !s.aw.window_oct(pt, 8).bounded(), "an uncommitted launch: the target is unknown");
        CHECK(s.aw.support_oct.bounded(), "... the current set is not");
        s.pass(pt, 8);          // writes its whole window
        CHECK(s.aw.dirty_oct.bounded() && s.aw.window_oct(pt, 8).bounded(), "the pass after: bounded again");
        s.pass(pt, 8);
        s.check_touched("after a trial", 1);
        s.aw.invalidate();
        CHECK(!s.aw.support_oct.bounded() && !s.aw.window_oct(pt, 8).bounded(), "invalidate: unbounded");
        s.aw.reset();
        CHECK(s.aw.support_oct.empty() && s.aw.dirty_oct.empty(), "reset: empty");
    }
    // supports approaching each of the four edges, step by step: check() asserts that the bounds are dropped no later
    // than the step before a frame cell turns non-zero
    const Rect near[4] = {Rect{14, 15, 70, 71}, Rect{R - 15, R - 14, 70, 71}, Rect{60, 61, 14, 15}, Rect{60, 61, C - 15, C - 14}};
    for (int e = 0; e < 4; ++e)
        for (int len : {1, 2, 3}) {
            Sim s;
            s.start();
            bool ever = false;
            for (int k = 0; k < 24; k += len) {
                s.pass(k < 6 ? near[e] : Rect{}, len);
                ever = ever || s.aw.support_oct.bounded();
            }
            CHECK(ever && !s.aw.support_oct.bounded(), "edge %d: bounds first, none at the frame", e);
            s.pass(near[(e + 2) % 4], 4);
            CHECK(!s.aw.support_oct.bounded(), "edge %d: the bounds do not come back", e);
        }
    {   // a source inside the margin never has bounds
        Sim s;
        s.start();
        s.point(Rect{3, 4, 70, 71});
        CHECK(!s.aw.support_oct.bounded(), "a source within MARGIN of an edge");
        s.pass(Rect{}, 4);
    }
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int sequences = argc > 2 ? std::atoi(argv[2]) : 200;
    tighten = argc > 3 ? std::atoi(argv[3]) : 0;
    fixed_cases();
    std::mt19937 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const int grids[][2] = {{70, 110}, {96, 96}, {83, 61}, {130, 80}};
    const int lens[] = {1, 2, 4, 8, 16, 20};
    long long events = 0;
    for (int q = 0; q < sequences; ++q) {
        R = grids[q % 4][0];
        C = grids[q % 4][1];
        Sim s;
        s.start();
        auto source = [&]() {       // mostly interior (the bounds live there), sometimes anywhere
            const int h = rnd(0, 3) ? 1 : rnd(1, 6), w = rnd(0, 3) ? 1 : rnd(1, 9);
            const int m = rnd(0, 5) ? 25 : 0;
            const int r = rnd(m, R - h - m), c = rnd(m, C - w - m);
            return Rect{r, r + h, c, c + w};
        };
        const int nev = rnd(3, 9);
        for (int e = 0; e < nev; ++e, ++events) {
            const int ev = rnd(0, 99);
            if (ev < 55) {
                s.pass(rnd(0, 3) ? source() : Rect{}, lens[rnd(0, rnd(0, 2) ? 3 : 5)], rnd(0, 5) == 0);
            } else if (ev < 63) {
                s.half_h();
            } else if (ev < 71) {
                s.half_e();
            } else if (ev < 80) {
                s.point(source());
            } else if (ev < 86) {
                s.trial();
            } else if (ev < 92) {
                s.copy();
            } else if (ev < 95) {
                s.set[s.cur].ez.assign((size_t)R * C, 1);
                s.set[s.hcur].hx.assign((size_t)R * C, 1);
                s.set[s.hcur].hy.assign((size_t)R * C, 1);
                s.aw.invalidate();
                s.check("upload");
            } else {
                s.set[0].fill(0);
                s.set[1].fill(0);
                s.cur = s.hcur = 0;
                s.aw.reset();
                s.check("reset");
            }
        }
    }
    std::printf("%lld events, %d failures\n", events, failures);
    return failures ? 1 : 0;
}
