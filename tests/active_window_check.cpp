// Host check of csrc/active_window.hpp (built and run by tests/test_active_window_cpu.py with the address and
// undefined-behaviour sanitizers).  It propagates boolean "may be non-zero" maps of the two buffer sets through random
// event sequences with the exact dependency pattern of one leapfrog step -- H from E, then stages A-D of mur_rules.hpp,
// then the source -- and asserts after every event that the current set's map lies inside `support` and the other set's
// inside `dirty_other`; for every committed pass also that writing only the window would have been enough, and that the
// rows and strips restrict_launch picks cover the window.
#include "../fdtd-2d_amd/csrc/active_window.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using fdtd_aw::Rect;
typedef std::vector<unsigned char> Map;

static int R, C;
static int failures = 0;

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

// H half-step in place: rows 0 .. R-2, columns 0 .. C-2
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

static bool inside(const Map &m, const Rect &w, int *bi, int *bj)
{
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < C; ++j)
            if (at(m, i, j) && !w.contains(i, j)) {
                *bi = i, *bj = j;
                return false;
            }
    return true;
}

struct Sim {
    Fields set[2];
    int cur = 0, hcur = 0;      // Ez and H change sets separately on the single-step path
    fdtd_aw::ActiveWindow aw;

    void check(const char *what)
    {
        int i = 0, j = 0;
        const Rect &s = aw.support, &o = aw.dirty_other;
        CHECK(inside(set[cur].ez, s, &i, &j), "%s: Ez (%d,%d) outside support [%d,%d)x[%d,%d)", what, i, j, s.r0, s.r1, s.c0, s.c1);
        CHECK(inside(set[hcur].hx, s, &i, &j), "%s: Hx (%d,%d) outside support [%d,%d)x[%d,%d)", what, i, j, s.r0, s.r1, s.c0, s.c1);
        CHECK(inside(set[hcur].hy, s, &i, &j), "%s: Hy (%d,%d) outside support [%d,%d)x[%d,%d)", what, i, j, s.r0, s.r1, s.c0, s.c1);
        CHECK(inside(set[cur ^ 1].ez, o, &i, &j), "%s: other Ez (%d,%d) outside dirty_other [%d,%d)x[%d,%d)", what, i, j, o.r0, o.r1, o.c0, o.c1);
        CHECK(inside(set[hcur ^ 1].hx, o, &i, &j), "%s: other Hx (%d,%d) outside dirty_other [%d,%d)x[%d,%d)", what, i, j, o.r0, o.r1, o.c0, o.c1);
        CHECK(inside(set[hcur ^ 1].hy, o, &i, &j), "%s: other Hy (%d,%d) outside dirty_other [%d,%d)x[%d,%d)", what, i, j, o.r0, o.r1, o.c0, o.c1);
    }

    // a committed pass of n steps that writes only the window: the target keeps what it held elsewhere
    void pass(const Rect &src, int n, bool dense)
    {
        const Rect W = aw.window(src, n);
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
                if (dense || W.contains(i, j)) {
                    te.ez[o] = ez[o], th.hx[o] = hx[o], th.hy[o] = hy[o];
                } else {
                    CHECK(!ez[o] && !hx[o] && !hy[o], "pass of %d: new state (%d,%d) outside the window", n, i, j);
                    CHECK(!te.ez[o] && !th.hx[o] && !th.hy[o], "pass of %d: target holds (%d,%d) outside the window", n, i, j);
                }
            }
        cur ^= 1;
        hcur ^= 1;
        aw.commit_pass(src, n);
    }
};

// restrict_launch: what the chosen bands, zones and strips write covers the window; bands away from a zone stay clear
// of the frame; the strips that hold source columns are among those launched
static void check_launch(const Rect &W, const Rect &src, int nt, int ow, int hc)
{
    if (W.empty()) return;
    const int zo = 5 + nt, lo = zo, hi = R - zo;
    if (hi - lo < 1) return;
    const int ns = (C + ow - 1) / ow;
    const fdtd_aw::Launch L = fdtd_aw::restrict_launch(W, src, R, C, nt, lo, hi, ow, hc, ns);
    CHECK(L.band_lo >= lo && L.band_hi <= hi && L.band_lo <= L.band_hi, "bands [%d,%d) outside [%d,%d)", L.band_lo, L.band_hi, lo, hi);
    CHECK(L.ztop || L.band_lo - nt >= zo, "band at %d without the top zone reads into it", L.band_lo);
    CHECK(L.zbot || L.band_hi + nt <= R - zo, "band to %d without the bottom zone reads into it", L.band_hi);
    CHECK(L.n_inner == 0 || (L.strip_first >= 1 && L.strip_first + L.n_inner <= ns - 1), "inner strips [%d,+%d) of %d", L.strip_first, L.n_inner, ns);
    auto strip_on = [&](int s) { return (s == 0 || s == ns - 1) ? L.edges : (s >= L.strip_first && s < L.strip_first + L.n_inner); };
    for (int i = W.r0; i < W.r1; ++i) {
        const bool zone = (i < zo && L.ztop) || (i >= R - zo && L.zbot);
        const bool band = i >= L.band_lo && i < L.band_hi;
        CHECK(zone || band, "window row %d not written (bands [%d,%d), zones %d %d)", i, L.band_lo, L.band_hi, L.ztop, L.zbot);
        if (zone) continue;
        for (int j = W.c0; j < W.c1; ++j)
            CHECK(strip_on(std::min(j / ow, ns - 1)), "window column %d: strip %d of %d not launched", j, j / ow, ns);
    }
    if (!src.empty())
        for (int s = 1; s <= ns - 2; ++s) {
            if (fdtd_aw::strip_holds(s, ow, hc, src.c0, src.c1)) CHECK(strip_on(s), "strip %d holds source columns but is not launched", s);
        }
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int sequences = argc > 2 ? std::atoi(argv[2]) : 300;
    std::mt19937 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const int grids[][2] = {{48, 80}, {64, 64}, {53, 41}, {110, 60}};
    const int lens[] = {1, 2, 4, 8, 16, 20};
    long long events = 0;
    for (int q = 0; q < sequences; ++q) {
        R = grids[q % 4][0];
        C = grids[q % 4][1];
        Sim s;
        s.set[0].fill(0);
        s.set[1].fill(0);
        s.aw.init(R, C, true);
        s.aw.reset();
        s.check("start");
        auto source = [&]() {
            // points and small patches anywhere: corners, edge rows and columns, the frame, the interior
            const int kind = rnd(0, 5), h = kind == 5 ? rnd(1, 4) : 1, w = kind == 5 ? rnd(1, 6) : 1;
            int r = rnd(0, R - h), c = rnd(0, C - w);
            if (kind == 0) r = rnd(0, 1) ? 0 : R - h, c = rnd(0, 1) ? 0 : C - w;
            if (kind == 1) r = rnd(0, 7);
            if (kind == 2) c = C - w - rnd(0, 7);
            return Rect{r, r + h, c, c + w};
        };
        const int nev = rnd(3, 10);
        for (int e = 0; e < nev; ++e, ++events) {
            const int ev = rnd(0, 99);
            if (ev < 50) {
                const int n = lens[rnd(0, 5)];
                const Rect src = rnd(0, 3) ? source() : Rect{};
                const Rect W = s.aw.window(src, n);
                check_launch(W, src, n <= 4 ? 4 : (n <= 8 ? 8 : n), rnd(9, 30), rnd(1, 4));
                s.pass(src, n, rnd(0, 4) == 0);
                s.check("pass");
            } else if (ev < 60) {
                step_h(s.set[s.cur].ez, s.set[s.hcur].hx, s.set[s.hcur].hy);
                s.aw.half_step();
                s.check("update_h");
            } else if (ev < 70) {
                step_e(s.set[s.cur].ez, s.set[s.hcur].hx, s.set[s.hcur].hy, s.set[s.cur ^ 1].ez);
                s.cur ^= 1;
                s.aw.half_step();
                s.check("update_e");
            } else if (ev < 78) {
                const Rect src = source();
                add_src(s.set[s.cur].ez, src);
                s.aw.add_source(src);
                s.check("add_point");
            } else if (ev < 84) {         // trial launches: anything may be left in the target set
                s.set[s.cur ^ 1].ez.assign((size_t)R * C, 1);
                s.set[s.hcur ^ 1].hx.assign((size_t)R * C, 1);
                s.set[s.hcur ^ 1].hy.assign((size_t)R * C, 1);
                s.aw.uncommitted();
                s.check("uncommitted");
            } else if (ev < 89) {
                s.set[s.cur ^ 1].ez = s.set[s.cur].ez;
                s.set[s.hcur ^ 1].hx = s.set[s.hcur].hx;
                s.set[s.hcur ^ 1].hy = s.set[s.hcur].hy;
                s.aw.copied_to_other();
                s.check("copy");
            } else if (ev < 93) {         // upload: the current set is arbitrary
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
                CHECK(s.aw.support.empty() && s.aw.dirty_other.empty(), "reset leaves a window");
                s.check("reset");
            }
        }
    }
    // an engine without tracking reports the whole grid whatever happens
    {
        fdtd_aw::ActiveWindow w;
        w.init(30, 40, false);
        w.reset();
        w.commit_pass(Rect{3, 4, 5, 6}, 8);
        CHECK(w.support.cells() == 1200 && w.dirty_other.cells() == 1200, "an untracked window must stay full");
    }
    std::printf("%lld events, %d failures\n", events, failures);
    return failures ? 1 : 0;
}
