"""Case table of tests/test_gpu_active_window_oct.py and tests/test_active_window_oct_cases_cpu.py -- TEST INFRASTRUCTURE.

The diagonal bounds of the active window (Oct in csrc/active_window.hpp) at a Courant number of 0.65 in vacuum, like
tests/active_window_cases.py, whose restated rules of the rectangles and the launch this module builds on.  Restated
HERE: the bounds' transitions (reset, add_point, commit_pass, half_step, copy), when they are dropped (a side of the
rectangle within MARGIN of an edge), the decoding of a launch into (strip, band) tasks (strip_of_block) and the test that
empties a task (task_meets_oct).  `simulate` replays a row and yields per segment the window, the bounds of the support
and, per windowed pass, its launch, its bounds and the number of tasks they empty.

Shapes: the smallest at which a whole (32-row band x 224-column strip) task can fall outside: T = 1000 x 2000 float32
with a source near the centre -- 320 steps in 16-step passes end at 21 bands x 3-4 strips, a window of 20 % of the grid;
float64 strips are 96 columns, so 600 x 900 and 150 steps suffice.  Along the axes the front of a point source underflows
(one path, a factor 0.4225 per cell); on the diagonals C(n, n/2) paths keep it at 0.845^n: that is where the field
touches the bounds, which tests/test_active_window_oct_cases_cpu.py proves per row.

A segment is (steps, row, col, seed) as in active_window_cases, or ("add_point", row, col, value) -- add_point alone, no
half-steps: the bounds are EXACT from there, where a run's source is grown one cell too far -- or ("copy",), measure_copy."""
import functools

import numpy as np

import active_window_cases as awc
from fused_cases import plan

DT, DX, NAMES, F32, F64, MARGIN = awc.DT, awc.DX, awc.NAMES, awc.F32, awc.F64, awc.MARGIN
BIG = 1 << 29
UNBOUNDED = (-BIG, BIG, -BIG, BIG)

ROWS = []


def _add(name, shape, segments, dtype=F32, kind="vacuum", extent=(1, 1), amp=1.0, options=None, set_shape=None, skips=True,
         n_src=None, lost=False):
    """skips: some windowed pass of the row must skip tasks; lost: the bounds are dropped on the way (a snapped side)."""
    assert all(r["name"] != name for r in ROWS), name
    o = dict(active_window=1, max_pass_steps=16)
    o.update(options or {})
    ROWS.append(dict(name=name, shape=shape, segments=tuple(segments), dtype=dtype, kind=kind, extent=extent, amp=amp,
                     options=o, set_shape=set_shape, probe=None, dft=None, skips=skips, n_src=n_src, lost=lost))


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


# ---- the bounds, restated: (s0, s1, d0, d1) closed, None = empty ---------------------------------------------------------

def oct_of(rect):
    if awc.empty(rect):
        return None
    r0, r1, c0, c1 = rect
    return (r0 + c0, r1 - 1 + c1 - 1, r0 - (c1 - 1), r1 - 1 - c0)


def hull(a, b):
    if a is None or b is None:
        return a if b is None else b
    return (min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]))


def grow_oct(o, n):
    if o is None:
        return None
    lo = lambda v: v if v <= -BIG else v - n
    hi = lambda v: v if v >= BIG else v + n
    return (lo(o[0]), hi(o[1]), lo(o[2]), hi(o[3]))


def clear_of_frame(rect, R, C):
    return awc.empty(rect) or (rect[0] >= MARGIN and rect[1] <= R - MARGIN and rect[2] >= MARGIN and rect[3] <= C - MARGIN)


def meets(o, ra, rb, ca, cb):
    """task_meets_oct: do the cells [ra, rb) x [ca, cb) meet all four half-planes?"""
    return rb - 1 + cb - 1 >= o[0] and ra + ca <= o[1] and rb - 1 - ca >= o[2] and ra - (cb - 1) <= o[3]


def inside(o, shape):
    """Boolean map of the cells inside the bounds."""
    i, j = np.ogrid[0:shape[0], 0:shape[1]]
    return (i + j >= o[0]) & (i + j <= o[1]) & (i - j >= o[2]) & (i - j <= o[3])


def tasks(row, launch, src):
    """[(strip, ra, rb)] of the bulk of a windowed launch, as strip_of_block decodes it (order aside)."""
    C = row["shape"][1]
    nt, br, er = launch["nt"], launch["band_rows"], launch["edge_rows"]
    lo, hi = launch["band_lo"], launch["band_hi"]
    ow, hc = awc.strip_ow(row["dtype"], nt), awc.hc_of(nt)
    ns = -(-C // ow)
    bands = lambda a, b, h: [(x, min(x + h, b)) for x in range(a, b, h)]
    out = []
    if launch["edges"]:
        for s in ([0] if ns == 1 else [0, ns - 1]):
            out += [(s, a, b) for a, b in bands(lo, hi, er)]
    held = []
    if launch["n_src"]:
        held = [s for s in range(1, ns - 1) if awc.strip_holds(s, ow, hc, src[2], src[3])]
        assert len(held) == launch["n_src"]
        brs = max(16, min(er, br // 3))
        clamp = lambda v, a, b: min(max(v, a), b)
        s_lo = clamp(src[0] - nt, lo, hi)
        s_hi = clamp(src[1] + 2 * nt, s_lo, hi)
        for s in held:
            out += [(s, a, b) for a, b in bands(lo, s_lo, br) + bands(s_lo, s_hi, brs) + bands(s_hi, hi, br)]
    for s in range(launch["strip_first"], launch["strip_first"] + launch["inner"]):
        if s not in held:
            out += [(s, a, b) for a, b in bands(lo, hi, br)]
    return out


def skipped(row, launch, src, o):
    C = row["shape"][1]
    ow = awc.strip_ow(row["dtype"], launch["nt"])
    return [t for t in tasks(row, launch, src) if not meets(o, t[1], t[2], t[0] * ow, min((t[0] + 1) * ow, C))]


def simulate(row):
    """Per segment: dict(window, oct = bounds of the support (None: empty), launches = [launch_shape + nt, nlev, oct = the
    bounds of the pass, skipped = tasks they empty, tasks = all of them, W = its rectangle] per windowed pass)."""
    (R, C), o = row["shape"], row["options"]
    support = dirty = None
    s_oct = d_oct = None
    lost = False
    cycle = min(o["max_pass_steps"], 16)
    longp = row["dtype"] == F32 and o["max_pass_steps"] >= 20
    passes = windowed = 0
    out = []

    def settle():
        nonlocal lost, s_oct, d_oct
        if not clear_of_frame(support, R, C):
            lost = True
        if lost:
            s_oct = UNBOUNDED
        if not clear_of_frame(dirty, R, C):
            d_oct = UNBOUNDED

    for seg in row["segments"]:
        launches = []
        if seg[0] == "add_point":
            p = (seg[1], seg[1] + 1, seg[2], seg[2] + 1)
            support, s_oct = awc.unite(support, p), hull(s_oct, oct_of(p))
            settle()
        elif seg[0] == "copy":
            dirty, d_oct = awc.unite(dirty, support), UNBOUNDED
        else:
            steps, r, c, seed = seg
            src = None if seed is None else (r, r + row["extent"][0], c, c + row["extent"][1])
            for nt, nlev in plan(steps, cycle, awc.level_split(row, cycle), long_passes=longp):
                grown = awc.grow(awc.unite(support, src), nlev, R, C)
                W = awc.unite(grown, dirty)
                assert 2 * awc.cells(W) <= R * C, "every pass of these rows launches a window"
                windowed += 1
                passes += 1
                if lost or not clear_of_frame(grown, R, C) or not clear_of_frame(dirty, R, C):
                    wo = UNBOUNDED
                else:
                    wo = hull(grow_oct(hull(s_oct, oct_of(src)), nlev), d_oct)
                if o.get("window_octagon") == 0:
                    wo = UNBOUNDED
                ow, hc = awc.strip_ow(row["dtype"], nt), awc.hc_of(nt)
                L = awc.restrict_launch(W, src, R, C, nt, ow, hc, -(-C // ow))
                launch = dict(awc.launch_shape(row, L, nt, src), nt=nt, nlev=nlev, oct=wo, W=W)
                launch["tasks"] = tasks(row, launch, src)
                launch["skipped"] = skipped(row, launch, src, wo)
                launches.append(launch)
                old, old_oct = support, s_oct
                support, s_oct = grown, grow_oct(hull(old_oct, oct_of(src)), nlev)
                dirty, d_oct = old, old_oct
                settle()
        out.append(dict(window=support or (0, 0, 0, 0), oct=s_oct, passes=passes, windowed=windowed, launches=launches))
    return out


# ---- inputs and the reference --------------------------------------------------------------------------------------------

amps_of = awc.amps_of
materials = awc.materials


@functools.lru_cache(maxsize=None)
def reference(name, fused=False):
    """The C oracle through the row's segments, from rest: [(Ez, Hx, Hy) after each segment], read-only, once per row."""
    from oracle import c_oracle as corc, fdtd_numpy as onp
    row = by_name(name)
    eps, mu = materials(row)
    f = list(onp.grid_zeros(*row["shape"], np.dtype(row["dtype"]).type))
    corc.set_threads(*row["shape"])
    states = []
    for seg in row["segments"]:
        if seg[0] == "add_point":
            onp.add_point(f[0], seg[1], seg[2], seg[3])
        elif seg[0] == "copy":
            pass
        else:
            steps, r, c, seed = seg
            a = amps_of(row, steps, seed) if seed is not None else None
            if tuple(row["extent"]) != (1, 1) or a is None:
                for s in range(steps):
                    corc.update_h(*f, mu, eps, DT, DX, fused=fused)
                    corc.update_e(*f, mu, eps, DT, DX, fused=fused)
                    if a is not None:
                        onp.add_source(f[0], r, c, a[s], row["extent"])
            else:
                corc.run(*f, eps, mu, DT, DX, steps, r, c, amps=a, fused=fused)
        snap = tuple(x.copy() for x in f)
        for x in snap:
            x.setflags(write=False)
        states.append(snap)
    return states


def span(state):
    """(min, max of i + j, min, max of i - j) over the non-zero cells of Ez, Hx and Hy, or None."""
    out = None
    for a in state:
        i, j = np.nonzero(a)
        if len(i):
            out = hull(out, (int((i + j).min()), int((i + j).max()), int((i - j).min()), int((i - j).max())))
    return out


# ---- the table -----------------------------------------------------------------------------------------------------------
# float32 16-step strips write 224 columns (8 steps: 240, 20 steps: 216), float64 96.  T: 9 strips of 224.
T, D = (1000, 2000), (600, 900)

# the issue's shape: a centred point, 320 steps in 16-step passes: 21 bands x 3-4 strips at the end
_add("point_16", T, [(160, 500, 990, 101), (160, 500, 990, 102)], n_src=1)
# the same from add_point alone: the bounds are exact (a run's source is grown one cell too far), so bounds one cell too
# tight drop tasks that hold non-zero cells (tests/test_active_window_oct_cases_cpu.py shows which)
_add("exact_point_16", T, [("add_point", 500, 990, 1.0), (160, 0, 0, None), (160, 0, 0, None)])
# 8-step passes with a short tail (150 = 17 x 8 + 7 + 7)
_add("point_8_tail", T, [(150, 500, 990, 103)], options=dict(max_pass_steps=8))
# one 20-step pass on a window wide enough to have empty tasks (radius 96 before it)
_add("point_20", T, [(96, 500, 990, 104), (20, 500, 990, 105)], options=dict(max_pass_steps=20))
# float64: 96-column strips
_add("f64_point", D, [(150, 300, 450, 106)], dtype=F64)
# the source on the seam 4 * 224 = 896: two source strips
_add("seam_point", T, [(160, 500, 896, 107)], n_src=2)
# octagons with flat sides: a 16 x 300 patch (224 steps: the cut corners must be wider than a strip's part of the
# window before a task falls outside), a vertical line of 300 rows
_add("patch_16x300", T, [(224, 492, 850, 108)], extent=(16, 300))
_add("vline_300", T, [(128, 350, 990, 109)], extent=(300, 1))
# two sources in turn: the hull
_add("two_sources", T, [(96, 300, 600, 110), (96, 700, 1400, 111)])
# launch options
_add("opt_xcd_map", T, [(160, 500, 990, 112)], options=dict(xcd_map=1))
_add("opt_split_waves_4", T, [(160, 500, 990, 113)], options=dict(split_waves=4))
_add("opt_given_shape_edge_rows", T, [(160, 500, 990, 114)], set_shape=(48, 4, 24))
# an eps array near vacuum
_add("eps_point", T, [(128, 500, 990, 115)], kind="eps")
# a stale target after measure_copy: nothing skipped in the pass after it, skipping resumes with the next one
_add("stale_copy", T, [(128, 500, 990, 116), ("copy",), (48, 500, 990, 117)])
# a source 40 cells from the left edge: the rectangle snaps in the third pass, the bounds are dropped, nothing is skipped
# from then on (before that the window is too small to have empty tasks)
_add("left_edge_40", T, [(160, 500, 40, 118)], skips=False, lost=True)
