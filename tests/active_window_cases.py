"""Case table of tests/test_gpu_active_window_filled.py and tests/test_active_window_cases_cpu.py -- TEST INFRASTRUCTURE.

The active window (csrc/active_window.hpp) at a Courant number of 0.65, where the field FILLS the window: at 0.15 (every
case of tests/test_gpu_active_window.py) the front of a point source loses a factor of 0.0225 per cell and underflows
float32 some 30 cells out, so the outer part of every window holds zeros in the oracle and in both buffer sets, and a
launch that dropped a band, a strip or a zone tile there would pass.  Here DT = S DX / c0 with S = 0.65 (the 2D limit with
eps_r >= 1 is 0.707) and materials at or near vacuum; amplitudes are scaled up (`amp`) where float32 would otherwise
underflow before the front arrives.  tests/test_active_window_cases_cpu.py proves per row, from the oracle alone, that
the non-zero cells come within one cell of every side of the expected window that is not a grid edge.

A row names: shape, dtype, materials (`kind`: vacuum | eps | eps+mu, arrays uniform(1, 1.5) times the vacuum value),
the source rectangle (`extent`), its segments, the engine options, and `prop`: what the row is listed for, as
assertions on the launches the restated rules below predict.  A segment is (steps, row, col, seed) -- a run() with
amplitudes `amp * standard_normal(steps)` of that seed, seed None: no source -- or an operation:
    ("time_launches", n, steps)   n dense, committed launches without a source
    ("reset",)                    both buffer sets zeroed
    ("upload",)                   the current state downloaded and uploaded again: the window becomes the whole grid
    ("point", row, col, value)    add_point, update_h, update_e (the single-step kernels: dense)

The rules of the library are RESTATED here (grow and restrict_launch of active_window.hpp, the strip widths, the
planning of passes, the band-height rule of a window, the source strips and the XCD pad of pass_impl.hpp): `simulate`
replays a row through them and yields, per segment, the window, the pass counts and what every windowed pass must have
launched.  The GPU module asserts these against what the library reports (Engine.last_window_launch)."""
import functools

import numpy as np

from fused_cases import plan

DX = 1e-4
C0 = 1.0 / np.sqrt(8.85418e-12 * 4 * np.pi * 1e-7)        # from the oracle's EPS0 and MU0
S = 0.65
DT = S * DX / C0
NAMES = ("Ez", "Hx", "Hy")
F32, F64 = "float32", "float64"
MARGIN = 6

ROWS = []


def _add(name, prop, shape, segments, dtype=F32, kind="vacuum", extent=(1, 1), amp=1.0, options=None, set_shape=None,
         probe=None, dft=None):
    assert all(r["name"] != name for r in ROWS), name
    o = dict(active_window=1, max_pass_steps=16)
    o.update(options or {})
    ROWS.append(dict(name=name, prop=prop, shape=shape, segments=tuple(segments), dtype=dtype, kind=kind, extent=extent,
                     amp=amp, options=o, set_shape=set_shape, probe=probe, dft=dft))


# ---- the rules, restated ---------------------------------------------------------------------------------------------

def hc_of(nt):
    """stream_hc: columns a strip loads beyond those it writes, per side."""
    return 4 if nt <= 4 else (8 if nt <= 8 else (16 if nt <= 16 else 20))


def strip_ow(dtype, nt):
    """Columns a strip writes: one wave of 64 lanes holds 4 (float32) or 2 (float64) columns per lane."""
    return 64 * (4 if dtype == F32 else 2) - 2 * hc_of(nt)


def empty(w):
    return w is None or w[0] >= w[1] or w[2] >= w[3]


def cells(w):
    return 0 if empty(w) else (w[1] - w[0]) * (w[3] - w[2])


def unite(a, b):
    if empty(a):
        return None if empty(b) else b
    if empty(b):
        return a
    return (min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]))


def grow(w, n, R, C):
    """w = (r0, r1, c0, c1) half-open, n cells out on every side; a side fewer than MARGIN cells from the edge snaps."""
    if empty(w):
        return None
    lo = lambda v: 0 if v - n < MARGIN else v - n
    hi = lambda v, N: N if v + n > N - MARGIN else v + n
    return (lo(w[0]), hi(w[1], R), lo(w[2]), hi(w[3], C))


def strip_holds(s, ow, hc, c0, c1):
    return c1 + hc > s * ow and c0 - hc < (s + 1) * ow


def restrict_launch(w, src, R, C, nt, ow, hc, nstrips):
    zo = 5 + nt
    lo, hi = zo, R - zo
    L = dict(ztop=int(w[0] < zo + nt), zbot=int(w[1] > R - zo - nt))
    L["band_lo"] = lo if L["ztop"] else min(w[0], hi)
    L["band_hi"] = hi if L["zbot"] else max(w[1], lo)
    L["band_hi"] = max(L["band_hi"], L["band_lo"])
    c0, c1 = w[2], w[3]
    if not empty(src):
        c0, c1 = min(c0, src[2] - hc), max(c1, src[3] + hc)
    c0, c1 = max(c0, 0), min(c1, C)
    if nstrips <= 2:
        L.update(edges=1, strip_first=1, inner=0)
        return L
    L["edges"] = int(c0 < ow or c1 > (nstrips - 2) * ow)
    sa, sb = max(1, c0 // ow), min(nstrips - 2, (c1 - 1) // ow)
    L["inner"] = max(0, sb - sa + 1)
    L["strip_first"] = sa if L["inner"] else 1
    return L


def level_split(row, nt):
    o = row["options"]
    if nt not in (8, 16, 20):
        return False
    if nt == 20:
        return row["dtype"] == F32
    if nt == 16:
        return row["dtype"] == F32 or not row["probe"]
    if row["kind"] != "vacuum" and o.get("zone_split") == 1:
        return False
    return o.get("level_split", 1) != 0


def window_band_rows(region, nw, ns, split):
    """The band height of a window without a given one: one round of workgroups where the strips allow it."""
    slots = 256 * 16 // nw * 9 // 10 if split else 3072
    per = max(1, slots // max(1, ns))
    return min(max(-(-region // per), 32), 448)


def launch_shape(row, L, nt, src):
    """What launch_pass / launch_pass_impl make of a restricted launch L: the entries of Engine.last_window_launch."""
    o, (R, C) = row["options"], row["shape"]
    region = max(0, L["band_hi"] - L["band_lo"])
    split = level_split(row, nt)
    gs = None if o.get("band_rows", 0) > 0 else row["set_shape"]
    if not split:
        nw = 1
    elif nt > 16:
        nw = 4
    elif o.get("split_waves"):
        nw = o["split_waves"]
    elif gs and gs[1]:
        nw = gs[1]
    else:
        nw = 8 if region * C < ((12 << 20) if nt == 16 else (3 << 20)) else 4
    if o.get("band_rows", 0) > 0:
        br = o["band_rows"]
    elif gs:
        br = gs[0]
    else:
        br = window_band_rows(region, nw, L["inner"] + 2 * L["edges"], split)
    er = gs[2] if gs and len(gs) > 2 and gs[2] > 0 else br
    ow, hc = strip_ow(row["dtype"], nt), hc_of(nt)
    nstrips = -(-C // ow)
    brs = max(16, min(er, br // 3))
    n_src = 0
    if not empty(src) and brs < br and nstrips > 2:
        held = [s for s in range(1, nstrips - 1) if strip_holds(s, ow, hc, src[2], src[3])]
        if held and held[-1] - held[0] + 1 <= 2:
            n_src = held[-1] - held[0] + 1
    out = dict(band_rows=br, waves=nw, strip_first=L["strip_first"], inner=L["inner"], n_src=n_src, edges=L["edges"],
               ztop=L["ztop"], zbot=L["zbot"], edge_rows=er, xcd_map=0, xcd_pad=0, band_lo=L["band_lo"], band_hi=L["band_hi"])
    main = max(0, L["inner"] - n_src)
    out["nbands"] = -(-region // br)
    out["main"] = main
    if o.get("xcd_map") == 1 and nt >= 8 and split and main > 0:
        out["xcd_map"] = 1
        clamp = lambda v, a, b: min(max(v, a), b)
        nbs = 0
        if n_src:
            s_lo = clamp(src[0] - nt, L["band_lo"], L["band_hi"])
            s_hi = clamp(src[1] + 2 * nt, s_lo, L["band_hi"])
            nbs = -(-(s_lo - L["band_lo"]) // br) - (-(s_hi - s_lo) // brs) - (-(L["band_hi"] - s_hi) // br)
        nbe = -(-region // er) if L["edges"] else 0
        # (zone tiles that ride in front of the bulk count too: predicted only for launches without any)
        out["xcd_pad"] = (8 - (2 * nbe + n_src * nbs) % 8) % 8 if not (L["ztop"] or L["zbot"]) else None
    return out


def simulate(row):
    """Replays the row's segments through the restated rules.  Per segment: dict(window = the support rectangle the
    engine must report, passes, windowed = counts so far, launches = [launch_shape of every windowed pass of the
    segment], windows = [the rectangle each of them had to write], dense = passes of the segment's run() that the
    half-grid cap made whole-grid launches)."""
    (R, C), o = row["shape"], row["options"]
    full = (0, R, 0, C)
    support = dirty = None          # after reset()
    cycle = min(o["max_pass_steps"], 16) if not (row["dtype"] == F64 and row["probe"]) else 8
    longp = row["dtype"] == F32 and o["max_pass_steps"] >= 20 and not row["probe"]
    passes = windowed = 0
    out = []

    def run(steps, src, may_window):
        nonlocal support, dirty, passes, windowed
        launches, windows = [], []
        dense = 0
        split_any = level_split(row, cycle)
        for nt, nlev in plan(steps, cycle, split_any, long_passes=longp):
            W = unite(grow(unite(support, src), nlev, R, C), dirty)
            if may_window and 2 * cells(W) <= R * C:
                windowed += 1
                if not empty(W):
                    ow, hc = strip_ow(row["dtype"], nt), hc_of(nt)
                    L = restrict_launch(W, src, R, C, nt, ow, hc, -(-C // ow))
                    launches.append(dict(launch_shape(row, L, nt, src), nt=nt, nlev=nlev))
                    windows.append(W)
            elif may_window:
                dense += 1
            passes += 1
            old = support
            support = grow(unite(old, src), nlev, R, C)
            dirty = old
        return launches, windows, dense

    for seg in row["segments"]:
        launches, windows, dense = [], [], 0
        if seg[0] == "reset":
            support = dirty = None
        elif seg[0] == "upload":
            support = dirty = full
        elif seg[0] == "point":
            support = unite(support, (seg[1], seg[1] + 1, seg[2], seg[2] + 1))
            for _ in range(2):                      # update_h, update_e: each grows by one
                old = support
                support = grow(old, 1, R, C)
                dirty = unite(dirty, old)
        elif seg[0] == "time_launches":
            for _ in range(seg[1]):
                run(seg[2], None, False)
        else:
            steps, r, c, seed = seg
            src = None if seed is None else (r, r + row["extent"][0], c, c + row["extent"][1])
            launches, windows, dense = run(steps, src, True)
        out.append(dict(window=support or (0, 0, 0, 0), passes=passes, windowed=windowed, launches=launches,
                        windows=windows, dense=dense))
    return out


# ---- inputs and the reference -----------------------------------------------------------------------------------------

def amps_of(row, steps, seed):
    return row["amp"] * np.random.default_rng(seed).standard_normal(steps)


@functools.lru_cache(maxsize=None)
def _materials(shape, dtype, kind):
    from oracle import fdtd_numpy as onp
    r, c = shape
    rng = np.random.default_rng(r * 131 + c)
    eps = onp.EPS0 * (rng.uniform(1, 1.5, (r, c)) if "eps" in kind else np.ones((r, c)))
    mu = onp.MU0 * (rng.uniform(1, 1.5, (r, c)) if "mu" in kind else np.ones((r, c)))
    if kind != "vacuum":
        eps[0, 0], mu[0, 0] = onp.EPS0, onp.MU0      # the Mur factor comes from this cell: the frame absorbs at c0
    eps, mu = eps.astype(dtype), mu.astype(dtype)
    eps.setflags(write=False)
    mu.setflags(write=False)
    return eps, mu


def materials(row):
    return _materials(row["shape"], row["dtype"], row["kind"])


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


@functools.lru_cache(maxsize=None)
def reference(name, fused=False):
    """The C oracle through the row's segments, from rest.  Returns dict(states = [(Ez, Hx, Hy) after each segment],
    series = Ez at the probe cell after every step of a run (rows with a probe), steps = [(step number, Ez of the
    transform window) for every step] (rows with a transform)).  Computed once per row and arithmetic; read-only."""
    from oracle import c_oracle as corc, fdtd_numpy as onp
    row = by_name(name)
    eps, mu = materials(row)
    f = list(onp.grid_zeros(*row["shape"], np.dtype(row["dtype"]).type))
    corc.set_threads(*row["shape"])
    states, series, dsteps, step = [], [], [], 0

    def one(src, a):
        nonlocal step
        corc.update_h(*f, mu, eps, DT, DX, fused=fused)
        corc.update_e(*f, mu, eps, DT, DX, fused=fused)
        if src is not None:
            onp.add_source(f[0], src[0], src[1], a, row["extent"])
        step += 1
        if row["probe"]:
            series.append(float(f[0][row["probe"]]))
        if row["dft"]:
            r0, c0, nr, nc = row["dft"]["window"]
            dsteps.append((step, f[0][r0:r0 + nr, c0:c0 + nc].astype(np.float64)))

    per_step = tuple(row["extent"]) != (1, 1) or row["probe"] or row["dft"]
    for seg in row["segments"]:
        if seg[0] == "point":
            onp.add_point(f[0], seg[1], seg[2], seg[3])
            corc.update_h(*f, mu, eps, DT, DX, fused=fused)
            corc.update_e(*f, mu, eps, DT, DX, fused=fused)
        elif seg[0] == "time_launches":
            for _ in range(seg[1] * seg[2]):
                one(None, 0.0)
        elif seg[0] == "reset":
            for a in f:
                a[...] = 0
        elif seg[0] == "upload":
            pass
        else:
            steps, r, c, seed = seg
            a = amps_of(row, steps, seed) if seed is not None else None
            if per_step or a is None:
                for s in range(steps):
                    one(None if a is None else (r, c), 0.0 if a is None else a[s])
            else:
                corc.run(*f, eps, mu, DT, DX, steps, r, c, amps=a, fused=fused)
                step += steps
        snap = tuple(x.copy() for x in f)
        for x in snap:
            x.setflags(write=False)
        states.append(snap)
    return dict(states=states, series=np.array(series), steps=dsteps)


def support_box(state):
    """Bounding box (r0, r1, c0, c1) of the non-zero cells of Ez, Hx and Hy, or None."""
    box = None
    for a in state:
        nz = np.nonzero(a)
        if len(nz[0]):
            box = unite(box, (int(nz[0].min()), int(nz[0].max()) + 1, int(nz[1].min()), int(nz[1].max()) + 1))
    return box


# ---- the table ---------------------------------------------------------------------------------------------------------
# float32 16-step strips write 224 columns (8 steps: 240, 20 steps: 216), float64 96 (8 steps: 112).  The bulk rows of an
# nt-step pass are [5 + nt, R - 5 - nt); a window whose rows come within 5 + 2 nt of the top / bottom takes that side's
# zone tiles.  G = 400 x 1400: 7 strips (inner 1 .. 5); P = 300 x 1000: 5 strips (inner 1 .. 3).
G, P = (400, 1400), (300, 1000)

# -- long runs that fill
# (Heights: a point source after n steps has a window of 2 n + 1 rows, and its outermost row and column are the injection
# that has not spread yet.  With n a multiple of 16 the LAST band of 32 rows is that one row of zeros, and a launch that
# dropped it would pass: the rows listed for bands end on n = 8 mod 16 or use a source 16 rows tall, so that the last band
# has 16 or 17 rows and all but one of them are non-zero.)
# 136 steps = 9 passes (16 x 7, 12, 12): the window ends 273 columns wide, [439, 712): strips 1, 2, 3; rows [64, 337) clear
# of both zones: 273 rows = 9 bands at the 32-row floor of the rule, the last one 17 rows.  The source column 575 lies in
# strip 2 alone: n_src = 1.
_add("fill_point_136", dict(passes=9, strips_min=3, bands_min=4, n_src=1, band_rows=32, ztop=0, zbot=0, last_band_rows=17), G,
     [(64, 200, 575, 1), (72, 200, 575, 2)], amp=1e20)
# a 16 x 800 patch, columns [520, 1320): 64 steps end at columns [456, 1384): strips 2 .. 6 of 9, no edge strip
# (1384 <= 7 * 224); the source lies over four strips: no source bands.  144 rows: 5 bands, the last one 16 rows.
_add("fill_line_5_strips", dict(passes=4, strips_min=5, strip_first_min=2, n_src=0, edges=0, bands_min=4, band_rows=32,
                                last_band_rows=16),
     (240, 1800), [(32, 120, 520, 3), (32, 120, 520, 4)], extent=(16, 800))
# the source on the seam 3 * 224: strips 2 and 3 hold it; the window [552, 793) is exactly these two
_add("fill_point_on_seam", dict(passes=8, n_src=2, inner=2, bands_min=4, band_rows=32, last_band_rows=17), G,
     [(48, 200, 672, 5), (72, 200, 672, 6)], amp=1e12)

# -- float64: 96-column strips (16 steps), 112 (8 steps)
_add("f64_16_point", dict(passes=5, strips_min=3, waves=8), P, [(32, 150, 500, 7), (48, 150, 500, 8)], dtype=F64)
_add("f64_8_eps_mu_tail", dict(passes=6, strips_min=2, short_tail=1), P, [(44, 150, 448, 9)], dtype=F64, kind="eps+mu",
     options=dict(max_pass_steps=8))

# -- pass lengths, each with a short tail (nlev < nt)
_add("f32_20_tail", dict(passes=3, short_tail=1, last_nt=20), P, [(51, 150, 500, 10)], options=dict(max_pass_steps=20))
_add("f32_16_tail", dict(passes=4, short_tail=1, last_nt=16), P, [(59, 150, 500, 11)])
_add("f32_8_tail", dict(passes=6, short_tail=1, last_nt=8), P, [(44, 150, 500, 12)], options=dict(max_pass_steps=8))
_add("f32_8_eps_tail", dict(passes=6, short_tail=1, last_nt=8), P, [(44, 150, 500, 13)], kind="eps",
     options=dict(max_pass_steps=8))
_add("f32_8_level_split_0", dict(passes=5, waves=1, last_nt=8), P, [(40, 150, 500, 14)],
     options=dict(max_pass_steps=8, level_split=0))

# -- the rule-made band height above its floor.  br = ceil(region / per) > 32 needs region > 32 * floor(460 / ns) rows
# (460 = 90 % of 256 CUs x 16 wave slots / 8 waves; ns strips in the launch).  A grid of one or two strips launches its
# edge strips only, ns = 2: region >= 7361 rows.  After two passes a vertical line is 65 columns wide, the grid must hold
# twice the window: 7500 x 200 = 1.5 M cells.  With ns >= 3 the window spans ns - 1 strips of 224 columns and the grid
# twice that: 32 * floor(460 / ns) * 2 * (ns - 1) * 224 >= 4.4 M cells for every ns, so this is the smallest.
# Line rows [100, 7400), 32 steps: window rows [68, 7432) = 7364 rows, clear of both zones: br = ceil(7364 / 230) = 33.
_add("tall_rule_33_rows", dict(passes=2, band_rows=33, edges=1, inner=0, ztop=0, zbot=0), (7500, 200),
     [(32, 100, 100, 15)], extent=(7300, 1))

# -- launch options on a filled window of several strips.  A 16 x 700 patch from column 8: the window touches column 0
# (edge strips) and its inner run is strips 1 .. 3; 144 rows = 5 bands, the last one 16 rows: 15 inner tasks, 10 edge tasks
# in front: pad 6.
_LINE0 = dict(shape=(240, 1800), segments=[(64, 120, 8, 16)], extent=(16, 700))
_add("opt_xcd_map", dict(passes=4, xcd_map=1, xcd_pad=6, tasks_mod8=7, edges=1, strip_first=1, inner=3, last_band_rows=16), **_LINE0,
     options=dict(xcd_map=1))
_add("opt_split_waves_4", dict(passes=4, waves=4, inner=3), **_LINE0, options=dict(split_waves=4))
_add("opt_split_waves_8", dict(passes=4, waves=8, inner=3), **_LINE0, options=dict(split_waves=8))
_add("opt_zone_split_ztop_alone", dict(passes=3, ztop=1, zbot=0), P, [(48, 30, 500, 17)], options=dict(zone_split=1))
_add("opt_given_shape_edge_rows", dict(passes=3, band_rows=48, edge_rows=24, edges=1, waves=4), (240, 1800),
     [(48, 120, 8, 18)], extent=(1, 300), set_shape=(48, 4, 24))

# -- the window's sides against the partition.  A 1 x 128 line, 48 steps: 224 columns, both sides on seams, and one
# column either way
for _d in (-1, 0, 1):
    _add(f"seams_{'m1' if _d < 0 else 'p' + str(_d)}", dict(passes=3, c0=448 + _d, c1=672 + _d, strip_first=2 if _d >= 0 else 1,
                                                            inner=1 if _d == 0 else 2), P,
         [(48, 150, 496 + _d, 20 + _d)], extent=(1, 128))
# 1130 = 5 * 224 + 10 columns: the last strip, shifted left to end at the edge, overlaps strip 4 almost entirely
_add("right_edge_shifted_strip", dict(passes=3, edges=1, strip_first=4, inner=1, c1=1130), (300, 1130),
     [(48, 150, 1100, 23)])
# r0 at 5 + 2 * 16 = 37 (no top zone) and at 36 (top zone alone); the mirror at the bottom of 300 rows
_add("ztop_off_r0_37", dict(passes=3, ztop=0, zbot=0, r0=37), P, [(48, 85, 500, 24)])
_add("ztop_on_r0_36", dict(passes=3, ztop=1, zbot=0, r0=36), P, [(48, 84, 500, 25)])
_add("zbot_off_r1_263", dict(passes=3, ztop=0, zbot=0, r1=263), P, [(48, 214, 500, 26)])
_add("zbot_on_r1_264", dict(passes=3, ztop=0, zbot=1, r1=264), P, [(48, 215, 500, 27)])

# -- MARGIN: after 32 steps a bound at index 5 snaps to the edge, one at index 6 stays; 16 more steps run the Mur frame
# on non-zero cells in either case.  (row, column): (snaps, free) and (free, snaps), at the top left and the bottom right.
_add("margin_top_snaps_left_free", dict(mid_window=(0, 70, 6, 71)), P, [(32, 37, 38, 28), (16, 37, 38, 29)])
_add("margin_top_free_left_snaps", dict(mid_window=(6, 71, 0, 70)), P, [(32, 38, 37, 30), (16, 38, 37, 31)])
_add("margin_bottom_snaps_right_free", dict(mid_window=(230, 300, 929, 994)), P, [(32, 262, 961, 32), (16, 262, 961, 33)])
_add("margin_bottom_free_right_snaps", dict(mid_window=(229, 294, 930, 1000)), P, [(32, 261, 962, 34), (16, 261, 962, 35)])

# -- stale targets: both buffer sets hold non-zero cells that a later window has to overwrite or to leave as they are
_add("stale_time_launches", dict(passes=3 + 2 + 3), G, [(48, 200, 700, 36), ("time_launches", 2, 16), (48, 200, 700, 37)],
     amp=1e12)
_add("stale_two_sources", dict(passes=6), (500, 1600), [(48, 150, 300, 38), (48, 350, 1300, 39)], amp=1e6)
_add("stale_single_steps", dict(passes=3), P, [("point", 150, 448, 0.75), (48, 150, 448, 40)])
_add("stale_reset", dict(passes=6), P, [(48, 100, 300, 41), ("reset",), (48, 200, 700, 42)])
_add("stale_upload", dict(passes=6, dense_after_upload=1), P, [(48, 150, 500, 43), ("upload",), (48, 150, 500, 44)])

# -- consumers on the front: a probe 40 cells from the source (reached in the third pass only), a transform window over
# the outer 20 columns of the final window [452, 549) and 11 columns beyond
_add("probe_on_the_front", dict(passes=3), P, [(48, 150, 500, 45)], probe=(150, 540))
_add("dft_on_the_front", dict(passes=3), P, [(48, 150, 500, 46)],
     dft=dict(window=(140, 529, 21, 31), omega=(2 * np.pi * 20e9, 2 * np.pi * 45e9), every=16))
