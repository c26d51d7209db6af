"""Case table of tests/test_gpu_active_window_waves.py and tests/test_active_window_waves_cpu.py -- TEST INFRASTRUCTURE.

Waves per strip of a windowed launch with none given: the size thresholds of split_waves_for (12 Mi cells for 16-step
passes, 3 Mi for 8-step ones) applied to the cells the launch COVERS -- the rows of its bulk times the columns its strips
write -- and not to rows x grid columns.  The rows of tests/active_window_cases.py all lie where both quantities are
below the threshold; the rows here lie where they differ (a tall, narrow window on a wide grid: 8 waves now, 4 before)
and where both are above it (4 either way).

Same physics as active_window_cases: Courant number 0.65, vacuum, the C oracle cell for cell.  Everything but the waves
rule is taken from that module's restated rules: a launch is replayed through its `simulate`, and the waves the new rule
gives are then handed to its `launch_shape` as a forced `split_waves`, which the library treats like a rule-made one
(the band height of a window takes the waves as input)."""
import functools

import numpy as np

import active_window_cases as awc

F32, F64 = awc.F32, awc.F64
ROWS = []


def _add(name, waves, shape, segments, dtype=F32, extent=(1, 1), options=None, set_shape=None, old_waves=None):
    o = dict(active_window=1, max_pass_steps=16)
    o.update(options or {})
    ROWS.append(dict(name=name, waves=waves, old_waves=old_waves, shape=shape, segments=tuple(segments), dtype=dtype,
                     kind="vacuum", extent=extent, amp=1.0, options=o, set_shape=set_shape, probe=None, dft=None, prop={}))


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


def threshold(nt):
    return (12 << 20) if nt == 16 else (3 << 20)


def launched_cells(row, launch):
    """Rows of the bulk times the columns written by the strips in the launch (never more than the grid's)."""
    ow = awc.strip_ow(row["dtype"], launch["nt"])
    return (launch["band_hi"] - launch["band_lo"]) * min(row["shape"][1], (launch["inner"] + 2 * launch["edges"]) * ow)


def rule_waves(row, launch):
    """Waves per strip of a windowed level-split launch of 8 or 16 steps: the caller's, else by launched cells."""
    o, gs = row["options"], row["set_shape"]
    if o.get("split_waves"):
        return o["split_waves"]
    if gs and gs[1]:
        return gs[1]
    return 8 if launched_cells(row, launch) < threshold(launch["nt"]) else 4


def simulate(row):
    """awc.simulate with every launch re-made on the waves of the new rule.  Each launch also carries `old_waves`, what
    rows x grid columns gave, and `cells` / `old_cells`, the two quantities."""
    sim = awc.simulate(row)
    for seg, s in zip(row["segments"], sim):
        src = None
        if isinstance(seg[0], int) and seg[3] is not None:
            src = (seg[1], seg[1] + row["extent"][0], seg[2], seg[2] + row["extent"][1])
        made = []
        for old in s["launches"]:
            assert old["nt"] in (8, 16) and awc.level_split(row, old["nt"])
            nw = rule_waves(row, old)
            forced = dict(row, options=dict(row["options"], split_waves=nw))
            L = {k: old[k] for k in ("band_lo", "band_hi", "strip_first", "inner", "edges", "ztop", "zbot")}
            new = dict(awc.launch_shape(forced, L, old["nt"], src), nt=old["nt"], nlev=old["nlev"])
            new.update(old_waves=old["waves"], cells=launched_cells(row, old),
                       old_cells=(old["band_hi"] - old["band_lo"]) * row["shape"][1])
            assert new["cells"] <= new["old_cells"]
            made.append(new)
        s["launches"] = made
    return sim


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, extent, segments, fused):
    from oracle import c_oracle as corc, fdtd_numpy as onp
    eps, mu = awc._materials(shape, dtype, "vacuum")
    f = list(onp.grid_zeros(*shape, np.dtype(dtype).type))
    corc.set_threads(*shape)
    states = []
    for steps, r, c, seed in segments:
        a = np.random.default_rng(seed).standard_normal(steps)
        for s in range(steps):
            corc.update_h(*f, mu, eps, awc.DT, awc.DX, fused=fused)
            corc.update_e(*f, mu, eps, awc.DT, awc.DX, fused=fused)
            onp.add_source(f[0], r, c, a[s], extent)
        snap = tuple(x.copy() for x in f)
        for x in snap:
            x.setflags(write=False)
        states.append(snap)
    return states


def reference(name, fused=False):
    """(Ez, Hx, Hy) of the C oracle after each segment, from rest; computed once per (grid, source, segments) and
    arithmetic -- rows that differ in launch options only share it -- and read-only."""
    row = by_name(name)
    return _reference(row["shape"], row["dtype"], row["extent"], row["segments"], fused)


# ---- the table ---------------------------------------------------------------------------------------------------------
# W = 1000 x 16384: 74 float32 16-step strips.  A vertical line of 800 cells at column 8000 from row 100: after the first
# 16-step pass the window is rows [84, 916), columns [7984, 8017): 832 rows x 16384 grid columns = 13.6 M >= 12 Mi, the
# old rule's 4 waves; the launch holds 2 or 3 strips, under 0.6 M cells: 8 waves.  One pass per segment, so that every
# pass's launch is read back: 16 + 16 + 8 steps (the last an 8-step pass: 880 rows x 16384 = 14.4 M >= 3 Mi).
W = (1000, 16384)
_LINE = dict(shape=W, extent=(800, 1))
_SEG = [(16, 100, 8000, 51), (16, 100, 8000, 52), (8, 100, 8000, 53)]
_add("flips_to_8_f32_16", 8, segments=_SEG, old_waves=4, **_LINE)
# 8-step passes (threshold 3 Mi): 816 rows x 16384 = 13.4 M after the first
_add("flips_to_8_f32_8", 8, segments=[(8, 100, 8000, 54), (8, 100, 8000, 55), (8, 100, 8000, 56)], old_waves=4,
     options=dict(max_pass_steps=8), **_LINE)
# float64: 96-column strips
_add("flips_to_8_f64_16", 8, segments=_SEG, old_waves=4, dtype=F64, **_LINE)
# the caller's waves still win
_add("forced_split_waves_4", 4, segments=_SEG, options=dict(split_waves=4), **_LINE)
# (a shape given without a pass length is that of the full-length passes: the two 16-step passes only)
_add("given_shape_waves_4", 4, segments=_SEG[:2], set_shape=(48, 4, 24), **_LINE)
# Both quantities at or above 12 Mi: 4096 x 8192 (33.5 M cells, half 16.8 M), a 3400 x 3800 patch from (348, 2196).  The
# window of the first pass is 3432 x 3832 = 13.15 M cells, rows [332, 3764), columns [2180, 6012); that of the second
# 3464 x 3864 = 13.38 M, rows [316, 3780), columns [2164, 6028): at least 6 cells from every edge, under half the grid.
# Each launches strips 9 .. 26, 18 x 224 = 4032 columns: 13.8 M and 14.0 M launched cells.
STAYS_4_WINDOWS = ((332, 3764, 2180, 6012), (316, 3780, 2164, 6028))
_add("stays_at_4", 4, (4096, 8192), [(16, 348, 2196, 57), (16, 348, 2196, 58)], extent=(3400, 3800), old_waves=4)
