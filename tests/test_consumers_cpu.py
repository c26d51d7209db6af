"""The probe-case table of tests/test_gpu_consumers.py and CPU-only checks of it.

The single-grid Engine records a point probe inside a temporally blocked pass with one extra workgroup, k_probe<T, NT,
CE_ARR, CH_ARR>: a (4 NT + 5)^2 tile around the probe cell, clipped to the grid, advanced NT steps.  Where that kernel can
go wrong depends on four things a case decides: which sides the clip cuts, which rule of the Mur frame the probe cell
itself obeys, whether the source rectangle covers the cell, and which instance runs.  CASES lists single-grid runs; this
module restates, in plain Python and independently of the product code,
  * the tile's clip (M = 2 NT + 2),
  * the Mur class of a cell (oracle/fdtd_numpy.py update_e: 5-cell bands, 5 x 5 corner blocks, the outermost row / column),
  * the pass length a case runs on (cycle_steps: 16 for float32, 8 for float64 while a probe is set, min(max_pass_steps, 8)
    below 16) and the passes fdtd2d_run plans for n steps (plan_pass),
  * pass_geometry's size rule (rows >= 2 (2 nt + 6), cols >= 16),
and asserts that the table as a whole reaches every Mur class, every clip side, both column sides at once, all four
material instances, NT in {1, 2, 4, 8, 16} for float32 and {1, 2, 4, 8} for float64 (float64 has no 16-step probe tile:
its LDS tile would not fit, the engine stays with 8-step passes while a probe is set), and a probe cell inside the
source rectangle.  Every length is reachable through set_option(max_pass_steps=...)."""
from collections import namedtuple

import pytest

BAND = 5
STEPS, LEAD = 45, 3                 # steps of a case; the probe is set after LEAD of them
MATERIALS = ("uniform", "eps", "mu", "both")            # which of eps / mu is an array (CE_ARR, CH_ARR)
SOURCE = {(130, 470): (60, 230, 4, 12), (76, 64): (36, 29, 4, 6), (44, 48): (20, 22, 3, 5)}     # row, col, rows, cols

Case = namedtuple("Case", "R C dtype materials max_pass_steps row col source")

# 130 x 470: crosses a strip seam and the side bands (the grid of test_probe_time_series_matches_oracle, which covers
# (0, 0), the left and top bands next to it and the interior); 76 x 64: the smallest grid with 16-step passes, narrower
# than their 69-cell tile
_BIG = [
    (76, 64, "f32", "both", 16, 38, 31),        # interior, in the source, clipped left and right at once
    (76, 64, "f32", "mu", 16, 75, 63),
    (76, 64, "f32", "uniform", 16, 0, 63),
    (76, 64, "f32", "eps", 16, 75, 0),
    (76, 64, "f32", "eps", 16, 75, 30),
    (76, 64, "f32", "mu", 16, 40, 63),
    (76, 64, "f32", "uniform", 16, 73, 20),
    (76, 64, "f32", "both", 16, 30, 61),
    (76, 64, "f32", "mu", 16, 2, 33),
    (76, 64, "f32", "uniform", 16, 40, 2),
    (76, 64, "f32", "both", 16, 0, 30),
    (76, 64, "f32", "eps", 8, 38, 0),
    (130, 470, "f64", "eps", 16, 129, 469),
    (130, 470, "f32", "mu", 16, 0, 469),
    (130, 470, "f64", "both", 16, 129, 0),
    (130, 470, "f32", "both", 16, 2, 2),
    (130, 470, "f32", "eps", 16, 127, 300),
    (130, 470, "f64", "mu", 16, 60, 467),
    (130, 470, "f32", "both", 16, 129, 200),
    (130, 470, "f32", "uniform", 16, 64, 469),
    (130, 470, "f64", "uniform", 16, 0, 100),
    (130, 470, "f32", "eps", 16, 70, 0),
    (130, 470, "f32", "eps", 16, 62, 233),      # in the source
    (130, 470, "f64", "mu", 16, 62, 233),
    (130, 470, "f32", "mu", 8, 2, 250),
    (130, 470, "f64", "both", 8, 64, 2),
]
# 44 x 48: the smallest grid with 8-step passes; every class of cell at 1-, 2-, 4- and 8-step passes in turn
_SMALL_CELLS = [(21, 24), (43, 47), (0, 47), (43, 0), (2, 2), (41, 20), (20, 45), (3, 20), (20, 3), (43, 20), (20, 47),
                (0, 20), (20, 0)]


def _cases():
    out = [Case(*row, SOURCE[row[0], row[1]]) for row in _BIG]
    for k, (i, j) in enumerate(_SMALL_CELLS):
        for d, dtype in enumerate(("f32", "f64")):
            out.append(Case(44, 48, dtype, MATERIALS[(k + 2 * d + k // 4) % 4], (1, 2, 4, 8)[(k + d) % 4], i, j,
                            SOURCE[44, 48]))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.R}x{c.C}-{c.dtype}-{c.materials}-max{c.max_pass_steps}-{c.row}_{c.col}"


# ---- the rules, restated ---------------------------------------------------------------------------------------------------

def cycle_steps(dtype, max_pass_steps, probe=True):
    """Longest pass of a Mur engine whose max_pass_steps option was set (the option lifts the size rule)."""
    if max_pass_steps >= 16 and (dtype == "f32" or not probe):
        return 16
    return min(max_pass_steps, 8)


def planned_passes(n, cycle):
    """(kernel length, levels advanced) of the passes fdtd2d_run(n) plans on a grid large enough for `cycle`: full passes
    while more than two remain, a remainder between one and two passes in halves, a remainder of at most one pass on the
    shortest kernel that holds it -- short passes exist for the level-split kernels (8 and 16 steps) only, else the longest
    full pass below it."""
    out, lens = [], [c for c in (1, 2, 4, 8, 16) if c <= cycle]
    while n > 0 and lens:
        take = cycle if n > 2 * cycle else (n + 1) // 2 if n > cycle else n
        fit = [c for c in lens if c >= take and (c == take or c >= 8)]
        nt, lev = (fit[0], take) if fit else (max(c for c in lens if c < take),) * 2
        out.append((nt, lev))
        n -= lev
    return out


def pass_fits(R, C, nt):
    return R >= 2 * (2 * nt + 6) and C >= 16


def tile_clip(c, nt):
    m = 2 * nt + 2
    return {"top": c.row - m < 0, "bottom": c.row + m + 1 > c.R, "left": c.col - m < 0, "right": c.col + m + 1 > c.C}


def mur_class(R, C, i, j):
    top, bottom, left, right = i < BAND, i >= R - BAND, j < BAND, j >= C - BAND
    if (top or bottom) and (left or right):
        return "corner_" + ("t" if top else "b") + ("l" if left else "r")
    if i == 0 or i == R - 1:
        return "edge_row_" + ("top" if top else "bottom")
    if j == 0 or j == C - 1:
        return "edge_col_" + ("left" if left else "right")
    for hit, name in ((top, "top"), (bottom, "bottom"), (left, "left"), (right, "right")):
        if hit:
            return "band_" + name
    return "interior"


def in_source(c):
    r, q, nr, nc = c.source
    return r <= c.row < r + nr and q <= c.col < q + nc


def instance(c):
    """(NT values of the probe tiles the run launches, CE_ARR, CH_ARR)."""
    nts = {nt for nt, _ in planned_passes(STEPS - LEAD, cycle_steps(c.dtype, c.max_pass_steps))}
    return nts, c.materials in ("eps", "both"), c.materials in ("mu", "both")


MUR_CLASSES = {"interior", "band_top", "band_bottom", "band_left", "band_right", "corner_tl", "corner_tr", "corner_bl",
               "corner_br", "edge_row_top", "edge_row_bottom", "edge_col_left", "edge_col_right"}


# ---- the table against the rules --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_row_is_inside_its_grid_and_large_enough_for_its_passes(c):
    assert 0 <= c.row < c.R and 0 <= c.col < c.C
    r, q, nr, nc = c.source
    assert 0 <= r and r + nr <= c.R and 0 <= q and q + nc <= c.C and nr * nc > 1
    cyc = cycle_steps(c.dtype, c.max_pass_steps)
    assert cyc in (1, 2, 4, 8, 16)
    plan = planned_passes(STEPS - LEAD, cyc)
    assert sum(lev for _, lev in plan) == STEPS - LEAD and plan[0] == (cyc, cyc)
    for nt, lev in plan + planned_passes(LEAD, cyc):
        assert pass_fits(c.R, c.C, nt) and 1 <= lev <= nt <= cyc


def test_plan_restated():
    assert planned_passes(42, 16) == [(16, 16), (16, 13), (16, 13)]
    assert planned_passes(42, 8) == [(8, 8)] * 4 + [(8, 5), (8, 5)]
    assert planned_passes(42, 4) == [(4, 4)] * 9 + [(2, 2), (4, 4)]
    assert planned_passes(42, 2) == [(2, 2)] * 21 and planned_passes(42, 1) == [(1, 1)] * 42
    assert planned_passes(3, 16) == [(8, 3)] and planned_passes(3, 4) == [(2, 2), (1, 1)]
    assert planned_passes(5, 0) == []
    assert [planned_passes(n, 16) for n in (16, 5, 21)] == [[(16, 16)], [(8, 5)], [(16, 11), (16, 10)]]


def test_table_reaches_every_mur_class_clip_side_instance_and_pass_length():
    classes = {mur_class(c.R, c.C, c.row, c.col) for c in CASES}
    assert classes == MUR_CLASSES
    reached = {"f32": set(), "f64": set()}
    clips, both_columns, mats = set(), False, set()
    for c in CASES:
        nts, ce, ch = instance(c)
        reached[c.dtype] |= nts
        mats.add((ce, ch))
        clip = tile_clip(c, max(nts))
        clips |= {side for side, hit in clip.items() if hit}
        both_columns |= clip["left"] and clip["right"]
    assert reached == {"f32": {1, 2, 4, 8, 16}, "f64": {1, 2, 4, 8}}
    assert clips == {"top", "bottom", "left", "right"} and both_columns
    assert mats == {(False, False), (True, False), (False, True), (True, True)}
    assert any(in_source(c) for c in CASES) and not all(in_source(c) for c in CASES)
    # per dtype too: every class and every instance, and an unclipped tile (the 130 x 470 interior rows)
    for dtype in ("f32", "f64"):
        rows = [c for c in CASES if c.dtype == dtype]
        assert {mur_class(c.R, c.C, c.row, c.col) for c in rows} == MUR_CLASSES
        assert {instance(c)[1:] for c in rows} == mats
        assert any(in_source(c) for c in rows)
        assert any(not any(tile_clip(c, max(instance(c)[0])).values()) for c in rows)
    # the 16-step tile at every class that has a side of its own, and each corner
    long_rows = {mur_class(c.R, c.C, c.row, c.col) for c in CASES if 16 in instance(c)[0]}
    assert long_rows == MUR_CLASSES
    assert len({case_id(c) for c in CASES}) == len(CASES)


def test_mur_class_restated_against_the_oracle_stages():
    """The class of a cell = the last stage of the oracle's E half-step that writes it."""
    import numpy as np
    R, C, b = 23, 31, BAND
    last = np.full((R, C), "none", dtype=object)
    last[1:-1, 1:-1] = "interior"
    last[1:-1, 0:b], last[1:-1, -b:] = "left", "right"
    last[0:b, 1:-1], last[-b:, 1:-1] = "top", "bottom"
    last[0:b, 0:b], last[0:b, -b:], last[-b:, 0:b], last[-b:, -b:] = "corner_tl", "corner_tr", "corner_bl", "corner_br"
    for i in range(R):
        for j in range(C):
            cls = mur_class(R, C, i, j)
            want = cls.replace("band_", "").replace("edge_row_", "").replace("edge_col_", "")
            assert last[i, j] == want, (i, j, cls)
            assert cls.startswith("edge") == ((i in (0, R - 1) or j in (0, C - 1)) and not cls.startswith("corner"))
