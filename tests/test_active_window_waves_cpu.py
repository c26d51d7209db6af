"""CPU-only: the rows of tests/active_window_waves_cases.py are what they are listed for, from the oracle and the restated
rules alone -- so that tests/test_gpu_active_window_waves.py compares non-zero cells where it claims to, on launches
whose waves the two quantities (launched cells, rows x grid columns) decide as the table says."""
import os

import pytest

import active_window_cases as awc
import active_window_waves_cases as wvc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [r["name"] for r in wvc.ROWS]


def test_the_rule_is_where_the_table_restates_it():
    pi = open(os.path.join(ROOT, "fdtd-2d_amd", "csrc", "pass_impl.hpp")).read()
    assert "(long long)(win->n_inner + (win->edges ? 2 : 0)) * OW" in pi
    assert "h->shape_now.waves = cells < (nt == 16 ? (size_t)12 << 20 : (size_t)3 << 20) ? 8 : 4;" in pi
    assert wvc.threshold(16) == 12 << 20 and wvc.threshold(8) == 3 << 20


@pytest.mark.parametrize("name", IDS)
def test_waves_by_either_quantity(name):
    """Every windowed pass: the waves the new rule gives, what the old quantity gave, and the band height that follows."""
    row = wvc.by_name(name)
    n = 0
    for s in wvc.simulate(row):
        assert s["dense"] == 0 and len(s["launches"]) == len(s["windows"]) > 0
        for l in s["launches"]:
            print(name, "nt", l["nt"], "rows", l["band_hi"] - l["band_lo"], "launched cells", l["cells"], "rows x grid columns",
                  l["old_cells"], "waves", l["waves"], "before", l["old_waves"], "band rows", l["band_rows"])
            assert l["waves"] == row["waves"]
            n += 1
            if row["old_waves"] is None:         # waves given by the caller
                continue
            assert l["old_waves"] == row["old_waves"] and l["old_cells"] >= wvc.threshold(l["nt"])
            assert (l["cells"] < wvc.threshold(l["nt"])) == (row["waves"] == 8)
            ns = l["inner"] + 2 * l["edges"]
            assert l["band_rows"] == awc.window_band_rows(l["band_hi"] - l["band_lo"], row["waves"], ns, True)
    assert n == len(row["segments"]), "one pass per segment, so that the GPU test reads every launch back"


def test_stays_at_4_windows():
    """The two windows as the table states them: at least 6 cells from every edge, at least 12 Mi cells, under half the grid."""
    row = wvc.by_name("stays_at_4")
    R, C = row["shape"]
    wins = [w for s in wvc.simulate(row) for w in s["windows"]]
    assert tuple(wins) == wvc.STAYS_4_WINDOWS
    assert [awc.cells(w) for w in wins] == [3432 * 3832, 3464 * 3864]
    for w in wins:
        assert min(w[0], R - w[1], w[2], C - w[3]) >= awc.MARGIN
        assert 12 << 20 <= awc.cells(w) and 2 * awc.cells(w) <= R * C


@pytest.mark.parametrize("name", IDS)
def test_fill_condition(name):
    """After every segment the oracle's non-zero bounding box comes within one cell of every free side of the window."""
    row = wvc.by_name(name)
    R, C = row["shape"]
    for k, (s, state) in enumerate(zip(wvc.simulate(row), wvc.reference(name))):
        win, box = s["window"], awc.support_box(state)
        print(name, "segment", k, "window", win, "non-zero box", box)
        assert box is not None
        assert win[0] <= box[0] and box[1] <= win[1] and win[2] <= box[2] and box[3] <= win[3], "the oracle leaves the window"
        for i, (v, edge) in enumerate(zip(win, (0, R, 0, C))):
            if v != edge:
                assert abs(box[i] - v) <= 1, f"segment {k}: side {i} of the window at {v}, the field reaches {box[i]}"
        for W in s["windows"]:
            assert 2 * awc.cells(W) <= R * C
