"""CPU-only: every row of tests/active_window_cases.py keeps what it is listed for, from the oracle and the restated rules
alone -- so that tests/test_gpu_active_window_filled.py compares non-zero cells where it claims to.

Per row: the FILL CONDITION (after every segment the oracle's non-zero bounding box over Ez, Hx and Hy comes within one
cell of every side of the expected window that is not a grid edge; the one missing cell is the last step's injection,
which has not spread yet), the half-grid cap for every pass meant to launch a window, and the listed property."""
import os
import re

import numpy as np
import pytest

import active_window_cases as awc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fdtd-2d_amd", "csrc")
IDS = [r["name"] for r in awc.ROWS]


def test_restated_constants_are_the_library_s():
    """MARGIN, the strip geometry and the band rule as the sources state them."""
    aw = open(os.path.join(CSRC, "active_window.hpp")).read()
    assert re.search(r"constexpr int MARGIN = (\d+);", aw).group(1) == str(awc.MARGIN)
    ks = open(os.path.join(CSRC, "kernels_stream.hpp")).read()
    assert "constexpr int stream_hc(int nt) { return nt <= 4 ? 4 : (nt <= 8 ? 8 : (nt <= 16 ? 16 : 20)); }" in ks
    pi = open(os.path.join(CSRC, "pass_impl.hpp")).read()
    assert "const int slots = split4 ? 256 * 16 / nw * 9 / 10 : 3072;" in pi
    assert "br = std::min(std::max((region + per - 1) / per, 32), 448);" in pi
    # float32 16-step strips write 224 columns, float64 96; the 8- and 20-step widths follow from stream_hc
    assert [awc.strip_ow(awc.F32, nt) for nt in (8, 16, 20)] == [240, 224, 216]
    assert [awc.strip_ow(awc.F64, nt) for nt in (8, 16)] == [112, 96]
    assert awc.window_band_rows(257, 8, 3, True) == 32 and awc.window_band_rows(7364, 8, 2, True) == 33
    assert awc.window_band_rows(7360, 8, 2, True) == 32 and awc.window_band_rows(10 ** 6, 4, 1, True) == 448
    assert abs(awc.DT * awc.C0 / awc.DX - 0.65) < 1e-15


def test_restated_grow_and_restrict_launch():
    g = awc.grow
    assert g((37, 38, 38, 39), 32, 300, 1000) == (0, 70, 6, 71)             # index 5 snaps, index 6 stays
    assert g((262, 263, 961, 962), 32, 300, 1000) == (230, 300, 929, 994)
    assert g((261, 262, 962, 963), 32, 300, 1000) == (229, 294, 930, 1000)
    assert g(None, 16, 300, 1000) is None and g((10, 5, 0, 1), 3, 300, 1000) is None
    L = awc.restrict_launch((100, 200, 448, 672), None, 300, 1000, 16, 224, 16, 5)
    assert (L["strip_first"], L["inner"], L["edges"], L["ztop"], L["zbot"], L["band_lo"], L["band_hi"]) == (2, 1, 0, 0, 0, 100, 200)
    L = awc.restrict_launch((36, 264, 447, 673), None, 300, 1000, 16, 224, 16, 5)
    assert (L["strip_first"], L["inner"], L["edges"], L["ztop"], L["zbot"], L["band_lo"], L["band_hi"]) == (1, 3, 1, 1, 1, 21, 279)
    L = awc.restrict_launch((37, 263, 0, 100), None, 300, 1000, 16, 224, 16, 5)
    assert (L["strip_first"], L["inner"], L["edges"], L["ztop"], L["zbot"]) == (1, 0, 1, 0, 0)
    # a source widens the run by the strips that hold its columns
    L = awc.restrict_launch((140, 160, 660, 670), (150, 151, 665, 666), 300, 1000, 16, 224, 16, 5)
    assert (L["strip_first"], L["inner"]) == (2, 2)


def _sides(win, shape):
    """(index into a (r0, r1, c0, c1) box, value) of the sides that are not grid edges."""
    R, C = shape
    return [(k, v) for k, (v, edge) in enumerate(zip(win, (0, R, 0, C))) if v != edge]


@pytest.mark.parametrize("name", IDS)
def test_fill_condition_and_half_grid_cap(name):
    row = awc.by_name(name)
    sim = awc.simulate(row)
    ref = awc.reference(name)
    R, C = row["shape"]
    after_upload = False
    for k, (seg, s, state) in enumerate(zip(row["segments"], sim, ref["states"])):
        win = s["window"]
        box = awc.support_box(state)
        print(name, "segment", k, seg[:4], "window", win, "non-zero box", box, "windowed", s["windowed"], "dense", s["dense"])
        if seg[0] == "upload":
            after_upload = True
        if seg[0] == "reset":
            assert win == (0, 0, 0, 0) and box is None
            after_upload = False
            continue
        assert box is not None
        assert win[0] <= box[0] and box[1] <= win[1] and win[2] <= box[2] and box[3] <= win[3], "the oracle leaves the window"
        for i, v in _sides(win, row["shape"]):
            assert abs(box[i] - v) <= 1, f"segment {k}: side {i} of the window at {v}, the field reaches {box[i]}"
        # every pass of a run() from a tracked state launches a window: 2 |W| <= R C
        if isinstance(seg[0], int):
            if after_upload:
                assert s["dense"] > 0 and not s["launches"]
            else:
                assert s["dense"] == 0 and len(s["launches"]) == len(s["windows"]) > 0
                for W in s["windows"]:
                    assert 2 * awc.cells(W) <= R * C


@pytest.mark.parametrize("name", IDS)
def test_listed_property(name):
    row = awc.by_name(name)
    sim = awc.simulate(row)
    prop = dict(row["prop"])
    last = [s for s in sim if s["launches"]][-1]["launches"][-1]
    every = [l for s in sim for l in s["launches"]]
    print(name, "last windowed launch", last)
    assert sim[-1]["passes"] == prop.pop("passes", sim[-1]["passes"])
    for key in ("band_rows", "edge_rows", "waves", "strip_first", "inner", "n_src", "edges", "ztop", "zbot", "xcd_map", "xcd_pad"):
        if key in prop:
            assert last[key] == prop.pop(key), key
    if "strips_min" in prop:
        assert last["inner"] >= prop.pop("strips_min")
    if "strip_first_min" in prop:
        assert last["strip_first"] >= prop.pop("strip_first_min")
    if "bands_min" in prop:
        assert last["nbands"] >= prop.pop("bands_min")
    if "last_band_rows" in prop:
        assert (last["band_hi"] - last["band_lo"]) - (last["nbands"] - 1) * last["band_rows"] == prop.pop("last_band_rows") >= 16
    if "tasks_mod8" in prop:
        assert (last["nbands"] * last["main"]) % 8 == prop.pop("tasks_mod8") != 0
    if "short_tail" in prop:
        prop.pop("short_tail")
        assert every[-1]["nlev"] < every[-1]["nt"]
    if "last_nt" in prop:
        assert every[-1]["nt"] == prop.pop("last_nt")
    for i, key in enumerate(("r0", "r1", "c0", "c1")):
        if key in prop:
            assert sim[-1]["window"][i] == prop.pop(key), key
    if "mid_window" in prop:
        assert sim[0]["window"] == prop.pop("mid_window")
        assert sim[1]["launches"][-1]["ztop"] + sim[1]["launches"][-1]["zbot"] + sim[1]["launches"][-1]["edges"] >= 2
    if "dense_after_upload" in prop:
        prop.pop("dense_after_upload")
        assert sim[-1]["dense"] > 0 and sim[-1]["window"] == (0,) + (row["shape"][0], 0, row["shape"][1])
    assert not prop, f"unchecked properties {prop}"


def test_the_table_covers_what_it_is_for():
    """Across the table: every option of a windowed launch, both element types, all three pass lengths, one zone side
    alone each way, a run of inner strips that starts beyond strip 1 with three or more strips."""
    every = [(r, l) for r in awc.ROWS for s in awc.simulate(r) for l in s["launches"]]
    assert {l["nt"] for _, l in every} == {8, 16, 20}
    assert {l["waves"] for _, l in every} == {1, 4, 8}
    assert {(l["ztop"], l["zbot"]) for _, l in every} >= {(0, 0), (1, 0), (0, 1)}
    assert any(l["strip_first"] > 1 and l["inner"] >= 3 for _, l in every)
    assert {l["n_src"] for _, l in every} == {0, 1, 2}
    assert any(l["xcd_map"] and l["xcd_pad"] for _, l in every)
    assert any(l["band_rows"] > 32 and "band_rows" not in r["options"] and not r["set_shape"] for r, l in every)
    assert any(l["edge_rows"] != l["band_rows"] and l["edges"] for _, l in every)
    assert any(r["options"].get("zone_split") == 1 and l["ztop"] for r, l in every)
    assert {r["dtype"] for r in awc.ROWS} == {awc.F32, awc.F64}
    assert not any("band_rows" in r["options"] for r in awc.ROWS if r["name"].startswith("fill_"))


def test_window_launch_info_ids_are_declared_and_bound():
    """FDTD2D_INFO_WIN_* (31 .. 41): read-only, behind the ids of the window itself, named in the binding and by
    Engine.last_window_launch in the header's order."""
    import inspect
    from fdtd2d_amd import _abi, engine
    txt = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"#define\s+FDTD2D_INFO_(WIN_\w+)\s+(\d+)", txt)}
    assert sorted(ids.values()) == list(range(31, 42))
    for k, v in ids.items():
        assert getattr(_abi, "INFO_" + k) == v, k
    every = [int(v) for v in re.findall(r"#define\s+FDTD2D_INFO_\w+\s+(\d+)", txt)]
    assert sorted(every) == list(range(42))                      # no id taken twice, none left out
    src = inspect.getsource(engine.Engine.last_window_launch.fget)
    keys = re.findall(r'"(\w+)"', src.split("keys = ")[1].split(")")[0])
    assert ["WIN_" + k.upper() for k in keys] == sorted(ids, key=ids.get)
