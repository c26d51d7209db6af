"""GPU tests of the waves per strip of windowed passes: every row of tests/active_window_waves_cases.py.

A window with no waves given runs 8 waves per strip while the cells its launch covers stay below the size threshold of
its pass length, whatever the grid's width; the caller's waves (split_waves, a given shape) still win; a window whose
launch is at or above the threshold keeps 4.  tests/test_active_window_waves_cpu.py proves from the oracle alone that
the field fills every asserted window.

Per row, after every segment (one pass each): what the pass launched (Engine.last_window_launch: the waves, and the band
height that follows from them) against the restated rules, the window, the pass counts, zeros outside the window, and
every cell of Ez, Hx and Hy against the C oracle by np.array_equal (the fused build against its fused arithmetic).  Once
per row the same run with active_window=0 has to give the same arrays."""
import numpy as np
import pytest

import active_window_cases as awc
import active_window_waves_cases as wvc

pytestmark = pytest.mark.gpu

INFO_PASSES = 16
LAUNCH_KEYS = ("band_rows", "edge_rows", "waves", "strip_first", "inner", "n_src", "edges", "ztop", "zbot", "xcd_map", "xcd_pad")


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _engine(fd, row, **over):
    r, c = row["shape"]
    eng = fd.Engine(r, c, awc.DT, awc.DX, dtype=np.dtype(row["dtype"]))
    eps, mu = awc.materials(row)
    eng.set_materials(eps, mu, allow_uniform=True)
    eng.set_option(**dict(row["options"], **over))
    if row["set_shape"]:
        eng.set_shape(row["set_shape"])
    eng.set_source_extent(*row["extent"])
    return eng


def _run(eng, row, seg):
    steps, r, c, seed = seg
    eng.run(steps, r, c, awc.amps_of(row, steps, seed))


def _assert_equal(name, got, ref, what):
    for a, b, k in zip(got, ref, awc.NAMES):
        if a.dtype == b.dtype and np.array_equal(a, b):
            continue
        bad = np.argwhere(a != b)
        box = (bad[:, 0].min(), bad[:, 0].max() + 1, bad[:, 1].min(), bad[:, 1].max() + 1)
        raise AssertionError(f"{name} {what}: {k} differs in {len(bad)} cells inside {box}; first: {bad[:4].tolist()}")


@pytest.mark.parametrize("name", [r["name"] for r in wvc.ROWS])
def test_waves_of_a_window(fd, name):
    row = wvc.by_name(name)
    sim = wvc.simulate(row)
    ref = wvc.reference(name, fused=fd._abi.ARITHMETIC == "fused")
    with _engine(fd, row) as eng:
        eng.reset()
        assert eng.active_window == (0, 0, 0, 0) and eng.window_enabled
        for k, (seg, want, state) in enumerate(zip(row["segments"], sim, ref)):
            _run(eng, row, seg)
            what = f"after segment {k} {seg}"
            (launch,) = want["launches"]
            told = eng.last_window_launch
            print(name, what, "launched", told, "cells", launch["cells"], "rows x grid columns", launch["old_cells"])
            assert told["waves"] == row["waves"] == launch["waves"], what
            for key in LAUNCH_KEYS:
                if launch[key] is not None:
                    assert told[key] == launch[key], f"{what}: {key} {told[key]}, the rules give {launch[key]}"
            assert eng.active_window == want["window"], what
            assert (eng.info(INFO_PASSES), eng.windowed_launches) == (want["passes"], want["windowed"]), what
            got = eng.download()
            r0, r1, c0, c1 = want["window"]
            for a, f in zip(got, awc.NAMES):
                assert not a[:r0].any() and not a[r1:].any() and not a[:, :c0].any() and not a[:, c1:].any(), \
                    f"{f} {what}: non-zero outside the reported window {want['window']}"
            _assert_equal(name, got, state, what)
    # the same run without the window
    with _engine(fd, row, active_window=0) as eng:
        eng.reset()
        for seg in row["segments"]:
            _run(eng, row, seg)
        assert eng.windowed_launches == 0 and not eng.window_enabled
        dense = eng.download()
    _assert_equal(name, dense, ref[-1], "active_window=0 against the oracle")
