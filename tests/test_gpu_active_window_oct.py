"""GPU tests of the octagonal support of windowed passes: every row of tests/active_window_oct_cases.py.

Away from the frame the fields spread one cell per step in L1 distance, so a window also has diagonal bounds, and the
(band, strip) tasks of a windowed launch that lie wholly outside them return at once (strip_of_block).  Per row, after
every segment: every cell of Ez, Hx and Hy against the C oracle by np.array_equal (the exact build against the oracle's
exact arithmetic, the fused build against its fused arithmetic); zeros outside the rectangle and outside the bounds; the
bounds and the number of skipped tasks the library reports (Engine.last_window_octagon) against the restated rules; and
the pinned values of Engine.last_window_launch, which the bounds must not change.  tests/test_active_window_oct_cases_cpu.py
proves that the oracle's field touches the bounds in every row, so a task skipped wrongly leaves zeros where the oracle
has none.  Once per row the same run with window_octagon=0 (nothing skipped, same launch, same arrays) and with
active_window=0."""
import numpy as np
import pytest

import active_window_oct_cases as oc

pytestmark = pytest.mark.gpu

LAUNCH_KEYS = ("band_rows", "edge_rows", "waves", "strip_first", "inner", "n_src", "edges", "ztop", "zbot", "xcd_map", "xcd_pad")


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _engine(fd, row, **over):
    r, c = row["shape"]
    eng = fd.Engine(r, c, oc.DT, oc.DX, dtype=np.dtype(row["dtype"]))
    eps, mu = oc.materials(row)
    eng.set_materials(eps, mu, allow_uniform=row["kind"] == "vacuum")
    eng.set_option(**dict(row["options"], **over))
    if row["set_shape"]:
        eng.set_shape(row["set_shape"])
    eng.set_source_extent(*row["extent"])
    return eng


def _do(eng, row, seg):
    if seg[0] == "add_point":
        eng.add_point(seg[1], seg[2], seg[3])
    elif seg[0] == "copy":
        assert eng.measure_copy(1) > 0
    else:
        steps, r, c, seed = seg
        eng.run(steps, r, c, None if seed is None else oc.amps_of(row, steps, seed))


def _assert_equal(name, got, ref, what):
    for a, b, k in zip(got, ref, oc.NAMES):
        if a.dtype == b.dtype and np.array_equal(a, b):
            continue
        bad = np.argwhere(a != b)
        box = (bad[:, 0].min(), bad[:, 0].max() + 1, bad[:, 1].min(), bad[:, 1].max() + 1)
        raise AssertionError(f"{name} {what}: {k} differs in {len(bad)} cells inside {box}; first: {bad[:4].tolist()}")


def _told(eng):
    t = eng.last_window_octagon
    return (t["sum_lo"], t["sum_hi"], t["diff_lo"], t["diff_hi"]), t["skipped"]


@pytest.mark.parametrize("name", [r["name"] for r in oc.ROWS])
def test_octagon(fd, name):
    row = oc.by_name(name)
    sim = oc.simulate(row)
    ref = oc.reference(name, fused=fd._abi.ARITHMETIC == "fused")
    launches = []
    with _engine(fd, row) as eng:
        eng.reset()
        assert eng.active_window == (0, 0, 0, 0) and eng.window_enabled
        for k, (seg, want, state) in enumerate(zip(row["segments"], sim, ref)):
            _do(eng, row, seg)
            what = f"after segment {k} {seg[:4]}"
            got = eng.download()
            if want["launches"]:
                last = want["launches"][-1]
                told, bounds = eng.last_window_launch, _told(eng)
                launches.append(told)
                print(name, what, "launched", told, "bounds", bounds, "of", len(last["tasks"]), "tasks")
                for key in LAUNCH_KEYS:
                    if last[key] is not None:
                        assert told[key] == last[key], f"{what}: {key} {told[key]}, the rules give {last[key]}"
                assert bounds == (last["oct"], len(last["skipped"])), f"{what}: the rules give {last['oct']}, {len(last['skipped'])}"
            assert eng.active_window == want["window"], what
            assert eng.windowed_launches == want["windowed"], what
            r0, r1, c0, c1 = want["window"]
            zero = ~oc.inside(want["oct"], row["shape"])
            zero[:r0], zero[r1:], zero[:, :c0], zero[:, c1:] = True, True, True, True
            for a, f in zip(got, oc.NAMES):
                assert not a[zero[:a.shape[0], :a.shape[1]]].any(), f"{f} {what}: non-zero outside the octagon"
            _assert_equal(name, got, state, what)
    if row["skips"]:
        assert sum(len(l["skipped"]) for s in sim for l in s["launches"]) > 0
    # the same run on the rectangle alone: nothing skipped, the same launch, the same arrays
    plain = []
    with _engine(fd, row, window_octagon=0) as eng:
        eng.reset()
        for seg, want in zip(row["segments"], sim):
            _do(eng, row, seg)
            if want["launches"]:
                plain.append(eng.last_window_launch)
                assert _told(eng) == (oc.UNBOUNDED, 0)
        rect = eng.download()
    assert plain == launches
    _assert_equal(name, rect, got, "window_octagon=0 against the default")
    # ... and without the window
    with _engine(fd, row, active_window=0) as eng:
        eng.reset()
        for seg in row["segments"]:
            _do(eng, row, seg)
        assert eng.windowed_launches == 0 and not eng.window_enabled
        dense = eng.download()
    _assert_equal(name, dense, got, "active_window=0 against the windowed run")
