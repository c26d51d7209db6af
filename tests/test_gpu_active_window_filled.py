"""GPU tests of the active window where the field fills it: every row of tests/active_window_cases.py (Courant number 0.65,
materials at or near vacuum, amplitudes scaled so that float32 does not underflow before the front arrives).

tests/test_gpu_active_window.py runs at a Courant number of 0.15, where the outer part of every window holds zeros: what
a restricted launch does there is invisible.  Here tests/test_active_window_cases_cpu.py proves per row that the oracle's
non-zero cells come within one cell of every free side of the window, so a dropped band, a run of strips that starts one
late, a skipped zone tile or a stale target cell changes cells this module compares.

Per row, after every segment: every cell of Ez, Hx and Hy against the C oracle by np.array_equal (the exact build against
the oracle's exact arithmetic, the fused build -- FDTD2D_ARITHMETIC=fused -- against its fused arithmetic: the oracle has
arrays, and line sources are added between its half steps, so no row falls back to the library's own dense run); the
reported window, the pass count and the windowed launches against the restated rules; zeros outside the window; and what
the last windowed pass launched (Engine.last_window_launch) against what the rules predict.  Once per row the same run
with active_window=0 has to give the same arrays."""
import numpy as np
import pytest

import active_window_cases as awc

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
    eng.set_materials(eps, mu, allow_uniform=row["kind"] == "vacuum")
    eng.set_option(**dict(row["options"], **over))
    if row["set_shape"]:
        eng.set_shape(row["set_shape"])
    eng.set_source_extent(*row["extent"])
    return eng


def _do(eng, row, seg):
    if seg[0] == "reset":
        eng.reset()
    elif seg[0] == "upload":
        eng.upload(*eng.download())
    elif seg[0] == "point":
        eng.add_point(seg[1], seg[2], seg[3])
        eng.update_h()
        eng.update_e()
    elif seg[0] == "time_launches":
        assert len(eng.time_launches(seg[1], seg[2])) == seg[1]
    else:
        steps, r, c, seed = seg
        eng.run(steps, r, c, None if seed is None else awc.amps_of(row, steps, seed))


def _where(row, launch, cell):
    """The part of the launch a cell falls in: zone or band, and the strip that writes its column."""
    i, j = cell
    ow = awc.strip_ow(row["dtype"], launch["nt"])
    if i < launch["band_lo"]:
        part = "top zone" if launch["ztop"] else "above the bands"
    elif i >= launch["band_hi"]:
        part = "bottom zone" if launch["zbot"] else "below the bands"
    else:
        part = f"band {(i - launch['band_lo']) // launch['band_rows']} of {launch['band_rows']} rows"
    return f"({i}, {j}): {part}, strip {j // ow} (run {launch['strip_first']} + {launch['inner']}, edges {launch['edges']})"


def _assert_equal(row, got, ref, launch, what):
    for a, b, k in zip(got, ref, awc.NAMES):
        if a.dtype == b.dtype and np.array_equal(a, b):
            continue
        bad = np.argwhere(a != b)
        box = (bad[:, 0].min(), bad[:, 0].max() + 1, bad[:, 1].min(), bad[:, 1].max() + 1)
        first = "; ".join(_where(row, launch, tuple(int(v) for v in c)) for c in bad[:4]) if launch else bad[:4].tolist()
        raise AssertionError(f"{row['name']} {what}: {k} differs in {len(bad)} cells inside {box}; first: {first}")


def _assert_zero_outside(got, win, what):
    r0, r1, c0, c1 = win
    for a, k in zip(got, awc.NAMES):
        m = np.ones(a.shape, bool)
        m[r0:r1, c0:c1] = False
        assert not a[m].any(), f"{k} {what}: non-zero outside the reported window {win}"


@pytest.mark.parametrize("name", [r["name"] for r in awc.ROWS])
def test_filled_window(fd, name):
    row = awc.by_name(name)
    sim = awc.simulate(row)
    ref = awc.reference(name, fused=fd._abi.ARITHMETIC == "fused")
    nsteps = sum(s[0] for s in row["segments"] if isinstance(s[0], int))
    launch = None
    with _engine(fd, row) as eng:
        eng.reset()
        assert eng.active_window == (0, 0, 0, 0) and eng.window_enabled
        if row["probe"]:
            eng.set_probe(*row["probe"], nsteps)
        if row["dft"]:
            eng.set_dft(row["dft"]["window"], np.array(row["dft"]["omega"]), row["dft"]["every"])
        for k, (seg, want, state) in enumerate(zip(row["segments"], sim, ref["states"])):
            _do(eng, row, seg)
            what = f"after segment {k} {seg[:4]}"
            got = eng.download()
            if want["launches"]:
                launch = want["launches"][-1]
                told = eng.last_window_launch
                print(name, what, "launched", told)
                for key in LAUNCH_KEYS:
                    if launch[key] is not None:
                        assert told[key] == launch[key], f"{what}: {key} {told[key]}, the rules give {launch[key]}"
            assert eng.active_window == want["window"], what
            assert (eng.info(INFO_PASSES), eng.windowed_launches) == (want["passes"], want["windowed"]), what
            _assert_zero_outside(got, want["window"], what)
            _assert_equal(row, got, state, launch, what)
        series = eng.read_probe() if row["probe"] else None
        spectrum = eng.read_dft() if row["dft"] else None
    if row["probe"]:
        assert np.array_equal(series, ref["series"])
        assert not ref["series"][:32].any() and ref["series"][40:].all()         # the front arrives in the last pass
    if row["dft"]:
        d = row["dft"]
        want = np.zeros((len(d["omega"]),) + tuple(d["window"][2:]), np.complex128)
        for n, w in ref["steps"]:
            if n % d["every"] == 0:
                for f, om in enumerate(d["omega"]):
                    want[f] += w * np.cos(om * (n * awc.DT)) + 1j * (w * -np.sin(om * (n * awc.DT)))
        # the outer 20 columns of the window (its last one is the injection that has not spread yet), zeros beyond
        assert want[:, :, :19].any(axis=(0, 1)).all() and not want[:, :, 20:].any()
        err = np.abs(spectrum - want).max() / np.abs(want).max()
        print(name, "transform: relative error", err)
        assert err <= 1e-12, err          # float64 sums on the device: the bound of the dense engine's own test
    # the same run without the window
    with _engine(fd, row, active_window=0) as eng:
        eng.reset()
        for seg in row["segments"]:
            _do(eng, row, seg)
        assert eng.windowed_launches == 0 and not eng.window_enabled
        dense = eng.download()
    _assert_equal(row, dense, got, None, "active_window=0 against the windowed run")
