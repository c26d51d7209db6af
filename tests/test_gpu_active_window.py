"""GPU tests of the active window (csrc/active_window.hpp; FDTD2D_OPT_ACTIVE_WINDOW): passes of run() that launch only
the bands and strips the fields can have reached.

Every case forces active_window=1 (the automatic mode only starts at 4 Mi cells; one case below is that large) and
compares EVERY cell of Ez, Hx and Hy with the oracle by np.array_equal -- which treats -0 and +0 alike, the contract of
the window: a cell it never writes stays +0 where the dense sweep may compute -0.  Grids are a few strips wide (a strip
writes 224 columns in float32 16-step passes, 96 in float64) so that a window is a real restriction.

Every case here runs at a Courant number of 0.15, where the field underflows some 30 cells from a point source: the outer
part of these windows holds zeros.  tests/test_gpu_active_window_filled.py runs the window where the field fills it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, DX = 5e-14, 1e-4
NAMES = ("Ez", "Hx", "Hy")
INFO_PASSES = 16


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _onp():
    from oracle import fdtd_numpy
    return fdtd_numpy


def _amps(n, seed=7):
    return np.random.default_rng(seed).standard_normal(n)


@functools.lru_cache(maxsize=None)
def _materials(shape, dtype, kind):
    """uniform: scalars; eps / eps+mu: seeded random arrays (read-only, shared)."""
    onp = _onp()
    r, c = shape
    rng = np.random.default_rng(r * 31 + c)
    if kind == "uniform":
        eps = np.full((r, c), 1.7 * onp.EPS0, dtype)
    else:
        eps = (onp.EPS0 * rng.uniform(1, 6, (r, c))).astype(dtype)
    mu = (onp.MU0 * (rng.uniform(1, 2, (r, c)) if kind == "eps+mu" else np.ones((r, c)))).astype(dtype)
    eps.setflags(write=False)
    mu.setflags(write=False)
    return eps, mu


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, kind, segments, extent=(1, 1)):
    """The NumPy oracle from zero fields through `segments` = ((steps, row, col, amplitude seed or None), ...);
    a seed of None is a stretch without a source (amplitude 0 at (0, 0): adds +0.0).  Computed once per case."""
    onp = _onp()
    eps, mu = _materials(shape, dtype, kind)
    ref = onp.grid_zeros(shape[0], shape[1], dtype)
    for steps, row, col, seed in segments:
        amps = np.zeros(steps) if seed is None else _amps(steps, seed)
        onp.leapfrog(*ref, eps, mu, DT, DX, steps, row, col, amps=amps, extent=extent)
    for a in ref:
        a.setflags(write=False)
    return ref


def _engine(fd, shape, dtype, kind, **opts):
    eng = fd.Engine(shape[0], shape[1], DT, DX, dtype=dtype)
    eps, mu = _materials(shape, dtype, kind)
    eng.set_materials(eps, mu)
    o = dict(active_window=1, max_pass_steps=16, band_rows=40)
    o.update(opts)
    eng.set_option(**{k: v for k, v in o.items() if v is not None})
    return eng


def _assert_equal(got, ref, what=""):
    for a, b, k in zip(got, ref, NAMES):
        assert np.array_equal(a, b), f"{k} {what}: differs at {np.argwhere(a != b)[:4].tolist()}"


def _assert_zero_outside(got, win, what=""):
    r0, r1, c0, c1 = win
    for a, k in zip(got, NAMES):
        m = np.ones(a.shape, bool)
        m[r0:r1, c0:c1] = False
        assert not a[m].any(), f"{k} {what}: non-zero outside the reported window {win}"


def _run_segments(eng, segments):
    for steps, row, col, seed in segments:
        eng.run(steps, row, col, None if seed is None else _amps(steps, seed))


# ---- the main case -----------------------------------------------------------------------------------------------------------

MAIN = ((700, 1800), np.float32, "uniform")
MAIN_SEG = ((16, 350, 900, 1), (54, 350, 900, 2))           # 70 steps: 16 | 16 + 16 + 11 + 11


def test_main_case_window_grows_with_the_pulse(fd):
    """700 x 1800 float32 (9 strips), from reset(), source in the middle, 70 steps as passes of 16, 16, 16, 11, 11."""
    shape = MAIN[0]
    with _engine(fd, *MAIN) as eng:
        eng.reset()
        assert eng.active_window == (0, 0, 0, 0)
        _run_segments(eng, MAIN_SEG[:1])
        win = eng.active_window
        assert win == (350 - 16, 351 + 16, 900 - 16, 901 + 16)
        assert eng.windowed_launches == 1 and eng.info(INFO_PASSES) == 1
        _assert_zero_outside(eng.download(), win, "after the first pass")
        _run_segments(eng, MAIN_SEG[1:])
        assert eng.step_count == 70 and eng.info(INFO_PASSES) == 5 and eng.windowed_launches == 5
        win = eng.active_window
        assert win == (350 - 70, 351 + 70, 900 - 70, 901 + 70)
        assert (win[1] - win[0]) * (win[3] - win[2]) < shape[0] * shape[1]
        got = eng.download()
    _assert_zero_outside(got, win, "after 70 steps")
    _assert_equal(got, _reference(*MAIN, MAIN_SEG), "main case")


def test_option_off_gives_the_same_arrays(fd):
    with _engine(fd, *MAIN, active_window=0) as eng:
        eng.reset()
        _run_segments(eng, MAIN_SEG)
        assert eng.windowed_launches == 0 and eng.info(INFO_PASSES) == 5
        got = eng.download()
    _assert_equal(got, _reference(*MAIN, MAIN_SEG), "active_window=0")


# ---- source positions ------------------------------------------------------------------------------------------------------------

POS = ((300, 1000), np.float32, "uniform")                  # 5 strips; 40 steps = 16 + 12 + 12


@pytest.mark.parametrize("src,extent", [((0, 0), (1, 1)), ((150, 999), (1, 1)), ((296, 500), (1, 1)), ((150, 448), (1, 1)),
                                        ((150, 447), (1, 1)), ((150, 449), (1, 1)), ((149, 446), (3, 5)),
                                        ((100, 200), (90, 500))],
                         ids=["corner", "last_column", "3_rows_from_bottom", "seam", "seam-1", "seam+1", "patch_3x5_on_seam",
                              "patch_90x500"])
def test_source_positions(fd, src, extent):
    """Corner, last column, next to the bottom zone, on a strip seam (column 224 k) and beside it, a patch across it --
    and a patch over several bands and strips: the pulse of a point source underflows ~25 cells out, a patch keeps most of
    the window non-zero."""
    seg = ((40, src[0], src[1], 3),)
    with _engine(fd, *POS) as eng:
        eng.set_source_extent(*extent)
        eng.reset()
        _run_segments(eng, seg)
        assert eng.windowed_launches == 3 and eng.info(INFO_PASSES) == 3
        win, got = eng.active_window, eng.download()
    _assert_zero_outside(got, win, f"source {src}")
    _assert_equal(got, _reference(*POS, seg, extent), f"source {src} extent {extent}")


# ---- growth to the whole grid ---------------------------------------------------------------------------------------------------

def test_window_grows_to_the_full_grid_and_falls_back_to_dense(fd):
    cfg = ((300, 700), np.float32, "uniform")
    seg = tuple((100, 140, 330, 10 + k) for k in range(4))
    with _engine(fd, *cfg) as eng:
        eng.reset()
        counts = []
        for s in seg:
            _run_segments(eng, (s,))
            counts.append(eng.windowed_launches)
        assert eng.active_window == (0, 300, 0, 700)
        # the window passes half the grid within the first 200 steps (300 rows are covered after 160): dense from there on
        assert 0 < counts[0] and counts[1] == counts[2] == counts[3] < eng.info(INFO_PASSES)
        got = eng.download()
    _assert_equal(got, _reference(*cfg, seg), "400 steps")


# ---- two sources in turn ---------------------------------------------------------------------------------------------------------

def test_two_sources_in_turn_give_a_bounding_box(fd):
    seg = ((16, 100, 300, 4), (20, 300, 1100, 5))
    with _engine(fd, *MAIN) as eng:
        eng.reset()
        _run_segments(eng, seg)
        win = eng.active_window
        assert win == (100 - 36, 301 + 20, 300 - 36, 1101 + 20)
        assert eng.windowed_launches == eng.info(INFO_PASSES) == 3          # 16 | 10 + 10
        got = eng.download()
    _assert_zero_outside(got, win, "two sources")
    _assert_equal(got, _reference(*MAIN, seg), "two sources")


# ---- kernel variants ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,kind,max_steps,passes", [(np.float32, "uniform", 20, 2), (np.float32, "uniform", 8, 5),
                                                         (np.float64, "uniform", 16, 3), (np.float32, "eps", 16, 3),
                                                         (np.float32, "eps+mu", 16, 3), (np.float64, "eps+mu", 8, 5)],
                         ids=["f32_20_steps", "f32_8_steps", "f64_16_steps", "f32_eps", "f32_eps_mu", "f64_eps_mu_8_steps"])
def test_kernel_variants(fd, dtype, kind, max_steps, passes):
    """20-step passes (40 = 20 + 20), 8-step passes, float64 (128-column strips), array materials."""
    cfg = ((300, 1000), dtype, kind)
    seg = ((20, 141, 452, 6), (20, 141, 452, 7))
    with _engine(fd, *cfg, max_pass_steps=max_steps) as eng:
        eng.reset()
        _run_segments(eng, seg)
        n = eng.info(INFO_PASSES)
        assert eng.windowed_launches == n and n >= passes
        win, got = eng.active_window, eng.download()
    assert win == (141 - 40, 142 + 40, 452 - 40, 453 + 40)
    _assert_zero_outside(got, win, f"{kind} {max_steps}")
    _assert_equal(got, _reference(*cfg, seg), f"{np.dtype(dtype).name} {kind} max_pass_steps={max_steps}")


# ---- what other launches leave in the target set ---------------------------------------------------------------------------------

def test_dense_launches_in_between_leave_a_dirty_target(fd):
    """reset; run(16, src); time_launches(2, 16) -- dense, committed, no source --; run(16, src)."""
    cfg = ((300, 1000), np.float32, "uniform")
    seg = ((16, 150, 500, 8), (32, 0, 0, None), (16, 150, 500, 9))
    with _engine(fd, *cfg) as eng:
        eng.reset()
        _run_segments(eng, seg[:1])
        assert eng.windowed_launches == 1
        ms = eng.time_launches(2, 16)
        assert len(ms) == 2 and eng.windowed_launches == 1 and eng.info(INFO_PASSES) == 3
        _run_segments(eng, seg[2:])
        assert eng.windowed_launches == 2
        win, got = eng.active_window, eng.download()
    assert win == (150 - 64, 151 + 64, 500 - 64, 501 + 64)
    _assert_equal(got, _reference(*cfg, seg), "run, time_launches, run")


# ---- state changes -----------------------------------------------------------------------------------------------------------------

def test_upload_makes_the_window_full_and_reset_empties_it(fd):
    onp = _onp()
    cfg = ((300, 1000), np.float32, "uniform")
    r, c = cfg[0]
    rng = np.random.default_rng(5)
    state = [rng.standard_normal((r, c)).astype(np.float32), (rng.standard_normal((r, c - 1)) * 1e-3).astype(np.float32),
             (rng.standard_normal((r - 1, c)) * 1e-3).astype(np.float32)]
    amps = _amps(16, 11)
    ref = [a.copy() for a in state]
    onp.leapfrog(*ref, *_materials(*cfg), DT, DX, 16, 150, 500, amps=amps)
    seg = ((32, 150, 500, 12),)
    with _engine(fd, *cfg) as eng:
        eng.upload(*state)
        assert eng.active_window == (0, r, 0, c)
        eng.run(16, 150, 500, amps)
        assert eng.windowed_launches == 0 and eng.active_window == (0, r, 0, c)
        _assert_equal(eng.download(), ref, "from an uploaded state")
        eng.reset()                                     # stale data is gone from BOTH buffer sets
        assert eng.active_window == (0, 0, 0, 0)
        _run_segments(eng, seg)
        assert eng.windowed_launches == 2
        got = eng.download()
    _assert_equal(got, _reference(*cfg, seg), "from zero after reset()")


def test_mixed_api_single_steps_then_a_pass(fd):
    """reset; add_point; update_h; update_e; run(16): the single-step kernels stay dense, the window follows them."""
    onp = _onp()
    cfg = ((300, 1000), np.float32, "uniform")
    eps, mu = _materials(*cfg)
    amps = _amps(16, 13)
    ref = onp.grid_zeros(*cfg[0], np.float32)
    onp.add_point(ref[0], 150, 448, 0.75)
    onp.update_h(*ref, mu, eps, DT, DX)
    onp.update_e(*ref, mu, eps, DT, DX)
    onp.leapfrog(*ref, eps, mu, DT, DX, 16, 150, 448, amps=amps)
    with _engine(fd, *cfg) as eng:
        eng.reset()
        eng.add_point(150, 448, 0.75)
        assert eng.active_window == (150, 151, 448, 449)
        eng.update_h()
        eng.update_e()
        eng.run(16, 150, 448, amps)
        assert eng.windowed_launches == 1
        win, got = eng.active_window, eng.download()
    assert win[0] <= 150 - 17 and win[1] >= 151 + 17 and (win[1] - win[0]) * (win[3] - win[2]) < 300 * 1000
    _assert_zero_outside(got, win, "mixed API")
    _assert_equal(got, ref, "mixed API")


# ---- monitors ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", [(20, 40), (150, 505)], ids=["probe_outside", "probe_inside"])
def test_probe_and_transform_with_a_window(fd, cell):
    """A probe cell outside the window (all zeros) or inside it; a transform window that straddles the window's edge.
    The transform sums in float64 on the device: 1e-12 of its largest value, the bound of the dense engine's own test."""
    onp = _onp()
    cfg = ((300, 1000), np.float32, "uniform")
    n, every, dwin = 48, 16, (140, 490, 30, 70)           # columns 490 .. 559: the window ends at 500 + 48, inside it
    om = 2 * np.pi * np.array([20e9, 45e9])
    amps = _amps(n, 14)
    seq = []
    ref = onp.grid_zeros(*cfg[0], np.float32)
    onp.leapfrog(*ref, *_materials(*cfg), DT, DX, n, 150, 500, amps=amps, on_step=lambda i, E, *_: seq.append(E.copy()))
    want = np.zeros((2,) + dwin[2:], np.complex128)
    for k in range(1, n + 1):
        if k % every == 0:
            w = seq[k - 1][dwin[0]:dwin[0] + dwin[2], dwin[1]:dwin[1] + dwin[3]].astype(np.float64)
            for f, o in enumerate(om):
                want[f] += w * np.cos(o * (k * DT)) + 1j * (w * -np.sin(o * (k * DT)))
    with _engine(fd, *cfg) as eng:
        eng.reset()
        eng.set_probe(cell[0], cell[1], n)
        eng.set_dft(dwin, om, every)
        eng.run(n, 150, 500, amps)
        assert eng.windowed_launches == 3
        series, got, fields = eng.read_probe(), eng.read_dft(), eng.download()
    assert np.array_equal(series, np.array([float(e[cell]) for e in seq]))
    assert (not series.any()) == (cell == (20, 40))
    assert np.abs(want).max() > 0 and not want[:, :, 59:].any()
    err = np.abs(got - want).max() / np.abs(want).max()
    print("transform: relative error", err)
    assert err <= 1e-12, err
    _assert_equal(fields, ref, "with monitors")


# ---- engines without a window ---------------------------------------------------------------------------------------------------

def test_pml_engine_reports_the_whole_grid(fd):
    from oracle import pml_numpy as pm
    onp = _onp()
    r, c, L, S, n = 200, 301, 40, 0.15, 20
    eps, mu = np.full((r, c), onp.EPS0, np.float32), np.full((r, c), onp.MU0, np.float32)
    P = pm.profiles(r, c, S, L=L, dtype=np.float32)
    amps = _amps(n, 15)
    ref = [np.zeros((r, c), np.float32), np.zeros((r, c), np.float32), np.zeros((r, c - 1), np.float32), np.zeros((r - 1, c), np.float32)]
    pm.leapfrog(*ref, eps, mu, DT, DX, n, r // 2, c // 3, amps, P)
    with fd.Engine(r, c, DT, DX, dtype=np.float32, boundary="pml") as eng:
        eng.set_materials(eps, mu).set_pml(L=L, courant00=S).set_option(active_window=1)
        eng.reset()
        assert eng.active_window == (0, r, 0, c)
        eng.run(n, r // 2, c // 3, amps)
        assert eng.active_window == (0, r, 0, c) and eng.windowed_launches == 0
        got = eng.download()
    _assert_equal(got, (ref[0], ref[2], ref[3]), "PML engine")


def test_slab_engine_reports_the_whole_grid(fd):
    cfg = ((300, 1000), np.float32, "uniform")
    r, c = cfg[0]
    seg = ((16, 60, 500, 16),)
    eps, mu = _materials(*cfg)
    with fd.Engine(r, c, DT, DX, dtype=np.float32, slab=(0, 150, 16)) as eng:
        eng.set_materials(eps[:166], mu[:166]).set_option(active_window=1, max_pass_steps=16, band_rows=40)
        eng.reset()
        assert eng.active_window == (0, r, 0, c)
        _run_segments(eng, seg)
        assert eng.active_window == (0, r, 0, c) and eng.windowed_launches == 0 and eng.info(INFO_PASSES) == 1
        got = eng.download()
    ref = _reference(*cfg, seg)
    _assert_equal(got, (ref[0][:150], ref[1][:150], ref[2][:150]), "top slab, owned rows")


# ---- automatic mode, with the tuner ----------------------------------------------------------------------------------------------

def test_automatic_mode_with_the_tuner_at_4096x4200(fd):
    """No option set: 17 Mi cells are above the 4 Mi rule.  prepare() tunes with uncommitted trial launches, which leave
    the target set dirty: the first pass of the run is dense, the later ones are windowed.  Against the C oracle."""
    from oracle import c_oracle as corc
    onp = _onp()
    r, c, n = 4096, 4200, 40
    eps, mu = np.full((r, c), onp.EPS0, np.float32), np.full((r, c), onp.MU0, np.float32)
    amps = _amps(n, 17)
    ref = onp.grid_zeros(r, c, np.float32)
    corc.run(*ref, eps, mu, DT, DX, n, r // 2, c // 2, amps=amps)
    with fd.Engine(r, c, DT, DX, dtype=np.float32) as eng:
        eng.set_materials()
        eng.prepare(n, r // 2, c // 2)
        eng.run(n, r // 2, c // 2, amps)
        assert 0 < eng.windowed_launches < eng.info(INFO_PASSES)
        win, got = eng.active_window, eng.download()
    assert win == (r // 2 - n, r // 2 + 1 + n, c // 2 - n, c // 2 + 1 + n)
    _assert_zero_outside(got, win, "automatic mode")
    _assert_equal(got, ref, "automatic mode")


# ---- what switches the automatic mode off for a handle ----------------------------------------------------------------------------

AUTO = (2048, 2048)          # 4 Mi cells: the smallest grid of the automatic mode; 16 steps are two 8-step passes there
AUTO_SRC = (1024, 1000)


@functools.lru_cache(maxsize=None)
def _auto_reference():
    from oracle import c_oracle as corc
    onp = _onp()
    r, c = AUTO
    eps, mu = np.full((r, c), onp.EPS0, np.float32), np.full((r, c), onp.MU0, np.float32)
    ref = onp.grid_zeros(r, c, np.float32)
    corc.run(*ref, eps, mu, DT, DX, 16, *AUTO_SRC, amps=_amps(16, 18))
    for a in ref:
        a.setflags(write=False)
    return ref


def _auto_run(eng):
    eng.reset()
    n0, w0 = eng.info(INFO_PASSES), eng.windowed_launches
    eng.run(16, *AUTO_SRC, _amps(16, 18))
    return eng.info(INFO_PASSES) - n0, eng.windowed_launches - w0, eng.download()


def test_device_ptr_marks_everything_and_ends_the_automatic_mode(fd):
    """reduce() hands nothing out and changes nothing; device_ptr() makes the window the whole grid and switches the
    automatic mode off for the handle, also after a reset(); the option set to 1 takes that back."""
    r, c = AUTO
    with fd.Engine(r, c, DT, DX, dtype=np.float32) as eng:
        eng.set_materials()
        eng.reset()
        assert eng.window_enabled and eng.active_window == (0, 0, 0, 0)
        eng.reduce("Ez")
        assert eng.window_enabled and eng.active_window == (0, 0, 0, 0)
        assert eng.device_ptr("Ez") != 0
        assert not eng.window_enabled and eng.active_window == (0, r, 0, c)
        passes, windowed, got = _auto_run(eng)
        assert not eng.window_enabled and (passes, windowed) == (2, 0)
        _assert_equal(got, _auto_reference(), "dense after device_ptr")
        eng.set_option(active_window=1)
        assert eng.window_enabled
        passes, windowed, got = _auto_run(eng)
        assert (passes, windowed) == (2, 2)
        win = eng.active_window
    assert win == (AUTO_SRC[0] - 16, AUTO_SRC[0] + 17, AUTO_SRC[1] - 16, AUTO_SRC[1] + 17)
    _assert_equal(got, _auto_reference(), "windowed, option 1 after device_ptr")


def test_a_given_shape_ends_the_automatic_mode_and_is_honoured_with_the_option_on(fd):
    """set_shape() pins launches: in the automatic mode they then sweep the whole grid with exactly that shape; with the
    option at 1 the window's launch takes its band heights and waves from the shape.  last_shape reports what ran."""
    r, c = AUTO
    shape = (48, 4, 24)
    with fd.Engine(r, c, DT, DX, dtype=np.float32) as eng:
        eng.set_materials()
        assert eng.window_enabled
        eng.set_shape(shape)
        assert not eng.window_enabled
        passes, windowed, got = _auto_run(eng)
        assert (passes, windowed) == (2, 0) and eng.last_shape[:3] == shape
        _assert_equal(got, _auto_reference(), "dense, given shape")
        eng.set_option(active_window=1)
        assert eng.window_enabled
        passes, windowed, got = _auto_run(eng)
        assert (passes, windowed) == (2, 2) and eng.last_shape[:3] == shape
        _assert_zero_outside(got, eng.active_window, "windowed, given shape")
        _assert_equal(got, _auto_reference(), "windowed, given shape")
        eng.set_option(active_window=-1)
        assert not eng.window_enabled
        eng.set_shape((0,))
        assert eng.window_enabled
