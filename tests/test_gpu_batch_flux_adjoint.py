"""GPU: line sources on the flux lines of PML and periodic batches (fdtd2d_batch_flux_adjoint.h,
kernels_batch_flux_adjoint.hpp) against the stand-in of tests/oracle_batch_flux_adjoint.py.

The shapes, lines and monitors are those of tests/test_gpu_batch_flux.py: three members that differ in eps, sources,
frequencies, weights and channels, 320 steps from rest, K = 6 channels per member; float32 periodic 40x17 (4 cells per
thread) and 150x33 (8 per thread), float64 periodic 40x17, "pml" 40x40 with a 6-cell layer, lossless, with a conductivity
patch and with a pole, periodic 40x17 with a pole, and periodic 40x17 with point sources beside the line sources.  Every
shape runs resident with the sums in LDS, resident with them in global memory and streamed; one also with 7 steps per
launch.  The four lines: a whole-period (whole-width) row line, a row line inside the layer, a column line at column 0 of
the periodic members (the cyclic neighbour Hy[:, C-2] takes half of its H part, and the image column repeats its E part;
column 1 in the box), a column line at C-2, and the first row line crosses both column lines (one cell on two lines: two
entries, two E parts in one float64 sum).

Tolerances.  The fields are bit-identical to the stand-in's (exact build): the injected sums are float64 dot products in
the stated order, and NumPy multiplies and adds the same numbers.  The monitors then differ only by the device's sin and
cos against NumPy's: 1e-12 max|stand-in| per array and 4e-12 dx sum|E||H| for the flux, the bounds of
tests/test_gpu_batch_flux.py.  The weights formed on the device differ from the host's by the same sin and cos and a
2F-term sum: 1e-12 max|weight|.  The end-to-end gradient is a product of two windows that agree to 1e-12 each, driven by
weights that agree to 1e-12 times the channel system's condition number (below 10): bound 1e-9 of max|gradient|, as for
the probe gradients in tests/test_gpu_batch_adjoint.py; the measured difference is printed."""
import ctypes

import numpy as np
import pytest

from oracle_batch_flux_adjoint import line_source_oracle_for

pytestmark = pytest.mark.gpu

DT, DX = 5e-14, 1e-4
E_ARG, E_STATE = -1, -4
B, NSTEPS, EVERY, LAYER, K = 3, 320, 3, 6, 6
# case: (boundary, rows, cols, dtype, conductivity, pole, point sources)
CASES = {"per40x17f32": ("periodic", 40, 17, np.float32, False, False, False),
         "per150x33f32": ("periodic", 150, 33, np.float32, False, False, False),
         "per40x17f64": ("periodic", 40, 17, np.float64, False, False, False),
         "pml40x40": ("pml", 40, 40, np.float32, False, False, False),
         "pml40x40sigma": ("pml", 40, 40, np.float32, True, False, False),
         "pml40x40pole": ("pml", 40, 40, np.float32, False, True, False),
         "per40x17pole": ("periodic", 40, 17, np.float32, False, True, False),
         "per40x17points": ("periodic", 40, 17, np.float32, False, False, True)}
MODES = ("lds", "global", "streamed")
SPL_CASE = "per40x17f32"


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the stand-in restates the exact build's arithmetic")


def _mid(R):
    return min(R // 2, 20)


def _lines(boundary, R, C):
    mid = _mid(R)
    if boundary == "periodic":
        return [("row", mid, 0, C - 1), ("row", 3, 2, 5), ("col", 0, 4, R - 10), ("col", C - 2, mid - 6, 12)]
    return [("row", mid, 0, C), ("row", 3, 8, 20), ("col", 1, 0, R), ("col", C - 2, mid - 6, 12)]


def _cfg(case):
    from fdtd2d_amd.api import EPS0, MU0, ricker_amplitude
    boundary, R, C, dtype, sigma, pole, points = CASES[case]
    rng = np.random.default_rng(11)
    mid, box = _mid(R), boundary == "pml"
    lines = _lines(boundary, R, C)
    cells = sum(l[3] for l in lines)
    t = np.arange(NSTEPS) * DT
    cfg = dict(case=case, boundary=boundary, R=R, C=C, dtype=dtype,
               eps=(EPS0 * (1 + 2 * rng.random((B, R, C)))).astype(dtype),
               mu=(MU0 * (1 + 0.5 * rng.random((B, R, C)))).astype(dtype),
               rects=np.array([[mid - 5 + m, ((8, 12, C - 12) if box else (0, 2, C - 4))[m], 1,
                                ((C - 20, 3, 2) if box else (C - 1, 3, 2))[m]] for m in range(B)]),
               amps=np.stack([[ricker_amplitude(k * DT, 60e9 * (1 + 0.1 * m)) for k in range(NSTEPS)]
                              for m in range(B)]),
               omegas=2 * np.pi * np.array([[40e9, 60e9, 85e9], [35e9, 55e9, 75e9], [45e9, 65e9, 90e9]]),
               win_omegas=2 * np.pi * np.array([50e9, 70e9]), window=(mid - 2, 1, 5, 6),
               probes=np.array([[mid, 0], [mid + 3, C - 2], [4, 5]]), lines=lines, sigma=None, pole=None, points=None)
    # Ez is of order 1 from the rectangle source; the E parts are of the same order and the H parts of order Ez / 377
    cfg["we"] = 0.3 * rng.standard_normal((B, cells, K))
    cfg["wh"] = 1e-3 * rng.standard_normal((B, cells, K))
    cfg["chan"] = np.stack([[np.sin(2 * np.pi * 45e9 * (1 + 0.2 * c + 0.05 * m) * t + c) for c in range(K)]
                            for m in range(B)])
    if sigma:
        s = np.zeros((B, R, C))
        s[:, 24:28, 12:25] = 5.0 * (1 + rng.random((B, 4, 13)))
        cfg["sigma"] = s
    if pole:
        wp2 = np.zeros((B, R, C))
        wp2[:, 25:30, (slice(0, C) if boundary == "periodic" else slice(10, 30))] = (2 * np.pi * 70e9) ** 2
        cfg["pole"] = (wp2, np.array([1e11, 0.0, 5e10]), 2 * np.pi * np.array([0.0, 50e9, 60e9]))
    if points:      # one on a line cell (the point source adds first), one in column 0, one elsewhere
        cfg["points"] = (np.array([[mid, 3], [mid + 4, 0], [mid - 3, 7]]), 0.2 * rng.standard_normal((B, 3, K)))
    return cfg


def _setup(b, cfg, lines=True):
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
    b.set_pml(LAYER, courant00=np.array(c00))
    if cfg["sigma"] is not None:
        b.set_conductivity(cfg["sigma"])
    if cfg["pole"] is not None:
        b.set_dispersion(*cfg["pole"])
    b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2).set_probes(cfg["probes"], NSTEPS)
    if lines:
        b.set_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)


def _results(b, cfg):
    out = dict(fields=tuple(b.download()), dft=b.read_dft_window(), probes=b.read_probes())
    out["fields"] += (b.download_ezx() if hasattr(b, "download_ezx") else b.Ezx.copy(),)
    if cfg["pole"] is not None:
        out["fields"] += tuple(b.download_dispersion())
    out["E"], out["H"] = b.read_flux_lines(raw=True)
    out["P"] = b.flux()
    return out


def _drive(b, cfg):
    """The same calls on a BatchEngine and on the stand-in."""
    _setup(b, cfg)
    if cfg["points"] is not None:
        b.set_point_sources(*cfg["points"])
    b.set_flux_line_sources(cfg["we"], cfg["wh"])
    before = getattr(b, "launches", 0)
    b.run(NSTEPS, cfg["amps"], cfg["chan"])
    launches = getattr(b, "launches", 0) - before       # the run's own: flux() is a launch too
    out = _results(b, cfg)
    out["launches"] = launches
    return out


_refs, _runs = {}, {}


def _stand_in(case):
    if case not in _refs:
        cfg = _cfg(case)
        ref = line_source_oracle_for(cfg["boundary"], cfg["pole"] is not None)(B, cfg["R"], cfg["C"], DT, DX,
                                                                              dtype=cfg["dtype"], boundary=cfg["boundary"])
        _refs[case] = _drive(ref, cfg)
        _refs[case]["scale"] = ref.flux_scale()
    return _refs[case]


def _device(fd, case, mode):
    """mode: "lds", "global", "streamed" or "spl7" (resident, 7 steps per launch)."""
    if (case, mode) not in _runs:
        cfg = _cfg(case)
        with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"]) as b:
            b.set_option(resident=0 if mode == "streamed" else None, steps_per_launch=7 if mode == "spl7" else None)
            b.set_flux_lds(mode != "global")
            out = _drive(b, cfg)
            assert b.resident == (mode != "streamed") and b.flux_lines_in_lds == (mode in ("lds", "spl7"))
            assert b.info(23) == K
            # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            want = 2 * NSTEPS if mode == "streamed" else -(-NSTEPS // 7) if mode == "spl7" else 1
            assert out["launches"] == want
        _runs[case, mode] = out
    return _runs[case, mode]


def _modes(case):
    return MODES + (("spl7",) if case == SPL_CASE else ())


ALL = [(c, m) for c in CASES for m in _modes(c)]
NAMES = ("Ez", "Hx", "Hy", "Ezx", "Jh", "Q")


# ---- 1. against the stand-in, on every path ------------------------------------------------------------------------

@pytest.mark.parametrize("case,mode", ALL, ids=[f"{c}-{m}" for c, m in ALL])
def test_fields_and_monitors_match_the_stand_in(fd, case, mode):
    _exact_only(fd)
    got, want = _device(fd, case, mode), _stand_in(case)
    assert len(got["fields"]) == len(want["fields"]) == (6 if CASES[case][5] else 4)
    for name, a, w in zip(NAMES, got["fields"], want["fields"]):
        assert a.dtype == w.dtype and np.array_equal(a, w), name
    for name in ("E", "H", "dft", "probes"):
        err, top = np.abs(got[name] - want[name]).max(), np.abs(want[name]).max()
        print(f"{case} {mode} {name}: max error {err:.3e}, max |stand-in| {top:.3e}, ratio {err / top:.2e}")
        assert top > 0 and err <= 1e-12 * top, name
    err = np.abs(got["P"] - want["P"])
    print(f"{case} {mode} P: worst error over its scale {np.max(err / want['scale']):.2e}")
    assert np.all(want["scale"] > 0) and np.all(err <= 4e-12 * want["scale"])


def test_the_sources_reach_every_kind_of_cell():
    """The stand-in's run differs from a run without line sources where the issue's lines put their parts: the image
    column, the cyclic neighbour Hy[:, C-2] of column 0 after one step, and both parts matter."""
    cfg = _cfg("per40x17f32")
    C = cfg["C"]
    runs = []
    for we, wh in ((cfg["we"], cfg["wh"]), (None, cfg["wh"]), (cfg["we"], None)):
        ref = line_source_oracle_for("periodic")(B, cfg["R"], C, DT, DX, dtype=cfg["dtype"], boundary="periodic")
        _setup(ref, cfg)
        ref.set_flux_line_sources(we, wh)
        ref.run(1, None, cfg["chan"][:, :, 1:2])        # one step from rest with non-zero channels: the parts alone
        runs.append(ref.download())
    (ez, hx, hy), (ez_h, _, hy_h), (ez_e, hx_e, hy_e) = runs
    assert np.all(ez[:, 4:cfg["R"] - 6, 0] != 0) and np.array_equal(ez[:, :, -1], ez[:, :, 0])
    assert np.all(hy_h[:, 4:cfg["R"] - 6, C - 2] != 0) and np.all(hy_h[:, 4:cfg["R"] - 6, 0] != 0)
    assert not np.any(hx_e) and not np.any(hy_e) and np.any(ez_e) and np.any(ez_h != ez)


# ---- 2. whatever the path, the placement and the launch split ----------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_results_do_not_depend_on_path_placement_or_split(fd, case):
    first = _device(fd, case, "lds")
    for mode in _modes(case)[1:]:
        other = _device(fd, case, mode)
        for k in ("E", "H", "P", "dft", "probes"):
            assert np.array_equal(first[k], other[k]), (mode, k)
        for a, b in zip(first["fields"], other["fields"]):
            assert np.array_equal(a, b), mode


# ---- 3. a one-cell line with an E part alone is a point source ----------------------------------------------------------

@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("case,cell", [("per40x17f32", (20, 0)), ("pml40x40", (20, 9))])
def test_an_electric_one_cell_line_equals_a_point_source(fd, case, cell, resident):
    cfg = _cfg(case)
    w = cfg["we"][:, :1, :]
    outs = []
    for kind in ("line", "point"):
        with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"]) as b:
            b.set_option(resident=resident)
            _setup(b, cfg, lines=False)
            b.set_flux_lines([("row", cell[0], cell[1], 1)], cfg["omegas"], every=EVERY)
            if kind == "line":
                b.set_flux_line_sources(w, None)
            else:
                b.set_point_sources(np.array([cell]), w)
            b.run(NSTEPS, cfg["amps"], cfg["chan"])
            outs.append(_results(b, cfg))
    a, c = outs
    assert np.abs(a["fields"][0]).max() > 0
    for x, y in zip(a["fields"], c["fields"]):
        assert np.array_equal(x, y)
    for k in ("E", "H", "P", "dft", "probes"):
        assert np.array_equal(a[k], c[k]), k


# ---- 4. removed line sources leave nothing behind ------------------------------------------------------------------------

@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
def test_removed_line_sources_leave_the_flux_kernels(fd, resident):
    cfg = _cfg("per40x17f32")
    outs = []
    for had in (True, False):
        with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic") as b:
            b.set_option(resident=resident)
            _setup(b, cfg)
            if had:
                b.set_flux_line_sources(cfg["we"], cfg["wh"])
                assert b.info(23) == K
                b.set_flux_line_sources(None, None)
            assert b.info(23) == 0
            before = b.launches
            b.run(NSTEPS, cfg["amps"])
            launches = b.launches - before
            out = _results(b, cfg)
            out["launches"] = launches
            chan = np.ascontiguousarray(cfg["chan"][:, :, :4])      # and nothing takes channels any more
            assert fd._abi.load().fdtd2d_batch_run_channels(
                b._h, 4, None, chan.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1) == E_STATE
        outs.append(out)
    a, c = outs
    assert a["launches"] == c["launches"] == (1 if resident is None else 2 * NSTEPS)
    for x, y in zip(a["fields"], c["fields"]):
        assert np.array_equal(x, y)
    for k in ("E", "H", "P", "dft", "probes"):
        assert np.array_equal(a[k], c[k]), k


def test_silent_and_kept_across_reset_and_dropped_with_the_lines(fd):
    cfg = _cfg("per40x17f32")
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic") as b:
        _setup(b, cfg)
        b.set_flux_line_sources(cfg["we"], cfg["wh"])
        b.run(40, cfg["amps"][:, :40])                   # a run without channels leaves them silent
        silent = b.download()
        we, wh = b.read_flux_line_sources()
        assert np.array_equal(we, cfg["we"]) and np.array_equal(wh, cfg["wh"])
        b.reset()
        assert b.info(23) == K                           # reset keeps them
        b.run(40, cfg["amps"][:, :40], cfg["chan"])
        driven = b.download()
        assert not np.array_equal(silent[0], driven[0])
        b.set_flux_lines(cfg["lines"], cfg["omegas"])    # new lines drop them
        assert b.info(23) == 0
        b.set_flux_line_sources(cfg["we"], None)
        assert not np.any(b.read_flux_line_sources()[1])
        b.set_flux_lines(None, None)
        assert b.info(23) == 0
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic") as b:
        _setup(b, cfg)
        b.run(40, cfg["amps"][:, :40])
        for x, y in zip(silent, b.download()):
            assert np.array_equal(x, y)


# ---- 5. the weights formed on the device ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shared", [False, True], ids=["solve-per-member", "solve-shared"])
@pytest.mark.parametrize("case", ["per40x17f64", "pml40x40"])
def test_device_weights_equal_the_host_path(fd, case, shared):
    from fdtd2d_amd.adjoint import flux_adjoint_weights
    cfg = _cfg(case)
    rng = np.random.default_rng(5)
    F, cells = cfg["omegas"].shape[1], cfg["we"].shape[1]
    dJdP = rng.standard_normal((B, len(cfg["lines"]), F))
    solve = rng.standard_normal((2 * F, 2 * F) if shared else (B, 2 * F, 2 * F))
    se, sh = 1 + rng.random((B, cells)), -(1 + rng.random((B, cells)))
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"]) as b:
        _setup(b, cfg)
        b.run(NSTEPS, cfg["amps"])
        E, H = b.read_flux_lines(raw=True)
        b.flux_adjoint_sources(dJdP, solve, se, sh)
        assert b.info(23) == 2 * F
        got = b.read_flux_line_sources()
        b.flux_adjoint_sources(dJdP, solve)              # scales default to ones
        plain = b.read_flux_line_sources()
    want = flux_adjoint_weights(E, H, dJdP, cfg["lines"], cfg["omegas"], DT, DX, solve, se, sh)
    ones = flux_adjoint_weights(E, H, dJdP, cfg["lines"], cfg["omegas"], DT, DX, solve)
    for name, g, w in zip(("we", "wh", "we (ones)", "wh (ones)"), got + plain, want + ones):
        err, top = np.abs(g - w).max(), np.abs(w).max()
        print(f"{case} {name}: max error {err:.3e}, max |weight| {top:.3e}, ratio {err / top:.2e}")
        assert top > 0 and err <= 1e-12 * top, name


# ---- 6. end to end: batch_flux_gradient on the device against the stand-in ------------------------------------------------

def test_batch_flux_gradient_matches_the_stand_in(fd):
    _exact_only(fd)
    from fdtd2d_amd.api import EPS0
    R, C, n, dt, fc = 40, 17, 800, 2e-13, 60e9
    eps = np.full((2, R, C), EPS0)
    eps[:, 16:20, 3:9] = EPS0 * (1 + 2 * np.random.default_rng(3).random((2, 4, 6)))
    sigma = np.zeros((2, R, C))
    sigma[:, 16:20, 3:9] = 0.3
    lines = [("row", 26, 0, C - 1), ("col", 12, 21, 4)]

    def objective(P):
        w = np.array([1.0, -0.5, 2.0])[None, None, :] * np.array([1.0, 0.3])[None, :, None]
        return (w * P).sum(axis=(1, 2)), np.broadcast_to(w, P.shape).copy()
    args = dict(nsteps=n, sources=np.array([[10, 0, 1, C - 1], [10, 2, 1, 5]]), flux_lines=lines,
                omegas=2 * np.pi * np.array([45e9, 60e9, 80e9]), design=(16, 3, 4, 6), objective=objective, fc=fc, dt=dt,
                dx=DX, dtype=np.float64, boundary="periodic", pml_cells=8)
    Jr, gr, sr, Pr, ir = fd.batch_flux_gradient(eps, sigma, engine=line_source_oracle_for("periodic"), **args)
    J, g, s, P, info = fd.batch_flux_gradient(eps, sigma, **args)
    for name, a, w in (("P", P, Pr), ("J", J, Jr), ("grad_eps", g, gr), ("grad_sigma", s, sr)):
        err, top = np.abs(a - w).max(), np.abs(w).max()
        print(f"{name}: max error {err:.3e}, max |stand-in| {top:.3e}, ratio {err / top:.2e}")
        assert top > 0 and err <= 1e-9 * top, name
    assert np.allclose(info["residual_forward"], ir["residual_forward"], rtol=1e-9)


def test_flux_adjoint_session_matches_the_helper(fd):
    from fdtd2d_amd.api import EPS0
    R, C, n, dt, fc = 40, 17, 800, 2e-13, 60e9
    eps = np.full((2, R, C), EPS0)
    eps[:, 16:20, 3:9] = EPS0 * (1 + 2 * np.random.default_rng(3).random((2, 4, 6)))
    args = dict(nsteps=n, sources=np.array([[10, 0, 1, C - 1], [10, 2, 1, 5]]), flux_lines=[("row", 26, 0, C - 1)],
                omegas=2 * np.pi * np.array([45e9, 60e9, 80e9]), design=(16, 3, 4, 6), fc=fc, dt=dt, dx=DX,
                dtype=np.float64, boundary="periodic", pml_cells=8)

    def objective(P):
        return P.sum(axis=(1, 2)), np.ones_like(P)
    J, g, _, P, info = fd.batch_flux_gradient(eps, **args, objective=objective)
    with fd.FluxAdjointSession(eps, **args) as s:
        for _ in range(2):                               # the second iteration starts from the first one's sources
            Js, gs, Ps, infos = s.value_and_grad(objective)
            assert np.array_equal(Ps, P) and np.array_equal(Js, J)
            err = np.abs(gs - g).max() / np.abs(g).max()
            print(f"session vs helper: {err:.3e} of max|gradient|")
            assert err <= 1e-9
        new = EPS0 * np.full((2, 4, 6), 2.5)
        s.set_design_eps(new)
        J2 = s.value_and_grad(objective)[0]
    eps2 = eps.copy()
    eps2[:, 16:20, 3:9] = new
    assert np.allclose(J2, fd.batch_flux_gradient(eps2, **args, objective=objective)[0], rtol=1e-9, atol=0)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_return_the_stated_codes_and_leave_the_engine_usable(fd):
    cfg = _cfg("per40x17f32")
    lib, dp = fd._abi.load(), ctypes.POINTER(ctypes.c_double)
    cells = cfg["we"].shape[1]
    w = np.ascontiguousarray(cfg["we"])
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic") as b:
        _setup(b, cfg, lines=False)
        assert lib.fdtd2d_batch_set_flux_line_sources(b._h, K, w.ctypes.data_as(dp), None) == E_STATE   # no lines
        assert lib.fdtd2d_batch_flux_line_weights(b._h, w.ctypes.data_as(dp), w.ctypes.data_as(dp), 0, None, None) == E_STATE
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.set_flux_line_sources(cfg["we"], None)
        assert ei.value.code == E_STATE
        b.set_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        big = np.zeros((B, cells, 33))
        assert lib.fdtd2d_batch_set_flux_line_sources(b._h, 33, big.ctypes.data_as(dp), None) == E_ARG
        assert lib.fdtd2d_batch_set_flux_line_sources(b._h, -1, big.ctypes.data_as(dp), None) == E_ARG
        bad = w.copy()
        bad[1, 2, 3] = np.nan
        assert lib.fdtd2d_batch_set_flux_line_sources(b._h, K, bad.ctypes.data_as(dp), None) == E_ARG
        assert lib.fdtd2d_batch_flux_line_weights(b._h, None, w.ctypes.data_as(dp), 0, None, None) == E_ARG
        with pytest.raises(ValueError):
            b.set_flux_line_sources(cfg["we"][:, :-1], None)
        with pytest.raises(ValueError):
            b.set_flux_line_sources(cfg["we"], cfg["wh"][:, :, :4])
        with pytest.raises(ValueError):
            b.set_flux_line_sources(np.zeros((B, cells, 33)), None)
        # point sources with another channel count, either way round
        b.set_point_sources(np.array([[20, 3]]), np.ones((B, 1, 4)))
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.set_flux_line_sources(cfg["we"], cfg["wh"])
        assert ei.value.code == E_STATE and b.info(23) == 0
        b.set_point_sources(None)
        b.set_flux_line_sources(cfg["we"], cfg["wh"])
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.set_point_sources(np.array([[20, 3]]), np.ones((B, 1, 4)))
        assert ei.value.code == E_STATE and b.info(23) == K
        # a refused call leaves the sources in place and the engine usable: the run equals the plain one
        b.run(NSTEPS, cfg["amps"], cfg["chan"])
        got = b.download()
    want = _device(fd, "per40x17f32", "lds")["fields"]
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", ["mur", "bloch", "lattice"])
def test_batches_without_flux_lines_refuse_line_sources(fd, kind):
    from fdtd2d_amd.api import EPS0, MU0
    boundary = {"mur": "mur", "bloch": "periodic", "lattice": "lattice"}[kind]
    with fd.BatchEngine(2, 40, 17, DT, DX, boundary=boundary) as b:
        b.set_materials(np.full((2, 40, 17), EPS0), np.full((2, 40, 17), MU0))
        if kind == "bloch":
            b.set_bloch_phase(0.4)
            b.set_bloch_flux_lines([("row", 20, 0, 16)], np.array([3e11]))     # Bloch lines are not these lines
        w = np.ones((2, 16, 2))
        rc = fd._abi.load().fdtd2d_batch_set_flux_line_sources(b._h, 2, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                               None)
        assert rc == E_STATE and b.info(23) == 0
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.flux_adjoint_sources(np.ones((2, 1, 1)), np.eye(2))
        assert ei.value.code == E_STATE
