"""CPU-only checks of the line sources and of the adjoint gradients of flux (fdtd2d_batch_flux_adjoint.h, adjoint.py).

The surface: the entry points are declared, exported and bound, the constants are named, bad arguments are refused before
any device is touched, the handle is checked and the package does not import the oracle.

The method: ``batch_flux_gradient`` driven by the stand-in of tests/oracle_batch_flux_adjoint.py in float64, against
central finite differences (h = 1e-4 eps0, 1e-4 S/m) of the stand-in's own flux(); no adjoint code runs on the
finite-difference side.  Two configurations, dx = 1e-3, dt = 1.6e-12, Ricker fc = 40 GHz, 25 / 40 / 55 GHz, 5000 steps, an
8-cell layer, eps random in [1, 3] eps0 on the design window, 8 fixed cells including the window's corners:
  pml       48x48, source (24, 12), design (16, 18, 16, 12), the line ("col", 38, 14, 20): test_batch_adjoint_cpu.py's
            configuration with its probes replaced by the line;
  periodic  48x25, a whole-period source on row 12, design (20, 4, 10, 12) with a conductivity of 0.3-0.6 S/m (which
            also damps the modes the block guides along the columns), the whole-period line ("row", 34, 0, 24) beyond it.
Two objectives: J = sum_k P_k, and J = sum_k w_k P_k^2 / 1e-5 with w = (1, -2, 0.5), whose dJ/dP differs per frequency.
Measured worst error / max|gradient|: pml 8.5e-5 and 1.1e-4 (the two objectives); periodic 1.5e-4 and 9.1e-5 for eps,
2.6e-5 and 4.3e-5 for sigma (the truncation of fields that still ring: residuals 4e-3 and 1e-4).  The bounds are three
times the larger of each pair, all far below 0.03; a wrong sign or factor is above 0.1.
float32 against float64 over the whole window was measured at 1.4e-6 and 1.7e-6 (pml), 1.2e-6 and 6.2e-7 (periodic, eps),
4.7e-7 and 1.2e-6 (periodic, sigma); the bound is 1e-5, the margin of test_batch_adjoint_cpu.py.

The weights: flux_adjoint_sources as the stand-in restates the device kernel against the host path
(adjoint.flux_adjoint_weights), to 1e-12 of max|weight|.

The one-way source: on a periodic vacuum member (64x9, Courant 0.48) an electric sheet s_e on a whole-period row line
and a magnetic sheet s_h(t) = s_e(t - dt/2) / (eta cos(k/2)) on the same line, k the discrete wavenumber of the carrier
(sin(k/2) = sin(omega dt/2) / Courant): the discrete plane-wave relation between Ez and the averaged Hx.  The power
through a line 10 rows behind the pair over the power through a line 10 rows ahead, at the carrier, was measured at
5.4e-9, 1.6e-8 and 3.0e-9 (25, 40, 55 GHz; what is left is the envelope, which the pair treats as constant over half a
step); the bound is three times the largest, 4.8e-8.  The electric sheet alone gives 1.000 (it radiates both ways)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch_flux_adjoint import line_source_oracle_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_flux_adjoint.h")

EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7
DX, DT, FC, NSTEPS, LAYER = 1e-3, 1.6e-12, 40e9, 5000, 8
OMEGAS = 2 * np.pi * np.array([25e9, 40e9, 55e9])
CFG = {"pml": dict(R=48, C=48, source=(24, 12, 1, 1), design=(16, 18, 16, 12), lines=[("col", 38, 14, 20)], sigma=None,
                   cells=[(16, 18), (31, 29), (18, 27), (23, 20), (24, 24), (27, 22), (29, 19), (21, 28)]),
       "periodic": dict(R=48, C=25, source=(12, 0, 1, 24), design=(20, 4, 10, 12), lines=[("row", 34, 0, 24)], sigma=0.3,
                        cells=[(20, 4), (29, 15), (20, 15), (29, 4), (24, 9), (22, 13), (27, 6), (25, 11)])}
FD_BOUND = {("pml", "eps"): 3.4e-4, ("periodic", "eps"): 4.6e-4, ("periodic", "sigma"): 1.3e-4}
ONE_WAY_BOUND = 4.8e-8


def design_eps(c, count=1):
    r0, c0, nr, nc = c["design"]
    eps = np.full((count, c["R"], c["C"]), EPS0)
    for b in range(count):
        eps[b, r0:r0 + nr, c0:c0 + nc] = EPS0 * (1 + 2 * np.random.default_rng(b).random((nr, nc)))
    return eps


def design_sigma(c, count=1):
    if c["sigma"] is None:
        return None
    r0, c0, nr, nc = c["design"]
    s = np.zeros((count, c["R"], c["C"]))
    for b in range(count):
        s[b, r0:r0 + nr, c0:c0 + nc] = c["sigma"] * (1 + np.random.default_rng(10 + b).random((nr, nc)))
    return s


def objective_sum(P):
    return P.sum(axis=(1, 2)), np.ones_like(P)


def objective_weighted(P):
    w = np.array([1.0, -2.0, 0.5])[None, None, :]
    return (w * P * P).sum(axis=(1, 2)) / 1e-5, 2 * w * P / 1e-5


OBJECTIVES = {"sum": objective_sum, "weighted": objective_weighted}


def gradient(fd, config, dtype, objective, nsteps=NSTEPS, engine="stand-in", **kw):
    """batch_flux_gradient on configuration `config` of CFG; kw overrides any argument."""
    c, boundary = CFG[config], config
    args = dict(nsteps=nsteps, sources=np.tile(c["source"], (1, 1)), flux_lines=c["lines"], omegas=OMEGAS,
                design=c["design"], objective=objective, fc=FC, dt=DT, dx=DX, dtype=dtype, boundary=boundary,
                pml_cells=LAYER, engine=line_source_oracle_for(boundary) if engine == "stand-in" else engine)
    args.update(kw)
    eps = args.pop("eps", design_eps(c))
    sigma = args.pop("sigma", design_sigma(c))
    return fd.batch_flux_gradient(eps, sigma, **args)


def oracle_flux(boundary, eps, sigma):
    """flux() of every member from a forward run of the stand-in alone (no adjoint code involved)."""
    from fdtd2d_amd.api import ricker_amplitude
    c, B = CFG[boundary], eps.shape[0]
    amps = np.tile(np.array([ricker_amplitude(n * DT, FC) for n in range(NSTEPS)]), (B, 1))
    eng = line_source_oracle_for(boundary)(B, c["R"], c["C"], DT, DX, dtype=np.float64, boundary=boundary)
    eng.set_materials(eps, MU0)
    eng.set_pml(LAYER, courant00=(1 / np.sqrt(EPS0 * MU0) * DT) / DX)
    if sigma is not None:
        eng.set_conductivity(sigma)
    eng.set_sources(np.tile(c["source"], (B, 1))).set_flux_lines(c["lines"], OMEGAS)
    eng.run(NSTEPS, amps)
    return eng.flux()


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


_grads, _fluxes = {}, {}


def grad64(fd, boundary, name):
    if (boundary, name) not in _grads:
        _grads[boundary, name] = gradient(fd, boundary, np.float64, OBJECTIVES[name])
    return _grads[boundary, name]


def perturbed_flux(boundary):
    """flux() of the members with one cell's eps (then, with a conductivity, sigma) moved up and down: one forward run,
    shared by the objectives."""
    if boundary not in _fluxes:
        c, n = CFG[boundary], len(CFG[boundary]["cells"])
        h, hs = 1e-4 * EPS0, 1e-4
        lossy = c["sigma"] is not None
        eps = np.repeat(design_eps(c), (4 if lossy else 2) * n, axis=0)
        sigma = np.repeat(design_sigma(c), 4 * n, axis=0) if lossy else None
        for k, (r, cc) in enumerate(c["cells"]):
            eps[2 * k, r, cc] += h
            eps[2 * k + 1, r, cc] -= h
            if lossy:
                sigma[2 * n + 2 * k, r, cc] += hs
                sigma[2 * n + 2 * k + 1, r, cc] -= hs
        _fluxes[boundary] = (oracle_flux(boundary, eps, sigma), h, hs)
    return _fluxes[boundary]


# ---- 1. the surface -------------------------------------------------------------------------------------------------

NAMES = ["fdtd2d_batch_flux_line_weights", "fdtd2d_batch_read_flux_line_sources", "fdtd2d_batch_set_flux_line_sources"]


def test_flux_adjoint_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt))) == NAMES
    assert sorted(_abi.BATCH_FLUX_ADJOINT_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared but not exported"
    loaded = _abi.load()
    for n in NAMES:
        assert getattr(loaded, n).argtypes == _abi.BATCH_FLUX_ADJOINT_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_FLUX_ADJOINT_SIGNATURES[n][0]


def test_flux_adjoint_constants_are_named_and_free():
    from fdtd2d_amd import _abi
    txt = open(HEADER).read()
    assert re.search(r"FDTD2D_BATCH_INFO_FLUX_LINE_SOURCES\s*=\s*FDTD2D_BATCH_INFO_FLUX_LDS\s*\+\s*1", txt)
    assert _abi.BATCH_FLUX_LINE_SOURCES_INFO == _abi.BATCH_INFO_FLUX_LDS + 1 == 23
    assert not re.findall(r"#define\s+FDTD2D_BATCH_(?:INFO|OPT)_\w+\s+-?\d+", txt)    # no numbered id of its own
    taken = [v for k, v in vars(_abi).items() if k.startswith("BATCH_INFO_") and isinstance(v, int)]
    assert len(taken) == len(set(taken)) and max(taken) == 22                           # and 23 was free
    assert _abi.BATCH_MAX_CHANNELS == 32


def test_flux_adjoint_python_surface():
    import fdtd2d_amd as fd
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_flux_line_sources).parameters) == ["self", "we", "wh"]
    assert list(inspect.signature(E.flux_adjoint_sources).parameters) == ["self", "dJdP", "solve", "scale_e", "scale_h"]
    assert list(inspect.signature(E.read_flux_line_sources).parameters) == ["self"]
    p = inspect.signature(fd.batch_flux_gradient).parameters
    assert list(p) == ["eps", "sigma", "mu", "nsteps", "sources", "flux_lines", "omegas", "design", "objective", "fc",
                       "waveform", "dt", "dx", "dtype", "boundary", "pml_cells", "device", "engine"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k not in ("eps", "sigma", "mu"))
    assert issubclass(fd.FluxAdjointSession, fd.AdjointSession)
    assert "batch_flux_gradient" in fd.__all__ and "FluxAdjointSession" in fd.__all__
    ref = line_source_oracle_for("pml")
    for name in ("set_flux_lines", "set_flux_line_sources", "read_flux_line_sources", "flux_adjoint_sources", "flux",
                 "read_flux_lines", "run", "reset", "hold_dft_window", "dft_window_product"):
        assert callable(getattr(E, name)) and callable(getattr(ref, name)), name


def test_the_package_does_not_import_the_oracle():
    for name in ("adjoint.py", "batch.py"):
        src = open(os.path.join(ROOT, "fdtd-2d_amd", name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), name


def test_flux_adjoint_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    dp = np.zeros(16).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.fdtd2d_batch_set_flux_line_sources(None, 1, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_flux_line_sources(None, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_flux_line_weights(None, dp, dp, 0, None, None) == _abi.E_ARG


def _no_device(monkeypatch, fd):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)


@pytest.mark.parametrize("kwargs,match", [
    (dict(flux_lines=[("col", 42, 14, 20)]), r"cell \(14, 42\) lies in the 8-cell PML"),
    (dict(flux_lines=[("col", 38, 3, 20)]), r"cell \(3, 38\) lies in the 8-cell PML"),
    (dict(flux_lines=[("col", 30, 14, 20)]), r"cell \(15, 30\) is closer than 2 cells to the design window"),
    (dict(flux_lines=[("row", 15, 20, 6)]), "closer than 2 cells to the design window"),
    (dict(flux_lines=[("col", 13, 14, 20)]), "member 0: .*closer than 2 cells to the forward source"),
    (dict(flux_lines=[("col", 48, 14, 20)]), "column 48 outside"),
    (dict(flux_lines=[("col", 38, 14, 20)] * 5), "1..4 lines"),
    (dict(flux_lines=[("col", 38, 14, 20)], sigma="at the line"), "sigma is non-zero at a flux line cell"),
    (dict(flux_lines=[("col", 38, 14, 20)], mu="step at the line"), "mu differs between the two H values"),
    (dict(boundary="mur"), '"pml" or "periodic"'),
    (dict(design=(7, 18, 16, 12)), "8 cells from every edge.*PML"),
    (dict(omegas=np.ones(17)), "1..16"),
    (dict(nsteps=0), "nsteps"),
])
def test_batch_flux_gradient_refuses_bad_arguments_on_the_host(monkeypatch, kwargs, match):
    import fdtd2d_amd as fd
    _no_device(monkeypatch, fd)
    kwargs = dict(kwargs)
    if kwargs.get("sigma") == "at the line":
        kwargs["sigma"] = np.zeros((1, 48, 48))
        kwargs["sigma"][0, 20, 38] = 0.1
    if kwargs.get("mu") == "step at the line":
        kwargs["mu"] = np.full((1, 48, 48), MU0)
        kwargs["mu"][0, :, 38:] *= 2
    with pytest.raises(ValueError, match=match):
        gradient(fd, "pml", np.float64, objective_sum, nsteps=kwargs.pop("nsteps", 400), engine=None, **kwargs)


def test_objective_shapes_are_checked(fd):
    with pytest.raises(ValueError, match="dJ/dP of shape"):
        gradient(fd, "pml", np.float64, lambda P: (P.sum(axis=(1, 2)), np.ones((1, 3))), nsteps=200)


def test_the_stand_in_refuses_what_the_library_refuses():
    ref = line_source_oracle_for("pml")(1, 48, 48, DT, DX, dtype=np.float64, boundary="pml")
    ref.set_materials(np.full((1, 48, 48), EPS0), MU0).set_pml(LAYER, courant00=0.48)
    with pytest.raises(AssertionError):
        ref.set_flux_line_sources(np.ones((20, 2)), None)               # without lines
    ref.set_flux_lines([("col", 38, 14, 20)], OMEGAS)
    with pytest.raises(AssertionError):
        ref.set_flux_line_sources(np.ones((20, 33)), None)              # K > 32
    with pytest.raises(AssertionError):
        ref.set_flux_line_sources(np.ones((19, 2)), None)               # the wrong number of entries
    ref.set_point_sources(np.array([[20, 20]]), np.ones((1, 4)))
    with pytest.raises(AssertionError):
        ref.set_flux_line_sources(np.ones((20, 2)), None)               # another channel count than the point sources
    ref.set_flux_line_sources(np.ones((20, 4)), np.ones((20, 4)))
    ref.set_flux_lines([("col", 38, 14, 20)], OMEGAS)                   # new lines drop them
    assert ref.linesrc is None


# ---- 2. the method ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(OBJECTIVES))
@pytest.mark.parametrize("boundary", ["pml", "periodic"])
def test_flux_gradient_matches_finite_differences_of_the_oracle(fd, boundary, name):
    c, n = CFG[boundary], len(CFG[boundary]["cells"])
    J, grad, grad_sigma, P, info = grad64(fd, boundary, name)
    r0, c0, nr, nc = c["design"]
    assert grad.shape == (1, nr, nc) and P.shape == (1, 1, 3) and J.shape == (1,) and info["condition"] < 10
    assert (grad_sigma is None) == (c["sigma"] is None)
    Pp, h, hs = perturbed_flux(boundary)
    assert np.array_equal(oracle_flux(boundary, design_eps(c), design_sigma(c)), P)
    Jp = OBJECTIVES[name](Pp)[0]
    for what, g, lo, step in (("eps", grad, 0, h), ("sigma", grad_sigma, 2 * n, hs)):
        if g is None:
            continue
        fdiff = (Jp[lo:lo + 2 * n:2] - Jp[lo + 1:lo + 2 * n:2]) / (2 * step)
        adj = np.array([g[0, r - r0, cc - c0] for r, cc in c["cells"]])
        err = np.abs(adj - fdiff).max() / np.abs(g[0]).max()
        print(f"{boundary} {name} d/d{what}: adjoint vs central FD on {n} cells, worst / max|gradient| = {err:.3e}; "
              f"residuals {info['residual_forward'][0]:.2e} {info['residual_adjoint'][0]:.2e}")
        assert err <= FD_BOUND[boundary, what] < 0.03


# ---- 3. precision ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(OBJECTIVES))
@pytest.mark.parametrize("boundary", ["pml", "periodic"])
def test_flux_gradient_in_float32_agrees_with_float64(fd, boundary, name):
    g64 = grad64(fd, boundary, name)
    g32 = gradient(fd, boundary, np.float32, OBJECTIVES[name])
    for what, a, b in (("eps", g32[1], g64[1]), ("sigma", g32[2], g64[2])):
        if b is None:
            continue
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{boundary} {name} d/d{what}: float32 vs float64 over the window, worst / max|gradient| = {err:.3e}")
        assert err <= 1e-5


# ---- 4. the weights: the device's arithmetic against the host path ------------------------------------------------------

@pytest.mark.parametrize("boundary", ["pml", "periodic"])
def test_device_weights_as_restated_equal_the_host_path(fd, boundary):
    from fdtd2d_amd.adjoint import flux_adjoint_weights
    from fdtd2d_amd.api import ricker_amplitude
    R, C, B, n = 40, 17 if boundary == "periodic" else 40, 2, 300
    lines = [("row", 20, 0, 16), ("col", 12, 15, 10), ("row", 25, 10, 4)]        # the first two cross: a cell twice
    om = 2 * np.pi * np.array([[25e9, 40e9, 55e9], [30e9, 45e9, 60e9]])
    rng = np.random.default_rng(4)
    ref = line_source_oracle_for(boundary)(B, R, C, DT, DX, dtype=np.float64, boundary=boundary)
    ref.set_materials(EPS0 * (1 + rng.random((B, R, C))), MU0).set_pml(LAYER, courant00=0.48)
    ref.set_sources(np.array([[14, 3, 1, 8], [15, 5, 2, 2]])).set_flux_lines(lines, om)
    ref.run(n, np.stack([[ricker_amplitude(k * DT, FC * (1 + 0.2 * m)) for k in range(n)] for m in range(B)]))
    E, H = ref.read_flux_lines(raw=True)
    cells = E.shape[2]
    dJdP, solve = rng.standard_normal((B, 3, 3)), rng.standard_normal((B, 6, 6))
    se, sh = 1 + rng.random((B, cells)), -(1 + rng.random((B, cells)))
    for scales in ((se, sh), (None, None)):
        for s in (solve, solve[0]):
            ref.flux_adjoint_sources(dJdP, s, *scales)
            got = ref.read_flux_line_sources()
            want = flux_adjoint_weights(E, H, dJdP, lines, om, DT, DX, s, *scales)
            for g, w in zip(got, want):
                assert g.shape == w.shape == (B, cells, 6) and np.abs(w).max() > 0
                assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max()
    # the crossing cell's two entries carry their own line's sign and derivative
    k0, k1 = 12, 16 + 5
    assert (ref.fluxmon["i"][k0], ref.fluxmon["j"][k0]) == (ref.fluxmon["i"][k1], ref.fluxmon["j"][k1]) == (20, 12)
    assert not np.allclose(got[0][:, k0], got[0][:, k1])


# ---- 5. the one-way source ---------------------------------------------------------------------------------------------

def _sheet_run(pair):
    """(P ahead, P behind) at the carriers 25 / 40 / 55 GHz, one member each."""
    R, C, rs, d, n = 64, 9, 32, 10, 3000
    om = OMEGAS
    t = np.arange(n) * DT
    env = np.exp(-((t - 4.5 / FC) / (0.9 / FC)) ** 2)
    chan = np.stack([np.stack([env * np.cos(w * t), env * np.sin(w * t)]) for w in om])
    courant, eta = DT / (DX * np.sqrt(EPS0 * MU0)), np.sqrt(MU0 / EPS0)
    theta = om * DT
    k = 2 * np.arcsin(np.sin(theta / 2) / courant)
    alpha = 1 / (eta * np.cos(k / 2))
    lines = [("row", rs, 0, C - 1), ("row", rs + d, 0, C - 1), ("row", rs - d, 0, C - 1)]
    we, wh = np.zeros((3, 3 * (C - 1), 2)), np.zeros((3, 3 * (C - 1), 2))
    we[:, :C - 1, 0] = 1.0                                   # s_e = env cos(omega t)
    wh[:, :C - 1, 0] = (alpha * np.cos(theta / 2))[:, None]  # s_h = alpha env cos(omega (t - dt/2))
    wh[:, :C - 1, 1] = (alpha * np.sin(theta / 2))[:, None]
    eng = line_source_oracle_for("periodic")(3, R, C, DT, DX, dtype=np.float64, boundary="periodic")
    eng.set_materials(np.full((3, R, C), EPS0), MU0).set_pml(LAYER, courant00=courant)
    eng.set_flux_lines(lines, om[:, None]).set_flux_line_sources(we, wh if pair else None)
    eng.run(n, None, chan)
    P = eng.flux()[:, :, 0]
    return P[:, 1], P[:, 2]


def test_an_electric_and_a_magnetic_sheet_radiate_one_way():
    ahead, behind = _sheet_run(True)
    ahead_e, behind_e = _sheet_run(False)
    ratio, ratio_e = np.abs(behind) / ahead, np.abs(behind_e) / ahead_e
    print(f"one-way ratios {ratio}, the electric sheet alone {ratio_e}; ahead {ahead} against {ahead_e}")
    assert np.all(ahead > 0) and np.all(ahead_e > 0) and np.all(behind_e < 0)
    assert np.all(ratio <= ONE_WAY_BOUND) and np.all(ratio < ratio_e)
    assert np.all(np.abs(ratio_e - 1) < 1e-3)               # alone it radiates both ways alike
    assert np.all(np.abs(ahead / ahead_e - 4) < 1e-2)       # and the pair doubles the amplitude ahead
