"""CPU-only checks of the adjoint eps-gradients of the batched engine (fdtd2d_batch_adjoint.h, adjoint.py).

The surface: the entry points are declared, exported and bound, the Python surface has its shape, bad arguments are
refused before any device is touched, and without a device the new calls fail with the library's error.

The method: ``batch_eps_gradient`` driven by the oracle-backed stand-in of tests/oracle_batch.py, on the
configuration the method was worked out on (48x48, dx = 1e-3, dt = 1.6e-12, Ricker fc = 40 GHz at (24, 12), eps random
in [1, 3] eps0 on the design window (16, 18, 16, 12), 8 probes at rows 20..27 of column 38, 25 / 40 / 55 GHz, 5000
steps), against central finite differences (h = 1e-4 eps0) of the same oracle objective J = sum_k mean_p |Eobs[p, k]|.
Measured on that configuration with 24 random cells: pml 1.6e-3, mur 5.0e-3 of max|gradient| (the truncation of fields
that still ring; it falls 120-fold from 2500 to 10000 steps); the bounds are three times that.  A wrong factor in the
formula is above 0.1.  float32 against float64 over the whole window was measured at 1.2e-6 (pml) and 1.6e-6 (mur);
the bound is 1e-5."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch import OracleBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_adjoint.h")

EPS0 = 8.85418e-12
R = C = 48
DX, DT, FC, NSTEPS, LAYER = 1e-3, 1.6e-12, 40e9, 5000, 8
OMEGAS = 2 * np.pi * np.array([25e9, 40e9, 55e9])
SOURCE = (24, 12)
PROBES = np.array([(20 + k, 38) for k in range(8)])
DESIGN = (16, 18, 16, 12)
FD_CELLS = [(16, 18), (31, 29), (18, 27), (23, 20), (24, 24), (27, 22), (29, 19), (21, 28)]   # fixed, window corners in
FD_BOUND = {"pml": 5e-3, "mur": 1.5e-2}


def design_eps(seed=0, count=1):
    eps = np.full((count, R, C), EPS0)
    for b in range(count):
        rng = np.random.default_rng(seed + b)
        eps[b, 16:32, 18:30] = EPS0 * (1 + 2 * rng.random((16, 12)))
    return eps


def objective(spectra):
    """J = sum_k mean_p |Eobs[p, k]| and its cotangent g = dJ/dRe + i dJ/dIm."""
    mag = np.abs(spectra)
    return mag.mean(axis=1).sum(axis=1), spectra / mag / spectra.shape[1]


def gradient(fd, boundary, dtype, eps=None, engine=OracleBatch, nsteps=NSTEPS):
    eps = design_eps() if eps is None else eps
    B = eps.shape[0]
    return fd.batch_eps_gradient(eps, nsteps=nsteps, sources=np.tile(SOURCE, (B, 1)), probes=PROBES, omegas=OMEGAS,
                                 design=DESIGN, objective=objective, fc=FC, dt=DT, dx=DX, dtype=dtype,
                                 boundary=boundary, pml_cells=LAYER, engine=engine)


def oracle_objective(boundary, eps):
    """J of every member of eps from a forward run of the stand-in alone (no adjoint code involved)."""
    from fdtd2d_amd.adjoint import probe_spectra
    from fdtd2d_amd.api import ricker_amplitude
    B = eps.shape[0]
    amps = np.tile(np.array([ricker_amplitude(n * DT, FC) for n in range(NSTEPS)]), (B, 1))
    eng = OracleBatch(B, R, C, DT, DX, dtype=np.float64, boundary=boundary)
    eng.set_materials(eps, 4 * np.pi * 1e-7)
    if boundary == "pml":
        eng.set_pml(LAYER, courant00=(1 / np.sqrt(EPS0 * 4 * np.pi * 1e-7) * DT) / DX)
    eng.set_sources(np.tile(SOURCE, (B, 1))).set_probes(PROBES, NSTEPS)
    eng.run(NSTEPS, amps)
    return objective(probe_spectra(eng.read_probes(), np.tile(OMEGAS, (B, 1)), DT))[0]


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


_cache = {}


def grad64(fd, boundary):
    if boundary not in _cache:
        _cache[boundary] = gradient(fd, boundary, np.float64)
    return _cache[boundary]


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_batch_adjoint_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["fdtd2d_batch_dft_window_product", "fdtd2d_batch_hold_dft_window", "fdtd2d_batch_run_channels",
                     "fdtd2d_batch_set_point_sources"]
    assert sorted(_abi.BATCH_ADJOINT_SIGNATURES) == names
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared but not exported"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_ADJOINT_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_ADJOINT_SIGNATURES[n][0]


def test_batch_adjoint_constants_are_named_and_free():
    from fdtd2d_amd import _abi
    defs = dict(re.findall(r"#define\s+FDTD2D_(BATCH_\w+)\s+(-?\d+)", open(HEADER).read()))
    assert defs == {"BATCH_INFO_POINT_SOURCES": "12", "BATCH_INFO_HELD_WINDOW": "13",
                    "BATCH_MAX_POINT_SOURCES": "64", "BATCH_MAX_CHANNELS": "32"}
    for k, v in defs.items():
        assert getattr(_abi, k) == int(v), k
    taken = {}
    for h in ("fdtd2d.h", "fdtd2d_batch_pml.h", "fdtd2d_batch_monitor.h"):
        taken.update(re.findall(r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)",
                                open(os.path.join(ROOT, "include", h)).read()))
    assert max(int(v) for k, v in taken.items() if k.startswith("BATCH_INFO")) == 11


def test_batch_adjoint_python_surface():
    import fdtd2d_amd as fd
    E = fd.BatchEngine
    p = inspect.signature(E.run).parameters
    assert list(p) == ["self", "nsteps", "amps", "channels"] and p["amps"].default is None
    assert p["channels"].default is None
    assert list(inspect.signature(E.set_point_sources).parameters) == ["self", "cells", "weights"]
    assert list(inspect.signature(E.hold_dft_window).parameters) == ["self"]
    assert list(inspect.signature(E.dft_window_product).parameters) == ["self", "coef"]
    p = inspect.signature(fd.batch_eps_gradient).parameters
    assert list(p) == ["eps", "mu", "nsteps", "sources", "probes", "omegas", "design", "objective", "fc", "waveform",
                       "dt", "dx", "dtype", "boundary", "pml_cells", "device", "engine"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k not in ("eps", "mu"))
    want = dict(mu=None, fc=30e9, waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml",
                pml_cells=40, device=0, engine=None)
    assert {k: p[k].default for k in want} == want
    assert "batch_eps_gradient" in fd.__all__
    # the stand-in offers what the helper calls on an engine
    for name in ("set_materials", "set_pml", "set_sources", "set_dft_window", "set_probes", "run", "read_probes",
                 "download", "hold_dft_window", "reset", "set_point_sources", "dft_window_product"):
        assert callable(getattr(E, name)) and callable(getattr(OracleBatch, name)), name


def test_the_package_does_not_import_the_oracle():
    for name in ("adjoint.py", "batch.py"):
        src = open(os.path.join(ROOT, "fdtd-2d_amd", name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), name


def _no_device(monkeypatch, fd):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)


@pytest.mark.parametrize("kwargs,match", [
    (dict(sources=np.array([[24, 12], [24, 19]])), "member 1: .*forward source"),
    (dict(design=(5, 18, 16, 12), boundary="mur"), "6 cells from every edge"),
    (dict(design=(16, 18, 27, 12), boundary="mur"), "6 cells from every edge"),
    (dict(design=(7, 18, 16, 12)), "8 cells from every edge.*PML"),
    (dict(design=(16, 18, 0, 12)), "empty"),
    (dict(design=(16, 18, 16)), "4 integers"),
    (dict(boundary="none"), "rings down"),
    (dict(omegas=2 * np.pi * np.array([40e9, 40e9 * (1 + 1e-13)])), "member 0: .*condition number"),
    (dict(omegas=np.ones(17)), "1..16"),
    (dict(probes=np.zeros((65, 2), int)), "1..64"),
    (dict(probes=[[20, 38], [20, 38]]), "member 0: .*twice"),
    (dict(probes=[[48, 3]]), "in the 48x48 grid"),
    (dict(pml_cells=23), "does not fit"),
    (dict(nsteps=0), "nsteps"),
])
def test_batch_eps_gradient_refuses_bad_arguments_on_the_host(monkeypatch, kwargs, match):
    import fdtd2d_amd as fd
    _no_device(monkeypatch, fd)
    args = dict(nsteps=400, sources=np.array([[24, 12], [24, 12]]), probes=PROBES, omegas=OMEGAS, design=DESIGN,
                objective=objective, fc=FC, dt=DT, dx=DX, boundary="pml", pml_cells=LAYER)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        fd.batch_eps_gradient(design_eps(count=2), **args)


def test_batch_adjoint_without_a_device_has_no_fallback():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 4, 40, 40, 5e-14, 1e-4, _abi.F32, _abi.BOUNDARY_MUR5, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    import fdtd2d_amd as fd
    with pytest.raises(fd.Fdtd2dError) as ei:
        gradient(fd, "pml", np.float32, engine=None, nsteps=400)
    assert ei.value.code == _abi.E_NODEVICE


def test_batch_adjoint_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cells = np.zeros(2, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_point_sources(None, 1, cells, 1, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_run_channels(None, 1, None, dp, 0) == _abi.E_ARG
    assert lib.fdtd2d_batch_hold_dft_window(None) == _abi.E_ARG
    assert lib.fdtd2d_batch_dft_window_product(None, dp, dp, dp) == _abi.E_ARG


# ---- 2. the method ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_adjoint_gradient_matches_finite_differences_of_the_oracle(fd, boundary):
    J, grad, spectra, info = grad64(fd, boundary)
    assert grad.shape == (1, 16, 12) and spectra.shape == (1, 8, 3) and J.shape == (1,)
    assert info["condition"] < 10
    gmax = np.abs(grad[0]).max()
    h = 1e-4 * EPS0
    eps = np.repeat(design_eps(), 2 * len(FD_CELLS), axis=0)
    for k, (r, c) in enumerate(FD_CELLS):
        eps[2 * k, r, c] += h
        eps[2 * k + 1, r, c] -= h
    Jp = oracle_objective(boundary, eps)
    assert np.array_equal(oracle_objective(boundary, design_eps()), J)
    fdiff = (Jp[0::2] - Jp[1::2]) / (2 * h)
    adj = np.array([grad[0, r - DESIGN[0], c - DESIGN[1]] for r, c in FD_CELLS])
    err = np.abs(adj - fdiff).max() / gmax
    print(f"{boundary}: adjoint vs central FD on {len(FD_CELLS)} cells, worst / max|gradient| = {err:.3e}; "
          f"residuals {info['residual_forward'][0]:.2e} {info['residual_adjoint'][0]:.2e}")
    assert err <= FD_BOUND[boundary]


# ---- 3. precision ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_adjoint_gradient_in_float32_agrees_with_float64(fd, boundary):
    g64 = grad64(fd, boundary)[1]
    g32 = gradient(fd, boundary, np.float32)[1]
    err = np.abs(g32 - g64).max() / np.abs(g64).max()
    print(f"{boundary}: float32 vs float64 adjoint over the window, worst / max|gradient| = {err:.3e}")
    assert err <= 1e-5
