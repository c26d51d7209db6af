"""CPU-only checks of dispersive (Drude-Lorentz) materials in the batched engine (fdtd2d_batch_dispersive.h, batch.py,
adjoint.py), on the stand-in of tests/oracle_batch_dispersive.py.

The surface: the three entry points are declared, exported and bound, the constant is named and its id free, the Python
surface has its shape, bad arguments are refused before any device is touched, and without a device nothing falls back.

The arithmetic: with wp2 = 0 the stand-in equals the lossy and the periodic stand-ins bit for bit; a periodic member of
period Q equals both halves of a member of period 2Q, Jh and Q included.

The physics: a periodic, column-uniform member (220 x 5, a 20-cell layer on the rows, dt = 5e-14, dx = 1e-4) with a 20-cell
slab, a Ricker line source at 60 GHz and 6000 steps; the probe spectrum behind the slab over the same run without the
slab, at 40, 50, 60, 70 and 80 GHz, against |T| of the analytic slab formula for eps(w) = 1 + chi(w).  Worst error of
the stand-in itself, the same in float32 and float64 to three digits:
    Drude    wp = 2 pi 70 GHz, gamma = 1e11              8.3e-4     bound 1.7e-3
    Lorentz  d_eps = 3 at 60 GHz, gamma = 6e10           4.7e-3     bound 9.4e-3
The bound is twice the measured error (the scheme's own dispersion error at 50 cells per wavelength and what the layer
reflects).  Without the pole the same check misses by 0.84 and 1.0.

Stability: a lossless member whose cells sit at 3.9 on dt^2 (omega0^2 + wp2 EPS0 / eps) + 8 dt^2 / (eps mu dx^2) stays
bounded over 5000 steps (see test_a_lossless_pole_at_3p9_stays_bounded)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch_dispersive import (DispersivePeriodicOracle, DispersivePmlOracle, EPS0, pole_coefficients,
                                     stability)
from oracle_batch_lossy import LossyOracle
from oracle_batch_periodic import PeriodicOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_dispersive.h")
NAMES = ["fdtd2d_batch_set_dispersion", "fdtd2d_batch_set_dispersion_window", "fdtd2d_batch_transfer_dispersion"]
MU0 = 4 * np.pi * 1e-7
DT, DX = 5e-14, 1e-4
COURANT0 = (1 / np.sqrt(EPS0 * MU0) * DT) / DX

# the slab case
SLAB_R, SLAB_C, SLAB_L, SLAB_SRC, SLAB_ROWS, SLAB_PROBE, SLAB_STEPS = 220, 5, 20, 40, (100, 120), 170, 6000
FREQS = np.array([40e9, 50e9, 60e9, 70e9, 80e9])
POLES = {"drude": ((2 * np.pi * 70e9) ** 2, 1e11, 0.0),
         "lorentz": (3 * (2 * np.pi * 60e9) ** 2, 6e10, 2 * np.pi * 60e9)}
SLAB_MEASURED = {"drude": 8.3e-4, "lorentz": 4.7e-3}
SLAB_BOUND = {k: 2 * v for k, v in SLAB_MEASURED.items()}


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- the surface ----------------------------------------------------------------------------------------------------

def test_batch_dispersive_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_DISPERSIVE_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_DISPERSIVE_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_DISPERSIVE_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "const void *": ctypes.c_void_p,
             "void *": ctypes.c_void_p, "const int": ctypes.POINTER(ctypes.c_int),
             "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = []
        for a in args.split(","):
            a = " ".join(a.split())
            got.append(kinds[re.match(r"(.*?[ *])\w+(\[4\])?$", a).group(1).strip()])
        assert got == _abi.BATCH_DISPERSIVE_SIGNATURES[n][1], n


def test_batch_dispersive_constant_is_named_and_its_id_free():
    from fdtd2d_amd import _abi
    pat = r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)"
    mine = dict(re.findall(pat, open(HEADER).read()))
    assert mine == {"BATCH_INFO_DISPERSIVE": "19"} and _abi.BATCH_INFO_DISPERSIVE == 19
    taken = {}
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != os.path.basename(HEADER):
            taken.update(re.findall(pat, open(os.path.join(ROOT, "include", h)).read()))
    assert max(int(v) for k, v in taken.items() if k.startswith("BATCH_INFO")) == 18
    assert "BATCH_INFO_DISPERSIVE" not in taken


def test_batch_dispersive_python_surface():
    import fdtd2d_amd as fd
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_dispersion).parameters) == ["self", "wp2", "gamma", "omega0"]
    assert list(inspect.signature(E.set_dispersion_window).parameters) == ["self", "window", "wp2"]
    assert isinstance(E.dispersive, property)
    assert list(inspect.signature(E.download_dispersion).parameters) == ["self"]
    assert list(inspect.signature(E.upload_dispersion).parameters) == ["self", "Jh", "Q"]
    p = inspect.signature(fd.run_fdtd_batch).parameters
    assert p["dispersion"].default is None and p["dispersion"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (DispersivePmlOracle, DispersivePeriodicOracle):
        for name in ("set_dispersion", "set_dispersion_window", "download_dispersion", "upload_dispersion"):
            assert callable(getattr(cls, name))


def test_batch_dispersive_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    w = np.array([1, 1, 2, 2], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_dispersion(None, d.ctypes.data, _abi.F64, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_dispersion_window(None, w, d.ctypes.data, _abi.F64) == _abi.E_ARG
    assert lib.fdtd2d_batch_transfer_dispersion(None, d.ctypes.data, d.ctypes.data, _abi.F64, 0) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_INFO_DISPERSIVE) == _abi.E_ARG


def test_batch_dispersive_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 2, 40, 40, DT, DX, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, 40, 40), EPS0), nsteps=10, sources=np.array([[20, 20]] * 2), boundary="pml",
                          pml_cells=8, dispersion=(1e22, 1e11, 0.0))
    assert ei.value.code == _abi.E_NODEVICE


# ---- 1. wp2 = 0 is the stand-in without the pole ------------------------------------------------------------------------

def _members(boundary, dtype, R, C, seed=0):
    """Two members with random materials, a conductivity, a source, a window, probes and a random state."""
    rng = np.random.default_rng(seed)
    periodic = boundary == "periodic"
    cls = DispersivePeriodicOracle if periodic else DispersivePmlOracle
    eng = cls(2, R, C, DT, DX, dtype=dtype, boundary=boundary)
    eng.set_materials(EPS0 * (1 + rng.random((2, R, C))), MU0 * (1 + rng.random((2, R, C))))
    eng.set_pml(4, courant00=COURANT0)
    g = eng.margin()
    sigma = np.zeros((2, R, C))
    if periodic:
        sigma[:, g:R - g, :] = 0.3 * rng.random((2, R - 2 * g, C))
    else:
        sigma[:, g:R - g, g:C - g] = 0.3 * rng.random((2, R - 2 * g, C - 2 * g))
    eng.set_conductivity(sigma)
    eng.set_sources(np.array([[9, 3, 2, 2], [10, 4, 1, 3]]))
    eng.set_dft_window((7, 2, 5, 6), 2 * np.pi * np.array([30e9, 55e9]), every=2)
    eng.set_probes(np.array([[8, 0], [11, C - 1], [12, 5]]), 40)
    eng.upload(rng.standard_normal((2, R, C)), rng.standard_normal((2, R, C - 1)), rng.standard_normal((2, R - 1, C)))
    return eng, rng


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("boundary", ["pml", "periodic"])
def test_zero_strength_leaves_the_stand_in_bit_identical(boundary, dtype):
    R, C = 23, 19 if boundary == "pml" else 11
    amps = np.random.default_rng(5).standard_normal((2, 40))
    out = []
    for wp2 in (None, 0.0):
        eng, _ = _members(boundary, dtype, R, C)
        if wp2 is not None:
            eng.set_dispersion(wp2, np.array([1e11, 0.0]), np.array([0.0, 3e11]))
        assert eng.dispersive == (wp2 is not None)
        eng.run(40, amps)
        out.append(eng.download() + (eng.download_ezx() if boundary == "periodic" else eng.Ezx.copy(),
                                     eng.read_dft_window(), eng.read_probes()))
        if wp2 is not None:
            assert not np.any(eng.Jh) and not np.any(eng.Q)
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    # and the class without the pole is the one it is built on
    base = (PeriodicOracle if boundary == "periodic" else LossyOracle)(2, R, C, DT, DX, dtype=dtype, boundary=boundary)
    eng, _ = _members(boundary, dtype, R, C)
    for k in ("eps", "mu", "sigma", "profiles", "rects"):
        setattr(base, k, getattr(eng, k))
    base.upload(eng.Ez, eng.Hx, eng.Hy)
    base.run(40, amps)
    for a, b in zip(base.download(), out[1][:3]):
        assert np.array_equal(a, b)


def test_zero_strength_coefficients_are_exact_zeros():
    for dtype in (np.float32, np.float64):
        a, ck, cj = pole_coefficients(np.zeros(5), 1e11, 3e11, DT, DX, dtype)
        assert a.dtype == ck.dtype == cj.dtype == dtype and not np.any(cj)
        a, ck, cj = pole_coefficients(np.ones(5), 0.0, 0.0, DT, DX, dtype)
        assert a == 1 and ck == 0


# ---- 2. a member of period Q is both halves of a member of period 2Q --------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_period_equals_both_halves_of_two_periods(dtype):
    R, Q, L = 25, 7, 4
    rng = np.random.default_rng(11)
    eps1, mu1 = EPS0 * (1 + rng.random((R, Q))), MU0 * (1 + rng.random((R, Q)))
    wp1 = np.zeros((R, Q))
    wp1[6:R - 6] = (2 * np.pi * 70e9) ** 2 * rng.random((R - 12, Q))
    sg1 = np.zeros((R, Q))
    sg1[6:R - 6] = 0.2 * rng.random((R - 12, Q))
    state = [rng.standard_normal((R, Q)) for _ in range(6)]      # Ez, Hx, Hy, Ezx, Jh, Q
    amps = rng.standard_normal((1, 60))

    def build(periods):
        def tile(a, cols):          # `periods` copies and the image column (or one short, for Hx)
            return np.concatenate([a] * periods + [a[:, :1]], axis=1)[None, :, :cols]
        C = periods * Q + 1
        eng = DispersivePeriodicOracle(1, R, C, DT, DX, dtype=dtype)
        eng.set_materials(tile(eps1, C), tile(mu1, C)).set_pml(L, courant00=COURANT0)
        eng.set_conductivity(tile(sg1, C))
        eng.set_dispersion(tile(wp1, C), 8e10, 2 * np.pi * 50e9)
        eng.set_sources(np.array([[9, 0, 1, C - 1]]))
        eng.upload(tile(state[0], C), tile(state[1], C - 1), tile(state[2], C)[:, :R - 1])
        eng.upload_ezx(tile(state[3], C))
        eng.upload_dispersion(tile(state[4], C), tile(state[5], C))
        eng.run(60, amps)
        return eng.download() + (eng.download_ezx(),) + eng.download_dispersion()

    one, two = build(1), build(2)
    for name, a, b in zip(("Ez", "Hx", "Hy", "Ezx", "Jh", "Q"), one, two):
        n = Q if name in ("Hx", "Hy") else Q + 1        # Hy's column C-1 is never updated
        assert np.array_equal(a[..., :n], b[..., :n]), name
        assert np.array_equal(a[..., :n], b[..., Q:Q + n]), name
    assert np.any(one[4]) and np.any(one[5])


# ---- 3. transmission through a dispersive slab --------------------------------------------------------------------------

def slab_spectrum(dtype, pole):
    """The probe spectrum at FREQS behind the slab (pole None: no slab)."""
    from fdtd2d_amd.api import ricker_amplitude
    R, C = SLAB_R, SLAB_C
    eng = DispersivePeriodicOracle(1, R, C, DT, DX, dtype=dtype)
    eng.set_materials(np.full((1, R, C), EPS0), MU0)
    eng.set_pml(SLAB_L, courant00=COURANT0)
    w = np.zeros((1, R, C))
    w[:, SLAB_ROWS[0]:SLAB_ROWS[1], :] = 0.0 if pole is None else pole[0]
    eng.set_dispersion(w, *((0.0, 0.0) if pole is None else pole[1:]))
    eng.set_sources(np.array([[SLAB_SRC, 0, 1, C - 1]]))
    eng.set_probes(np.array([[SLAB_PROBE, 1]]), SLAB_STEPS)
    eng.run(SLAB_STEPS, np.array([[ricker_amplitude(n * DT, 60e9) for n in range(SLAB_STEPS)]]))
    tr = eng.read_probes()[0, 0]
    t = (np.arange(SLAB_STEPS) + 1) * DT
    return np.array([np.sum(tr * np.exp(-2j * np.pi * f * t)) for f in FREQS])


def slab_transmission(pole):
    """|T| of a slab of thickness d in vacuum at normal incidence, eps(w) = 1 + wp2 / (omega0^2 - w^2 - i gamma w)."""
    wp2, gamma, omega0 = pole
    w = 2 * np.pi * FREQS
    n = np.sqrt((1 + wp2 / (omega0 ** 2 - w ** 2 - 1j * gamma * w)).astype(complex))
    n = np.where(n.imag < 0, -n, n)
    ph = np.exp(1j * w * np.sqrt(EPS0 * MU0) * n * (SLAB_ROWS[1] - SLAB_ROWS[0]) * DX)
    return np.abs(4 * n * ph / ((1 + n) ** 2 - (1 - n) ** 2 * ph ** 2))


_vacuum = {}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["drude", "lorentz"])
def test_slab_transmission_follows_the_analytic_formula(kind, dtype):
    if dtype not in _vacuum:
        _vacuum[dtype] = slab_spectrum(dtype, None)
    T = np.abs(slab_spectrum(dtype, POLES[kind])) / np.abs(_vacuum[dtype])
    want = slab_transmission(POLES[kind])
    err = np.abs(T - want).max()
    print(f"{kind} {np.dtype(dtype).name}: worst error in |T| {err:.3e} (bound {SLAB_BOUND[kind]:.1e})")
    assert err <= SLAB_BOUND[kind]
    # the run without the pole transmits everything: it cannot pass
    assert np.abs(1.0 - want).max() > 0.3


# ---- 4. the stability bound ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["drude", "lorentz"])
def test_a_lossless_pole_at_3p9_stays_bounded(kind):
    """gamma = 0, no conductivity, PEC rows and periodic columns: nothing leaves or damps.  Every cell that may carry the
    pole sits at 3.9 on the stability expression.  A stable leapfrog conserves a positive quadratic form of its state, so
    max|Ez| stays of the order of what the source put in; an unstable one grows by a fixed factor per step (the 1-D
    probe at 4.05 overflowed).  Measured: the largest |Ez| of steps 1000..5000 is 0.27 (Drude) and 1.1 (Lorentz) times
    that of the first 1000; the bound is 10: no growth beyond what redistributing the conserved form among its terms
    allows, and a decade under what any growth rate visible in 4000 steps would reach."""
    R, C, N = 30, 9, 5000
    omega0 = 0.0 if kind == "drude" else 1.0 / DT
    courant = 8 * DT * DT / (EPS0 * MU0 * DX * DX)
    wp2 = (3.9 - courant - (DT * omega0) ** 2) / (DT * DT)
    assert abs(stability(wp2, omega0, EPS0, MU0, DT, DX) - 3.9) < 1e-12
    eng = DispersivePeriodicOracle(1, R, C, DT, DX, dtype=np.float32)
    eng.set_materials(np.full((1, R, C), EPS0), MU0)
    eng.set_dispersion(wp2, 0.0, omega0)
    assert np.count_nonzero(eng.wp2) == (R - 12) * C
    eng.set_sources(np.array([[3, 2, 1, 1]]))
    eng.set_probes(np.array([[r, c] for r in (4, 10, 15, 20) for c in (1, 5)]), N)
    amps = np.zeros((1, N))
    amps[0, :200] = np.sin(2 * np.pi * 60e9 * DT * np.arange(200)) * np.hanning(200)
    eng.run(N, amps)
    tr = np.abs(eng.read_probes()[0])
    assert np.all(np.isfinite(eng.Ez)) and np.all(np.isfinite(eng.Q))
    early, late = tr[:, :1000].max(), tr[:, 1000:].max()
    print(f"{kind}: early {early:.3e} late {late:.3e} ratio {late / early:.3f}")
    assert early > 0 and late <= 10 * early


# ---- 5. the host refusals -----------------------------------------------------------------------------------------------

def test_the_stand_in_refuses_what_the_library_refuses():
    eng = DispersivePmlOracle(2, 23, 19, DT, DX, dtype=np.float32)
    eng.set_materials(np.full((2, 23, 19), EPS0), MU0).set_pml(4, courant00=COURANT0)
    ok = np.zeros((2, 23, 19))
    ok[:, 6:17, 6:13] = 1e22
    eng.set_dispersion(ok, 1e11, 0.0)
    for bad, at in ((-1.0, (1, 10, 10)), (np.nan, (0, 10, 10)), (np.inf, (0, 10, 10)), (1e22, (1, 5, 10)),
                    (1e22, (1, 10, 13)), (4.0 / DT ** 2, (0, 10, 10))):
        w = ok.copy()
        w[at] = bad
        with pytest.raises(AssertionError):
            eng.set_dispersion(w, 1e11, 0.0)
    for gamma, omega0 in ((-1.0, 0.0), (np.nan, 0.0), (0.0, -1.0), (0.0, np.inf)):
        with pytest.raises(AssertionError):
            eng.set_dispersion(ok, gamma, omega0)
    with pytest.raises(AssertionError):
        eng.set_dispersion(ok, 0.0, 2.0 / DT)                    # omega0 alone breaks the bound
    with pytest.raises(AssertionError):
        DispersivePmlOracle(1, 23, 19, boundary="mur")
    per = DispersivePeriodicOracle(1, 23, 11, DT, DX, dtype=np.float32)
    per.set_materials(np.full((1, 23, 11), EPS0), MU0)
    with pytest.raises(AssertionError):
        per.set_dispersion_window((8, 0, 2, 2), np.ones((1, 2, 2)))          # no pole yet
    w = np.zeros((1, 23, 11))
    w[:, 6:17, :] = 1e22                                                   # every column of the period, the image too
    per.set_dispersion(w, 0.0, 0.0)
    w[:, 5, 3] = 1e22
    with pytest.raises(AssertionError):
        per.set_dispersion(w, 0.0, 0.0)
    assert per.dispersive and np.count_nonzero(per.wp2) == 11 * 11


@pytest.mark.parametrize("kwargs,match", [
    (dict(boundary="mur"), 'dispersion needs boundary="pml" or "periodic"'),
    (dict(boundary="none"), 'dispersion needs boundary="pml" or "periodic"'),
    (dict(boundary="periodic", bloch_phase=0.3), "dispersion is not available with bloch_phase"),
    (dict(boundary="pml", dispersion=(1e22, 1e11)), r"dispersion must be \(wp2, gamma, omega0\)"),
])
def test_run_fdtd_batch_refuses_bad_dispersion_on_the_host(monkeypatch, kwargs, match):
    import fdtd2d_amd as fd

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    args = dict(nsteps=10, sources=np.array([[20, 20]] * 2), pml_cells=8, dispersion=(1e22, 1e11, 0.0))
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        fd.run_fdtd_batch(np.full((2, 40, 40), EPS0), **args)


def test_the_adjoint_helpers_refuse_a_dispersive_engine(fd):
    """An engine factory that sets a pole: batch_eps_gradient, batch_material_gradient and AdjointSession raise E_STATE
    before any run."""
    import test_batch_adjoint_cpu as cpu
    from fdtd2d_amd import _abi

    class Dispersive(DispersivePmlOracle):
        ran = False

        def __init__(self, *a, **k):
            DispersivePmlOracle.__init__(self, *a, **k)
            self.wp2 = np.zeros((self.count, self.rows, self.cols))
            self.gamma = self.omega0 = np.zeros(self.count)

        def run(self, *a, **k):
            Dispersive.ran = True
            return DispersivePmlOracle.run(self, *a, **k)

    eps = cpu.design_eps(count=2)
    args = dict(nsteps=50, sources=np.tile(cpu.SOURCE, (2, 1)), probes=cpu.PROBES, omegas=cpu.OMEGAS, design=cpu.DESIGN,
                fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, dtype=np.float64, boundary="pml", pml_cells=cpu.LAYER, engine=Dispersive)
    for call in (lambda: fd.batch_eps_gradient(eps, objective=cpu.objective, **args),
                 lambda: fd.batch_material_gradient(eps, np.zeros(eps.shape), objective=cpu.objective, **args),
                 lambda: fd.AdjointSession(eps, **args)):
        with pytest.raises(fd.Fdtd2dError, match="dispersive pole") as ei:
            call()
        assert ei.value.code == _abi.E_STATE
    assert not Dispersive.ran
    with pytest.raises(AssertionError):
        Dispersive(1, 23, 19).hold_dft_window()
