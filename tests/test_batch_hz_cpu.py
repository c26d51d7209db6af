"""CPU-only checks of the Hz polarisation of PML and periodic batches (fdtd2d_batch_hz.h, batch.py), on the stand-in of
tests/oracle_batch_hz.py.

The surface: the five entry points are declared, exported and bound, the header adds no numbered info id, the Python
surface has its shape, bad arguments are refused before any device is touched, and without a device nothing falls back.

1. Duality.  The pole-free stand-in equals the Ez stand-ins (PeriodicOracle, LossyOracle) with eps and mu exchanged and E
   negated, bit for bit: Hz = Ez, Ex = -Hx, Ey = -Hy.  Zero sigma, zero wp2 and zero state equal the pole-free run.

2. Polariser.  Periodic 121 x 9, a 12-cell layer, float64, vacuum; Drude strips (wp = 2e13 rad/s, gamma = 1e11) on rows
   60-61, columns 0-3 of the 8-cell period; a row-line Ricker source at 45 GHz on row 20; the window DFT of row 95 at 30,
   45 and 60 GHz over 6000 steps.  T = sum |F|^2 with the strips over the same without them.  Measured with this stand-in:
       Hz   0.97981  0.95641  0.92541        (E across the wires: they pass)
       Ez   0.00130  0.00297  0.00537        (E along the wires: they reflect; periodic_step_dispersive)
   asserted: T_hz > 0.9 and T_ez < 0.01 at all three.

3. Drude slab.  The same member with wp2 = (6e11)^2, gamma = 5e10 on rows 60-63 across the period, against
   t = 1 / (cos(n k0 d) - (i/2)(n + 1/n) sin(n k0 d)), n^2 = 1 - wp^2 / (w^2 + i gamma w), d = 4 dx:
       analytic  0.27896  0.45896  0.60370
       Hz        0.28124  0.46132  0.60520      worst |T_hz - analytic| = 2.4e-3   (bound 5e-3: twice the staircase error)
       Ez        0.28125  0.46130  0.60522      worst |T_hz - T_ez|     = 1.7e-5   (bound 1e-4: at normal incidence on a
                                                                                     uniform slab the two are degenerate)
   (the two margins re-measured with this stand-in: see test_drude_slab_follows_the_analytic_formula)."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from oracle_batch_dispersive import DispersivePeriodicOracle, EPS0
from oracle_batch_hz import HzPeriodicOracle, HzPmlOracle
from oracle_batch_lossy import LossyOracle
from oracle_batch_periodic import PeriodicOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_hz.h")
NAMES = ["fdtd2d_batch_polarization", "fdtd2d_batch_set_hz_conductivity", "fdtd2d_batch_set_hz_dispersion",
         "fdtd2d_batch_set_polarization", "fdtd2d_batch_transfer_hz_dispersion"]
MU0 = 4 * np.pi * 1e-7
DT, DX = 5e-14, 1e-4
COURANT0 = (1 / np.sqrt(EPS0 * MU0) * DT) / DX

# the polariser and the slab
G_R, G_C, G_L, G_SRC, G_MON, G_STEPS = 121, 9, 12, 20, 95, 6000
FREQS = np.array([30e9, 45e9, 60e9])
SLAB_ANALYTIC = np.array([0.27896, 0.45896, 0.60370])


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- the surface ----------------------------------------------------------------------------------------------------

def test_batch_hz_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_HZ_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_HZ_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_HZ_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "const fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int,
             "const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_HZ_SIGNATURES[n][1], n


def test_batch_hz_adds_no_numbered_info_id():
    from fdtd2d_amd import _abi
    txt = open(HEADER).read()
    assert not re.findall(r"#define\s+FDTD2D_BATCH_(?:INFO|OPT)_\w+", txt)
    assert dict(re.findall(r"#define\s+FDTD2D_(POL_\w+)\s+(\d+)", txt)) == {"POL_EZ": "0", "POL_HZ": "1"}
    assert (_abi.POL_EZ, _abi.POL_HZ) == (0, 1)
    assert max(v for k, v in vars(_abi).items() if k.startswith("BATCH_INFO_") and isinstance(v, int)) == 22


def test_batch_hz_python_surface():
    import fdtd2d_amd as fd
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_polarization).parameters) == ["self", "polarization"]
    assert isinstance(E.polarization, property)
    assert list(inspect.signature(E.upload_hz_dispersion).parameters) == ["self", "Jx", "Qx", "Jy", "Qy"]
    p = inspect.signature(fd.run_fdtd_batch).parameters
    assert p["polarization"].default == "ez" and p["polarization"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["conductivity"].default is None and p["conductivity"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (HzPmlOracle, HzPeriodicOracle):
        for name in ("set_conductivity", "set_dispersion", "download_dispersion", "upload_dispersion",
                     "upload_hz_dispersion"):
            assert callable(getattr(cls, name))
        assert cls.polarization == "hz"


def test_batch_hz_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.fdtd2d_batch_set_polarization(None, _abi.POL_HZ) == _abi.E_ARG
    assert lib.fdtd2d_batch_polarization(None) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_hz_conductivity(None, d.ctypes.data, _abi.F64) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_hz_dispersion(None, d.ctypes.data, _abi.F64, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_transfer_hz_dispersion(None, d.ctypes.data, None, None, None, _abi.F64, 0) == _abi.E_ARG


def test_batch_hz_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 2, 40, 40, DT, DX, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, 40, 40), EPS0), nsteps=10, sources=np.array([[20, 20]] * 2), boundary="pml",
                          pml_cells=8, polarization="hz", dispersion=(1e22, 1e11, 0.0))
    assert ei.value.code == _abi.E_NODEVICE


@pytest.mark.parametrize("kwargs,match", [
    (dict(polarization="te"), 'polarization must be "ez" or "hz"'),
    (dict(polarization="hz", boundary="mur"), 'polarization="hz" needs boundary="pml" or "periodic"'),
    (dict(polarization="hz", boundary="lattice"), 'polarization="hz" needs boundary="pml" or "periodic"'),
    (dict(polarization="hz", boundary="periodic", bloch_phase=0.3), "bloch_phase is not available with polarization"),
    (dict(polarization="hz", boundary="pml", flux_lines=[("row", 20, 1, 30)], flux_omegas=[3e11]),
     "flux_lines is not available with polarization"),
])
def test_run_fdtd_batch_refuses_bad_polarization_on_the_host(monkeypatch, kwargs, match):
    import fdtd2d_amd.batch as batch

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(batch, "BatchEngine", no_engine)
    args = dict(nsteps=5, sources=np.array([[20, 20]] * 2), boundary="pml", pml_cells=8)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        batch.run_fdtd_batch(np.full((2, 40, 40), EPS0), **args)


def test_the_adjoint_helpers_refuse_an_hz_engine(fd):
    from fdtd2d_amd import _abi, adjoint
    eng = types.SimpleNamespace(polarization="hz", dispersive=False, _bloch=None)
    for refuse in (adjoint._refuse_bloch, adjoint._refuse_dispersion, adjoint._refuse_phase,
                   adjoint._refuse_bloch_flux_pole, fd.AdjointSession._check_engine,
                   fd.BlochFluxAdjointSession._check_engine):
        with pytest.raises(fd.Fdtd2dError, match="Hz polarisation") as ei:
            refuse(eng)
        assert ei.value.code == _abi.E_STATE
        refuse(types.SimpleNamespace(polarization="ez", dispersive=False, _bloch=None))


# ---- 1. duality -------------------------------------------------------------------------------------------------------

CASES = {"per23x11": ("periodic", 23, 11, 4), "per29x13pec": ("periodic", 29, 13, 0), "pml23x19": ("pml", 23, 19, 4)}


def _pair(case, dtype, seed=1, B=3, steps=50):
    """An Hz stand-in and the Ez stand-in of the dual problem, from the same random state, both run `steps` steps."""
    boundary, R, C, L = CASES[case]
    rng = np.random.default_rng(seed)
    eps, mu = EPS0 * (1 + 3 * rng.random((B, R, C))), MU0 * (1 + rng.random((B, R, C)))
    hz = (HzPeriodicOracle if boundary == "periodic" else HzPmlOracle)(B, R, C, DT, DX, dtype, boundary)
    ez = (PeriodicOracle if boundary == "periodic" else LossyOracle)(B, R, C, DT, DX, dtype, boundary)
    hz.set_materials(eps, mu)
    ez.set_materials(mu, eps)
    if L:
        c00 = (1 / np.sqrt(eps[:, 0, 0] * mu[:, 0, 0]) * DT) / DX        # symmetric in eps and mu
        hz.set_pml(L=L, courant00=c00)
        ez.set_pml(L=L, courant00=c00)
    f = [rng.standard_normal(s) for s in ((B, R, C), (B, R, C - 1), (B, R - 1, C), (B, R, C))]
    if boundary == "periodic":
        f[3][:, :, -1] = f[3][:, :, 0]
    hz.upload(f[0], f[1], f[2])
    ez.upload(f[0], -f[1], -f[2])
    hz.Ezx[...] = f[3].astype(dtype)
    ez.Ezx[...] = f[3].astype(dtype)
    rects = np.array([[R // 2, 0, 1, 3], [9, C - 3, 2, 2], [12, 3, 1, 1]])
    amps = rng.standard_normal((B, steps))
    for o in (hz, ez):
        o.set_sources(rects).set_dft_window((8, 0, 3, C - 1), 2 * np.pi * FREQS[:2]).set_probes(np.array([[9, 0], [11, 4]]), steps)
    return hz, ez, amps, steps


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_the_pole_free_stand_in_is_the_ez_stand_in_with_exchanged_materials(case, dtype):
    hz, ez, amps, steps = _pair(case, dtype)
    hz.run(steps, amps)
    ez.run(steps, amps)
    (h, ex, ey), (e, hx, hy) = hz.download(), ez.download()
    assert np.any(h) and np.all(np.isfinite(h))
    assert np.array_equal(h, e) and np.array_equal(ex, -hx) and np.array_equal(ey, -hy)
    assert np.array_equal(hz.Ezx, ez.Ezx)
    assert np.array_equal(hz.read_dft_window(), ez.read_dft_window())
    assert np.array_equal(hz.read_probes(), ez.read_probes())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_zero_sigma_zero_strength_and_zero_state_are_the_pole_free_run(case, dtype):
    plain, _, amps, steps = _pair(case, dtype)
    poled, _, _, _ = _pair(case, dtype)
    poled.set_conductivity(0.0).set_dispersion(0.0, [1e11, 0.0, 4e10], [0.0, 3e11, 2e11])
    plain.run(steps, amps)
    poled.run(steps, amps)
    for a, b in zip(plain.download() + (plain.Ezx,), poled.download() + (poled.Ezx,)):
        assert np.array_equal(a, b)
    assert not any(np.any(s) for s in poled.download_dispersion())
    assert np.array_equal(plain.read_dft_window(), poled.read_dft_window())


# ---- 2 and 3. the polariser and the slab -----------------------------------------------------------------------------

def _transmission(cls, wp2_rows_cols, wp2, gamma):
    """sum |F|^2 on row G_MON with the metal over the same without it, at FREQS: member 0 carries the metal."""
    from fdtd2d_amd.api import ricker_amplitude
    o = cls(2, G_R, G_C, DT, DX, np.float64, "periodic")
    o.set_materials(EPS0, MU0).set_pml(L=G_L, courant00=COURANT0)
    w = np.zeros((2, G_R, G_C))
    rows, cols = wp2_rows_cols
    w[0, rows, cols] = wp2
    o.set_dispersion(w, gamma, 0.0)
    o.set_sources(np.tile([G_SRC, 0, 1, G_C - 1], (2, 1))).set_dft_window((G_MON, 0, 1, G_C - 1), 2 * np.pi * FREQS)
    o.run(G_STEPS, np.tile([ricker_amplitude(k * DT, 45e9) for k in range(G_STEPS)], (2, 1)))
    p = (np.abs(o.read_dft_window()) ** 2).sum(axis=(2, 3))
    return p[0] / p[1]


_T = {}


def _T_of(kind, pol):
    if (kind, pol) not in _T:
        cls = HzPeriodicOracle if pol == "hz" else DispersivePeriodicOracle
        if kind == "strips":
            _T[kind, pol] = _transmission(cls, (slice(60, 62), slice(0, 4)), (2e13) ** 2, 1e11)
        else:
            _T[kind, pol] = _transmission(cls, (slice(60, 64), slice(0, G_C)), (6e11) ** 2, 5e10)
    return _T[kind, pol]


def test_a_wire_grid_passes_hz_and_reflects_ez():
    t_hz, t_ez = _T_of("strips", "hz"), _T_of("strips", "ez")
    print("wire grid: T_hz", t_hz, "T_ez", t_ez)
    assert np.all(t_hz > 0.9) and np.all(t_hz < 1.0)
    assert np.all(t_ez < 0.01) and np.all(t_ez > 0)


def test_drude_slab_follows_the_analytic_formula():
    """Margins re-measured with this stand-in: worst |T_hz - analytic| 2.4e-3 against 5e-3, worst |T_hz - T_ez| 1.7e-5
    against 1e-4."""
    w = 2 * np.pi * FREQS
    n = np.sqrt(1 - (6e11) ** 2 / (w ** 2 + 1j * 5e10 * w) + 0j)
    kd = n * w * np.sqrt(EPS0 * MU0) * 4 * DX
    t = 1 / (np.cos(kd) - 0.5j * (n + 1 / n) * np.sin(kd))
    assert np.abs(np.abs(t) ** 2 - SLAB_ANALYTIC).max() < 5e-6          # the issue's figures are this formula's
    t_hz, t_ez = _T_of("slab", "hz"), _T_of("slab", "ez")
    print("slab: analytic", np.abs(t) ** 2, "T_hz", t_hz, "T_ez", t_ez, "errors", np.abs(t_hz - np.abs(t) ** 2).max(),
          np.abs(t_hz - t_ez).max())
    assert np.abs(t_hz - np.abs(t) ** 2).max() <= 0.005
    assert np.abs(t_hz - t_ez).max() <= 1e-4


# ---- 4. the stand-in's surface ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["per23x11", "pml23x19"])
def test_the_allowed_set_is_exact_and_refusals_leave_the_stand_in_as_it_was(case):
    boundary, R, C, L = CASES[case]
    o, _, amps, steps = _pair(case, np.float64)
    g = o.margin()
    assert g == 6
    ok = np.zeros((3, R, C))
    ok[:, g, :] = ok[:, R - 2 - g, :] = 1.0                      # the first and the last row that may conduct
    if boundary == "pml":
        ok[:, :, :g] = ok[:, :, C - 1 - g:] = 0.0
        assert ok[0, g, g] and ok[0, R - 2 - g, C - 2 - g]
    o.set_conductivity(ok).set_dispersion(ok * 1e23, 1e11, [0.0, 1e11, 2e11])
    before = (o.sigma.copy(), o.wp2.copy(), o.gamma.copy(), o.omega0.copy())
    bad = [(R - 1 - g, 8), (g - 1, 8)] + ([(10, C - 1 - g), (10, g - 1)] if boundary == "pml" else [])
    for at in bad:
        for setter in (o.set_conductivity, lambda w: o.set_dispersion(w * 1e23, 1e11, 0.0)):
            w = ok.copy()
            w[(1,) + at] = 1.0
            with pytest.raises(AssertionError, match="non-zero where"):
                setter(w)
    if boundary == "periodic":                                   # the image column is accepted and never read
        w = ok.copy()
        w[:, 10, C - 1] = 1.0
        o.set_conductivity(w).set_conductivity(ok)
    for w in (-ok, ok * np.nan):
        with pytest.raises(AssertionError):
            o.set_conductivity(w)
        with pytest.raises(AssertionError):
            o.set_dispersion(w, 1e11, 0.0)
    hot = ok * 1e23
    hot[2, g, 8] = 4.1 / DT ** 2 * 4
    with pytest.raises(AssertionError, match="member 2: the pole is unstable"):
        o.set_dispersion(hot, 1e11, 0.0)
    for call in (o.hold_dft_window, lambda: o.dft_window_product([1.0, 1.0]),
                 lambda: o.set_conductivity_window((10, 8, 1, 1), np.zeros((3, 1, 1))),
                 lambda: o.set_dispersion_window((10, 8, 1, 1), np.zeros((3, 1, 1)))):
        with pytest.raises(AssertionError, match="Hz polarisation"):
            call()
    for a, b in zip(before, (o.sigma, o.wp2, o.gamma, o.omega0)):
        assert np.array_equal(a, b)


def test_scalars_fill_exactly_the_cells_that_may_conduct():
    for case in CASES:
        o = _pair(case, np.float32)[0]
        o.set_conductivity(2.0).set_dispersion(1e22, 1e11, 0.0)
        assert np.array_equal(o.sigma != 0, np.broadcast_to(o.allowed(), o.sigma.shape))
        assert np.array_equal(o.wp2 != 0, np.broadcast_to(o.allowed(), o.wp2.shape))
        R, C, g = o.rows, o.cols, o.margin()
        assert o.allowed()[g:R - 1 - g].any() and not o.allowed()[:g].any() and not o.allowed()[R - 1 - g:].any()


def test_uploaded_state_round_trips_without_an_image_column():
    o = _pair("per23x11", np.float32)[0]
    rng = np.random.default_rng(5)
    s = [rng.standard_normal((3, 23, 11)) for _ in range(4)]
    o.set_dispersion(1e22, 1e11, 0.0).upload_hz_dispersion(*s)
    for got, sent in zip(o.download_dispersion(), s):
        assert got.dtype == np.float32 and np.array_equal(got, sent.astype(np.float32))
    o.upload_dispersion((None, 2 * s[2]), None)                  # BatchEngine's pairs: Jy alone
    again = o.download_dispersion()
    assert np.array_equal(again[2], (2 * s[2]).astype(np.float32)) and np.array_equal(again[0], s[0].astype(np.float32))
    o.reset()
    assert not any(np.any(a) for a in o.download_dispersion())
