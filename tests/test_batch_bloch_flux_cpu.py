"""CPU-only checks of the flux lines of Bloch batches (fdtd2d_batch_bloch_flux.h, batch.py), on the stand-in of
tests/oracle_batch_bloch_flux.py.

The surface: the three entry points are declared, exported and bound, no header gains a numbered id, the Python surface
has its shape, bad arguments are refused before any device is touched, and without a device nothing falls back.

The stand-in: with phi = 0 and a real source it is the real lines' stand-in bit for bit; lines never change a field or
another monitor; `every`, the step count and reset follow the window's rule.

The physics, on the stand-in: the member of tests/test_batch_flux_cpu.py (periodic vacuum, 120 x 9 cells, dx = 1e-4,
dt = 1.6e-13, a 12-row layer top and bottom, float64, a line source over the period on row 40) with the Bloch phase 0.9
and "ramp" weights, 1600 steps, wavelengths of 20, 16 and 13 cells.  The pulse is narrow-band,
exp(-((k - 456) / 57)^2 / 2) sin(w0 (k - 456) dt) with w0 at a wavelength of 16 cells, not the Ricker wavelet: under a
phase the Ricker pulse excites the grazing cut-off at w = c phi / period (a wavelength of 56 cells), which rings for tens
of thousands of steps, and the record is then truncated whatever the definition of the flux.  The narrow-band pulse has
less than 1e-13 of its spectrum there.  Measured values (printed again by the tests):

    end field                                         4.5e-14                      bound 1e-12
    conservation |P50 - P75| / P50                    2.7e-14, 4.2e-16, 2.8e-14    bound 1e-9 (mis-centring: > 1e-3)
    upstream |P25 / P50 + 1|                          <= 3.3e-5                    bound 1e-3
    translation |P0 - P4| / |P4|, columns 0 and 4     <= 1.5e-16                   bound 1e-9 (unrotated seam: 0.167)
    both column-line P negative (phi = 0.9, w > 0)    holds
    whole-period row line vs 8 x a one-cell line      <= 1.5e-15                   bound 1e-9 relative
    |Im / Re| of sum E conj(H) with the half step     <= 3.2e-5                    bound tan(w dt / 2) / 4
    sigma = 20 S/m on rows 60..65: |P50 - P56| / P50  <= 7.1e-15                   bound 1e-9
    sigma = 20 S/m on rows 60..65: P75 / P56          0.039, 0.030, 0.023          bound 0 < . < 0.1
    flux_orders, orders m != 0 over order 0           <= 6.9e-31                   bound 1e-12
"""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from oracle import fdtd_numpy as onp
from oracle_batch_bloch_flux import BlochDispersiveFluxOracle, BlochFluxOracle
from oracle_batch_flux import FluxPeriodicOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_bloch_flux.h")
NAMES = ["fdtd2d_batch_bloch_flux", "fdtd2d_batch_read_bloch_flux_lines", "fdtd2d_batch_set_bloch_flux_lines"]
EPS0, MU0 = onp.EPS0, onp.MU0
C0 = 1 / np.sqrt(EPS0 * MU0)


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- the surface ----------------------------------------------------------------------------------------------------

def test_bloch_flux_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r'#include\s+"fdtd2d_batch_flux.h"', txt)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_BLOCH_FLUX_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_BLOCH_FLUX_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_BLOCH_FLUX_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "const int *": ctypes.POINTER(ctypes.c_int),
             "double *": ctypes.POINTER(ctypes.c_double), "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_BLOCH_FLUX_SIGNATURES[n][1], n


def test_no_header_gains_a_numbered_id():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.search(r"FDTD2D_BATCH_(INFO|OPT)_\w+", txt) and "enum" not in txt and "#define FDTD2D_BATCH_MAX" not in txt
    info, opt = {}, {}
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "fdtd2d_batch_flux.h":
            other = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            info.update(re.findall(r"FDTD2D_(BATCH_INFO_\w+)\s*(?:=\s*|\s+)(-?\d+)\b", other))
            opt.update(re.findall(r"FDTD2D_(BATCH_OPT_\w+)\s*(?:=\s*|\s+)(-?\d+)\b", other))
    assert sorted(int(v) for v in info.values()) == list(range(21))
    assert sorted(int(v) for v in opt.values()) == [0, 1, 2]
    assert (_abi.BATCH_INFO_FLUX_LINES, _abi.BATCH_INFO_FLUX_LDS, _abi.BATCH_OPT_FLUX_LDS) == (21, 22, 3)
    assert max(getattr(_abi, k) for k in dir(_abi) if k.startswith("BATCH_INFO_")) == 22
    assert max(getattr(_abi, k) for k in dir(_abi) if k.startswith("BATCH_OPT_")) == 3


def test_bloch_flux_python_surface(fd):
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_bloch_flux_lines).parameters) == ["self", "lines", "omegas", "every"]
    assert inspect.signature(E.set_bloch_flux_lines).parameters["every"].default == 1
    assert list(inspect.signature(E.flux_orders).parameters) == ["self", "line"]
    assert inspect.signature(E.flux_orders).parameters["line"].default == 0
    assert list(inspect.signature(E.read_flux_lines).parameters) == ["self", "raw"]
    assert list(inspect.signature(E.flux).parameters) == ["self"]
    assert isinstance(E.flux_lines_in_lds, property)
    p = inspect.signature(fd.run_fdtd_batch).parameters
    for name in ("bloch_flux_lines", "bloch_flux_omegas"):
        assert p[name].default is None and p[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[-4:] == ["bloch_flux_lines", "bloch_flux_omegas", "flux_lines", "flux_omegas"]
    for cls in (BlochFluxOracle, BlochDispersiveFluxOracle):
        for name in ("set_bloch_flux_lines", "read_flux_lines", "flux", "flux_orders"):
            assert callable(getattr(cls, name))


def test_bloch_flux_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ln = np.array([0, 5, 0, 4], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_bloch_flux_lines(None, 1, ln, 1, dp, 1) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_bloch_flux_lines(None, 0, dp, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_bloch_flux(None, dp) == _abi.E_ARG


R0, C0_ = 40, 17
BAD = [
    ([("row", 5 + k, 0, 4) for k in range(5)], [1e11], 1, "1..4 lines"),
    ([("row", 5, 0, 4)], np.linspace(1e11, 2e11, 17), 1, "1..16 frequencies"),
    ([("row", 0, 0, 4)], [1e11], 1, "row 0 outside"),
    ([("row", R0 - 1, 0, 4)], [1e11], 1, f"row {R0 - 1} outside"),
    ([("col", C0_ - 1, 0, 4)], [1e11], 1, "image of column 0"),
    ([("col", -1, 0, 4)], [1e11], 1, "column -1 outside"),
    ([("row", 5, 0, C0_)], [1e11], 1, "run past"),
    ([("col", 5, R0 - 3, 4)], [1e11], 1, "run past"),
    ([("row", 5, 0, 0)], [1e11], 1, "empty"),
    ([("row", 5, 0, 4)], [1e11], 0, "every must be >= 1"),
    ([("row", 5, 0, 4)], [np.inf], 1, "finite"),
    ([("diag", 5, 0, 4)], [1e11], 1, '"row"'),
]


@pytest.mark.parametrize("lines,omegas,every,msg", BAD, ids=[b[3] + str(k) for k, b in enumerate(BAD)])
def test_bad_bloch_flux_arguments_are_refused_before_a_device_is_touched(fd, lines, omegas, every, msg):
    """run_fdtd_batch raises ValueError before it creates an engine, so this passes with and without a device."""
    with pytest.raises(ValueError, match=re.escape(msg)):
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), nsteps=5, sources=np.array([[20, 8]] * 2), boundary="periodic",
                          pml_cells=6, dft_every=every, bloch_phase=0.4, bloch_flux_lines=lines, bloch_flux_omegas=omegas)


def test_bloch_flux_arguments_come_together_with_a_phase_on_periodic_columns(fd):
    kw = dict(nsteps=5, sources=np.array([[20, 8]] * 2), pml_cells=6)
    eps, ln = np.full((2, R0, C0_), EPS0), [("row", 5, 0, 4)]
    with pytest.raises(ValueError, match="together"):
        fd.run_fdtd_batch(eps, bloch_flux_lines=ln, boundary="periodic", bloch_phase=0.3, **kw)
    with pytest.raises(ValueError, match="together"):
        fd.run_fdtd_batch(eps, bloch_flux_omegas=[1e11], boundary="periodic", bloch_phase=0.3, **kw)
    with pytest.raises(ValueError, match="bloch_phase"):
        fd.run_fdtd_batch(eps, bloch_flux_lines=ln, bloch_flux_omegas=[1e11], boundary="periodic", **kw)
    with pytest.raises(ValueError, match='boundary="periodic"'):
        fd.run_fdtd_batch(eps, bloch_flux_lines=ln, bloch_flux_omegas=[1e11], boundary="pml", **kw)
    with pytest.raises(ValueError, match='boundary="periodic"'):
        fd.run_fdtd_batch(np.full((2, 17, 17), EPS0), bloch_flux_lines=ln, bloch_flux_omegas=[1e11], boundary="lattice",
                          bloch_phase=(0.1, 0.2), nsteps=5, sources=np.array([[8, 8]] * 2))
    # the real lines keep refusing a phase
    with pytest.raises(ValueError, match="bloch_phase"):
        fd.run_fdtd_batch(eps, flux_lines=ln, flux_omegas=[1e11], boundary="periodic", bloch_phase=0.3, **kw)


def test_bloch_flux_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 2, R0, C0_, 5e-14, 1e-4, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), nsteps=10, sources=np.array([[20, 8]] * 2), boundary="periodic",
                          pml_cells=6, bloch_phase=0.4, bloch_flux_lines=[("row", 12, 0, C0_ - 1)],
                          bloch_flux_omegas=[2e11])
    assert ei.value.code == _abi.E_NODEVICE


# ---- the stand-in -----------------------------------------------------------------------------------------------------

def _member(cls, dtype=np.float32, R=24, C=13, seed=3, phi=(0.7, -1.9), pole=False):
    rng = np.random.default_rng(seed)
    eng = cls(2, R, C, 5e-14, 1e-4, dtype=dtype, boundary="periodic")
    eng.set_materials(EPS0 * (1 + rng.random((2, R, C))), MU0 * (1 + rng.random((2, R, C))))
    eng.set_pml(4, courant00=(C0 * 5e-14) / 1e-4)
    eng.set_sources(np.array([[9, 3, 2, 2], [10, 4, 1, 3]]))
    if phi is not None:
        eng.set_bloch_phase(np.array(phi)).set_bloch_source("ramp")
    if pole:
        g = eng.margin()
        wp2 = np.zeros((2, R, C))
        wp2[:, g:R - g, :] = 4e22
        eng.set_bloch_dispersion(wp2, np.array([1e11, 0.0]), np.array([0.0, 3e11]))
    eng.set_dft_window((7, 2, 5, 6), 2 * np.pi * np.array([30e9, 55e9]), every=2)
    eng.set_probes(np.array([[8, 0], [11, C - 2], [12, 5]]), 40)
    return eng


LINES = [("row", 9, 0, 12), ("col", 0, 0, 24), ("col", 11, 7, 5), ("row", 2, 3, 4)]


def test_phase_zero_is_the_real_lines_stand_in_bit_for_bit():
    """phi = 0 and a real source: the real part's sums are FluxPeriodicOracle's, the imaginary part's are zero."""
    om = 2 * np.pi * np.array([[30e9, -55e9, 80e9], [20e9, 45e9, -70e9]])
    amps = np.random.default_rng(5).standard_normal((2, 30))
    real = _member(FluxPeriodicOracle, phi=None)
    real.set_flux_lines(LINES, om, every=3)
    real.run(30, amps)
    for cls in (BlochFluxOracle, BlochDispersiveFluxOracle):
        eng = _member(cls, phi=(0.0, 0.0))
        eng.set_bloch_source(None).set_bloch_flux_lines(LINES, om, every=3)
        eng.run(30, amps)
        (er, hr), (ei, hi) = eng.read_bloch_flux_parts()
        E, H = real.read_flux_lines(raw=True)
        assert np.abs(E).max() > 0 and np.abs(H).max() > 0
        assert np.array_equal(er, E) and np.array_equal(hr, H)
        assert not np.any(ei) and not np.any(hi)
        assert np.array_equal(eng.flux(), real.flux())
        for a, b in zip(eng.read_flux_lines(), real.read_flux_lines()):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("pole", [False, True])
def test_lines_never_change_a_field_or_another_monitor(pole):
    amps = np.random.default_rng(5).standard_normal((2, 30)) + 1j * np.random.default_rng(6).standard_normal((2, 30))
    out = []
    for with_lines in (False, True):
        eng = _member(BlochDispersiveFluxOracle, pole=pole)
        if with_lines:
            eng.set_bloch_flux_lines(LINES, 2 * np.pi * np.array([[30e9, -55e9, 80e9], [20e9, 45e9, 70e9]]), every=3)
        eng.run(30, amps)
        out.append(eng.download() + (eng.download_ezx(), eng.read_dft_window(), eng.read_probes()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    E, H = eng.read_flux_lines(raw=True)
    assert E.shape == H.shape == (2, 3, 45) and np.all(np.abs(E).max(axis=(1, 2)) > 0) and np.abs(H).max() > 0
    (er, hr), (ei, hi) = eng.read_bloch_flux_parts()
    assert np.abs(ei).max() > 0 and np.abs(hi).max() > 0 and np.array_equal(E, er + 1j * ei)
    # the cell (9, 0) lies on the row line (its cell 0) and on the column line (its cell 9): one Ez, two H
    assert np.array_equal(E[:, :, 0], E[:, :, 12 + 9])
    assert not np.array_equal(H[:, :, 0], H[:, :, 12 + 9])
    # rows 0 and R-1 of the column line at column 0 are PEC: Ez is zero there
    assert not np.any(E[:, :, 12]) and not np.any(E[:, :, 12 + 23])


def test_the_seam_neighbour_is_rotated_back_in_the_batch_dtype():
    """Column 0's left neighbour is unrotate(c, s, Hy[:, C-2]) in float32, not the stored value and not a float64 one."""
    from oracle_batch_bloch import unrotate
    eng = _member(BlochFluxOracle)
    eng.set_bloch_flux_lines([("col", 0, 0, 24)], [2 * np.pi * 40e9])
    amps = np.random.default_rng(7).standard_normal((2, 12)) + 0j
    eng.run(12, amps)
    for b in range(2):
        hr, hi = eng._tangential_h(b)
        c, s = eng.rho[0][b], eng.rho[1][b]
        lr, li = unrotate(c, s, eng.Hy[b][:, -2], eng.Hy_i[b][:, -2])
        assert lr.dtype == np.float32
        want_r = 0.5 * (lr.astype(np.float64) + eng.Hy[b][:, 0].astype(np.float64))
        want_i = 0.5 * (li.astype(np.float64) + eng.Hy_i[b][:, 0].astype(np.float64))
        assert np.array_equal(hr[:23], want_r) and np.array_equal(hi[:23], want_i)
        assert hr[23] == 0 and hi[23] == 0                       # row R-1: both slots read as zero
        raw = 0.5 * (eng.Hy[b][:, -2].astype(np.float64) + eng.Hy[b][:, 0].astype(np.float64))
        assert not np.array_equal(hr[:23], raw)


def test_sampling_follows_the_window_rule_and_reset_zeroes():
    om = 2 * np.pi * np.array([40e9, -70e9])
    amps = np.random.default_rng(6).standard_normal((2, 40)) * (1 + 0.5j)
    eng = _member(BlochFluxOracle)
    eng.run(7, amps[:, :7])
    eng.set_dft_window((9, 0, 1, 12), om, every=3)       # the same cells, frequencies and rule as the line's Ez
    eng.set_bloch_flux_lines([("row", 9, 0, 12)], om, every=3)
    eng.run(33, amps[:, 7:])
    E, _ = eng.read_flux_lines(raw=True)
    assert np.array_equal(E, eng.read_dft_window()[:, :, 0, :])
    # one run or two, the same sums
    one = _member(BlochFluxOracle)
    one.run(7, amps[:, :7])
    one.set_bloch_flux_lines([("row", 9, 0, 12)], om, every=3)
    one.run(20, amps[:, 7:27])
    one.set_bloch_phase(np.array([0.7, -1.9]))            # the same phase again: the lines and their sums stay
    one.run(13, amps[:, 27:])
    for a, b in zip(one.read_flux_lines(), eng.read_flux_lines()):
        assert np.array_equal(a, b)
    assert np.array_equal(one.flux(), eng.flux())
    with pytest.raises(AssertionError):
        one.set_bloch_phase(None)
    eng.reset()
    assert not np.any(eng.read_flux_lines()[0]) and not np.any(eng.read_flux_lines()[1]) and not np.any(eng.flux())
    eng.run(3, amps[:, :3])                              # the count restarts: step 3 is sampled
    assert np.any(eng.read_flux_lines()[0])


# ---- the physics -----------------------------------------------------------------------------------------------------

PR, PC, PDX, PDT, PSTEPS, PL, PSRC, PHI = 120, 9, 1e-4, 1.6e-13, 1600, 12, 40, 0.9
PLINES = (25, 50, 56, 75)
POMEGA = 2 * np.pi * C0 / (np.array([20.0, 16.0, 13.0]) * PDX)
PW0 = 2 * np.pi * C0 / (16.0 * PDX)
ROWS = [("row", r, 0, PC - 1) for r in PLINES]
COLS = [("col", 0, 45, 30), ("col", 4, 45, 30), ("row", 50, 0, PC - 1), ("row", 50, 3, 1)]


def _physics(lines, sigma=None):
    k = np.arange(PSTEPS) - 456
    amps = np.exp(-0.5 * (k / 57.0) ** 2) * np.sin(PW0 * k * PDT)
    eng = BlochFluxOracle(1, PR, PC, PDT, PDX, dtype=np.float64, boundary="periodic")
    eng.set_materials(np.full((1, PR, PC), EPS0), np.full((1, PR, PC), MU0))
    eng.set_pml(PL, courant00=(C0 * PDT) / PDX)
    if sigma is not None:
        s = np.zeros((1, PR, PC))
        s[:, 60:66, :] = sigma
        eng.set_conductivity(s)
    eng.set_sources(np.array([[PSRC, 0, 1, PC - 1]]))
    eng.set_bloch_phase(PHI).set_bloch_source("ramp")
    eng.set_bloch_flux_lines(lines, POMEGA)
    eng.run(PSTEPS, amps[None] + 0j)
    end = max(np.abs(eng.Ez).max(), np.abs(eng.Ez_i).max())
    print("end field:", end)                              # measured 4.5e-14
    assert end < 1e-12                                    # the record is complete
    return eng


@pytest.fixture(scope="module")
def lossless():
    return _physics(ROWS)


@pytest.fixture(scope="module")
def columns():
    return _physics(COLS)


def test_flux_is_conserved_between_lines_and_reverses_behind_the_source(lossless):
    P = lossless.flux()[0]                               # (line, frequency)
    assert np.all(P[1] > 0)
    cons = np.abs(P[1] - P[3]) / P[1]
    print("conservation |P50 - P75| / P50:", cons)       # measured 2.7e-14, 4.2e-16, 2.8e-14
    assert np.all(cons <= 1e-9)
    up = np.abs(P[0] / P[1] + 1)
    print("upstream |P25 / P50 + 1|:", up)                # measured <= 3.3e-5
    assert np.all(up <= 1e-3)


def test_column_lines_are_translation_invariant_across_the_seam(columns):
    """The wave exp(i (k x + w t)) has the same power through every column; column 0 reads across the seam."""
    P = columns.flux()[0]
    diff = np.abs(P[0] - P[1]) / np.abs(P[1])
    print("translation |P0 - P4| / |P4|:", diff)          # measured <= 1.5e-16; an unrotated neighbour gives 0.167
    assert np.all(diff <= 1e-9)
    assert np.all(P[0] < 0) and np.all(P[1] < 0)          # it travels towards decreasing column


def test_a_whole_period_line_is_its_cells_together(columns):
    P = columns.flux()[0]
    rel = np.abs(P[2] - (PC - 1) * P[3]) / np.abs(P[2])
    print("whole-period row line against 8 x one cell:", rel)
    assert np.all(P[2] > 0) and np.all(rel <= 1e-9)       # E H without the conjugate fails this


def test_half_step_factor_makes_the_flux_real(lossless):
    tan = np.tan(POMEGA * PDT / 2)
    n = PC - 1
    E, H = lossless.read_flux_lines()
    z = (E[0] * np.conj(H[0])).reshape(3, len(PLINES), n).sum(axis=2)     # (frequency, line)
    ratio = np.abs(z.imag / z.real)
    print("with the factor |Im / Re|:", ratio.max(axis=1))                # measured <= 3.2e-5
    assert np.all(ratio <= 0.25 * tan[:, None])
    E, H = lossless.read_flux_lines(raw=True)
    z = (E[0] * np.conj(H[0])).reshape(3, len(PLINES), n).sum(axis=2)
    raw = np.abs(z.imag / z.real)
    print("raw |Im / Re| over tan(w dt / 2):", (raw / tan[:, None]).min(), (raw / tan[:, None]).max())
    assert np.all(np.abs(raw / tan[:, None] - 1) <= 0.01)


def test_a_conducting_slab_absorbs_what_the_lines_miss(lossless):
    P = _physics(ROWS, sigma=20.0).flux()[0]
    same = np.abs(P[1] - P[2]) / P[1]
    print("|P50 - P56| / P50:", same, " P75 / P56:", P[3] / P[2])    # measured <= 7.1e-15; 0.039, 0.030, 0.023
    assert np.all(same <= 1e-9)
    assert np.all(P[3] > 0) and np.all(P[3] < 0.1 * P[2])


# ---- the orders -------------------------------------------------------------------------------------------------------

def test_flux_orders_of_the_ramp_driven_vacuum_member_are_order_zero_alone(lossless):
    Pm = lossless.flux_orders(1)                          # (1, F, Q) in fftfreq order: index 0 is m = 0
    assert Pm.shape == (1, 3, PC - 1)
    rest = np.abs(Pm[0, :, 1:]).max(axis=1) / np.abs(Pm[0, :, 0])
    print("orders m != 0 over order 0:", rest)
    assert np.all(rest < 1e-12)
    for line in range(4):
        tot = lossless.flux_orders(line).sum(axis=2)
        assert np.all(np.abs(tot - lossless.flux()[:, line, :]) <= 1e-12 * lossless.flux_scale()[:, line, :])


def test_engine_flux_orders_is_the_stand_ins_sum(fd):
    """BatchEngine.flux_orders is host NumPy over read_flux_lines(): run it on the stand-in's spectra."""
    rng = np.random.default_rng(9)
    eng = _member(BlochFluxOracle, dtype=np.float64)
    eng.set_bloch_flux_lines([("row", 3, 2, 5), ("row", 9, 0, 12), ("col", 0, 0, 24)],
                             2 * np.pi * np.array([[30e9, -55e9], [20e9, 45e9]]))
    eng.run(40, rng.standard_normal((2, 40)) + 1j * rng.standard_normal((2, 40)))
    f = eng.bfluxmon
    ln = np.array([[k == "col", at, first, n] for k, at, first, n in f["lines"]], np.int32)
    fake = types.SimpleNamespace(_bflux=True, _flux=(ln, f["omega"]), cols=eng.cols, dx=eng.dx, _phi=eng.phi,
                                 _bloch=(np.cos(eng.phi), np.sin(eng.phi)), read_flux_lines=eng.read_flux_lines)
    got, want = fd.BatchEngine.flux_orders(fake, 1), eng.flux_orders(1)
    assert got.shape == want.shape == (2, 2, 12) and np.abs(want).max() > 0
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want).max())
    scale = eng.flux_scale()[:, 1, :]
    assert np.all(np.abs(got.sum(axis=2) - eng.flux()[:, 1, :]) <= 1e-12 * scale)
    assert np.abs(got[:, :, 1:]).max() > 1e-3 * np.abs(got).max()        # a structured member: more than one order
    # without the phases as given, the rotation's angle serves
    fake._phi = None
    assert np.all(np.abs(fd.BatchEngine.flux_orders(fake, 1) - want) <= 1e-12 * np.abs(want).max())
    for line in (0, 2):
        with pytest.raises(ValueError, match="whole period"):
            fd.BatchEngine.flux_orders(fake, line)
        with pytest.raises(ValueError):
            eng.flux_orders(line)
    with pytest.raises(ValueError, match="outside"):
        fd.BatchEngine.flux_orders(fake, 3)
