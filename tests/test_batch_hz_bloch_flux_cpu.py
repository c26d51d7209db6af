"""CPU-only checks of the flux lines of Hz Bloch batches (fdtd2d_batch_hz_bloch_flux.h, batch.py), on the stand-in of
tests/oracle_batch_hz_bloch_flux.py.  Measured values (float64 NumPy; the tests print them again):

1. The surface: the three entry points are declared, exported and bound, no numbered id is added, BatchEngine and the
   stand-in have the new methods, run_fdtd_batch has the two keyword-only parameters in front of the last four.

2. Identities on the stand-ins.  (b) Lossless members at the phases 0.4, 1.3 and -2.2, both dtypes: against
   BlochFluxOracle with eps and mu exchanged the Hz sums equal its Ez sums, the Et sums minus its Ht sums and P its P, bit
   for bit.  (a) At phi = 0 with real amplitudes the real part's sums are HzFluxPeriodicOracle's value for value and the
   imaginary part's are zero, with a conductivity and a pole.

3. The seam, by physics.  Periodic vacuum, 120 x 9, dx = 1e-4, dt = 1.6e-13, a 12-row layer, float64, a ramp-weighted
   line source over the period on row 40, phi = 2.4 across the 8-cell period, a narrow-band pulse at a wavelength of 10
   cells (the grazing cut-off of this phase lies at 20.9 cells, nine of the pulse's spectral widths away), 1600 steps,
   wavelengths of 12, 10 and 9 cells.  S_x of a Bloch wave in a uniform period does not depend on x:
       |P(column 0) - P(column 1)| / |P(column 1)|      <= 2.5e-15      bound 2.5e-14
       the same with the neighbour rotated by rho, not conj(rho)      0.53      (2e13 times the bound)

4. Energy and Brewster's angle by flux.  The member of tests/test_batch_hz_bloch_cpu.py (160 x 13, a 20-cell layer, a
   4-cell eps_r = 4 slab on rows 70..73, k_x = 2.2495 / (12 dx), Brewster incidence at 100 GHz) and a vacuum copy, driven
   by exp(-((n - 5200) / 1300)^2 / 2) exp(i w (n - 5200) dt) at 100 GHz for 14000 steps (the cut-off of this phase lies at
   89.5 GHz, 4.3 spectral widths below), row lines on rows 50 (between source and slab), 100 and 120:
       |P50 - P100| / P100 on the slab member          4.7e-6      bound 4.7e-5      (end field 9.7e-4 of the peak 1)
       T_Hz = P100(slab) / P100(vacuum)                0.98043     asserted > 0.95   (window DFT: 0.978)
       R_Hz = 1 - P50(slab) / P50(vacuum)              0.01958     T + R = 1.0000023
       T_Ez (BlochFluxOracle, the same member)         0.21761     asserted < 0.25   (window DFT: 0.217), R 0.78239

5. The orders: flux_orders(k).sum(axis=2) = flux()[:, k, :] to rtol 1e-10 (measured 1.2e-16 of the scale); on the
   ramp-driven vacuum member of 3. the orders m != 0 over order 0 are <= 7.4e-30 (bound 1e-12); BatchEngine.flux_orders
   run on a fake object carrying the stand-in's spectra equals the stand-in's.

6. The Drude strips under the phase: the polariser of tests/test_batch_hz_cpu.py (121 x 9, a 12-cell layer, strips with
   wp = 2e13 rad/s, gamma = 1e11 on rows 60..61 of columns 0..3, source row 20, dt = 5e-14), phi = 0, 0.1, 0.2, 0.3 across
   the 8-cell period, a vacuum copy per phase, row lines on rows 40, 50, 75, 95.  The drive is the sum of three tones at
   30, 45 and 60 GHz under exp(-((n - 4950) / 1100)^2 / 2), 11000 steps: the README's Ricker pulse excites the grazing
   cut-off of the phase (17.9 GHz at phi = 0.3), which rings for tens of thousands of steps; with it the vacuum copy's
   P40 / P95 is off by up to 5e-2 after 6000 steps and A = 1 - T - R comes out at -1.3e-3 (phi = 0.3, 45 GHz).  With the
   tones the vacuum copy's |P40 / P95 - 1| is <= 2e-5 and A agrees with (P50 - P75) / P95(vacuum) to 1e-5:
       phi    T (30, 45, 60 GHz)              R                              A = 1 - T - R
       0      0.97981  0.95641  0.92541      0.01947  0.04280  0.07371      7.2e-4  7.9e-4  8.8e-4
       0.1    0.98094  0.95748  0.92640      0.01833  0.04172  0.07271      7.3e-4  7.9e-4  8.8e-4
       0.2    0.98429  0.96070  0.92940      0.01493  0.03849  0.06971      7.8e-4  8.1e-4  8.9e-4
       0.3    0.98978  0.96608  0.93441      0.00935  0.03309  0.06469      8.7e-4  8.4e-4  9.0e-4
   Asserted: A > 0 everywhere, and at phi = 0 T agrees with the README's 0.97981, 0.95641, 0.92541 to 1e-4.

7. The capacity rule, restated from the header: which of the cases of tests/test_gpu_batch_hz_bloch_flux.py keep their
   sums in LDS and which cannot."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from oracle import fdtd_numpy as onp
from oracle_batch_bloch import rotate
from oracle_batch_bloch_flux import BlochFluxOracle
from oracle_batch_hz_bloch_flux import HzBlochFluxOracle
from oracle_batch_hz_flux import HzFluxPeriodicOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_hz_bloch_flux.h")
NAMES = ["fdtd2d_batch_hz_bloch_flux", "fdtd2d_batch_read_hz_bloch_flux_lines", "fdtd2d_batch_set_hz_bloch_flux_lines"]
EPS0, MU0 = onp.EPS0, onp.MU0
C0 = 1 / np.sqrt(EPS0 * MU0)
DT, DX = 5e-14, 1e-4
COURANT0 = (C0 * DT) / DX


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- 1. the surface ---------------------------------------------------------------------------------------------------

def test_hz_bloch_flux_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r'#include\s+"fdtd2d_batch_flux.h"', txt) and re.search(r'#include\s+"fdtd2d_batch_hz_bloch.h"', txt)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_HZ_BLOCH_FLUX_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_HZ_BLOCH_FLUX_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_HZ_BLOCH_FLUX_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "const int *": ctypes.POINTER(ctypes.c_int),
             "double *": ctypes.POINTER(ctypes.c_double), "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_HZ_BLOCH_FLUX_SIGNATURES[n][1], n
    # the prototypes are those of the Ez Bloch lines
    for n in names:
        assert _abi.BATCH_HZ_BLOCH_FLUX_SIGNATURES[n] == _abi.BATCH_BLOCH_FLUX_SIGNATURES[n.replace("hz_bloch", "bloch")]


def test_hz_bloch_flux_adds_no_numbered_id():
    from fdtd2d_amd import _abi
    txt = open(HEADER).read()
    assert not re.findall(r"#define\s+FDTD2D_BATCH_(?:INFO|OPT)_\w+", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert not re.findall(r"FDTD2D_BATCH_(?:INFO|OPT)_\w+\s*=", code) and "enum" not in code
    assert max(v for k, v in vars(_abi).items() if k.startswith("BATCH_INFO_") and isinstance(v, int)) == 22


def test_hz_bloch_flux_python_surface(fd):
    """Fails on the commit before the lines: neither the methods nor the parameters exist there."""
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_hz_bloch_flux_lines).parameters) == ["self", "lines", "omegas", "every"]
    assert inspect.signature(E.set_hz_bloch_flux_lines).parameters["every"].default == 1
    assert list(inspect.signature(E.read_hz_bloch_flux_parts).parameters) == ["self"]
    assert list(inspect.signature(E.read_flux_lines).parameters) == ["self", "raw"]
    assert list(inspect.signature(E.flux_orders).parameters) == ["self", "line"]
    assert list(inspect.signature(E.flux).parameters) == ["self"]
    assert isinstance(E.flux_lines_in_lds, property) and callable(E.set_flux_lds)
    p = inspect.signature(fd.run_fdtd_batch).parameters
    for name in ("hz_bloch_flux_lines", "hz_bloch_flux_omegas"):
        assert p[name].default is None and p[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[-6:] == ["hz_bloch_flux_lines", "hz_bloch_flux_omegas", "bloch_flux_lines", "bloch_flux_omegas",
                            "flux_lines", "flux_omegas"]
    assert list(p)[-4:] == ["bloch_flux_lines", "bloch_flux_omegas", "flux_lines", "flux_omegas"]
    O = HzBlochFluxOracle
    assert list(inspect.signature(O.set_hz_bloch_flux_lines).parameters) == ["self", "lines", "omegas", "every"]
    assert list(inspect.signature(O.read_flux_lines).parameters) == ["self", "raw"]
    assert list(inspect.signature(O.flux_orders).parameters) == ["self", "line"]
    for name in ("read_hz_bloch_flux_parts", "flux", "flux_scale"):
        assert list(inspect.signature(getattr(O, name)).parameters) == ["self"]


def test_hz_bloch_flux_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ln = np.array([0, 5, 0, 4], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_hz_bloch_flux_lines(None, 1, ln, 1, dp, 1) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_hz_bloch_flux_lines(None, 0, dp, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_hz_bloch_flux(None, dp) == _abi.E_ARG


R0, C0_ = 40, 17
LN = [("row", 5, 0, 4)]
BAD = [
    (dict(hz_bloch_flux_lines=LN), "together"),
    (dict(hz_bloch_flux_omegas=[1e11]), "together"),
    (dict(hz_bloch_phase=None, hz_bloch_flux_lines=LN, hz_bloch_flux_omegas=[1e11]), "hz_bloch_flux_lines needs hz_bloch_phase"),
    (dict(hz_flux_lines=LN, hz_flux_omegas=[1e11]), "hz_flux_lines is not available with hz_bloch_phase"),
    (dict(hz_bloch_flux_lines=[("row", 5 + k, 0, 4) for k in range(5)], hz_bloch_flux_omegas=[1e11]), "1..4 lines"),
    (dict(hz_bloch_flux_lines=LN, hz_bloch_flux_omegas=np.linspace(1e11, 2e11, 17)), "1..16 frequencies"),
    (dict(hz_bloch_flux_lines=[("row", 0, 0, 4)], hz_bloch_flux_omegas=[1e11]), "row 0 outside"),
    (dict(hz_bloch_flux_lines=[("col", C0_ - 1, 0, 4)], hz_bloch_flux_omegas=[1e11]), "image of column 0"),
    (dict(hz_bloch_flux_lines=[("row", 5, 0, C0_)], hz_bloch_flux_omegas=[1e11]), "run past"),
    (dict(hz_bloch_flux_lines=LN, hz_bloch_flux_omegas=[1e11], dft_every=0), "every must be >= 1"),
]


@pytest.mark.parametrize("kwargs,match", BAD, ids=[f"{k}-{b[1]}" for k, b in enumerate(BAD)])
def test_run_fdtd_batch_refuses_bad_hz_bloch_flux_arguments_before_an_engine_exists(monkeypatch, kwargs, match):
    import fdtd2d_amd.batch as batch

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(batch, "BatchEngine", no_engine)
    args = dict(nsteps=5, sources=np.array([[20, 8]] * 2), boundary="periodic", pml_cells=6, polarization="hz",
                hz_bloch_phase=0.4)
    args.update(kwargs)
    with pytest.raises(ValueError, match=re.escape(match)):
        batch.run_fdtd_batch(np.full((2, R0, C0_), EPS0), **args)


def test_the_host_refuses_the_lines_without_the_phase_and_the_phase_off_beside_them(fd):
    from fdtd2d_amd import _abi

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")
    eng = object.__new__(fd.BatchEngine)
    eng._lib, eng._h = NoLibrary(), ctypes.c_void_p()
    eng.count, eng.rows, eng.cols, eng.dt, eng.dx, eng.boundary = 3, 30, 13, DT, DX, "periodic"
    eng._flux, eng._bflux, eng._hzflux, eng._hz, eng._hzb = None, False, False, True, False
    with pytest.raises(fd.Fdtd2dError, match="needs the phase of the Hz polarisation") as ei:
        eng.set_hz_bloch_flux_lines(LN, [1e11])
    assert ei.value.code == _abi.E_STATE
    eng._hzb, eng._hzbflux = True, True
    with pytest.raises(fd.Fdtd2dError, match="turning the Bloch phase off") as ei:
        eng.set_hz_bloch_phase(None)
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(AssertionError, match="the library was called"):      # the arguments are good: the call goes through
        eng.set_hz_bloch_flux_lines(LN, [1e11])


def test_hz_bloch_flux_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 2, R0, C0_, DT, DX, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), nsteps=10, sources=np.array([[20, 8]] * 2), boundary="periodic",
                          pml_cells=6, polarization="hz", hz_bloch_phase=0.4,
                          hz_bloch_flux_lines=[("row", 12, 0, C0_ - 1)], hz_bloch_flux_omegas=[2e11])
    assert ei.value.code == _abi.E_NODEVICE


# ---- 2. the identities, bit for bit -----------------------------------------------------------------------------------

LINES = [("row", 20, 0, 16), ("row", 3, 2, 5), ("col", 0, 0, 40), ("col", 15, 14, 12)]
FREQS = np.array([30e9, 45e9, 60e9])


def _members(cls, dtype, hz, B=3, R=40, C=17, L=6, seed=11):
    rng = np.random.default_rng(seed)
    eps, mu = EPS0 * (1 + 3 * rng.random((B, R, C))), MU0 * (1 + rng.random((B, R, C)))
    o = cls(B, R, C, DT, DX, dtype, "periodic")
    o.set_materials(*((eps, mu) if hz else (mu, eps)))
    o.set_pml(L, courant00=(1 / np.sqrt(eps[:, 0, 0] * mu[:, 0, 0]) * DT) / DX)        # symmetric in eps and mu
    o.set_sources(np.array([[18, 3, 2, 3], [22, C - 4, 1, 2], [15, 0, 1, C - 1]]))
    return o, rng


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_lossless_lines_are_the_ez_bloch_lines_of_the_dual_problem_bit_for_bit(dtype):
    """Identity (b)."""
    phi, steps = np.array([0.4, 1.3, -2.2]), 200
    om = 2 * np.pi * np.array([FREQS, -FREQS * 1.3, FREQS * 0.8])
    hz, rng = _members(HzBlochFluxOracle, dtype, True)
    ez, _ = _members(BlochFluxOracle, dtype, False)
    amps = rng.standard_normal((3, steps)) + 1j * rng.standard_normal((3, steps))
    hz.set_hz_bloch_phase(phi).set_hz_bloch_source("ramp").set_hz_bloch_flux_lines(LINES, om, every=3)
    ez.set_bloch_phase(phi).set_bloch_source("ramp").set_bloch_flux_lines(LINES, om, every=3)
    hz.run(steps, amps)
    ez.run(steps, amps)
    (h, ex, ey), (e, hx, hy) = hz.download(), ez.download()
    assert np.any(h.imag) and np.array_equal(h, e) and np.array_equal(ex, -hx) and np.array_equal(ey, -hy)
    for (hk, ek), (zk, tk) in zip(hz.read_hz_bloch_flux_parts(), ez.read_bloch_flux_parts()):
        assert np.all(np.abs(hk).max(axis=(1, 2)) > 0) and np.all(np.abs(ek).max(axis=(1, 2)) > 0)
        assert np.array_equal(hk, zk) and np.array_equal(ek, -tk)
    for raw in (True, False):
        (et_hat, hz_hat), (ez_hat, ht_hat) = hz.read_flux_lines(raw), ez.read_flux_lines(raw)
        assert np.array_equal(hz_hat, ez_hat) and np.array_equal(et_hat, -ht_hat)
    assert np.all(hz.flux() != 0) and np.array_equal(hz.flux(), ez.flux())
    assert np.array_equal(hz.flux_scale(), ez.flux_scale())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_phase_zero_is_the_real_hz_lines_stand_in_value_for_value(dtype):
    """Identity (a), with a conductivity and a pole on a strip that touches the seam."""
    steps, om = 150, 2 * np.pi * np.array([FREQS, -FREQS * 1.3, FREQS * 0.8])
    out = []
    for cls in (HzFluxPeriodicOracle, HzBlochFluxOracle):
        o, rng = _members(cls, dtype, True)
        w, s = np.zeros((3, 40, 17)), np.zeros((3, 40, 17))
        w[:, 25:30, :], s[:, 25:30, :] = (2 * np.pi * 70e9) ** 2, 3.0
        o.set_conductivity(s)
        o.set_dispersion(w, np.array([1e11, 0.0, 5e10]), 2 * np.pi * np.array([0.0, 50e9, 60e9]))
        amps = rng.standard_normal((3, steps))
        if cls is HzBlochFluxOracle:
            o.set_hz_bloch_phase(0.0).set_hz_bloch_flux_lines(LINES, om, every=3)
        else:
            o.set_hz_flux_lines(LINES, om, every=3)
        o.run(steps, amps)
        out.append(o)
    real, bloch = out
    et, hz = real.read_flux_lines(raw=True)
    (hr, er), (hi, ei) = bloch.read_hz_bloch_flux_parts()
    assert np.abs(hz).max() > 0 and np.abs(et).max() > 0
    assert np.array_equal(hr, hz) and np.array_equal(er, et)
    assert not np.any(hi) and not np.any(ei)
    assert np.array_equal(bloch.flux(), real.flux())
    for a, b in zip(bloch.read_flux_lines(), real.read_flux_lines()):
        assert np.array_equal(a, b)


def test_lines_never_change_a_field_and_follow_the_sampling_rule():
    om = 2 * np.pi * np.array([40e9, -70e9])
    out = []
    for with_lines in (False, True):
        o, rng = _members(HzBlochFluxOracle, np.float32, True)
        amps = rng.standard_normal((3, 40)) * (1 + 0.5j)
        o.set_hz_bloch_phase(np.array([0.4, 1.3, -2.2])).set_hz_bloch_source("ramp")
        o.run(7, amps[:, :7])
        o.set_dft_window((20, 0, 1, 16), om, every=3)            # the same cells, frequencies and rule as the line's Hz
        if with_lines:
            o.set_hz_bloch_flux_lines([("row", 20, 0, 16)], om, every=3)
        o.run(33, amps[:, 7:])
        out.append(o.download() + (o.download_ezx(), o.read_dft_window()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    _, H = o.read_flux_lines(raw=True)
    assert np.abs(H).max() > 0 and np.array_equal(H, o.read_dft_window()[:, :, 0, :])
    with pytest.raises(AssertionError):
        o.set_hz_bloch_phase(None)
    o.set_hz_bloch_phase(np.array([0.4, 1.3, -2.2]))              # a new phase keeps the lines and their sums
    assert np.array_equal(o.read_flux_lines(raw=True)[1], H)
    o.reset()
    assert not np.any(o.read_flux_lines()[0]) and not np.any(o.read_flux_lines()[1]) and not np.any(o.flux())
    o.run(3, amps[:, :3])                                        # the count restarts: step 3 is sampled
    assert np.any(o.read_flux_lines()[1])


# ---- 3. the seam, by physics --------------------------------------------------------------------------------------------

PR, PC, PDX, PDT, PSTEPS, PL, PSRC, PHI = 120, 9, 1e-4, 1.6e-13, 1600, 12, 40, 2.4
POMEGA = 2 * np.pi * C0 / (np.array([12.0, 10.0, 9.0]) * PDX)
PW0 = 2 * np.pi * C0 / (10.0 * PDX)
SEAM_MEASURED = 2.5e-15
SEAM_BOUND = 10 * SEAM_MEASURED


class WrongSeam(HzBlochFluxOracle):
    """The stand-in with column 0's neighbour rotated by rho instead of conj(rho)."""

    def _seam(self, c, s, re, im):
        return rotate(c, s, re, im)


def _vacuum(cls):
    k = np.arange(PSTEPS) - 456
    amps = np.exp(-0.5 * (k / 57.0) ** 2) * np.sin(PW0 * k * PDT)
    eng = cls(1, PR, PC, PDT, PDX, dtype=np.float64, boundary="periodic")
    eng.set_materials(np.full((1, PR, PC), EPS0), np.full((1, PR, PC), MU0))
    eng.set_pml(PL, courant00=(C0 * PDT) / PDX)
    eng.set_sources(np.array([[PSRC, 0, 1, PC - 1]]))
    eng.set_hz_bloch_phase(PHI).set_hz_bloch_source("ramp")
    eng.set_hz_bloch_flux_lines([("col", 0, 45, 30), ("col", 1, 45, 30), ("row", 50, 0, PC - 1), ("row", 75, 0, PC - 1)],
                                POMEGA)
    eng.run(PSTEPS, amps[None] + 0j)
    end = max(np.abs(eng.Ez).max(), np.abs(eng.Ez_i).max())
    print("end field:", end)                              # measured 5.8e-16
    assert end < 1e-12                                    # the record is complete
    return eng


@pytest.fixture(scope="module")
def vacuum():
    return _vacuum(HzBlochFluxOracle)


def test_the_power_through_column_0_is_the_power_through_column_1(vacuum):
    """S_x of a Bloch wave in a uniform period does not depend on x; column 0 reads Ey across the seam.  Measured
    2.5e-15 (bound 2.5e-14); with the neighbour rotated by rho instead of conj(rho) 0.53."""
    P = vacuum.flux()[0]
    diff = np.abs(P[0] - P[1]) / np.abs(P[1])
    print("|P(col 0) - P(col 1)| / |P(col 1)|:", diff)
    assert np.all(P[1] != 0) and np.all(diff <= SEAM_BOUND)
    Pw = _vacuum(WrongSeam).flux()[0]
    wrong = np.abs(Pw[0] - Pw[1]) / np.abs(Pw[1])
    print("the same with rho for conj(rho):", wrong)
    assert np.array_equal(Pw[1:], P[1:]) and np.all(wrong >= 100 * SEAM_BOUND)
    # the rows: what crosses row 50 crosses row 75
    assert np.all(P[2] > 0) and np.all(np.abs(P[2] - P[3]) <= 1e-9 * P[2])       # measured 2.5e-14


# ---- 4. energy and Brewster's angle by flux ----------------------------------------------------------------------------

B_ROWS, B_Q, B_L, B_PHI, B_SRC_ROW, B_F, B_SIG, B_STEPS = 160, 12, 20, 2.2495, 30, 100e9, 1300, 14000
B_LINES = (50, 100, 120)
ENERGY_MEASURED = 4.7e-6
ENERGY_BOUND = 10 * ENERGY_MEASURED


def _brewster(pol):
    """P (member, line) at 100 GHz: member 0 the slab, member 1 vacuum."""
    cls = HzBlochFluxOracle if pol == "hz" else BlochFluxOracle
    n = np.arange(B_STEPS) - 4 * B_SIG
    amps = np.exp(-0.5 * (n / B_SIG) ** 2) * np.exp(1j * 2 * np.pi * B_F * n * DT)
    eps = np.full((2, B_ROWS, B_Q + 1), EPS0)
    eps[0, 70:74, :] = 4 * EPS0
    eng = cls(2, B_ROWS, B_Q + 1, DT, DX, dtype=np.float64, boundary="periodic")
    eng.set_materials(eps, np.full(eps.shape, MU0))
    eng.set_pml(B_L, courant00=COURANT0)
    eng.set_sources(np.array([(B_SRC_ROW, 0, 1, B_Q)] * 2))
    lines = [("row", r, 0, B_Q) for r in B_LINES]
    if pol == "hz":
        eng.set_hz_bloch_phase(B_PHI).set_hz_bloch_source("ramp").set_hz_bloch_flux_lines(lines, [2 * np.pi * B_F])
    else:
        eng.set_bloch_phase(B_PHI).set_bloch_source("ramp").set_bloch_flux_lines(lines, [2 * np.pi * B_F])
    eng.run(B_STEPS, np.tile(amps, (2, 1)))
    print(pol, "end field:", max(np.abs(eng.Ez).max(), np.abs(eng.Ez_i).max()))
    return eng.flux()[:, :, 0]


@pytest.fixture(scope="module")
def brewster():
    return {pol: _brewster(pol) for pol in ("hz", "ez")}


def test_the_net_flux_in_front_of_a_lossless_slab_is_the_flux_behind_it(brewster):
    P = brewster["hz"]
    rel = np.abs(P[0, 0] - P[0, 1]) / P[0, 1]
    print("|P50 - P100| / P100 on the slab member:", rel, "on the vacuum member:", np.abs(P[1, 0] - P[1, 1]) / P[1, 1])
    assert np.all(P > 0) and rel <= ENERGY_BOUND


def test_brewster_incidence_by_flux(brewster):
    T, R = {}, {}
    for pol, P in brewster.items():
        T[pol], R[pol] = P[0, 1] / P[1, 1], 1 - P[0, 0] / P[1, 0]
        print(f"{pol}: T = {T[pol]:.5f}, R = {R[pol]:.5f}, T + R = {T[pol] + R[pol]:.7f}")
    assert T["hz"] > 0.95            # measured 0.98043; the window DFT of tests/test_batch_hz_bloch_cpu.py: 0.978
    assert T["ez"] < 0.25            # measured 0.21761; the window DFT: 0.217


# ---- 5. the orders ----------------------------------------------------------------------------------------------------

def test_flux_orders_of_the_ramp_driven_vacuum_member_are_order_zero_alone(vacuum):
    Pm = vacuum.flux_orders(2)                            # (1, F, Q) in fftfreq order: index 0 is m = 0
    assert Pm.shape == (1, 3, PC - 1)
    rest = np.abs(Pm[0, :, 1:]).max(axis=1) / np.abs(Pm[0, :, 0])
    print("orders m != 0 over order 0:", rest)            # measured <= 7.4e-30
    assert np.all(rest <= 1e-12)
    for line in (2, 3):
        assert np.allclose(vacuum.flux_orders(line).sum(axis=2), vacuum.flux()[:, line, :], rtol=1e-10, atol=0)
    for line in (0, 1):
        with pytest.raises(ValueError):
            vacuum.flux_orders(line)


def test_engine_flux_orders_is_the_stand_ins_sum(fd):
    """BatchEngine.flux_orders is host NumPy over read_flux_lines(): run it on the stand-in's spectra."""
    eng, rng = _members(HzBlochFluxOracle, np.float64, True)
    eng.set_hz_bloch_phase(np.array([0.4, 1.3, -2.2])).set_hz_bloch_source("ramp")
    eng.set_hz_bloch_flux_lines([("row", 3, 2, 5), ("row", 20, 0, 16), ("col", 0, 0, 40)],
                                2 * np.pi * np.array([[30e9, -55e9], [20e9, 45e9], [35e9, 60e9]]))
    eng.run(60, rng.standard_normal((3, 60)) + 1j * rng.standard_normal((3, 60)))
    f = eng.hzbfluxmon
    ln = np.array([[k == "col", at, first, n] for k, at, first, n in f["lines"]], np.int32)
    fake = types.SimpleNamespace(_bflux=False, _hzbflux=True, _flux=(ln, f["omega"]), cols=eng.cols, dx=eng.dx,
                                 _phi=eng.phi, _bloch=(np.cos(eng.phi), np.sin(eng.phi)),
                                 read_flux_lines=eng.read_flux_lines)
    got, want = fd.BatchEngine.flux_orders(fake, 1), eng.flux_orders(1)
    assert got.shape == want.shape == (3, 2, 16) and np.abs(want).max() > 0
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want).max())
    assert np.allclose(got.sum(axis=2), eng.flux()[:, 1, :], rtol=1e-10, atol=1e-12 * eng.flux_scale()[:, 1, :].max())
    assert np.abs(got[:, :, 1:]).max() > 1e-3 * np.abs(got).max()        # structured members: more than one order
    fake._phi = None                                                     # the rotation's angle serves
    assert np.all(np.abs(fd.BatchEngine.flux_orders(fake, 1) - want) <= 1e-12 * np.abs(want).max())
    for line in (0, 2):
        with pytest.raises(ValueError, match="whole period"):
            fd.BatchEngine.flux_orders(fake, line)
    # without Bloch lines of either kind the refusal stays
    fake._hzbflux = False
    with pytest.raises(fd.Fdtd2dError, match="no Bloch flux lines are set"):
        fd.BatchEngine.flux_orders(fake, 1)


# ---- 6. the Drude strips under the phase -------------------------------------------------------------------------------

G_R, G_C, G_L, G_SRC, G_STEPS, G_SIG = 121, 9, 12, 20, 11000, 1100.0
G_LINES = (40, 50, 75, 95)
G_PHI = np.array([0.0, 0.1, 0.2, 0.3])
T_README = np.array([0.97981, 0.95641, 0.92541])


def test_the_drude_strips_under_the_phase_absorb_and_phase_zero_is_the_readme_figure():
    """Members 0..3: the strips at the four phases; 4..7: vacuum at the same phases.  T, R and A by flux are in this
    file's docstring."""
    o = HzBlochFluxOracle(8, G_R, G_C, DT, DX, np.float64, "periodic")
    o.set_materials(EPS0, MU0).set_pml(L=G_L, courant00=COURANT0)
    w = np.zeros((8, G_R, G_C))
    w[:4, 60:62, 0:4] = (2e13) ** 2
    o.set_dispersion(w, 1e11, 0.0)
    o.set_sources(np.tile([G_SRC, 0, 1, G_C - 1], (8, 1)))
    o.set_hz_bloch_phase(np.tile(G_PHI, 2)).set_hz_bloch_source("ramp")
    o.set_hz_bloch_flux_lines([("row", r, 0, G_C - 1) for r in G_LINES], 2 * np.pi * FREQS)
    k = np.arange(G_STEPS) - 4.5 * G_SIG
    pulse = np.exp(-0.5 * (k / G_SIG) ** 2) * sum(np.sin(2 * np.pi * f * k * DT) for f in FREQS)
    o.run(G_STEPS, np.tile(pulse, (8, 1)) + 0j)
    P = o.flux()
    T, R = P[:4, 3] / P[4:, 3], 1 - P[:4, 0] / P[4:, 0]
    A = 1 - T - R
    with np.printoptions(precision=5, suppress=True):
        print("T\n", T, "\nR\n", R, "\nA\n", A, "\n(P50 - P75) / P95(vacuum)\n", (P[:4, 1] - P[:4, 2]) / P[4:, 3],
              "\nvacuum P40 / P95\n", P[4:, 0] / P[4:, 3])
    assert np.all(P[4:] > 0)
    assert np.all(A > 0)
    assert np.abs(T[0] - T_README).max() <= 1e-4


# ---- 7. the capacity rule, restated from the header --------------------------------------------------------------------

LDS_LIMIT = 163840


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def lds_need(R, C, esz, pole, nf, wcells, nff, cells):
    """(what must fit for a resident run, that plus both window accumulators, that plus the lines' sums of both parts):
    11 arrays (20 with a pole), the 4R row factors, 16 (C - 1) bytes of source weights, 16 bytes per window frequency
    and per line frequency; 32 nf wcells; 64 nff cells."""
    base = (20 if pole else 11) * _seg(R * C, esz) + _seg(4 * R, esz) + 16 * (C - 1) + 16 * nf + 16 * nff
    return base, base + 32 * nf * wcells, base + 32 * nf * wcells + 64 * nff * cells


@pytest.mark.parametrize("case,R,C,esz,pole,tall,fits", [
    ("40x17f32", 40, 17, 4, False, 12, True), ("40x17f64", 40, 17, 8, False, 12, True),
    ("90x33f32", 90, 33, 4, False, 40, False), ("40x17f32pole", 40, 17, 4, True, 12, True),
    ("40x17f64pole", 40, 17, 8, True, 12, True), ("60x29f32pole", 60, 29, 4, True, 30, False)])
def test_the_rule_places_the_gpu_cases(case, R, C, esz, pole, tall, fits):
    """The lines of tests/test_gpu_batch_hz_bloch_flux.py: (C - 1) + 5 + R + tall cells at 3 frequencies, beside a
    5 x 6 window at 2 frequencies.  Every case is resident and keeps its window accumulators in LDS; the sums of the lines
    fit beside them or do not, as that file expects."""
    cells = (C - 1) + 5 + R + tall
    base, with_window, with_sums = lds_need(R, C, esz, pole, 2, 30, 3, cells)
    assert base <= LDS_LIMIT and with_window <= LDS_LIMIT
    assert (with_sums <= LDS_LIMIT) == fits
    threads = min(1024, -(-(-(-R * C // 4)) // 64) * 64)
    assert threads % C != 0 and -(-R * C // threads) == 4
    gpu = __import__("test_gpu_batch_hz_bloch_flux")
    assert gpu.CASES[case][:2] == (R, C) and gpu.CASES[case][3:] == (pole, fits)
    assert np.dtype(gpu.CASES[case][2]).itemsize == esz and gpu._lines(R, C)[3][3] == tall
    assert sum(l[3] for l in gpu._lines(R, C)) == cells
    assert gpu.capacity(R, C, esz, pole, 2, (18, 1, 5, 6), 3, cells) == (base, with_window - base, with_sums - with_window)
