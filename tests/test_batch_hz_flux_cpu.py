"""CPU-only checks of the flux lines of the Hz polarisation (fdtd2d_batch_hz_flux.h, batch.py), on the stand-in of
tests/oracle_batch_hz_flux.py.

1. The surface: the three entry points are declared, exported and bound, the header adds no numbered id, the Python
   surface has its shape, bad arguments are refused before any device is touched, and without a device nothing falls back.

2. Duality, bit for bit.  The Hz stand-in with (eps, mu) against the Ez flux stand-in with (mu, eps): the fields,
   Hz_hat == Ez_hat, Et_hat == -Ht_hat and P_hz == P_ez, all np.array_equal.

3. Physics: the member of tests/test_batch_flux_cpu.py (periodic vacuum 120 x 9, dx = 1e-4, dt = 1.6e-13, a 12-row layer, a
   Ricker line source on row 40 delayed by 2 / fc, fc = c / (20 dx), 1600 steps in float64, whole-period row lines at rows
   25, 50, 56 and 75, wavelengths of 30, 20 and 12 cells), with that file's bounds.  Measured with this stand-in:
       |P50 - P75| / P50                       1.2e-15, 2.9e-16, 4.6e-15          bound 1e-9
       |P25 / P50 + 1|                         3.2e-5, 1.4e-5, 9.9e-6             bound 1e-3
       |Im / Re| of sum H conj(E), the factor  <= 2.8e-5                          bound tan(w dt / 2) / 4
       the same raw                            within 4e-4 of tan(w dt / 2)       bound 1 %
       sigma = 20 S/m on rows 60..65           |P50 - P56| / P50 <= 5.1e-15       bound 1e-9
                                               P75 / P56 = 0.0680, 0.0416, 0.0223 bound 0 < . < 0.1

4. The polariser by flux: the member of tests/test_batch_hz_cpu.py (121 x 9, layer 12, dt 5e-14, Drude strips wp = 2e13,
   gamma = 1e11 on rows 60-61 and columns 0-3, 6000 steps), the source on row 20 delayed by 1 / fc more than that file's,
   lines at rows 40, 50, 75 and 95; member 1 is empty, member 2 carries that file's Drude slab.  Measured:
       T = P95[0] / P95[1]             0.97981, 0.95641, 0.92541   (that file's window-DFT figures; bound 1e-4)
       rows 75 and 95                  agree to 9e-9
       P40[0] / P40[1]                 0.98053, 0.95720, 0.92629   (the net flux in front of the strips)
       A = (P50 - P75)[0] / P95[1]     7.2e-4, 7.9e-4, 8.8e-4      bound 0 < A < 5e-3
       |P40 - P50| / P50               bound 1e-6
       slab                            T = 0.28124, 0.46132, 0.60520 (within 5e-3 of SLAB_ANALYTIC), A = 0.2156, 0.1640, 0.1226

5. Column lines.  (a) A pml batch of two 57 x 57 float64 members, member 1 being member 0 transposed: P of a row line of
   one is P of the column line of the other (measured 4.4e-16 relative, bound 1e-12).  (b) Two nested closed boxes around
   the source and the absorber, the outward power formed on the host with the corner cells at weight 1/2: they agree to
   7.9e-6, 4.9e-6 and 5.0e-6 at 3000 steps, where the field has fallen to 1.3e-5 (bound 1e-3; a wrong sign or centring of
   a column line moves it by more than 1e-2; with the corner cells at full weight, as flux() counts them, the two boxes
   differ by 5.7e-3).

6. Neutrality: the lines never change a field, the window DFT or the probes; `every`, the step count and reset follow the
   window's rule; a refused call keeps the old lines."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle import fdtd_numpy as onp
from oracle_batch_flux import FluxLossyOracle, FluxPeriodicOracle
from oracle_batch_hz_flux import HzFluxPeriodicOracle, HzFluxPmlOracle, hz_flux_oracle_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_hz_flux.h")
NAMES = ["fdtd2d_batch_hz_flux", "fdtd2d_batch_read_hz_flux_lines", "fdtd2d_batch_set_hz_flux_lines"]
EPS0, MU0 = onp.EPS0, onp.MU0
C0 = 1 / np.sqrt(EPS0 * MU0)
DT, DX = 5e-14, 1e-4
COURANT0 = (C0 * DT) / DX
FREQS = np.array([30e9, 45e9, 60e9])


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- 1. the surface ---------------------------------------------------------------------------------------------------

def test_batch_hz_flux_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_HZ_FLUX_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_HZ_FLUX_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_HZ_FLUX_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "const int *": ctypes.POINTER(ctypes.c_int),
             "double *": ctypes.POINTER(ctypes.c_double), "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_HZ_FLUX_SIGNATURES[n][1], n
    # the prototypes are those of the Ez lines
    for n in names:
        assert _abi.BATCH_HZ_FLUX_SIGNATURES[n] == _abi.BATCH_FLUX_SIGNATURES[n.replace("hz_", "")]


def test_batch_hz_flux_adds_no_numbered_id():
    from fdtd2d_amd import _abi
    txt = open(HEADER).read()
    assert not re.findall(r"#define\s+FDTD2D_BATCH_(?:INFO|OPT)_\w+", txt)
    assert not re.findall(r"FDTD2D_BATCH_(?:INFO|OPT)_\w+\s*=", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert max(v for k, v in vars(_abi).items() if k.startswith("BATCH_INFO_") and isinstance(v, int)) == 22


def test_batch_hz_flux_python_surface(fd):
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_hz_flux_lines).parameters) == ["self", "lines", "omegas", "every"]
    assert inspect.signature(E.set_hz_flux_lines).parameters["every"].default == 1
    assert list(inspect.signature(E.read_flux_lines).parameters) == ["self", "raw"]
    assert list(inspect.signature(E.flux).parameters) == ["self"]
    p = inspect.signature(fd.run_fdtd_batch).parameters
    for name in ("hz_flux_lines", "hz_flux_omegas"):
        assert p[name].default is None and p[name].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (HzFluxPmlOracle, HzFluxPeriodicOracle):
        for name in ("set_hz_flux_lines", "read_flux_lines", "flux"):
            assert callable(getattr(cls, name))
        assert cls.polarization == "hz"
    assert hz_flux_oracle_for("pml") is HzFluxPmlOracle and hz_flux_oracle_for("periodic") is HzFluxPeriodicOracle


def test_batch_hz_flux_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ln = np.array([0, 5, 0, 4], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_hz_flux_lines(None, 1, ln, 1, dp, 1) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_hz_flux_lines(None, dp, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_hz_flux(None, dp) == _abi.E_ARG


R0, C0_ = 40, 17
BAD = [
    (dict(polarization="hz", hz_flux_lines=[("row", 5, 0, 4)]), "together"),
    (dict(polarization="hz", hz_flux_omegas=[1e11]), "together"),
    (dict(hz_flux_lines=[("row", 5, 0, 4)], hz_flux_omegas=[1e11]), 'hz_flux_lines needs polarization="hz"'),
    (dict(polarization="ez", hz_flux_lines=[("row", 5, 0, 4)], hz_flux_omegas=[1e11]),
     'hz_flux_lines needs polarization="hz"'),
    (dict(polarization="hz", flux_lines=[("row", 5, 0, 4)], flux_omegas=[1e11]),
     "flux_lines is not available with polarization"),
    (dict(polarization="hz", hz_flux_lines=[("row", 5 + k, 0, 4) for k in range(5)], hz_flux_omegas=[1e11]), "1..4 lines"),
    (dict(polarization="hz", hz_flux_lines=[("row", 5, 0, 4)], hz_flux_omegas=np.linspace(1e11, 2e11, 17)),
     "1..16 frequencies"),
    (dict(polarization="hz", hz_flux_lines=[("row", 0, 0, 4)], hz_flux_omegas=[1e11]), "row 0 outside"),
    (dict(polarization="hz", hz_flux_lines=[("col", C0_ - 1, 0, 4)], hz_flux_omegas=[1e11]), "image of column 0"),
    (dict(polarization="hz", boundary="pml", hz_flux_lines=[("col", 0, 0, 4)], hz_flux_omegas=[1e11]), "column 0 outside"),
    (dict(polarization="hz", hz_flux_lines=[("row", 5, 0, C0_)], hz_flux_omegas=[1e11]), "run past"),
    (dict(polarization="hz", hz_flux_lines=[("row", 5, 0, 4)], hz_flux_omegas=[1e11], dft_every=0), "every must be >= 1"),
]


@pytest.mark.parametrize("kwargs,match", BAD, ids=[f"{k}-{b[1]}" for k, b in enumerate(BAD)])
def test_run_fdtd_batch_refuses_bad_hz_flux_arguments_before_an_engine_exists(monkeypatch, kwargs, match):
    import fdtd2d_amd.batch as batch

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(batch, "BatchEngine", no_engine)
    args = dict(nsteps=5, sources=np.array([[20, 8]] * 2), boundary="periodic", pml_cells=6)
    args.update(kwargs)
    with pytest.raises(ValueError, match=re.escape(match)):
        batch.run_fdtd_batch(np.full((2, R0, C0_), EPS0), **args)


def test_batch_hz_flux_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 2, R0, C0_, DT, DX, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), nsteps=10, sources=np.array([[20, 8]] * 2), boundary="periodic",
                          pml_cells=6, polarization="hz", hz_flux_lines=[("row", 12, 0, C0_ - 1)], hz_flux_omegas=[2e11])
    assert ei.value.code == _abi.E_NODEVICE


# ---- 2. duality, bit for bit ------------------------------------------------------------------------------------------

DUAL = {"periodic": (40, 17), "pml": (40, 40)}


def _dual_lines(boundary, R, C):
    periodic = boundary == "periodic"
    return [("row", 20, 0, C - 1 if periodic else C), ("row", 3, 2, 9), ("col", 0 if periodic else 1, 0, R),
            ("col", C - 2, 5, 20)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", list(DUAL))
def test_hz_lines_are_the_ez_lines_of_the_dual_problem_bit_for_bit(boundary, dtype):
    R, C = DUAL[boundary]
    B, L, steps = 2, 6, 200
    rng = np.random.default_rng(11)
    eps, mu = EPS0 * (1 + 3 * rng.random((B, R, C))), MU0 * (1 + rng.random((B, R, C)))
    hz = hz_flux_oracle_for(boundary)(B, R, C, DT, DX, dtype, boundary)
    ez = (FluxPeriodicOracle if boundary == "periodic" else FluxLossyOracle)(B, R, C, DT, DX, dtype, boundary)
    hz.set_materials(eps, mu)
    ez.set_materials(mu, eps)
    c00 = (1 / np.sqrt(eps[:, 0, 0] * mu[:, 0, 0]) * DT) / DX        # symmetric in eps and mu
    om = 2 * np.pi * np.array([FREQS, FREQS * 1.3])
    amps = rng.standard_normal((B, steps))
    for o in (hz, ez):
        o.set_pml(L=L, courant00=c00)
        o.set_sources(np.array([[18, 3, 2, 3], [22, C - 4, 1, 2]]))
    hz.set_hz_flux_lines(_dual_lines(boundary, R, C), om, every=3)
    ez.set_flux_lines(_dual_lines(boundary, R, C), om, every=3)
    hz.run(steps, amps)
    ez.run(steps, amps)
    (h, ex, ey), (e, hx, hy) = hz.download(), ez.download()
    assert np.any(h) and np.all(np.isfinite(h))
    assert np.array_equal(h, e) and np.array_equal(ex, -hx) and np.array_equal(ey, -hy)
    for raw in (True, False):
        (et_hat, hz_hat), (ez_hat, ht_hat) = hz.read_flux_lines(raw), ez.read_flux_lines(raw)
        assert np.all(np.abs(hz_hat).max(axis=(1, 2)) > 0) and np.all(np.abs(et_hat).max(axis=(1, 2)) > 0)
        assert np.array_equal(hz_hat, ez_hat) and np.array_equal(et_hat, -ht_hat)
    assert np.all(hz.flux() != 0) and np.array_equal(hz.flux(), ez.flux())
    assert np.array_equal(hz.flux_scale(), ez.flux_scale())


# ---- 3. the physics ---------------------------------------------------------------------------------------------------

PR, PC, PDX, PDT, PSTEPS, PL, PSRC = 120, 9, 1e-4, 1.6e-13, 1600, 12, 40
PLINES = (25, 50, 56, 75)
POMEGA = 2 * np.pi * C0 / (np.array([30.0, 20.0, 12.0]) * PDX)
PFC = C0 / (20 * PDX)


def _physics(sigma=None):
    # the library's Ricker wavelet, delayed by 2 / fc (tests/test_batch_flux_cpu.py says why)
    amps = np.array([onp.ricker_amplitude(i * PDT - 1 / PFC, PFC) for i in range(PSTEPS)])
    assert abs(amps[0]) < 1e-15 and abs(amps).max() > 0.99
    eng = HzFluxPeriodicOracle(1, PR, PC, PDT, PDX, dtype=np.float64)
    eng.set_materials(np.full((1, PR, PC), EPS0), np.full((1, PR, PC), MU0))
    eng.set_pml(PL, courant00=(C0 * PDT) / PDX)
    if sigma is not None:
        s = np.zeros((1, PR, PC))
        s[:, 60:66, :] = sigma
        eng.set_conductivity(s)
    eng.set_sources(np.array([[PSRC, 0, 1, PC - 1]]))
    eng.set_hz_flux_lines([("row", r, 0, PC - 1) for r in PLINES], POMEGA)
    eng.run(PSTEPS, amps[None])
    assert np.abs(eng.Ez).max() < 1e-12                  # the record is complete
    return eng


@pytest.fixture(scope="module")
def lossless():
    return _physics()


def test_hz_flux_is_conserved_between_lines_and_reverses_behind_the_source(lossless):
    P = lossless.flux()[0]                               # (line, frequency)
    assert np.all(P[1] > 0)
    cons = np.abs(P[1] - P[3]) / P[1]
    print("conservation |P50 - P75| / P50:", cons)       # measured 1.2e-15, 2.9e-16, 4.6e-15
    assert np.all(cons <= 1e-9)
    up = np.abs(P[0] / P[1] + 1)
    print("upstream |P25 / P50 + 1|:", up)                # measured 3.2e-5, 1.4e-5, 9.9e-6
    assert np.all(up <= 1e-3)


def test_half_step_factor_on_et_makes_the_hz_flux_real(lossless):
    tan = np.tan(POMEGA * PDT / 2)
    n = PC - 1
    for raw in (False, True):
        E, H = lossless.read_flux_lines(raw=raw)
        z = (H[0] * np.conj(E[0])).reshape(3, len(PLINES), n).sum(axis=2)     # (frequency, line)
        ratio = np.abs(z.imag / z.real)
        print("raw" if raw else "with the factor", "|Im / Re|:", ratio.max(axis=1))
        if raw:
            assert np.all(np.abs(ratio / tan[:, None] - 1) <= 0.01)            # measured: within 4e-4
            assert np.all(z.imag / z.real > 0) or np.all(z.imag / z.real < 0)
        else:
            assert np.all(ratio <= 0.25 * tan[:, None])                        # measured <= 2.8e-5


def test_a_conducting_slab_absorbs_what_the_hz_lines_miss(lossless):
    P = _physics(sigma=20.0).flux()[0]
    same = np.abs(P[1] - P[2]) / P[1]
    print("|P50 - P56| / P50:", same, " P75 / P56:", P[3] / P[2])              # measured <= 5.1e-15; 0.0680, 0.0416, 0.0223
    assert np.all(same <= 1e-9)
    assert np.all(P[3] > 0) and np.all(P[3] < 0.1 * P[2])
    # and the slab reflects: less net power reaches line 50 than without it
    assert np.all(P[1] < lossless.flux()[0][1])


# ---- 4. the polariser by flux -----------------------------------------------------------------------------------------

G_R, G_C, G_L, G_SRC, G_STEPS = 121, 9, 12, 20, 6000
G_LINES = (40, 50, 75, 95)
T_WINDOW = np.array([0.97981, 0.95641, 0.92541])          # tests/test_batch_hz_cpu.py, the window DFT of row 95
SLAB_ANALYTIC = np.array([0.27896, 0.45896, 0.60370])


@pytest.fixture(scope="module")
def polariser():
    """Member 0: the strips; member 1: empty; member 2: the Drude slab.  (P (member, line, frequency), the window DFT's
    sum |F|^2 on row 95 (member, frequency))."""
    o = HzFluxPeriodicOracle(3, G_R, G_C, DT, DX, np.float64, "periodic")
    o.set_materials(EPS0, MU0).set_pml(L=G_L, courant00=COURANT0)
    w = np.zeros((3, G_R, G_C))
    w[0, 60:62, 0:4] = (2e13) ** 2
    w[2, 60:64, :] = (6e11) ** 2
    o.set_dispersion(w, [1e11, 0.0, 5e10], 0.0)
    o.set_sources(np.tile([G_SRC, 0, 1, G_C - 1], (3, 1)))
    o.set_dft_window((G_LINES[3], 0, 1, G_C - 1), 2 * np.pi * FREQS)
    o.set_hz_flux_lines([("row", r, 0, G_C - 1) for r in G_LINES], 2 * np.pi * FREQS)
    fc = 45e9
    o.run(G_STEPS, np.tile([onp.ricker_amplitude(k * DT - 1 / fc, fc) for k in range(G_STEPS)], (3, 1)))
    return o.flux(), (np.abs(o.read_dft_window()) ** 2).sum(axis=(2, 3))


def test_the_wire_grid_transmission_by_flux_is_the_window_dft_figure(polariser):
    P, F2 = polariser
    T = P[0, 3] / P[1, 3]
    print("T by flux", T, "by the window DFT", F2[0] / F2[1], "P75 against P95", np.abs(P[0, 2] / P[0, 3] - 1),
          "net flux on row 40 over the empty member's", P[0, 0] / P[1, 0])
    assert np.all(P[1] > 0)
    assert np.abs(T - T_WINDOW).max() <= 1e-4
    assert np.abs(T - F2[0] / F2[1]).max() <= 1e-4
    assert np.abs(P[0, 2] / P[0, 3] - 1).max() <= 1e-6     # measured 9e-9: nothing absorbs behind the strips


def test_the_strips_absorb_little_and_the_flux_in_front_of_them_is_conserved(polariser):
    P, _ = polariser
    A = (P[0, 1] - P[0, 2]) / P[1, 3]
    front = np.abs(P[0, 0] - P[0, 1]) / P[0, 1]
    print("A", A, "|P40 - P50| / P50", front)              # measured 7.2e-4, 7.9e-4, 8.8e-4
    assert np.all(A > 0) and np.all(A < 5e-3)
    assert np.all(front <= 1e-6)


def test_the_drude_slab_by_flux_follows_the_analytic_formula(polariser):
    P, _ = polariser
    T = P[2, 3] / P[1, 3]
    A = (P[2, 1] - P[2, 2]) / P[1, 3]
    print("slab T", T, "A", A, "R + T + A", 1 - P[2, 0] / P[1, 0] + T + A)    # measured T 0.28124, 0.46132, 0.60520
    assert np.abs(T - SLAB_ANALYTIC).max() <= 5e-3
    assert np.all(A > 0) and np.all(A < 1 - T)              # measured 0.2156, 0.1640, 0.1226; R = 1 - T - A > 0
    # what enters the slab's side of row 50 is what leaves through row 75 plus what the slab absorbs
    assert np.abs(P[2, 0] / P[1, 0] - (T + A)).max() <= 1e-6


# ---- 5. column lines --------------------------------------------------------------------------------------------------

N5, L5, STEPS5 = 57, 10, 3000


def _scene(transposed=(False,)):
    """57 x 57 float64 pml members: eps x 2.5 on [26:34, 22:27], sigma = 5 S/m on [36:40, 20:30], a 1 x 1 source at
    (30, 24); a transposed member has all three transposed."""
    B = len(transposed)
    eps, sigma = np.full((B, N5, N5), EPS0), np.zeros((B, N5, N5))
    eps[:, 26:34, 22:27] *= 2.5
    sigma[:, 36:40, 20:30] = 5.0
    src = np.tile([30, 24, 1, 1], (B, 1))
    for b, t in enumerate(transposed):
        if t:
            eps[b], sigma[b], src[b] = eps[b].T.copy(), sigma[b].T.copy(), [24, 30, 1, 1]
    o = HzFluxPmlOracle(B, N5, N5, DT, DX, np.float64, "pml")
    o.set_materials(eps, MU0).set_pml(L=L5, courant00=COURANT0)
    o.set_conductivity(sigma).set_sources(src)
    fc = 45e9
    amps = np.tile([onp.ricker_amplitude(k * DT - 1 / fc, fc) for k in range(STEPS5)], (B, 1))
    return o, amps


def test_a_row_line_of_a_member_is_the_column_line_of_its_transpose():
    o, amps = _scene((False, True))
    o.set_hz_flux_lines([("row", 44, 16, 21), ("col", 44, 16, 21), ("row", 18, 16, 21), ("col", 18, 16, 21)],
                        2 * np.pi * FREQS)
    o.run(STEPS5, amps)
    P = o.flux()
    assert np.all(P[0, 0] > 0) and np.all(P[0, 1] > 0) and np.all(P[0, 2] < 0) and np.all(P[0, 3] < 0)
    rel = max(np.abs(P[0, a] / P[1, b] - 1).max() for a, b in ((0, 1), (1, 0), (2, 3), (3, 2)))
    print("row of one against column of the other:", rel)     # measured 4.4e-16
    assert rel <= 1e-12


def _outward(box):
    """The power that leaves the closed box (r0, r1, c0, c1) of member 0, per frequency: four lines, formed on the host
    from the transforms, the corner cells (each on two lines) at weight 1/2."""
    r0, r1, c0, c1 = box
    o, amps = _scene()
    nr, nc = r1 - r0 + 1, c1 - c0 + 1
    o.set_hz_flux_lines([("row", r0, c0, nc), ("row", r1, c0, nc), ("col", c0, r0, nr), ("col", c1, r0, nr)],
                        2 * np.pi * FREQS)
    o.run(STEPS5, amps)
    print("end field", np.abs(o.Ez).max())
    E, H = o.read_flux_lines()
    s = np.real(H[0] * np.conj(E[0])) * DX                     # (frequency, cell): S_y = -this on rows, S_x = +this
    w = np.ones(s.shape[1])
    sign = np.concatenate([np.full(nc, +1.0), np.full(nc, -1.0), np.full(nr, -1.0), np.full(nr, +1.0)])
    for first, n in ((0, nc), (nc, nc), (2 * nc, nr), (2 * nc + nr, nr)):
        w[first] = w[first + n - 1] = 0.5
    total = (s * (sign * w)[None, :]).sum(axis=1)
    # the same from flux(), which has the corners at full weight: it differs
    P = o.flux()[0]
    return total, -P[0] + P[1] - P[2] + P[3]


def test_two_nested_closed_boxes_pass_the_same_power():
    inner, inner_full = _outward((18, 44, 16, 36))
    outer, outer_full = _outward((14, 46, 13, 42))
    rel = np.abs(inner / outer - 1)
    print("outward power", inner, outer, "relative difference", rel, "with full-weight corners",
          np.abs(inner_full / outer_full - 1))                  # measured 7.9e-6; full-weight corners 5.7e-3
    assert np.all(inner > 0) and np.all(outer > 0)
    assert np.all(rel <= 1e-3)


# ---- 6. neutrality ----------------------------------------------------------------------------------------------------

def _member(boundary, pole, dtype=np.float32, R=24, C=13, seed=3):
    rng = np.random.default_rng(seed)
    eng = hz_flux_oracle_for(boundary)(2, R, C, DT, DX, dtype=dtype, boundary=boundary)
    eng.set_materials(EPS0 * (1 + rng.random((2, R, C))), MU0 * (1 + rng.random((2, R, C))))
    eng.set_pml(4, courant00=COURANT0)
    if pole:
        eng.set_conductivity(0.5).set_dispersion(4e22, np.array([1e11, 0.0]), np.array([0.0, 3e11]))
    eng.set_sources(np.array([[9, 3, 2, 2], [10, 4, 1, 3]]))
    eng.set_dft_window((7, 2, 5, 6), 2 * np.pi * np.array([30e9, 55e9]), every=2)
    eng.set_probes(np.array([[8, 0], [11, C - 2], [12, 5]]), 40)
    return eng


@pytest.mark.parametrize("pole", [False, True])
@pytest.mark.parametrize("boundary", ["pml", "periodic"])
def test_hz_lines_never_change_a_field_or_another_monitor(boundary, pole):
    amps = np.random.default_rng(5).standard_normal((2, 30))
    col = 0 if boundary == "periodic" else 1
    lines = [("row", 9, 0, 12), ("col", col, 2, 20), ("col", 11, 7, 5), ("row", 2, 3, 4)]
    out = []
    for with_lines in (False, True):
        eng = _member(boundary, pole)
        if with_lines:
            eng.set_hz_flux_lines(lines, 2 * np.pi * np.array([[30e9, 55e9, 80e9], [20e9, 45e9, 70e9]]), every=3)
        eng.run(30, amps)
        out.append(eng.download() + (eng.Ezx.copy(), eng.read_dft_window(), eng.read_probes()) +
                   (eng.download_dispersion() if pole else ()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    E, H = eng.read_flux_lines(raw=True)
    assert E.shape == H.shape == (2, 3, 41) and np.all(np.abs(H).max(axis=(1, 2)) > 0) and np.abs(E).max() > 0
    # the cell (9, col) lies on the row line (its cell `col`) and on the column line (its cell 9 - 2): one Hz, two Et
    assert np.array_equal(H[:, :, col], H[:, :, 12 + 7])
    assert not np.array_equal(E[:, :, col], E[:, :, 12 + 7])


def test_hz_sampling_follows_the_window_rule_reset_zeroes_and_a_refused_call_keeps_the_lines():
    om = 2 * np.pi * np.array([40e9, 70e9])
    amps = np.random.default_rng(6).standard_normal((2, 40))
    eng = _member("periodic", False)
    eng.run(7, amps[:, :7])
    eng.set_dft_window((9, 0, 1, 12), om, every=3)       # the same cells, frequencies and rule as the line's Hz
    eng.set_hz_flux_lines([("row", 9, 0, 12)], om, every=3)
    eng.run(33, amps[:, 7:])
    _, H = eng.read_flux_lines(raw=True)
    assert np.array_equal(H, eng.read_dft_window()[:, :, 0, :])
    # one run or two, the same sums
    one = _member("periodic", False)
    one.run(7, amps[:, :7])
    one.set_hz_flux_lines([("row", 9, 0, 12)], om, every=3)
    one.run(20, amps[:, 7:27])
    one.run(13, amps[:, 27:])
    for a, b in zip(one.read_flux_lines(), eng.read_flux_lines()):
        assert np.array_equal(a, b)
    assert np.array_equal(one.flux(), eng.flux())
    # refused calls keep the old lines and their sums
    before = eng.read_flux_lines() + (eng.flux(),)
    for bad in ([("row", 0, 0, 4)], [("col", 12, 0, 4)], [("row", 5, 0, 13)], [("row", 5 + k, 0, 4) for k in range(5)]):
        with pytest.raises(AssertionError):
            eng.set_hz_flux_lines(bad, om)
    with pytest.raises(AssertionError, match="Hz polarisation"):
        eng.set_flux_lines([("row", 9, 0, 12)], om)
    for a, b in zip(before, eng.read_flux_lines() + (eng.flux(),)):
        assert np.array_equal(a, b)
    eng.reset()
    assert not np.any(eng.read_flux_lines()[0]) and not np.any(eng.read_flux_lines()[1]) and not np.any(eng.flux())
    eng.run(3, amps[:, :3])                              # the count restarts: step 3 is sampled
    assert np.any(eng.read_flux_lines()[1])
