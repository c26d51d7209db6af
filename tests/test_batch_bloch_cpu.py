"""CPU-only checks of the Bloch phase of periodic batches (fdtd2d_batch_bloch.h, batch.py): the stand-in
(tests/oracle_batch_bloch.py) alone, plus the surface and the host refusals.

A complex field that repeats as F(x + Q) = F(x) e^{i phi} with phi = 2 pi m / N is periodic over N periods, and its real
and imaginary parts are two real fields of an N-period supercell driven, period n, with cos(phi n) and sin(phi n) times
the source.  So every supercell test runs the Bloch member (one period, a one-cell rectangle source with real amplitudes)
against ``PeriodicOracle`` members of N periods with one unit-channel point source per period, weight w_n.  For rho =
(1, 0), (-1, 0) and (0, 1) every product with rho is exact and negation commutes with every rounding, so these agree bit
for bit; for N = 3 and 5 the rotations round, and the two sides agree to rounding only.

Shapes: 40 rows, Q = 12, an 8-cell layer, dt 1.6e-13, dx 1e-4, Ricker 150 GHz, 300 steps, eps_r random in [1, 4] and
sigma random in [0, 2] S/m on rows 16..23.  ``tests/test_gpu_batch_bloch.py`` runs the same checks on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle_batch_bloch import BlochOracle
from oracle_batch_periodic import PeriodicOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_bloch.h")
NAMES = ["fdtd2d_batch_read_dft_window_bloch", "fdtd2d_batch_read_probes_bloch", "fdtd2d_batch_run_bloch",
         "fdtd2d_batch_set_bloch", "fdtd2d_batch_set_bloch_source", "fdtd2d_batch_transfer_bloch"]
EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7
C0 = 1 / np.sqrt(EPS0 * MU0)
ROWS, Q, LAYER, DT, DX, FC, NSTEPS = 40, 12, 8, 1.6e-13, 1e-4, 150e9, 300
SRC = (12, 4)                 # the source cell of period 0


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def ricker(nsteps, dt, fc):
    from fdtd2d_amd.api import ricker_amplitude
    return np.array([ricker_amplitude(n * dt, fc) for n in range(nsteps)])


def materials(seed=5):
    """(eps, sigma) of one period, (ROWS, Q + 1), the image column equal to column 0."""
    rng = np.random.default_rng(seed)
    eps, sigma = np.full((ROWS, Q + 1), EPS0), np.zeros((ROWS, Q + 1))
    eps[16:24, :Q] = EPS0 * (1 + 3 * rng.random((8, Q)))
    sigma[16:24, :Q] = 2 * rng.random((8, Q))
    eps[:, Q], sigma[:, Q] = eps[:, 0], sigma[:, 0]
    return eps, sigma


def tiled(a, n):
    """n periods of a one-period array and the image column."""
    return np.concatenate([a[:, :Q]] * n + [a[:, :1]], axis=1)


def run_bloch(engine, dtype, phi=None, rotation=None, nsteps=NSTEPS, **kw):
    """The Bloch member on `engine` (the stand-in, or the device engine): complex (Ez, Hx, Hy)."""
    eps, sigma = materials()
    with engine(1, ROWS, Q + 1, DT, DX, dtype=dtype, boundary="periodic", **kw) as eng:
        eng.set_materials(eps[None], MU0)
        eng.set_pml(LAYER, courant00=C0 * DT / DX)
        eng.set_conductivity(sigma[None])
        eng.set_sources(np.array([SRC]))
        eng.set_bloch_phase(phi, rotation=rotation)
        eng.run(nsteps, ricker(nsteps, DT, FC)[None])
        return [a[0] for a in eng.download()]


def run_supercell(engine, dtype, weights, nsteps=NSTEPS, **kw):
    """len(weights) periods on a plain periodic `engine`, one unit-channel point source per period: real (Ez, Hx, Hy)."""
    n = len(weights)
    eps, sigma = (tiled(a, n) for a in materials())
    with engine(1, ROWS, n * Q + 1, DT, DX, dtype=dtype, boundary="periodic", **kw) as eng:
        eng.set_materials(eps[None], MU0)
        eng.set_pml(LAYER, courant00=C0 * DT / DX)
        eng.set_conductivity(sigma[None])
        eng.set_point_sources(np.array([(SRC[0], SRC[1] + k * Q) for k in range(n)]),
                              np.asarray(weights, dtype=np.float64)[:, None])
        eng.run(nsteps, None, ricker(nsteps, DT, FC)[None])
        return [a[0] for a in eng.download()]


def period(fields, k):
    """Period k of a supercell's (Ez, Hx, Hy) in a one-period member's shapes (Ez with its image column)."""
    Ez, Hx, Hy = fields
    return Ez[:, k * Q:(k + 1) * Q + 1], Hx[:, k * Q:(k + 1) * Q], Hy[:, k * Q:(k + 1) * Q + 1]


def same(a, b):
    """array_equal of a member's fields; Hy's column C-1 is the supercell's next period there, a permanent zero here."""
    return all(np.array_equal(x[..., :Q], y[..., :Q]) for x, y in zip(a, b)) and np.array_equal(a[0], b[0])


def check_unit_rotation(bloch_engine, periodic_engine, dtype, **kw):
    got = run_bloch(bloch_engine, dtype, rotation=(1, 0), **kw)
    want = run_supercell(periodic_engine, dtype, [1.0], **kw)
    assert np.abs(want[0]).max() > 0 and np.abs(want[2]).max() > 0
    for g, w in zip(got, want):
        assert np.iscomplexobj(g) and np.array_equal(g.real, w) and not g.imag.any()


def check_half_turn(bloch_engine, periodic_engine, dtype, **kw):
    got = run_bloch(bloch_engine, dtype, rotation=(-1, 0), **kw)
    sup = run_supercell(periodic_engine, dtype, [1.0, -1.0], **kw)
    assert np.abs(got[0].real).max() > 0 and not any(g.imag.any() for g in got)
    assert same([g.real for g in got], period(sup, 0))
    assert same([-g.real for g in got], period(sup, 1))


def check_quarter_turn(bloch_engine, periodic_engine, dtype, **kw):
    got = run_bloch(bloch_engine, dtype, rotation=(0, 1), **kw)
    re = run_supercell(periodic_engine, dtype, [1.0, 0.0, -1.0, 0.0], **kw)
    im = run_supercell(periodic_engine, dtype, [0.0, 1.0, 0.0, -1.0], **kw)
    assert np.abs(got[0].real).max() > 0 and np.abs(got[0].imag).max() > 0
    assert same([g.real for g in got], period(re, 0))
    assert same([g.imag for g in got], period(im, 0))
    assert same([g.imag for g in got], period(re, 3))       # F(x + 3Q) = -i F(x)


def nth_root_difference(bloch_engine, periodic_engine, m, N, **kw):
    """max|difference| / max|field| between the Bloch member at phi = 2 pi m / N and period 0 of the N-period supercells
    driven with cos(phi n) and sin(phi n), float64, over Ez, Hx and Hy."""
    phi = 2 * np.pi * m / N
    got = run_bloch(bloch_engine, np.float64, phi=phi, **kw)
    re = period(run_supercell(periodic_engine, np.float64, np.cos(phi * np.arange(N)), **kw), 0)
    im = period(run_supercell(periodic_engine, np.float64, np.sin(phi * np.arange(N)), **kw), 0)
    worst = 0.0
    for g, r, i in zip(got, re, im):
        scale = max(np.abs(r).max(), np.abs(i).max())
        assert scale > 0
        worst = max(worst, np.abs(g.real[..., :Q] - r[..., :Q]).max() / scale, np.abs(g.imag[..., :Q] - i[..., :Q]).max() / scale)
    return worst


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_batch_bloch_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_BLOCH_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_BLOCH_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_BLOCH_SIGNATURES[n][0]
    main = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    assert "bloch" not in main.lower()                     # a companion header: fdtd2d.h declares none of it


def test_batch_bloch_constant_is_named_and_its_id_free():
    from fdtd2d_amd import _abi
    pat = r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)"
    mine = dict(re.findall(pat, open(HEADER).read()))
    assert mine == {"BATCH_INFO_BLOCH": "16"} and _abi.BATCH_INFO_BLOCH == 16
    taken = {}
    for h in ("fdtd2d.h", "fdtd2d_batch_pml.h", "fdtd2d_batch_monitor.h", "fdtd2d_batch_adjoint.h",
              "fdtd2d_batch_design.h", "fdtd2d_batch_lossy.h", "fdtd2d_batch_periodic.h"):
        taken.update(re.findall(pat, open(os.path.join(ROOT, "include", h)).read()))
    assert max(int(v) for k, v in taken.items() if k.startswith("BATCH_INFO")) == 15
    lib = _abi.load()
    assert lib.fdtd2d_batch_set_bloch(None, None, None) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_INFO_BLOCH) == _abi.E_ARG


def test_the_no_bloch_sentences_are_gone():
    for path, gone in (("README.md", "No Bloch phase"), ("fdtd-2d_amd/batch.py", "There is no Bloch phase"),
                       ("include/fdtd2d_batch_periodic.h", "Not supported: the Mur frame, a Bloch phase")):
        assert gone not in " ".join(open(os.path.join(ROOT, path)).read().split()), path


# ---- 2. exact properties of the stand-in ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_unit_rotation_is_the_periodic_batch(dtype):
    check_unit_rotation(BlochOracle, PeriodicOracle, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_half_turn_is_a_two_period_supercell(dtype):
    check_half_turn(BlochOracle, PeriodicOracle, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_quarter_turn_is_two_four_period_supercells(dtype):
    check_quarter_turn(BlochOracle, PeriodicOracle, dtype)


# measured here (NumPy, float64): max|difference| / max|field| over Ez, Hx, Hy after 300 steps
ROOT_MEASURED = {(1, 3): 3.3e-15, (2, 5): 5.9e-15}
ROOT_BOUND = {k: 10 * v for k, v in ROOT_MEASURED.items()}


@pytest.mark.parametrize("m,N", [(1, 3), (2, 5)])
def test_nth_root_phases_match_their_supercells_to_rounding(m, N):
    d = nth_root_difference(BlochOracle, PeriodicOracle, m, N)
    print(f"phi = 2 pi {m}/{N}: max|difference| / max|field| = {d:.3e} (bound {ROOT_BOUND[m, N]:.3e})")
    assert d <= ROOT_BOUND[m, N]


# ---- 3. the obliquely travelling wave obeys the Yee dispersion relation -----------------------------------------------

D_ROWS, D_Q, D_L, D_F, D_PHI, D_STEPS, D_SRC_ROW = 120, 12, 20, 150e9, np.pi / 3, 4000, 30
D_WINDOW = (50, 0, 40, 1)      # column 0, rows 50..89: below the source, above the layer
D_MEASURED = 6.8e-6              # measured here (NumPy, float64): worst |advance per row - k_y dx| / (k_y dx)
D_BOUND = 10 * D_MEASURED


def dispersion_residual(engine, dtype=np.float64, **kw):
    """A vacuum cell with a layer and the ramp line source across the period at exp(+i w t): after the transient the
    window DFT at w advances by -k_y dx per row below the source, k_y from the Yee dispersion relation with k_x =
    phi / (Q dx).  Returns the worst relative deviation of the advance per row over the window."""
    w = 2 * np.pi * D_F
    n = np.arange(D_STEPS)
    amps = (1 - np.exp(-(n / 400.0) ** 2)) * np.exp(1j * w * n * DT)
    with engine(1, D_ROWS, D_Q + 1, DT, DX, dtype=dtype, boundary="periodic", **kw) as eng:
        eng.set_materials(np.full((1, D_ROWS, D_Q + 1), EPS0), MU0)
        eng.set_pml(D_L, courant00=C0 * DT / DX)
        eng.set_sources(np.array([(D_SRC_ROW, 0, 1, D_Q)]))
        eng.set_bloch_phase(D_PHI).set_bloch_source("ramp")
        eng.run(D_STEPS - 1000, amps[None, :D_STEPS - 1000])
        eng.set_dft_window(D_WINDOW, [w])
        eng.run(1000, amps[None, D_STEPS - 1000:])
        W = eng.read_dft_window()[0, 0, :, 0]
    kx = D_PHI / (D_Q * DX)
    rhs = (np.sin(w * DT / 2) / (C0 * DT)) ** 2 - (np.sin(kx * DX / 2) / DX) ** 2
    ky = 2 / DX * np.arcsin(DX * np.sqrt(rhs))
    advance = np.angle(W[1:] / W[:-1])
    return np.abs(advance + ky * DX).max() / (ky * DX)


def test_oblique_wave_obeys_the_yee_dispersion_relation():
    r = dispersion_residual(BlochOracle)
    print(f"worst |advance per row + k_y dx| / (k_y dx) = {r:.3e} (bound {D_BOUND:.3e})")
    assert r <= D_BOUND


# ---- 4. host refusals ------------------------------------------------------------------------------------------------

class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def host_engine(fd, bloch=True, boundary="periodic", count=3, rows=30, cols=13):
    """A BatchEngine without a handle, for the checks that never reach the library."""
    eng = object.__new__(fd.BatchEngine)
    eng._lib, eng._h = _NoLibrary(), ctypes.c_void_p()
    eng.count, eng.rows, eng.cols, eng.dt, eng.dx = count, rows, cols, DT, DX
    eng.dtype, eng.boundary = np.dtype(np.float32), boundary
    eng._pml_on, eng._pml_chosen, eng._pml_L = False, True, 0
    eng._win, eng._nprobe, eng._npoint = (1, 2, 2), 1, (1, 1)
    eng._bloch = (np.ones(count), np.zeros(count)) if bloch else None
    eng._phi = np.zeros(count) if bloch else None
    return eng


@pytest.mark.parametrize("call,what", [
    (lambda e: e.set_dft(1e11), "the whole-grid transform"),
    (lambda e: e.set_point_sources(np.array([(5, 5)]), np.ones((1, 1))), "a point source"),
    (lambda e: e.run(4, None, np.zeros((1, 4))), "a run with channels"),
    (lambda e: e.hold_dft_window(), "the held window"),
    (lambda e: e.dft_window_product(np.ones(1)), "the window product"),
    (lambda e: e.probe_spectra([1e11]), "fdtd2d_batch_probe_spectra"),
    (lambda e: e.field_absmax("Ez"), "fdtd2d_batch_field_absmax"),
])
def test_what_a_bloch_phase_excludes_is_refused_on_the_host(fd, call, what):
    from fdtd2d_amd import _abi
    with pytest.raises(fd.Fdtd2dError, match="is not available while a Bloch phase is set") as ei:
        call(host_engine(fd))
    assert ei.value.code == _abi.E_STATE and what in str(ei.value)
    with pytest.raises(AssertionError, match="the library was called"):     # without a phase the call goes through
        call(host_engine(fd, bloch=False))


def test_monitors_in_the_image_column_are_refused_on_the_host(fd):
    from fdtd2d_amd import _abi
    for call in (lambda e: e.set_dft_window((4, 10, 3, 3), [1e11]), lambda e: e.set_probes([(4, 2), (9, 12)], 10),
                 lambda e: e.set_probes(np.array([[(4, 2)], [(4, 12)], [(4, 3)]]), 10)):
        with pytest.raises(fd.Fdtd2dError, match="touches column 12, the image of column 0") as ei:
            call(host_engine(fd))
        assert ei.value.code == _abi.E_ARG
    for call in (lambda e: e.set_dft_window((4, 9, 3, 3), [1e11]), lambda e: e.set_probes([(4, 0), (9, 11)], 10)):
        with pytest.raises(AssertionError, match="the library was called"):
            call(host_engine(fd))


def test_bad_bloch_arguments_are_refused_on_the_host(fd):
    from fdtd2d_amd import _abi
    with pytest.raises(ValueError, match=r"phi must be a scalar or have shape \(3,\)"):
        host_engine(fd).set_bloch_phase(np.zeros(2))
    with pytest.raises(ValueError, match=r"c must be a scalar or have shape \(3,\)"):
        host_engine(fd).set_bloch_phase(None, rotation=(np.ones(4), 0.0))
    with pytest.raises(ValueError, match="rotation must be a pair"):
        host_engine(fd).set_bloch_phase(None, rotation=(1.0, 0.0, 0.0))
    with pytest.raises(fd.Fdtd2dError, match="a Bloch phase needs periodic columns") as ei:
        host_engine(fd, bloch=False, boundary="pml").set_bloch_phase(0.3)
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(fd.Fdtd2dError, match="no Bloch phase is set") as ei:
        host_engine(fd, bloch=False).set_bloch_source("ramp")
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(ValueError, match=r"weights must have shape \(12,\) or \(3, 12\)"):
        host_engine(fd).set_bloch_source(np.ones(13))
    with pytest.raises(ValueError, match='weights must be "ramp", None or an array'):
        host_engine(fd).set_bloch_source("tilt")
    eng = host_engine(fd)
    eng._phi = None                                        # as after set_bloch_phase(None, rotation=...)
    with pytest.raises(ValueError, match="needs the phases"):
        eng.set_bloch_source("ramp")
    for call in (lambda e: e.upload(Ez=np.zeros((3, 30, 13), complex)), lambda e: e.upload_ezx(np.zeros((3, 30, 13), complex)),
                 lambda e: e.run(4, np.zeros((3, 4), complex))):
        with pytest.raises(ValueError, match="need a Bloch phase"):
            call(host_engine(fd, bloch=False))
    with pytest.raises(ValueError, match=r"Ez must have shape \(3, 30, 13\)"):
        host_engine(fd).upload(Ez=np.zeros((3, 30, 12), complex))
    with pytest.raises(ValueError, match="unknown boundary"):
        fd.BatchEngine(2, 40, 21, boundary="bloch")


def test_run_fdtd_batch_checks_its_bloch_arguments_on_the_host(monkeypatch, fd):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    eps = np.full((2, 30, 13), EPS0)
    kw = dict(nsteps=10, sources=np.array([(5, 5), (5, 5)]), dt=DT, dx=DX)
    with pytest.raises(ValueError, match='bloch_phase needs boundary="periodic"'):
        fd.run_fdtd_batch(eps, boundary="pml", pml_cells=5, bloch_phase=0.2, **kw)
    with pytest.raises(ValueError, match="source_weights needs bloch_phase"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, source_weights="ramp", **kw)
    with pytest.raises(ValueError, match="omega .* is not available with bloch_phase"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, bloch_phase=0.2, omega=1e11, **kw)
    with pytest.raises(ValueError, match="touches column 12"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, bloch_phase=0.2, dft_window=(3, 11, 2, 2),
                          window_omegas=[1e11], **kw)
    with pytest.raises(ValueError, match="a probe lies in column 12"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, bloch_phase=0.2, probes=[(3, 12)], **kw)
    with pytest.raises(AssertionError, match="the device was touched"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, bloch_phase=[0.2, 0.4], source_weights="ramp",
                          dft_window=(3, 10, 2, 2), window_omegas=[1e11], probes=[(3, 11)], **kw)


def test_the_adjoint_helpers_refuse_a_bloch_engine(fd):
    """An engine factory that sets a phase, and a phase set on a session's engine: E_STATE before any run."""
    from fdtd2d_amd import _abi
    from test_batch_periodic_cpu import g_args, g_materials, g_objective
    eps, sigma = g_materials()

    def factory(count, rows, cols, *a, **k):
        return host_engine(fd, count=count, rows=rows, cols=cols)

    for call in (lambda: fd.batch_eps_gradient(eps, objective=g_objective, **g_args(2, engine=factory, nsteps=50)),
                 lambda: fd.batch_material_gradient(eps, sigma, objective=g_objective, **g_args(2, engine=factory, nsteps=50)),
                 lambda: fd.AdjointSession(eps, **g_args(2, engine=factory, nsteps=50))):
        with pytest.raises(fd.Fdtd2dError, match="adjoint gradients are not available while a Bloch phase is set") as ei:
            call()
        assert ei.value.code == _abi.E_STATE
    with fd.AdjointSession(eps, **g_args(2, nsteps=50)) as s:          # the stand-in as the engine
        s.engine._bloch = (np.ones(2), np.zeros(2))
        with pytest.raises(fd.Fdtd2dError, match="adjoint gradients are not available"):
            s.value_and_grad(g_objective)
