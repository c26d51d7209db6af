"""CPU-only checks of the line sources on Bloch flux lines and of the adjoint gradients of flux under a Bloch phase
(fdtd2d_batch_bloch_flux_adjoint.h, adjoint.py), on the stand-in of tests/oracle_batch_bloch_flux_adjoint.py.

The surface: the entry points are declared, exported and bound, bad arguments are refused before any device is touched,
the handle is checked and the package does not import the stand-in.

phi = 0.  A Bloch stand-in run with phi = 0 and real weights has a real part bit-identical to
oracle_batch_flux_adjoint's periodic run of the same member, lines (a column line at column 0 and crossing lines among
them), weights and channels, in float32 and float64, and an imaginary part that is exactly zero: the new definition is
anchored to one that is already pinned to the hardware.

The transpose identity, float64, 40x17, phi = 1.3, an 8-cell layer, random eps, the lines ("row", 20, 0, 16) and
("col", 0, 10, 20), 160 steps, two frequencies.  With S the one-step operator, S^T = W S_c W^-1 where S_c steps with the
conjugated rotation and W = diag(1 / ch on H, -1 / ce on E), ch = dt / (mu dx), ce = dt / (eps dx); an E source of step n
is read from step n on and an H source (added before the H update) a step later.  So with the source time functions
f_E(n) = exp(-i w (N + 1 - n) dt) and f_H(n) = exp(-i w (N + 2 - n) dt), f_H(1) = 0, as the 4F real channels of both
runs (the time reversal the adjoint uses: the monitor phasor of step n is the source amplitude of step N + 1 - n),
    <y_E, E(x)> + <y_H, H(x)>  =  <x_E, -E_c(a) / ce> + <x_H, H_c(a) / ch>,    a_E = -ce y_E,  a_H = ch y_H,
where E(x), H(x) are the lines' raw sums of the run that x drives and E_c, H_c those of the conjugated run that a drives,
all pairings plain (nothing conjugated).  Measured: the two sides agree to 1.4e-16 of their size; the bound is 1e-13
(160 steps of float64 rounding on sums of 72 terms).  With the seam rotation dropped in both runs they differ by 2.3 times
their size, sixteen orders of magnitude more.

The gradients: ``batch_bloch_flux_gradient`` on the stand-in against central finite differences of the stand-in's own
flux() and flux_orders() (oracle_batch_bloch_flux.BlochFluxOracle: no adjoint code on that side), on the configuration
tests/test_batch_bloch_adjoint_cpu.py documents as ringing down: 64x17, an 8-cell layer, float64, 5000 steps, dt 4e-13, dx
2.5e-4, a Ricker of 40 GHz on (14, 0, 1, 16) with ramp weights, design (24, 0, 12, 16), 25 / 40 / 55 GHz, phi = 2.4 and
3.0, its 8 design cells; the probe row is replaced by the lines ("row", 50, 0, 16) and ("row", 10, 0, 16), and sigma is
zero on rows 10 and 50.  Three objectives: sum_k P_k on the far line; sum_k w_k P_k^2 / 0.01 over both lines, w = (1, -2,
0.5); the power into the diffraction order m = -1 of the far line, summed over the frequencies.  Measured worst error
over the two members / max|gradient| (eps, sigma): sum 4.9e-7, 7.3e-8; quadratic 4.4e-7, 3.3e-7; order 1.3e-7, 1.7e-7
(residuals 3e-8 forward, 2e-5 to 2e-4 adjoint) -- the range of the probe gradients of these phases (2e-7).  The bounds
are three times these.  With the magnetic part of the adjoint sources missing the error of the first objective is
0.56 to 0.74 (eps) and 0.92 to 1.03 (sigma) of max|gradient|, with its sign wrong 1.6 to 2.5 and 62 to 73: five orders and
more above the bounds.

The weights: the stand-in's restatement of the device kernel against ``bloch_flux_adjoint_weights`` to 1e-12 of
max|weight|, and the orders' cotangent = 1 against the plain cotangent = 1 on that line to 1e-12 (Parseval).

The oblique one-way source: a periodic vacuum member 64x9, Courant 0.48, phi = 0.9, an electric and a magnetic sheet on
the whole-period line of row 32 with the ramp weights exp(1j * phi * j / Q); s_h(t) = alpha s_e(t - dt / 2) with
alpha = sin(theta / 2) / (ce sin(ky / 2) cos(ky / 2)), theta = omega dt, sin^2(ky / 2) = sin^2(theta / 2) / Courant^2 -
sin^2(phi / (2 Q)): the discrete plane-wave relation between Ez and the averaged Hx at the Bloch phase.  Power 10 rows
behind over power 10 rows ahead at the carrier, measured 7.7e-8, 1.3e-8, 3.7e-9 (25, 40, 55 GHz; what is left is the
envelope, as at normal incidence); the bound is three times the largest, 2.3e-7.  The electric sheet alone gives 1.0001,
0.9997, 0.9998: 1 to three digits."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch_bloch_flux import BlochFluxOracle
from oracle_batch_bloch_flux_adjoint import BlochLineSourceOracle
from oracle_batch_flux_adjoint import line_source_oracle_for
from test_batch_bloch_adjoint_cpu import (A_C, A_CELLS, A_DESIGN, A_DT, A_DX, A_FC, A_L, A_NSTEPS, A_OMEGAS, A_PHI, A_R,
                                          A_SOURCE, C0, EPS0, MU0, a_materials, at_cells)
from test_batch_periodic_cpu import H_EPS, H_SIGMA, ricker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_bloch_flux_adjoint.h")
NAMES = ["fdtd2d_batch_bloch_flux_line_weights", "fdtd2d_batch_read_bloch_flux_line_sources",
         "fdtd2d_batch_set_bloch_flux_line_sources"]
DX, DT = 1e-3, 1.6e-12

F_LINES = [("row", 50, 0, 16), ("row", 10, 0, 16)]
M1 = A_C - 2                          # the order m = -1 in np.fft.fftfreq order
FD_BOUND = {("sum", "eps"): 1.5e-6, ("sum", "sigma"): 2.2e-7, ("quadratic", "eps"): 1.3e-6, ("quadratic", "sigma"): 1.0e-6,
            ("order", "eps"): 4.0e-7, ("order", "sigma"): 5.3e-7}
TRANSPOSE_BOUND = 1e-13
ONE_WAY_BOUND = 2.3e-7


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_bloch_flux_adjoint_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt))) == NAMES
    assert sorted(_abi.BATCH_BLOCH_FLUX_ADJOINT_SIGNATURES) == NAMES
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} declared but not exported"
    loaded = _abi.load()
    for n in NAMES:
        assert getattr(loaded, n).argtypes == _abi.BATCH_BLOCH_FLUX_ADJOINT_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_BLOCH_FLUX_ADJOINT_SIGNATURES[n][0]


def test_the_header_adds_no_id_and_states_the_transpose_argument():
    from fdtd2d_amd import _abi
    txt = open(HEADER).read()
    assert not re.findall(r"#define\s+FDTD2D_BATCH_(?:INFO|OPT)_\w+", txt) and "enum" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    taken = [v for k, v in vars(_abi).items() if k.startswith("BATCH_INFO_") and isinstance(v, int)]
    assert max(taken) == 22 and _abi.BATCH_FLUX_LINE_SOURCES_INFO == 23
    assert "transpose" in txt and "conj(rho)" in txt and "FDTD2D_BATCH_INFO_FLUX_LINE_SOURCES" in txt


def test_bloch_flux_adjoint_python_surface(fd):
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_bloch_flux_line_sources).parameters) == ["self", "we", "wh"]
    assert list(inspect.signature(E.read_bloch_flux_line_sources).parameters) == ["self"]
    assert list(inspect.signature(E.bloch_flux_adjoint_sources).parameters) == ["self", "dJdP", "solve", "scale_e", "scale_h"]
    p = inspect.signature(fd.batch_bloch_flux_gradient).parameters
    assert list(p)[:3] == ["eps", "sigma", "mu"]
    for k in ("bloch_phase", "source_weights", "nsteps", "sources", "flux_lines", "omegas", "design", "objective",
              "orders_line", "fc", "waveform", "dt", "dx", "dtype", "pml_cells", "device", "engine"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    S = fd.BlochFluxAdjointSession
    assert issubclass(S, fd.BlochAdjointSession) and issubclass(S, fd.FluxAdjointSession)
    for name in ("value_and_grad", "set_design_eps", "set_design_sigma", "set_conductivity", "sigma_gradient",
                 "set_bloch_phase"):
        assert callable(getattr(S, name)), name
    for name in ("batch_bloch_flux_gradient", "BlochFluxAdjointSession", "bloch_flux_adjoint_weights"):
        assert name in fd.__all__ and hasattr(fd, name)
    for name in ("set_bloch_flux_lines", "set_bloch_flux_line_sources", "read_bloch_flux_line_sources",
                 "bloch_flux_adjoint_sources", "flux", "flux_orders", "read_flux_lines", "run", "run_bloch_channels", "reset",
                 "hold_bloch_window", "bloch_window_product"):
        assert callable(getattr(E, name)) and callable(getattr(BlochLineSourceOracle, name)), name


def test_the_package_does_not_import_the_stand_in():
    for name in ("adjoint.py", "batch.py", "__init__.py"):
        src = open(os.path.join(ROOT, "fdtd-2d_amd", name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), name


def test_bloch_flux_adjoint_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    dp = np.zeros(16).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.fdtd2d_batch_set_bloch_flux_line_sources(None, 1, dp, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_bloch_flux_line_sources(None, dp, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_bloch_flux_line_weights(None, dp, dp, 0, None, None) == _abi.E_ARG


def test_engine_methods_refuse_bad_arguments_before_the_library(fd):
    from test_batch_bloch_cpu import host_engine
    eng = host_engine(fd)
    eng._flux, eng._bflux = None, False
    for call in (lambda: eng.set_bloch_flux_line_sources(np.ones((4, 2)), None),
                 lambda: eng.read_bloch_flux_line_sources(),
                 lambda: eng.bloch_flux_adjoint_sources(np.ones((3, 1, 1)), np.eye(2))):
        with pytest.raises(fd.Fdtd2dError, match="Bloch flux lines") as ei:
            call()
        assert ei.value.code == fd._abi.E_STATE
    eng._flux, eng._bflux = (np.array([[0, 5, 0, 4]], np.int32), np.full((3, 2), 1e11)), True
    with pytest.raises(ValueError, match=r"we must have shape \(4, K\)"):
        eng.set_bloch_flux_line_sources(np.ones((5, 2)), None)
    with pytest.raises(ValueError, match="same number of channels"):
        eng.set_bloch_flux_line_sources(np.ones((4, 2)), np.ones((4, 3)) * 1j)
    with pytest.raises(ValueError, match="1..32 channels"):
        eng.set_bloch_flux_line_sources(np.ones((4, 33)), None)
    with pytest.raises(ValueError, match=r"dJdP must have shape \(3, 1, 2\)"):
        eng.bloch_flux_adjoint_sources(np.ones((3, 1, 1)), np.eye(4))
    with pytest.raises(ValueError, match="solve must have shape"):
        eng.bloch_flux_adjoint_sources(np.ones((3, 1, 2)), np.eye(2))
    with pytest.raises(ValueError, match=r"scale_h must have shape \(3, 4\)"):
        eng.bloch_flux_adjoint_sources(np.ones((3, 1, 2)), np.eye(4), None, np.ones((3, 5)))


def test_the_stand_in_refuses_what_the_library_refuses():
    ref = BlochLineSourceOracle(1, 40, 17, DT, DX, dtype=np.float64, boundary="periodic")
    ref.set_materials(np.full((1, 40, 17), EPS0), MU0).set_pml(8, courant00=0.48)
    ref.set_bloch_phase(0.7).set_dft_window((15, 2, 4, 4), [2e11])
    with pytest.raises(AssertionError):
        ref.set_bloch_flux_line_sources(np.ones((16, 2)), None)         # without lines
    ref.set_bloch_flux_lines([("row", 20, 0, 16)], [2e11])
    for call in (lambda: ref.run_bloch_channels(4, None, np.zeros((2, 4))), lambda: ref.hold_bloch_window()):
        with pytest.raises(AssertionError):
            call()                                                      # lines without sources keep refusing
    with pytest.raises(AssertionError):
        ref.set_bloch_flux_line_sources(np.ones((16, 33)), None)        # K > 32
    with pytest.raises(AssertionError):
        ref.set_bloch_flux_line_sources(np.ones((15, 2)), None)         # the wrong number of entries
    with pytest.raises(AssertionError):
        ref.set_flux_line_sources(np.ones((16, 2)), None)               # the real entry
    ref.set_bloch_flux_line_sources(np.zeros((16, 2)), None)            # all-zero weights count
    ref.run_bloch_channels(4, None, np.zeros((2, 4)), conjugate=True).hold_bloch_window()
    with pytest.raises(AssertionError):
        ref.set_bloch_point_sources(np.array([[20, 3]]), np.ones((1, 2)))   # always, while the lines are set
    with pytest.raises(AssertionError):
        ref.set_bloch_flux_lines([("row", 21, 0, 16)], [2e11])          # a held window excludes new lines
    ref.set_dft_window((15, 2, 4, 4), [2e11])
    ref.set_bloch_flux_lines([("row", 21, 0, 16)], [2e11])              # new lines drop the sources
    assert ref.blinesrc is None


# ---- 2. phi = 0 against the real line sources -----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_phase_with_real_weights_is_the_periodic_stand_in(dtype):
    R, C, n, K = 40, 17, 120, 3
    lines = [("row", 20, 0, 16), ("col", 0, 0, 40), ("col", 15, 5, 20), ("row", 3, 2, 9)]
    rng = np.random.default_rng(0)
    eps = EPS0 * (1 + rng.random((1, R, C)))
    eps[:, :, -1] = eps[:, :, 0]
    cells = sum(l[3] for l in lines)
    we, wh = 0.3 * rng.standard_normal((cells, K)), 1e-3 * rng.standard_normal((cells, K))
    chan, amps = rng.standard_normal((K, n)), rng.standard_normal((1, n))
    om = 2 * np.pi * np.array([25e9, 40e9])
    a = BlochLineSourceOracle(1, R, C, DT, DX, dtype=dtype, boundary="periodic")
    b = line_source_oracle_for("periodic")(1, R, C, DT, DX, dtype=dtype, boundary="periodic")
    for e in (a, b):
        e.set_materials(eps, MU0).set_pml(8, courant00=0.48)
        e.set_sources(np.array([[14, 3, 1, 8]]))
    a.set_bloch_phase(0.0)
    a.set_bloch_flux_lines(lines, om).set_bloch_flux_line_sources(we, wh)
    a.run_bloch_channels(n, amps, chan)
    b.set_flux_lines(lines, om).set_flux_line_sources(we, wh)
    b.run(n, amps, chan)
    for x, y in zip(a.download(), b.download()):
        assert x.real.dtype == y.dtype and np.array_equal(x.real, y) and not np.any(x.imag) and np.abs(y).max() > 0
    for x, y in zip(a.read_flux_lines(raw=True), b.read_flux_lines(raw=True)):
        assert np.array_equal(x, y) and np.abs(y).max() > 0
    assert np.allclose(a.flux(), b.flux(), rtol=1e-12, atol=0)


# ---- 3. the transpose identity ----------------------------------------------------------------------------------------

def _transpose_sides(drop_seam_rotation):
    R, C, N, F = 40, 17, 160, 2
    lines = [("row", 20, 0, 16), ("col", 0, 10, 20)]
    om = 2 * np.pi * np.array([25e9, 55e9])
    rng = np.random.default_rng(0)
    eps = EPS0 * (1 + rng.random((1, R, C)))
    eps[:, :, -1] = eps[:, :, 0]
    li, lj = np.r_[np.full(16, 20), np.arange(10, 30)], np.r_[np.arange(16), np.zeros(20, int)]
    cells = len(li)
    ce, ch = (DT / (eps[0, li, lj] * DX))[:, None], DT / (MU0 * DX)
    n = np.arange(1, N + 1)
    fE = np.exp(-1j * om[:, None] * (N + 1 - n)[None, :] * DT)
    fH = np.exp(-1j * om[:, None] * (N + 2 - n)[None, :] * DT)
    fH[:, 0] = 0
    chan = np.concatenate([fE.real, fE.imag, fH.real, fH.imag])       # 4F real channels

    def run(zE, zH, conjugate):
        we, wh = np.zeros((cells, 4 * F), complex), np.zeros((cells, 4 * F), complex)
        we[:, :F], we[:, F:2 * F] = zE, 1j * zE                       # z f = z Re f + (i z) Im f
        wh[:, 2 * F:3 * F], wh[:, 3 * F:] = zH, 1j * zH
        a = BlochLineSourceOracle(1, R, C, DT, DX, dtype=np.float64, boundary="periodic")
        a.drop_seam_rotation = drop_seam_rotation
        a.set_materials(eps, MU0).set_pml(8, courant00=0.48)
        a.set_bloch_phase(1.3)
        a.set_bloch_flux_lines(lines, om).set_bloch_flux_line_sources(we, wh)
        a.run_bloch_channels(N, None, chan, conjugate=conjugate)
        E, H = a.read_flux_lines(raw=True)
        return E[0].T, H[0].T                                         # (cells, F)

    def cx():
        return rng.standard_normal((cells, F)) + 1j * rng.standard_normal((cells, F))
    xE, xH, yE, yH = cx(), 1e-3 * cx(), cx(), 1e3 * cx()
    E, H = run(xE, xH, False)
    lhs = (yE * E).sum() + (yH * H).sum()
    Ec, Hc = run(-ce * yE, ch * yH, True)
    rhs = (xE * (-1 / ce) * Ec).sum() + (xH * (1 / ch) * Hc).sum()
    return lhs, rhs


def test_the_conjugated_run_is_the_transpose_and_the_seam_rotation_is_what_makes_it_so():
    lhs, rhs = _transpose_sides(False)
    good = abs(lhs - rhs) / abs(lhs)
    lhs, rhs = _transpose_sides(True)
    bad = abs(lhs - rhs) / abs(lhs)
    print(f"transpose identity: |lhs - rhs| / |lhs| = {good:.2e}; with the seam rotation dropped {bad:.2e}")
    assert good <= TRANSPOSE_BOUND and bad > 1e-3


# ---- 4. the gradients against finite differences -------------------------------------------------------------------------

def f_materials():
    eps, sigma = a_materials()
    sigma[:, 10, :] = 0                   # the line rows carry no conductivity
    assert not np.any(sigma[:, 50, :])
    return eps, sigma


def o_sum(P):
    g = np.zeros_like(P)
    g[:, 0, :] = 1
    return P[:, 0, :].sum(axis=1), g


def o_quadratic(P):
    w = np.array([1.0, -2.0, 0.5])[None, None, :]
    return (w * P * P).sum(axis=(1, 2)) / 0.01, 2 * w * P / 0.01


def o_order(P, Pm):
    g = np.zeros_like(Pm)
    g[:, :, M1] = 1
    return Pm[:, :, M1].sum(axis=1), np.zeros_like(P), g


OBJECTIVES = {"sum": (o_sum, {}), "quadratic": (o_quadratic, {}), "order": (o_order, dict(orders_line=0))}


def f_args(count=2, engine=BlochLineSourceOracle, nsteps=A_NSTEPS, **kw):
    args = dict(bloch_phase=np.resize(A_PHI, count), source_weights="ramp", nsteps=nsteps,
                sources=np.tile(A_SOURCE, (count, 1)), flux_lines=F_LINES, omegas=A_OMEGAS, design=A_DESIGN, fc=A_FC,
                dt=A_DT, dx=A_DX, dtype=np.float64, pml_cells=A_L, engine=engine)
    args.update(kw)
    return args


def forward(eps, sigma, phi, nsteps=A_NSTEPS):
    """(flux(), flux_orders(0)) from a forward run of the Bloch flux stand-in alone: no adjoint code involved."""
    B = eps.shape[0]
    eng = BlochFluxOracle(B, A_R, A_C, A_DT, A_DX, dtype=np.float64)
    eng.set_materials(eps, MU0).set_pml(A_L, courant00=C0 * A_DT / A_DX)
    eng.set_conductivity(sigma)
    eng.set_sources(np.tile(A_SOURCE, (B, 1)))
    eng.set_bloch_phase(phi).set_bloch_source("ramp")
    eng.set_bloch_flux_lines(F_LINES, A_OMEGAS)
    eng.run(nsteps, np.tile(ricker(nsteps, A_DT, A_FC), (B, 1)))
    return eng.flux(), eng.flux_orders(0)


@pytest.fixture(scope="module")
def perturbed():
    """flux() and the orders of both members with each of the 8 cells' eps, then sigma, moved up and down."""
    eps0, sigma0 = f_materials()
    n, out = len(A_CELLS), []
    for b in range(2):
        eps, sigma = np.repeat(eps0[b:b + 1], 4 * n, axis=0), np.repeat(sigma0[b:b + 1], 4 * n, axis=0)
        for k, (r, c) in enumerate(A_CELLS):
            cols = [c, A_C - 1] if c == 0 else [c]          # column 0 and its image move together
            eps[4 * k, r, cols] += H_EPS
            eps[4 * k + 1, r, cols] -= H_EPS
            sigma[4 * k + 2, r, cols] += H_SIGMA
            sigma[4 * k + 3, r, cols] -= H_SIGMA
        out.append(forward(eps, sigma, np.full(4 * n, A_PHI[b])))
    return out


@pytest.mark.parametrize("name", list(OBJECTIVES))
def test_bloch_flux_gradients_match_finite_differences_of_the_stand_in(fd, perturbed, name):
    objective, kw = OBJECTIVES[name]
    eps, sigma = f_materials()
    J, grad, grad_sigma, P, info = fd.batch_bloch_flux_gradient(eps, sigma, objective=objective, **f_args(), **kw)
    assert grad.shape == grad_sigma.shape == (2,) + A_DESIGN[2:] and P.shape == (2, 2, 3) and info["condition"] < 10
    worst = {"eps": 0.0, "sigma": 0.0}
    for b in range(2):
        Jp = objective(*perturbed[b][:2 if kw else 1])[0]
        for what, g, d in (("eps", grad, (Jp[0::4] - Jp[1::4]) / (2 * H_EPS)),
                           ("sigma", grad_sigma, (Jp[2::4] - Jp[3::4]) / (2 * H_SIGMA))):
            worst[what] = max(worst[what], np.abs(at_cells(g, b) - d).max() / np.abs(g[b]).max())
    print(f"{name}: adjoint vs central FD on 8 cells of 2 members, worst / max|gradient|: eps {worst['eps']:.3e}, "
          f"sigma {worst['sigma']:.3e}; residuals {info['residual_forward']} {info['residual_adjoint']}")
    for what in worst:
        assert worst[what] <= FD_BOUND[name, what] < 1e-5


# ---- 5. the weights -----------------------------------------------------------------------------------------------------

def _short_run(B=2, n=300):
    rng = np.random.default_rng(4)
    lines = [("row", 20, 0, 16), ("col", 0, 15, 10), ("row", 25, 10, 4)]        # the first two cross: a cell twice
    om = 2 * np.pi * np.array([[25e9, 40e9, 55e9], [30e9, 45e9, 60e9]])
    ref = BlochLineSourceOracle(B, 40, 17, DT, DX, dtype=np.float64, boundary="periodic")
    eps = EPS0 * (1 + rng.random((B, 40, 17)))
    eps[:, :, -1] = eps[:, :, 0]
    ref.set_materials(eps, MU0).set_pml(8, courant00=0.48)
    ref.set_sources(np.array([[14, 3, 1, 8], [15, 5, 2, 2]]))
    ref.set_bloch_phase(np.array([0.9, -2.2])).set_bloch_source("ramp").set_bloch_flux_lines(lines, om)
    ref.run(n, np.stack([ricker(n, DT, 40e9 * (1 + 0.2 * m)) for m in range(B)]))
    return ref, lines, om, rng


def test_device_weights_as_restated_equal_the_host_path(fd):
    ref, lines, om, rng = _short_run()
    E, H = ref.read_flux_lines(raw=True)
    B, _, cells = E.shape
    assert np.abs(E.imag).max() > 0
    dJdP, solve = rng.standard_normal((B, 3, 3)), rng.standard_normal((B, 6, 6))
    se, sh = 1 + rng.random((B, cells)), -(1 + rng.random((B, cells)))
    for scales in ((se, sh), (None, None)):
        for s in (solve, solve[0]):
            ref.bloch_flux_adjoint_sources(dJdP, s, *scales)
            got = ref.read_bloch_flux_line_sources()
            want = fd.bloch_flux_adjoint_weights(E, H, dJdP, lines, om, DT, DX, s, *scales)
            for g, w in zip(got, want):
                assert g.shape == w.shape == (B, cells, 6) and np.abs(w).max() > 0 and not np.any(g.imag)
                assert np.abs(g.real - w).max() <= 1e-12 * np.abs(w).max()


def test_a_unit_cotangent_on_the_orders_is_a_unit_cotangent_on_the_line(fd):
    ref, lines, om, rng = _short_run()
    E, H = ref.read_flux_lines(raw=True)
    B, _, cells = E.shape
    solve = rng.standard_normal((B, 6, 6))
    on_line = np.zeros((B, 3, 3))
    on_line[:, 0, :] = 1
    plain = fd.bloch_flux_adjoint_weights(E, H, on_line, lines, om, DT, DX, solve)
    orders = fd.bloch_flux_adjoint_weights(E, H, np.zeros((B, 3, 3)), lines, om, DT, DX, solve,
                                           orders=(0, np.ones((B, 3, 16)), ref.phi))
    for a, b in zip(orders, plain):
        assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
        assert not np.any(a[:, 16:])                         # nothing off the line
    # and the orders sum to the line's flux
    assert np.allclose(ref.flux_orders(0).sum(axis=2), ref.flux()[:, 0, :], rtol=1e-10, atol=0)


# ---- 6. the session -----------------------------------------------------------------------------------------------------

def _guarded(name, allow):
    def call(self, *a, **k):
        if not allow and not self._inside:
            raise AssertionError(f"a bulk read-back: {name}")
        self._inside += 1
        try:
            return getattr(BlochLineSourceOracle, name)(self, *a, **k)
        finally:
            self._inside -= 1
    return call


class NoBulkReads(BlochLineSourceOracle):
    """The stand-in without the calls a session on P must not make (flux() and the weights read the sums where the
    device keeps them: inside those two calls the stand-in may)."""
    _inside = 0
    read_probes, download, read_dft_window = (_guarded(n, False) for n in ("read_probes", "download", "read_dft_window"))
    read_flux_lines, read_bloch_flux_parts = (_guarded(n, False) for n in ("read_flux_lines", "read_bloch_flux_parts"))
    flux, bloch_flux_adjoint_sources = (_guarded(n, True) for n in ("flux", "bloch_flux_adjoint_sources"))


def test_the_session_is_the_helper(fd):
    n = 300
    eps, sigma = f_materials()
    want = fd.batch_bloch_flux_gradient(eps, sigma, objective=o_quadratic, **f_args(nsteps=n))
    with fd.BlochFluxAdjointSession(eps, sigma, **f_args(nsteps=n, engine=NoBulkReads)) as s:
        J, grad, P, info = s.value_and_grad(o_quadratic)
        gs = s.sigma_gradient()
        assert np.array_equal(P, want[3]) and np.allclose(J, want[0], rtol=1e-12, atol=0)
        for a, w in ((grad, want[1]), (gs, want[2])):
            assert np.abs(a - w).max() <= 1e-12 * np.abs(w).max()
        assert sorted(info) == sorted(want[4])
        # a new design and new phases: an iteration is a fresh helper call
        r0, c0, nr, nc = A_DESIGN
        new = eps[:, r0:r0 + nr, c0:c0 + nc] * 1.1
        phi = np.array([1.9, -0.6])
        s.set_design_eps(new).set_bloch_phase(phi)
        with pytest.raises(RuntimeError, match="no gradient yet"):
            s.sigma_gradient()
        J2, grad2, P2, _ = s.value_and_grad(o_quadratic)
        eps2 = eps.copy()
        eps2[:, r0:r0 + nr, c0:c0 + nc] = new
        eps2[:, :, -1] = eps2[:, :, 0]
        fresh = fd.batch_bloch_flux_gradient(eps2, sigma, objective=o_quadratic, **f_args(nsteps=n, bloch_phase=phi))
        assert np.allclose(P2, fresh[3], rtol=1e-12, atol=0) and not np.allclose(P2, P, rtol=1e-3)
        assert np.abs(grad2 - fresh[1]).max() <= 1e-12 * np.abs(fresh[1]).max()
        assert np.abs(s.sigma_gradient() - fresh[2]).max() <= 1e-12 * np.abs(fresh[2]).max()
        with pytest.raises(ValueError, match="sigma is non-zero at a flux line cell"):
            s.set_conductivity(_sigma_on_the_line())
    # with the orders the session reads the line spectra back and takes the host path
    want = fd.batch_bloch_flux_gradient(eps, sigma, objective=o_order, orders_line=0, **f_args(nsteps=n))
    with fd.BlochFluxAdjointSession(eps, sigma, orders_line=0, **f_args(nsteps=n)) as s:
        J, grad, P, _ = s.value_and_grad(o_order)
        assert np.allclose(J, want[0], rtol=1e-12, atol=0) and np.abs(grad - want[1]).max() <= 1e-12 * np.abs(want[1]).max()


# ---- 7. the oblique one-way source ---------------------------------------------------------------------------------------

def _sheet_run(pair):
    """(P ahead, P behind) at the carriers 25 / 40 / 55 GHz, one member each, phi = 0.9."""
    R, C, rs, d, n, phi = 64, 9, 32, 10, 3000, 0.9
    Q, om, fc = C - 1, 2 * np.pi * np.array([25e9, 40e9, 55e9]), 40e9
    t = np.arange(n) * DT
    env = np.exp(-((t - 4.5 / fc) / (0.9 / fc)) ** 2)
    chan = np.stack([np.stack([env * np.cos(w * t), env * np.sin(w * t)]) for w in om])
    courant = DT / (DX * np.sqrt(EPS0 * MU0))
    theta = om * DT
    ky = 2 * np.arcsin(np.sqrt(np.sin(theta / 2) ** 2 / courant ** 2 - np.sin(phi / (2 * Q)) ** 2))
    alpha = np.sin(theta / 2) / ((DT / (EPS0 * DX)) * np.sin(ky / 2) * np.cos(ky / 2))
    ramp = np.exp(1j * phi * np.arange(Q) / Q)
    lines = [("row", rs, 0, Q), ("row", rs + d, 0, Q), ("row", rs - d, 0, Q)]
    we, wh = np.zeros((3, 3 * Q, 2), complex), np.zeros((3, 3 * Q, 2), complex)
    we[:, :Q, 0] = ramp[None, :]                                          # s_e = ramp env cos(omega t)
    wh[:, :Q, 0] = (alpha * np.cos(theta / 2))[:, None] * ramp[None, :]   # s_h = alpha ramp env cos(omega (t - dt/2))
    wh[:, :Q, 1] = (alpha * np.sin(theta / 2))[:, None] * ramp[None, :]
    eng = BlochLineSourceOracle(3, R, C, DT, DX, dtype=np.float64, boundary="periodic")
    eng.set_materials(np.full((3, R, C), EPS0), MU0).set_pml(8, courant00=courant)
    eng.set_bloch_phase(phi)
    eng.set_bloch_flux_lines(lines, om[:, None]).set_bloch_flux_line_sources(we, wh if pair else None)
    eng.run_bloch_channels(n, None, chan)
    P = eng.flux()[:, :, 0]
    return P[:, 1], P[:, 2]


def test_an_electric_and_a_magnetic_sheet_with_the_ramp_radiate_one_way_at_an_angle():
    ahead, behind = _sheet_run(True)
    ahead_e, behind_e = _sheet_run(False)
    ratio, ratio_e = np.abs(behind) / ahead, np.abs(behind_e) / ahead_e
    print(f"oblique one-way ratios {ratio}, the electric sheet alone {ratio_e}; ahead {ahead} against {ahead_e}")
    assert np.all(ahead > 0) and np.all(ahead_e > 0) and np.all(behind_e < 0)
    assert np.all(ratio <= ONE_WAY_BOUND) and np.all(ratio < ratio_e)
    assert np.all(np.abs(ratio_e - 1) < 1e-3)               # alone it radiates both ways alike


# ---- 8. the host refusals -------------------------------------------------------------------------------------------------

class Poled(BlochLineSourceOracle):
    """An engine factory that sets the pole with the phase."""

    def set_bloch_phase(self, phi, rotation=None):
        super().set_bloch_phase(phi, rotation)
        return self.set_bloch_dispersion((2 * np.pi * 10e9) ** 2, 1e10, 0.0) if not self.dispersive else self


def _sigma_on_the_line():
    s = f_materials()[1]
    s[0, 50, 4] = 0.1
    return s


@pytest.mark.parametrize("change,match", [
    (dict(omegas=A_OMEGAS * np.array([1, -1, 1])), "omegas must be positive"),
    (dict(omegas=np.array([0.0, 1e11])), "omegas must be positive"),
    (dict(flux_lines=[("row", 5, 0, 16)]), r"cell \(5, 0\) lies in the 8-cell PML"),
    (dict(flux_lines=[("row", 23, 0, 16)]), "closer than 2 cells to the design window"),
    (dict(flux_lines=[("row", 36, 0, 16)]), "closer than 2 cells to the design window"),
    (dict(flux_lines=[("row", 15, 0, 16)]), "closer than 2 cells to the forward source"),
    (dict(sigma="on the line"), "sigma is non-zero at a flux line cell"),
    (dict(flux_lines=[("row", 50, 0, 16), ("row", 10, 2, 8)], orders_line=1), "orders_line 1 must be a row line over the whole"),
    (dict(flux_lines=[("row", 50, 0, 16), ("col", 3, 40, 8)], orders_line=1), "orders_line 1 must be a row line over the whole"),
    (dict(orders_line=2), "orders_line 2 outside"),
    (dict(bloch_phase=None), "bloch_phase is required"),
    (dict(source_weights="slope"), 'source_weights must be "ramp"'),
])
def test_the_helper_and_the_session_refuse_bad_arguments_on_the_host(monkeypatch, fd, change, match):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    eps, sigma = f_materials()
    kw = f_args(engine=None, nsteps=200)
    kw.update(change)
    if kw.pop("sigma", None) == "on the line":
        sigma = _sigma_on_the_line()
    elif "flux_lines" in change:
        sigma = None                      # the background conductivity covers the rows these lines move to
    with pytest.raises(ValueError, match=match):
        fd.batch_bloch_flux_gradient(eps, sigma, objective=o_sum, **kw)
    with pytest.raises(ValueError, match=match):
        fd.BlochFluxAdjointSession(eps, sigma, **kw)


def test_an_engine_with_the_pole_is_refused(fd):
    eps, sigma = f_materials()
    with pytest.raises(ValueError, match="dispersive pole"):
        fd.batch_bloch_flux_gradient(eps, sigma, objective=o_sum, **f_args(engine=Poled, nsteps=50))
    with fd.BlochFluxAdjointSession(eps, sigma, **f_args(engine=Poled, nsteps=50)) as s:
        with pytest.raises(ValueError, match="dispersive pole"):
            s.value_and_grad(o_sum)


def test_objective_shapes_are_checked(fd):
    eps, sigma = f_materials()
    with pytest.raises(ValueError, match="dJ/dP of shape"):
        fd.batch_bloch_flux_gradient(eps, sigma, objective=lambda P: (P.sum(axis=(1, 2)), np.ones((2, 3))),
                                     **f_args(nsteps=50))
    with pytest.raises(ValueError, match="dJ/dPm of shape"):
        fd.batch_bloch_flux_gradient(eps, sigma, orders_line=0, **f_args(nsteps=50),
                                     objective=lambda P, Pm: (P.sum(axis=(1, 2)), np.ones_like(P), np.ones((2, 3))))
