"""CPU-only checks of the adjoint gradients of Bloch batches (fdtd2d_batch_bloch_adjoint.h, adjoint.py): the surface, the
helper and the session on the stand-in (tests/oracle_batch_bloch_adjoint.py) and the host refusals.

The finite-difference configuration is the one for which the stand-in is known to ring down: 64 x 17 members, an 8-cell
layer, float64, 5000 steps, dt 4e-13, dx 2.5e-4, a Ricker of 40 GHz on the rectangle (14, 0, 1, 16) with ramp weights,
the design window (24, 0, 12, 16) with eps_r in [1, 3] and sigma in [0.2, 0.7] S/m, 0.1 S/m on the other rows 8..55 except
the probe row 50, 6 probes on row 50 (columns 0 and C-2 among them: column 0's point cell is the one the library lists a
second time at its image), the frequencies 25 / 40 / 55 GHz, and two members with phi = 2.4 and 3.0.
``tests/test_gpu_batch_bloch_adjoint.py`` runs the device against the same stand-in."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle_batch_bloch import BlochOracle
from oracle_batch_bloch_adjoint import BlochAdjointOracle
from oracle_batch_periodic import PeriodicOracle
from test_batch_bloch_cpu import host_engine
from test_batch_periodic_cpu import G_BOUND, H_EPS, H_SIGMA, g_args, g_materials, g_objective, ricker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_bloch_adjoint.h")
NAMES = ["fdtd2d_batch_bloch_field_absmax", "fdtd2d_batch_bloch_probe_spectra", "fdtd2d_batch_bloch_window_product",
         "fdtd2d_batch_hold_bloch_window", "fdtd2d_batch_run_bloch_channels", "fdtd2d_batch_set_bloch_point_sources"]
METHODS = ["set_bloch_point_sources", "run_bloch_channels", "hold_bloch_window", "bloch_window_product",
           "bloch_probe_spectra", "bloch_field_absmax"]
EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7
C0 = 1 / np.sqrt(EPS0 * MU0)

A_R, A_C, A_L, A_DT, A_DX, A_FC, A_NSTEPS = 64, 17, 8, 4e-13, 2.5e-4, 40e9, 5000
A_DESIGN = (24, 0, 12, 16)
A_SOURCE = (14, 0, 1, 16)
A_PROBES = np.array([(50, c) for c in (0, 3, 6, 9, 12, 15)])
A_OMEGAS = 2 * np.pi * np.array([25e9, 40e9, 55e9])
A_PHI = np.array([2.4, 3.0])
A_CELLS = [(24, 0), (35, 15), (24, 15), (35, 0), (28, 7), (30, 3), (26, 12), (33, 9)]


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def a_materials(count=2, seed=3):
    """g_materials plus the background conductivity: 0.1 S/m on the other rows 8..55 except the probe row."""
    eps, sigma = g_materials(count, seed)
    r0, _, nr, _ = A_DESIGN
    rows = [i for i in range(A_L, A_R - A_L) if not r0 <= i < r0 + nr and i != 50]
    sigma[:, rows, :] = 0.1
    return eps, sigma


def a_args(count=2, engine=BlochAdjointOracle, nsteps=A_NSTEPS, dtype=np.float64, **kw):
    args = dict(bloch_phase=np.resize(A_PHI, count), source_weights="ramp", nsteps=nsteps,
                sources=np.tile(A_SOURCE, (count, 1)), probes=A_PROBES, omegas=A_OMEGAS, design=A_DESIGN, fc=A_FC,
                dt=A_DT, dx=A_DX, dtype=dtype, pml_cells=A_L, engine=engine)
    args.update(kw)
    return args


def a_gradient(fd, eps=None, sigma=None, **kw):
    e, s = a_materials()
    eps, sigma = e if eps is None else eps, s if sigma is None else sigma
    return fd.batch_bloch_gradient(eps, sigma, objective=g_objective, **a_args(eps.shape[0], **kw))


def a_forward_objective(eps, sigma, phi):
    """J of every member from a forward run of BlochOracle alone (no adjoint code, no point sources involved)."""
    from fdtd2d_amd.adjoint import probe_spectra
    B = eps.shape[0]
    eng = BlochOracle(B, A_R, A_C, A_DT, A_DX, dtype=np.float64)
    eng.set_materials(eps, MU0).set_pml(A_L, courant00=C0 * A_DT / A_DX)
    eng.set_conductivity(sigma)
    eng.set_sources(np.tile(A_SOURCE, (B, 1))).set_probes(A_PROBES, A_NSTEPS)
    eng.set_bloch_phase(phi).set_bloch_source("ramp")
    eng.run(A_NSTEPS, np.tile(ricker(A_NSTEPS, A_DT, A_FC), (B, 1)))
    tr = eng.read_probes()
    om = np.tile(A_OMEGAS, (B, 1))
    return g_objective(probe_spectra(tr.real, om, A_DT) + 1j * probe_spectra(tr.imag, om, A_DT))[0]


@pytest.fixture(scope="module")
def differences():
    """Central finite differences of the forward-only objective on A_CELLS of both members: (d_eps, d_sigma), (2, 8)."""
    eps0, sigma0 = a_materials()
    n = len(A_CELLS)
    out = np.empty((2, 2, n))
    for b in range(2):
        eps, sigma = np.repeat(eps0[b:b + 1], 4 * n, axis=0), np.repeat(sigma0[b:b + 1], 4 * n, axis=0)
        for k, (r, c) in enumerate(A_CELLS):
            cols = [c, A_C - 1] if c == 0 else [c]          # column 0 and its image move together
            eps[4 * k, r, cols] += H_EPS
            eps[4 * k + 1, r, cols] -= H_EPS
            sigma[4 * k + 2, r, cols] += H_SIGMA
            sigma[4 * k + 3, r, cols] -= H_SIGMA
        Jp = a_forward_objective(eps, sigma, np.full(4 * n, A_PHI[b]))
        out[0, b] = (Jp[0::4] - Jp[1::4]) / (2 * H_EPS)
        out[1, b] = (Jp[2::4] - Jp[3::4]) / (2 * H_SIGMA)
    return out


def at_cells(g, b):
    r0, c0 = A_DESIGN[:2]
    return np.array([g[b, r - r0, c - c0] for r, c in A_CELLS])


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_bloch_adjoint_symbols_are_declared_exported_and_bound(fd):
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_BLOCH_ADJOINT_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_BLOCH_ADJOINT_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_BLOCH_ADJOINT_SIGNATURES[n][0]
    # the argument lists of the header, type by type
    ctype = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "long long": ctypes.c_longlong,
             "const int *": ctypes.POINTER(ctypes.c_int), "const double *": ctypes.POINTER(ctypes.c_double),
             "double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in re.findall(r"int\s+(fdtd2d_[a-z0-9_]+)\s*\(([^)]*)\)", txt):
        got = [ctype[re.sub(r"\s*\w+$", "", " ".join(a.split())).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_BLOCH_ADJOINT_SIGNATURES[n][1], n
    for h in ("fdtd2d.h", "fdtd2d_batch_bloch.h"):           # companions: neither declares any of the new names
        other = open(os.path.join(ROOT, "include", h)).read()
        assert not any(re.search(rf"\b{n}\s*\(", other) for n in names), h
    for m in METHODS:
        assert callable(getattr(fd.BatchEngine, m))
    assert fd.batch_bloch_gradient is fd.adjoint.batch_bloch_gradient and "batch_bloch_gradient" in fd.__all__
    assert fd.BlochAdjointSession is fd.adjoint.BlochAdjointSession and "BlochAdjointSession" in fd.__all__
    assert issubclass(fd.BlochAdjointSession, fd.AdjointSession)


def test_bloch_adjoint_info_ids_are_named_here_alone():
    from fdtd2d_amd import _abi
    pat = r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)"
    mine = dict(re.findall(pat, open(HEADER).read()))
    assert mine == {"BATCH_INFO_BLOCH_POINT_SOURCES": "17", "BATCH_INFO_HELD_BLOCH_WINDOW": "18"}
    assert (_abi.BATCH_INFO_BLOCH_POINT_SOURCES, _abi.BATCH_INFO_HELD_BLOCH_WINDOW) == (17, 18)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != os.path.basename(HEADER):
            taken = dict(re.findall(pat, open(os.path.join(ROOT, "include", h)).read()))
            assert not {"17", "18"} & {v for k, v in taken.items() if k.startswith("BATCH_INFO")}, h
    lib = _abi.load()
    assert lib.fdtd2d_batch_info(None, 17) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_bloch_point_sources(None, 0, None, 0, None) == _abi.E_ARG
    assert lib.fdtd2d_batch_run_bloch_channels(None, 1, None, None, None, 0, 1) == _abi.E_ARG
    assert lib.fdtd2d_batch_hold_bloch_window(None) == _abi.E_ARG


def test_the_no_adjoint_sentences_are_gone():
    for path, gone in (("README.md", "No adjoint gradients of complex fields yet"),
                       ("include/fdtd2d_batch_bloch.h", "are not part of this interface yet"),
                       ("DESIGN.md", "Adjoint gradients of complex fields (Bloch batches)")):
        assert gone not in " ".join(open(os.path.join(ROOT, path)).read().split()), path


# ---- 2. the stand-in alone ---------------------------------------------------------------------------------------------

def small_engine(engine, dtype=np.float64, phi=(0.9, 2.2), conj_points=True, **kw):
    """Two 30 x 13 members with a 5-cell layer, a conductivity, a window, probes and three point cells (one in column 0)."""
    rng = np.random.default_rng(8)
    eps = EPS0 * (1 + 2 * rng.random((2, 30, 13)))
    eps[:, :, -1] = eps[:, :, 0]
    sigma = np.zeros((2, 30, 13))
    sigma[:, 8:22, :] = 0.5 * rng.random((2, 14, 13))
    eng = engine(2, 30, 13, A_DT, A_DX, dtype=dtype, boundary="periodic", **kw)
    eng.set_materials(eps, MU0).set_pml(5, courant00=C0 * A_DT / A_DX)
    eng.set_conductivity(sigma)
    eng.set_sources(np.array([(9, 2, 1, 5), (9, 0, 1, 12)]))
    eng.set_bloch_phase(np.array(phi)).set_bloch_source("ramp")
    eng.set_dft_window((10, 0, 6, 12), A_OMEGAS).set_probes(np.array([(20, 0), (20, 11), (12, 4)]), 120)
    return eng


def test_silent_points_leave_the_run_unchanged_and_conjugate_is_minus_phi():
    """Zero weights, conjugate False: BlochOracle's own run, bit for bit.  conjugate True: the member at -phi."""
    amps = np.tile(ricker(60, A_DT, A_FC), (2, 1)) * (1 + 0.5j)
    chan = np.random.default_rng(1).standard_normal((3, 60))
    cells = np.array([(15, 0), (15, 11), (8, 6)])
    plain = small_engine(BlochOracle).run(60, amps)
    silent = small_engine(BlochAdjointOracle).set_bloch_point_sources(cells, np.zeros((3, 3)))
    silent.run_bloch_channels(60, amps, chan)
    for a, b in zip(plain.download(), silent.download()):
        assert np.array_equal(a, b) and np.abs(a).max() > 0
    assert np.array_equal(plain.read_dft_window(), silent.read_dft_window())
    assert np.array_equal(plain.read_probes(), silent.read_probes())

    w = np.random.default_rng(2).standard_normal((2, 3, 3))
    conj = small_engine(BlochAdjointOracle).set_bloch_point_sources(cells, w)
    conj.run_bloch_channels(60, amps, chan, conjugate=True)
    c, s = np.cos(np.array([0.9, 2.2])), np.sin(np.array([0.9, 2.2]))
    minus = small_engine(BlochAdjointOracle)
    ramp = minus.weights.copy()
    minus.set_bloch_phase(None, rotation=(c, -s)).set_bloch_source(ramp).set_bloch_point_sources(cells, w)
    minus.run_bloch_channels(60, amps, chan)
    for a, b in zip(conj.download(), minus.download()):
        assert np.array_equal(a, b) and np.abs(a.imag).max() > 0
    assert np.array_equal(conj.read_probes(), minus.read_probes())
    # the real series reaches the imaginary part through the seam alone
    only = small_engine(BlochAdjointOracle).set_bloch_point_sources(cells, w).run_bloch_channels(60, None, chan)
    Ez = only.download()[0]
    assert np.abs(Ez.imag).max() > 1e-3 * np.abs(Ez.real).max() > 0


def test_product_spectra_and_maxima_restate_their_definitions():
    eng = small_engine(BlochAdjointOracle)
    amps = np.tile(ricker(100, A_DT, A_FC), (2, 1))
    eng.run(100, amps).hold_bloch_window()
    held = eng.read_dft_window().copy()
    eng.reset().run(70, 1j * amps)
    assert np.array_equal(eng.held_b, held)                  # the held window survives reset and a further run
    cur = eng.read_dft_window()
    coef = np.array([1 + 2j, -0.5j, 0.3])
    want = (coef[None, :, None, None] * held * cur).real.sum(axis=1)
    got = eng.bloch_window_product(coef)
    assert got.shape == (2, 6, 12) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    tr = eng.read_probes(0, 70)
    n = np.arange(70) + 1
    X = np.einsum("bpn,nk->bpk", tr, np.exp(-1j * np.outer(n * A_DT, A_OMEGAS)))
    S, peak = eng.bloch_probe_spectra(A_OMEGAS, peak=True)
    assert np.abs(S - X).max() <= 1e-12 * np.abs(X).max()
    assert np.array_equal(peak, np.maximum(np.abs(tr.real).max(axis=(1, 2)), np.abs(tr.imag).max(axis=(1, 2))))
    sub = eng.bloch_probe_spectra(A_OMEGAS, 10, 25)
    Xs = np.einsum("bpn,nk->bpk", tr[:, :, 10:35], np.exp(-1j * np.outer(n[10:35] * A_DT, A_OMEGAS)))
    assert np.abs(sub - Xs).max() <= 1e-12 * np.abs(X).max()
    Ez, Hx, Hy = eng.download()
    top = lambda f: np.maximum(np.abs(f.real).max(axis=(1, 2)), np.abs(f.imag).max(axis=(1, 2)))
    assert np.array_equal(eng.bloch_field_absmax("Ez"), top(Ez[:, :, :-1]))
    assert np.array_equal(eng.bloch_field_absmax("Hx"), top(Hx)) and np.array_equal(eng.bloch_field_absmax("Hy"), top(Hy))


# ---- 3. the gradients against finite differences -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gradient(fd):
    return a_gradient(fd)


def test_bloch_gradients_match_finite_differences_of_the_oracle(gradient, differences):
    """Adjoint against central finite differences of a forward-only objective on eight cells of both members (columns 0
    and C-2 among them), worst error over max|gradient|; bound 1e-5 for both gradients (G_BOUND of the periodic test).
    Measured here (NumPy, float64): phi = 2.4: eps 1.7e-7, sigma 3.8e-8; phi = 3.0: eps 3.7e-9, sigma 2.9e-9; residuals
    at most 4.8e-8 (forward) and 1.7e-7 (adjoint)."""
    J, geps, gsig, spectra, info = gradient
    assert geps.shape == gsig.shape == (2, 12, 16) and spectra.shape == (2, 6, 3) and J.shape == (2,)
    assert spectra.dtype == np.complex128 and np.abs(spectra.imag).max() > 0
    eps0, sigma0 = a_materials()
    assert np.allclose(a_forward_objective(eps0, sigma0, A_PHI), J, rtol=1e-12, atol=0)
    assert sorted(info) == ["channels_shared", "condition", "residual_adjoint", "residual_forward"]
    for b in range(2):
        err_eps = np.abs(at_cells(geps, b) - differences[0, b]).max() / np.abs(geps[b]).max()
        err_sig = np.abs(at_cells(gsig, b) - differences[1, b]).max() / np.abs(gsig[b]).max()
        print(f"phi = {A_PHI[b]}: adjoint vs central FD on {len(A_CELLS)} cells, worst / max|gradient|: eps {err_eps:.3e}, "
              f"sigma {err_sig:.3e}; residuals {info['residual_forward'][b]:.2e} {info['residual_adjoint'][b]:.2e}")
        assert err_eps <= G_BOUND
        assert err_sig <= G_BOUND


class _Unconjugated(BlochAdjointOracle):
    """The adjoint run with the forward rotation: the wrong sign of s."""

    def run_bloch_channels(self, nsteps, amps=None, channels=None, conjugate=False):
        return BlochAdjointOracle.run_bloch_channels(self, nsteps, amps, channels, conjugate=False)


class _ConjugatedProduct(BlochAdjointOracle):
    """The product with conj(Eadj) in place of Eadj."""

    def _window(self):
        w = BlochAdjointOracle._window(self)
        return w if self.held_b is None else np.conj(w)      # the held (forward) window is taken before any is held


def test_the_conjugation_matters(fd, gradient, differences):
    """The same gradient with the adjoint run un-conjugated, and with conj(Eadj) in the product, misses the finite
    differences on the eight cells by more than 0.1 of max|gradient| (of the right gradient).  Measured here at the
    test's phases (eps / sigma): un-conjugated run phi = 2.4: 4.2 / 1.4, phi = 3.0: 1.3 / 0.74; conj(Eadj)
    phi = 2.4: 4.6 / 1.6, phi = 3.0: 0.60 / 0.46."""
    for name, engine in (("un-conjugated run", _Unconjugated), ("conj(Eadj) in the product", _ConjugatedProduct)):
        _, geps, gsig, _, _ = a_gradient(fd, engine=engine)
        for b in range(2):
            err_eps = np.abs(at_cells(geps, b) - differences[0, b]).max() / np.abs(gradient[1][b]).max()
            err_sig = np.abs(at_cells(gsig, b) - differences[1, b]).max() / np.abs(gradient[2][b]).max()
            print(f"{name}, phi = {A_PHI[b]}: misses by eps {err_eps:.2f}, sigma {err_sig:.2f} of max|gradient|")
            assert err_eps > 0.1 and err_sig > 0.1


# ---- 4. the unit rotation is the periodic helper ---------------------------------------------------------------------------

def test_unit_rotation_is_the_periodic_gradient(fd):
    """rho = (1, 0), real amplitudes, unit weights: batch_bloch_gradient against batch_material_gradient(boundary=
    "periodic") on PeriodicOracle.  The order of every operation is the same, so exact equality is expected (and found
    here: all four differences are 0); the bound is 1e-12 of the maxima."""
    eps, sigma = g_materials()
    nsteps = 1500
    want = fd.batch_material_gradient(eps, sigma, objective=g_objective, **g_args(2, nsteps=nsteps))
    a = g_args(2, engine=BlochAdjointOracle, nsteps=nsteps)
    del a["boundary"]
    got = fd.batch_bloch_gradient(eps, sigma, objective=g_objective, bloch_phase=0.0, **a)
    worst = {}
    for name, g, w in (("J", got[0], want[0]), ("grad_eps", got[1], want[1]), ("grad_sigma", got[2], want[2]),
                       ("spectra", got[3], want[3])):
        worst[name] = max(np.abs(g[m] - w[m]).max() / np.abs(w[m]).max() for m in range(2))
        print(f"{name}: worst |difference| / max = {worst[name]:.2e}, equal: {np.array_equal(g, w)}")
    assert all(v <= 1e-12 for v in worst.values())
    assert got[3].dtype == np.complex128
    for k in ("residual_forward", "residual_adjoint"):
        assert np.allclose(got[4][k], want[4][k], rtol=1e-12)


# ---- 5. the session ----------------------------------------------------------------------------------------------------

class NoBulkReads(BlochAdjointOracle):
    """A stand-in whose bulk read-backs are forbidden."""

    def _refuse(self, *a, **k):
        raise AssertionError("a bulk read-back was called")

    read_probes = download = read_dft_window = _refuse


def test_bloch_session_is_the_helper(fd):
    """BlochAdjointSession against batch_bloch_gradient over two iterations with a set_design_eps, a set_design_sigma and
    a set_bloch_phase between them: 1e-9 of max|gradient| for both gradients; no trace, field or window is read back."""
    nsteps = 1500
    eps, sigma = a_materials()
    r0, c0, nr, nc = A_DESIGN

    def agree(s, eps, sigma, phi):
        want = a_gradient(fd, eps=eps, sigma=sigma, nsteps=nsteps, bloch_phase=phi)
        J, g, sp, info = s.value_and_grad(g_objective)
        gs = s.sigma_gradient()
        for m in range(2):
            assert np.abs(g[m] - want[1][m]).max() <= 1e-9 * np.abs(want[1][m]).max(), m
            assert np.abs(gs[m] - want[2][m]).max() <= 1e-9 * np.abs(want[2][m]).max(), m
            assert np.abs(sp[m] - want[3][m]).max() <= 1e-12 * np.abs(want[3][m]).max(), m
        assert np.allclose(J, want[0], rtol=1e-12, atol=0)
        assert sorted(info) == sorted(want[4])
        for k in ("residual_forward", "residual_adjoint"):
            assert np.allclose(info[k], want[4][k], rtol=1e-9), k
        return g

    args = a_args(2, engine=NoBulkReads, nsteps=nsteps)
    with fd.BlochAdjointSession(eps, **args) as s:
        assert s.engine.bloch and s.set_conductivity(sigma) is s and np.array_equal(s.bloch_phase, A_PHI)
        with pytest.raises(RuntimeError, match="no gradient yet"):
            s.sigma_gradient()
        g0 = agree(s, eps, sigma, A_PHI)
        rng = np.random.default_rng(11)
        new_eps = EPS0 * (1 + 2 * rng.random((2, nr, nc)))
        new_sigma = 0.2 + 0.5 * rng.random((2, nr, nc))
        new_phi = np.array([2.7, 2.1])
        assert s.set_design_eps(new_eps) is s and s.set_design_sigma(new_sigma) is s and s.set_bloch_phase(new_phi) is s
        with pytest.raises(RuntimeError, match="no gradient yet"):       # the windows belong to the old phases
            s.sigma_gradient()
        eps2, sigma2 = eps.copy(), sigma.copy()
        eps2[:, r0:r0 + nr, c0:c0 + nc] = new_eps
        sigma2[:, r0:r0 + nr, c0:c0 + nc] = new_sigma
        g1 = agree(s, eps2, sigma2, new_phi)
        assert not np.allclose(g1, g0, rtol=1e-3)
        with pytest.raises(ValueError, match="member 1: bloch_phase is not finite"):
            s.set_bloch_phase([0.3, np.inf])
        assert np.array_equal(s.bloch_phase, new_phi)
    with pytest.raises(RuntimeError, match="the session is closed"):
        s.set_bloch_phase(0.3)


# ---- 6. host refusals ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,call", [
    ("set_bloch_point_sources", lambda e: e.set_bloch_point_sources(np.array([(5, 5)]), np.ones((1, 1)))),
    ("run_bloch_channels", lambda e: e.run_bloch_channels(4, None, np.zeros((1, 4)))),
    ("hold_bloch_window", lambda e: e.hold_bloch_window()),
    ("bloch_window_product", lambda e: e.bloch_window_product(np.ones(1))),
    ("bloch_probe_spectra", lambda e: e.bloch_probe_spectra([1e11], 0, 4)),
    ("bloch_field_absmax", lambda e: e.bloch_field_absmax("Ez")),
])
def test_the_bloch_calls_need_a_phase_on_the_host(fd, method, call):
    from fdtd2d_amd import _abi
    with pytest.raises(fd.Fdtd2dError, match="no Bloch phase is set") as ei:
        call(host_engine(fd, bloch=False))
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(AssertionError, match="the library was called"):    # with a phase the call goes through
        call(host_engine(fd))


def test_bad_arguments_of_the_bloch_calls_are_refused_on_the_host(fd):
    from fdtd2d_amd import _abi
    with pytest.raises(fd.Fdtd2dError, match="member 1: a point source lies in column 12, the image of column 0") as ei:
        host_engine(fd).set_bloch_point_sources(np.array([[(4, 2)], [(4, 12)], [(4, 3)]]), np.ones((1, 2)))
    assert ei.value.code == _abi.E_ARG
    with pytest.raises(ValueError, match=r"weights must have shape \(1, K\) or \(3, 1, K\)"):
        host_engine(fd).set_bloch_point_sources(np.array([(4, 2)]), np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"channels must have shape \(1, 4\) or \(3, 1, 4\)"):
        host_engine(fd).run_bloch_channels(4, None, np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r"amps must have shape \(3, 4\)"):
        host_engine(fd).run_bloch_channels(4, np.zeros((2, 4)), np.zeros((1, 4)))
    with pytest.raises(ValueError, match=r"coef must have shape \(1,\) or \(3, 1\)"):
        host_engine(fd).bloch_window_product(np.ones(2))
    with pytest.raises(ValueError, match='which must be "Ez", "Hx" or "Hy"'):
        host_engine(fd).bloch_field_absmax("Ezx")


def _with(a, at, value):
    a = a.copy()
    a[at] = value
    return a


@pytest.mark.parametrize("change,match", [
    (dict(bloch_phase=None), r"member 0 \(and every other\): bloch_phase is required"),
    (dict(bloch_phase=np.array([0.4, np.nan])), r"member 1: bloch_phase is not finite"),
    (dict(probes=np.array([(50, c) for c in (0, 3, 6, 9, 12, 16)])), r"member 0: a probe cell lies in column 16"),
    (dict(design=(24, 0, 12, 17)), r"member 0 \(and every other\): design window \(24, 0, 12, 17\) must lie in columns"),
    (dict(design=(7, 0, 12, 16)), r"member 0 \(and every other\): design window .* must keep 8 rows"),
    (dict(sigma_at=((1, 50, 3), 0.1)), r"member 1: sigma is non-zero at the probe cell \(50, 3\)"),
    (dict(sigma_at=((1, 57, 0), 0.1)), r"member 1: sigma is non-zero at cell \(57, 0\), within 8 cells"),
    (dict(sources=np.array([(14, 0, 1, 16), (14, 3, 1, 14)])), r"member 1: the source \(14, 3, 1, 14\) reaches column 16"),
    (dict(source_weights="tilt"), r'source_weights must be "ramp", None or an array'),
    (dict(source_weights=np.ones(17)), r"source_weights must have shape \(16,\) or \(2, 16\)"),
])
def test_bloch_gradient_and_session_refuse_bad_arguments_on_the_host(monkeypatch, fd, change, match):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    eps, sigma = a_materials()
    change = dict(change)
    if "sigma_at" in change:
        at, v = change.pop("sigma_at")
        sigma = _with(sigma, at, v)
    with pytest.raises(ValueError, match=match):
        a_gradient(fd, eps=eps, sigma=sigma, engine=None, nsteps=400, **change)
    if "sigma" not in match:                                 # the session takes its conductivity after construction
        with pytest.raises(ValueError, match=match):
            fd.BlochAdjointSession(eps, **{**a_args(2, engine=None, nsteps=400), **change})
    with pytest.raises(AssertionError, match="the device was touched"):     # good arguments reach the engine
        a_gradient(fd, engine=None, nsteps=400)
