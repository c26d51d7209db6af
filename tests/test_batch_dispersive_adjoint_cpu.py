"""CPU-only checks of the adjoint gradients of dispersive batches (fdtd2d_batch_dispersive_adjoint.h, batch.py,
adjoint.py), on the stand-ins of tests/oracle_batch_dispersive_adjoint.py.

The surface: the two entry points are declared, exported and bound, the info id is named and distinct from every id of
include/*.h, the pinned parameter lists of the existing helpers are as they were.

The gradients, periodic: the configuration of tests/test_batch_periodic_cpu.py (64 x 17, an 8-cell layer, float64, 5000
steps, dt 4e-13, dx 2.5e-4, its design window, sources, probes, frequencies, cells, materials and objective) with a
pole on the design window: member 0 Drude, gamma = 5e10, wp2 = (2 pi 30 GHz)^2 (0.5 + U[0, 1)); member 1 Lorentz,
omega0 = 2 pi 45 GHz, gamma = 3e10, wp2 = omega0^2 (0.5 + U[0, 1)); default_rng(5).  ``batch_dispersive_gradient``
against central finite differences (1e-4 of each quantity's scale) of a forward-only run of DispersivePeriodicOracle.
Bound 1e-5 of max|gradient|, the project's G_BOUND; the measured values are in the test's docstring.

The gradients, PML: the configuration of tests/test_batch_adjoint_cpu.py (48 x 48, dx 1e-3, dt 1.6e-12, an 8-cell
layer, 5000 steps) with a Drude block (gamma = 5e10) on the design window; see the test's docstring for what was
measured and how the bound follows.

The session: ``DispersiveAdjointSession`` against the helper over two iterations, 1e-9 of max|gradient|.  A zero pole
gives batch_material_gradient's gradients bit for bit.  The host refusals, each with its message."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import test_batch_adjoint_cpu as pcfg
from oracle_batch_dispersive import DispersivePeriodicOracle, DispersivePmlOracle
from oracle_batch_dispersive_adjoint import DispersiveAdjointPeriodicOracle, DispersiveAdjointPmlOracle
from oracle_batch_periodic import PeriodicOracle
from test_batch_periodic_cpu import (C0, G_BOUND, G_C, G_CELLS, G_DESIGN, G_DT, G_DX, G_FC, G_L, G_NSTEPS, G_OMEGAS,
                                     G_PROBES, G_R, G_SOURCES, H_EPS, H_SIGMA, MU0, g_args, g_materials, g_objective,
                                     g_sources, ricker)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_dispersive_adjoint.h")
NAMES = ["fdtd2d_batch_dispersive_window_product", "fdtd2d_batch_hold_dispersive_window"]
EPS0 = 8.85418e-12

# the poles of the periodic configuration: (gamma, omega0) per member and the scale of wp2
D_GAMMA = np.array([5e10, 3e10])
D_OMEGA0 = np.array([0.0, 2 * np.pi * 45e9])
D_SCALE = np.array([(2 * np.pi * 30e9) ** 2, (2 * np.pi * 45e9) ** 2])
H_REL = 1e-4                                    # the finite-difference step of wp2, of its scale


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def d_wp2(count=2, seed=5):
    """wp2 = scale * (0.5 + U[0, 1)) on the design window, zero elsewhere, the image column equal to column 0."""
    rng = np.random.default_rng(seed)
    r0, c0, nr, nc = G_DESIGN
    wp2 = np.zeros((count, G_R, G_C))
    for b in range(count):
        wp2[b, r0:r0 + nr, c0:c0 + nc] = D_SCALE[b % 2] * (0.5 + rng.random((nr, nc)))
    wp2[:, :, -1] = wp2[:, :, 0]
    return wp2


def d_gradient(fd, eps=None, sigma=None, wp2=None, gamma=D_GAMMA, omega0=D_OMEGA0, **kw):
    e, s = g_materials()
    eps, sigma, wp2 = e if eps is None else eps, s if sigma is None else sigma, d_wp2() if wp2 is None else wp2
    kw.setdefault("engine", DispersiveAdjointPeriodicOracle)
    return fd.batch_dispersive_gradient(eps, sigma, (wp2, gamma, omega0), objective=g_objective,
                                        **g_args(eps.shape[0], **kw))


def d_forward_objective(eps, sigma, wp2, gamma, omega0, sources):
    """J of every member from a forward run of DispersivePeriodicOracle alone (no adjoint code involved)."""
    from fdtd2d_amd.adjoint import probe_spectra
    B = eps.shape[0]
    eng = DispersivePeriodicOracle(B, G_R, G_C, G_DT, G_DX, dtype=np.float64, boundary="periodic")
    eng.set_materials(eps, MU0).set_pml(G_L, courant00=C0 * G_DT / G_DX)
    eng.set_conductivity(sigma)
    eng.set_dispersion(wp2, gamma, omega0)
    eng.set_sources(sources).set_probes(G_PROBES, G_NSTEPS)
    eng.run(G_NSTEPS, np.tile(ricker(G_NSTEPS, G_DT, G_FC), (B, 1)))
    return g_objective(probe_spectra(eng.read_probes(), np.tile(G_OMEGAS, (B, 1)), G_DT))[0]


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_dispersive_adjoint_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_DISPERSIVE_ADJOINT_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_DISPERSIVE_ADJOINT_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_DISPERSIVE_ADJOINT_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "double *": ctypes.POINTER(ctypes.c_double),
             "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_DISPERSIVE_ADJOINT_SIGNATURES[n][1], n
    # nothing was added to fdtd2d.h
    assert "dispersive_window" not in open(os.path.join(ROOT, "include", "fdtd2d.h")).read()


def test_dispersive_adjoint_info_id_is_named_and_distinct():
    """The id is an enumerator of the new header; every FDTD2D_BATCH_INFO_* of include/*.h, macro or enumerator, has
    another value."""
    from fdtd2d_amd import _abi
    pat = r"FDTD2D_(BATCH_INFO_\w+)\s*(?:=\s*|\s+)(-?\d+)\b"
    mine = dict(re.findall(pat, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert mine == {"BATCH_INFO_HELD_DISPERSIVE_WINDOW": "20"} and _abi.BATCH_INFO_HELD_DISPERSIVE_WINDOW == 20
    assert _abi.BATCH_MAX_PRODUCT_SETS == 3 and re.search(r"FDTD2D_BATCH_MAX_PRODUCT_SETS = 3\b", open(HEADER).read())
    taken = {}
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != os.path.basename(HEADER):
            txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            taken.update(re.findall(pat, txt))
    assert len(taken) >= 20 and "BATCH_INFO_HELD_DISPERSIVE_WINDOW" not in taken
    assert 20 not in {int(v) for v in taken.values()}
    assert max(int(v) for v in taken.values()) == 19          # the next free id
    names = [k for k in dir(_abi) if k.startswith("BATCH_INFO_")]
    assert len({getattr(_abi, k) for k in names}) == len(names)


def test_pinned_parameter_lists_are_unchanged(fd):
    sig = lambda f: list(inspect.signature(f).parameters)
    grad = ["eps", "mu", "nsteps", "sources", "probes", "omegas", "design", "objective", "fc", "waveform", "dt", "dx",
            "dtype", "boundary", "pml_cells", "device", "engine"]
    assert sig(fd.batch_eps_gradient) == grad
    assert sig(fd.batch_material_gradient) == ["eps", "sigma"] + grad[1:]
    assert sig(fd.AdjointSession.__init__) == ["self"] + [k for k in grad if k != "objective"]
    assert sig(fd.BatchEngine.hold_dft_window) == ["self"]
    assert sig(fd.BatchEngine.dft_window_product) == ["self", "coef"]
    assert sig(fd.BatchEngine.set_dispersion) == ["self", "wp2", "gamma", "omega0"]
    # the new surface
    assert sig(fd.batch_dispersive_gradient) == ["eps", "sigma", "dispersion"] + grad[1:]
    p = inspect.signature(fd.batch_dispersive_gradient).parameters
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items()
               if k not in ("eps", "sigma", "dispersion", "mu"))
    assert sig(fd.DispersiveAdjointSession.__init__) == ["self", "eps", "mu", "dispersion", "sigma"] + \
        [k for k in grad[2:] if k != "objective"]
    assert sig(fd.BatchEngine.hold_dispersive_window) == ["self"]
    assert sig(fd.BatchEngine.dispersive_window_product) == ["self", "coefs", "scales"]
    assert sig(fd.pole_coefficients) == ["omegas", "dt", "gamma", "omega0"]
    assert isinstance(fd.DispersiveAdjointSession.wp2, property) and issubclass(fd.DispersiveAdjointSession,
                                                                                 fd.AdjointSession)
    for name in ("batch_dispersive_gradient", "DispersiveAdjointSession", "pole_coefficients"):
        assert name in fd.__all__
    for cls in (DispersiveAdjointPmlOracle, DispersiveAdjointPeriodicOracle):
        for name in ("hold_dispersive_window", "dispersive_window_product"):
            assert callable(getattr(cls, name)) and callable(getattr(fd.BatchEngine, name))


def test_dispersive_adjoint_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.fdtd2d_batch_hold_dispersive_window(None) == _abi.E_ARG
    assert lib.fdtd2d_batch_dispersive_window_product(None, 1, dp, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_INFO_HELD_DISPERSIVE_WINDOW) == _abi.E_ARG


def test_pole_coefficients_are_the_formula(fd):
    """-(z - 1) / ((z - a)(z - 1) + ck z) and bq, against the derivative of the operator's pole term by cj: the term is
    cj (z - 1)^2 / den, its share of the right side's D (z - 1) leaves (z - 1) / den."""
    om, dt = G_OMEGAS, G_DT
    c, bq = fd.pole_coefficients(om, dt, D_GAMMA, D_OMEGA0)
    assert c.shape == (2, 3) and bq.shape == (2,)
    for b in range(2):
        g = D_GAMMA[b] * dt / 2
        a, q = (1 - g) / (1 + g), dt / (1 + g)
        ck = q * D_OMEGA0[b] ** 2 * dt
        z = np.exp(1j * om * dt)
        assert np.allclose(c[b], -(z - 1) / ((z - a) * (z - 1) + ck * z), rtol=1e-14, atol=0) and bq[b] == q
        # the continuous limit: cj (z-1)^2/den -> dx EPS0 wp2 * (-i w) chi-like factor; at gamma = 0 = omega0 the
        # factor is -1 / (z - 1), purely a discrete integrator
    c0, _ = fd.pole_coefficients(om, dt, 0.0, 0.0)
    assert c0.shape == (1, 3) and np.allclose(c0[0], -1 / (np.exp(1j * om * dt) - 1), rtol=1e-14, atol=0)


def test_the_stand_in_product_is_the_single_product_per_set():
    """The multi-product of the stand-in: every set is window_product of the parent, scaled; one set with scale 1 is the
    lossy stand-in's dft_window_product of the same two windows bit for bit.  The parents keep refusing."""
    rng = np.random.default_rng(2)
    eng = DispersiveAdjointPmlOracle(2, 23, 19, 5e-14, 1e-4, dtype=np.float64)
    eng.set_materials(np.full((2, 23, 19), EPS0), MU0).set_pml(4, courant00=0.3)
    eng.set_dispersion(0.0, 1e10, 0.0)
    eng.set_dft_window((8, 7, 5, 4), 2 * np.pi * np.array([3e11, 5e11]))
    shape = eng.win["re"].shape
    eng.win["re"][...], eng.win["im"][...] = rng.standard_normal(shape), rng.standard_normal(shape)
    held = eng.read_dft_window().copy()
    eng.hold_dispersive_window()
    eng.win["re"][...], eng.win["im"][...] = rng.standard_normal(shape), rng.standard_normal(shape)
    coefs = rng.standard_normal((3, 2, 2)) + 1j * rng.standard_normal((3, 2, 2))
    scales = rng.standard_normal((2, 3))
    out = eng.dispersive_window_product(coefs, scales)
    one = eng.dispersive_window_product(coefs[:1])
    assert out.shape == (3, 2, 5, 4) and one.shape == (1, 2, 5, 4)
    with pytest.raises(AssertionError):
        eng.hold_dft_window()
    with pytest.raises(AssertionError):
        eng.dft_window_product(coefs[0])
    cur = eng.read_dft_window().copy()
    eng.set_dispersion(None)                 # the parents' calls again, on the same two windows
    assert eng.held_dispersive is None
    eng.win["re"][...], eng.win["im"][...] = held.real, held.imag
    eng.hold_dft_window()
    eng.win["re"][...], eng.win["im"][...] = cur.real, cur.imag
    for c in range(3):
        assert np.array_equal(out[c], scales[:, c, None, None] * eng.dft_window_product(coefs[c]))
    assert np.array_equal(one[0], eng.dft_window_product(coefs[0]))
    with pytest.raises(AssertionError, match="needs a dispersive pole"):
        eng.hold_dispersive_window()


# ---- 2. finite differences, periodic ---------------------------------------------------------------------------------------

_cache = {}


def periodic_gradient(fd):
    if "g" not in _cache:
        _cache["g"] = d_gradient(fd)
    return _cache["g"]


def test_periodic_dispersive_gradients_match_finite_differences_of_the_oracle(fd):
    """Adjoint against central finite differences on eight cells of both members, worst error over max|gradient|.
    Measured (members 0 and 1): eps 1.0e-7 and 8.7e-7, sigma 4.0e-9 and 2.3e-7, wp2 1.9e-8 and 1.2e-7; residuals (the
    end-of-run max|Ez| over the largest probe sample) 2.0e-5 and 9.3e-5 (forward), 5.2e-10 and 2.0e-9 (adjoint); bound
    1e-5 for all three."""
    J, geps, gsig, gwp2, spectra, info = periodic_gradient(fd)
    r0, c0, nr, nc = G_DESIGN
    assert geps.shape == gsig.shape == gwp2.shape == (2, nr, nc) and spectra.shape == (2, 16, 3) and J.shape == (2,)
    (eps0, sigma0), wp20 = g_materials(), d_wp2()
    assert np.array_equal(d_forward_objective(eps0, sigma0, wp20, D_GAMMA, D_OMEGA0, G_SOURCES), J)
    for b in range(2):
        n, hw = len(G_CELLS), H_REL * D_SCALE[b]
        eps, sigma, wp2 = (np.repeat(a[b:b + 1], 6 * n, axis=0) for a in (eps0, sigma0, wp20))
        for k, (r, c) in enumerate(G_CELLS):
            cols = [c, G_C - 1] if c == 0 else [c]          # column 0 and its image move together
            eps[6 * k, r, cols] += H_EPS
            eps[6 * k + 1, r, cols] -= H_EPS
            sigma[6 * k + 2, r, cols] += H_SIGMA
            sigma[6 * k + 3, r, cols] -= H_SIGMA
            wp2[6 * k + 4, r, cols] += hw
            wp2[6 * k + 5, r, cols] -= hw
        Jp = d_forward_objective(eps, sigma, wp2, np.full(6 * n, D_GAMMA[b]), np.full(6 * n, D_OMEGA0[b]),
                                 np.tile(G_SOURCES[b], (6 * n, 1)))
        at = lambda g: np.array([g[b, r - r0, c - c0] for r, c in G_CELLS])
        err_eps = np.abs(at(geps) - (Jp[0::6] - Jp[1::6]) / (2 * H_EPS)).max() / np.abs(geps[b]).max()
        err_sig = np.abs(at(gsig) - (Jp[2::6] - Jp[3::6]) / (2 * H_SIGMA)).max() / np.abs(gsig[b]).max()
        err_wp2 = np.abs(at(gwp2) - (Jp[4::6] - Jp[5::6]) / (2 * hw)).max() / np.abs(gwp2[b]).max()
        print(f"member {b}: adjoint vs central FD on {n} cells, worst / max|gradient|: eps {err_eps:.3e}, sigma "
              f"{err_sig:.3e}, wp2 {err_wp2:.3e}; residuals {info['residual_forward'][b]:.2e} "
              f"{info['residual_adjoint'][b]:.2e}")
        assert err_eps <= G_BOUND
        assert err_sig <= G_BOUND
        assert err_wp2 <= G_BOUND


# ---- 3. finite differences, PML ------------------------------------------------------------------------------------------

P_GAMMA, P_SCALE = 5e10, (2 * np.pi * 30e9) ** 2
P_BLOCK = (20, 21, 8, 6)                        # the Drude block: rows 20..27, columns 21..26 of the design window
P_CELLS = [(16, 18), (31, 29), (20, 21), (27, 26), (24, 24), (23, 22), (29, 19), (21, 28)]   # four of them in the block
P_MEASURED = {"eps": 1.8e-6, "sigma": 7.3e-7, "wp2": 7.8e-8}
P_BOUND = {k: min(G_BOUND, 10 * v) for k, v in P_MEASURED.items()}       # ten times the measured, at most the project's 1e-5


def p_materials():
    """design_eps of test_batch_adjoint_cpu.py, 0.2..0.7 S/m on the design window (as g_materials has it), and the Drude
    block."""
    rng = np.random.default_rng(7)
    eps = pcfg.design_eps()
    r0, c0, nr, nc = pcfg.DESIGN
    sigma, wp2 = np.zeros(eps.shape), np.zeros(eps.shape)
    sigma[:, r0:r0 + nr, c0:c0 + nc] = 0.2 + 0.5 * rng.random((nr, nc))
    br, bc, bnr, bnc = P_BLOCK
    wp2[:, br:br + bnr, bc:bc + bnc] = P_SCALE * (0.5 + rng.random((bnr, bnc)))
    return eps, sigma, wp2


def p_args(count, engine=DispersiveAdjointPmlOracle, nsteps=pcfg.NSTEPS):
    return dict(nsteps=nsteps, sources=np.tile(pcfg.SOURCE, (count, 1)), probes=pcfg.PROBES, omegas=pcfg.OMEGAS,
                design=pcfg.DESIGN, fc=pcfg.FC, dt=pcfg.DT, dx=pcfg.DX, dtype=np.float64, boundary="pml",
                pml_cells=pcfg.LAYER, engine=engine)


def p_forward_objective(eps, sigma, wp2):
    from fdtd2d_amd.adjoint import probe_spectra
    B = eps.shape[0]
    eng = DispersivePmlOracle(B, pcfg.R, pcfg.C, pcfg.DT, pcfg.DX, dtype=np.float64)
    eng.set_materials(eps, MU0).set_pml(pcfg.LAYER, courant00=(1 / np.sqrt(EPS0 * MU0) * pcfg.DT) / pcfg.DX)
    eng.set_conductivity(sigma)
    eng.set_dispersion(wp2, P_GAMMA, 0.0)
    eng.set_sources(np.tile(pcfg.SOURCE, (B, 1))).set_probes(pcfg.PROBES, pcfg.NSTEPS)
    eng.run(pcfg.NSTEPS, np.tile(ricker(pcfg.NSTEPS, pcfg.DT, pcfg.FC), (B, 1)))
    return pcfg.objective(probe_spectra(eng.read_probes(), np.tile(pcfg.OMEGAS, (B, 1)), pcfg.DT))[0]


def p_errors(fd):
    """The three worst errors over max|gradient| of the PML member, and the residuals."""
    eps0, sigma0, wp20 = p_materials()
    J, geps, gsig, gwp2, spectra, info = fd.batch_dispersive_gradient(eps0, sigma0, (wp20, P_GAMMA, 0.0),
                                                                      objective=pcfg.objective, **p_args(1))
    assert np.array_equal(p_forward_objective(eps0, sigma0, wp20), J)
    r0, c0, nr, nc = pcfg.DESIGN
    assert geps.shape == gsig.shape == gwp2.shape == (1, nr, nc)
    br, bc, bnr, bnc = P_BLOCK
    inblock = [(r, c) for r, c in P_CELLS if br <= r < br + bnr and bc <= c < bc + bnc]
    assert len(inblock) == 4
    n, hw = len(P_CELLS), H_REL * P_SCALE
    m = 4 * n + 2 * len(inblock)
    eps, sigma, wp2 = (np.repeat(a, m, axis=0) for a in (eps0, sigma0, wp20))
    for k, (r, c) in enumerate(P_CELLS):
        eps[4 * k, r, c] += H_EPS
        eps[4 * k + 1, r, c] -= H_EPS
        sigma[4 * k + 2, r, c] += H_SIGMA
        sigma[4 * k + 3, r, c] -= H_SIGMA
    for k, (r, c) in enumerate(inblock):        # central differences need wp2 > 0: the cells of the block
        wp2[4 * n + 2 * k, r, c] += hw
        wp2[4 * n + 2 * k + 1, r, c] -= hw
    Jp = p_forward_objective(eps, sigma, wp2)
    at = lambda g, cells: np.array([g[0, r - r0, c - c0] for r, c in cells])
    Je, Jw = Jp[:4 * n], Jp[4 * n:]
    errs = {"eps": np.abs(at(geps, P_CELLS) - (Je[0::4] - Je[1::4]) / (2 * H_EPS)).max() / np.abs(geps[0]).max(),
            "sigma": np.abs(at(gsig, P_CELLS) - (Je[2::4] - Je[3::4]) / (2 * H_SIGMA)).max() / np.abs(gsig[0]).max(),
            "wp2": np.abs(at(gwp2, inblock) - (Jw[0::2] - Jw[1::2]) / (2 * hw)).max() / np.abs(gwp2[0]).max()}
    return errs, info


def test_pml_dispersive_gradients_match_finite_differences_of_the_oracle(fd):
    """Adjoint against central finite differences on eight cells (eps, sigma) and on the four of them that carry the pole
    (wp2; the other four have wp2 = 0, where test_a_zero_pole_... differentiates), worst error over max|gradient|.
    Measured: eps 1.8e-6, sigma 7.2e-7, wp2 7.7e-8; residuals 3.0e-5 (forward) and 7.8e-8 (adjoint).  The lossless
    configuration of test_batch_adjoint_cpu.py misses by 1.6e-3 because its fields still ring; the conductivity of the
    design window and the pole's damping bring the residual down far enough, so no background conductivity is added (with
    0.05 S/m on every cell outside the margin the three errors were 1.0e-7, 6.3e-8 and 1.1e-7).  Bounds: ten times the
    measured value and at most 1e-5."""
    errs, info = p_errors(fd)
    print(f"pml: adjoint vs central FD on {len(P_CELLS)} cells, worst / max|gradient|: eps {errs['eps']:.3e}, sigma "
          f"{errs['sigma']:.3e}, wp2 {errs['wp2']:.3e} (the four cells of the block); "
          f"residuals {info['residual_forward'][0]:.2e} {info['residual_adjoint'][0]:.2e}")
    for k in ("eps", "sigma", "wp2"):
        assert errs[k] <= P_BOUND[k], k


# ---- 4. the session ----------------------------------------------------------------------------------------------------

def test_dispersive_session_is_the_helper(fd):
    """DispersiveAdjointSession against batch_dispersive_gradient over two iterations with a set_design_eps, a
    set_design_sigma and a set_design_wp2 between them: 1e-9 of max|gradient| for the three gradients (2500 steps)."""
    nsteps = 2500
    (eps, sigma), wp2 = g_materials(), d_wp2()
    r0, c0, nr, nc = G_DESIGN
    holds = []

    class Counting(DispersiveAdjointPeriodicOracle):
        def dispersive_window_product(self, coefs, scales=None):
            holds.append(np.asarray(coefs).shape[0])
            return DispersiveAdjointPeriodicOracle.dispersive_window_product(self, coefs, scales)

    def agree(s, eps, sigma, wp2):
        want = d_gradient(fd, eps=eps, sigma=sigma, wp2=wp2, nsteps=nsteps)
        before = len(holds)
        J, g, sp, _ = s.value_and_grad(g_objective)
        got = (g, s.sigma_gradient(), s.wp2_gradient())
        assert holds[before:] == [3]            # the three gradients: one pass over the windows
        for k in range(3):
            for m in range(2):
                assert np.abs(got[k][m] - want[1 + k][m]).max() <= 1e-9 * np.abs(want[1 + k][m]).max(), (k, m)
        assert np.allclose(J, want[0], rtol=1e-12, atol=0)
        assert np.allclose(sp, want[4], rtol=1e-12, atol=1e-12 * np.abs(want[4]).max())
        return got

    with fd.DispersiveAdjointSession(eps, dispersion=(wp2, D_GAMMA, D_OMEGA0), sigma=sigma,
                                     **g_args(2, nsteps=nsteps, engine=Counting)) as s:
        assert s.engine.periodic and s.engine.dispersive
        assert np.array_equal(s.wp2, wp2) and np.array_equal(s.sigma, sigma) and not s.wp2.flags.writeable
        with pytest.raises(RuntimeError, match="no gradient yet"):
            s.wp2_gradient()
        g0 = agree(s, eps, sigma, wp2)
        rng = np.random.default_rng(11)
        new_eps = EPS0 * (1 + 2 * rng.random((2, nr, nc)))
        new_sigma = 0.2 + 0.5 * rng.random((2, nr, nc))
        new_wp2 = D_SCALE[:, None, None] * (0.5 + rng.random((2, nr, nc)))
        assert s.set_design_eps(new_eps) is s and s.set_design_sigma(new_sigma) is s and s.set_design_wp2(new_wp2) is s
        eps2, sigma2, wp22 = eps.copy(), sigma.copy(), wp2.copy()
        for full, new in ((eps2, new_eps), (sigma2, new_sigma), (wp22, new_wp2)):
            full[:, r0:r0 + nr, c0:c0 + nc] = new
        assert np.array_equal(s.wp2, wp22)
        g1 = agree(s, eps2, sigma2, wp22)
        for k in range(3):
            assert np.abs(g1[k] - g0[k]).max() > 1e-3 * np.abs(g0[k]).max()      # the updates moved the gradients
        # the pole is required
        s.engine.set_dispersion(None)
        with pytest.raises(fd.Fdtd2dError, match="needs its dispersive pole"):
            s.value_and_grad(g_objective)


# ---- 5. a zero pole ------------------------------------------------------------------------------------------------------

def test_a_zero_pole_gives_the_lossy_gradients_and_a_wp2_gradient(fd):
    """wp2 = 0 everywhere: J, the eps and the sigma gradient are batch_material_gradient's bit for bit (jn is exactly
    zero, so the runs are the lossy ones), and the wp2 gradient matches finite differences taken from wp2 = 0 upward:
    (-3 J(0) + 4 J(h) - J(2h)) / 2h, whose error is of second order in h as the central difference's is, so it takes the
    same bound, 1e-5 of max|gradient| (h = 1e-4 of the scale).  Measured: 5.4e-8 and 4.9e-8 (members 0 and 1)."""
    eps0, sigma0 = g_materials()
    zero = np.zeros(eps0.shape)
    J, geps, gsig, gwp2, spectra, info = d_gradient(fd, wp2=zero)
    want = fd.batch_material_gradient(eps0, sigma0, objective=g_objective, **g_args(2))
    assert np.array_equal(J, want[0]) and np.array_equal(geps, want[1]) and np.array_equal(gsig, want[2])
    assert np.array_equal(spectra, want[3])
    r0, c0, nr, nc = G_DESIGN
    cells = G_CELLS[:4]
    for b in range(2):
        n, hw = len(cells), H_REL * D_SCALE[b]
        wp2 = np.zeros((2 * n + 1, G_R, G_C))
        for k, (r, c) in enumerate(cells):
            cols = [c, G_C - 1] if c == 0 else [c]
            wp2[2 * k, r, cols] = hw
            wp2[2 * k + 1, r, cols] = 2 * hw
        m = 2 * n + 1
        Jp = d_forward_objective(np.repeat(eps0[b:b + 1], m, axis=0), np.repeat(sigma0[b:b + 1], m, axis=0), wp2,
                                 np.full(m, D_GAMMA[b]), np.full(m, D_OMEGA0[b]), np.tile(G_SOURCES[b], (m, 1)))
        assert Jp[-1] == J[b]
        fdiff = (-3 * Jp[-1] + 4 * Jp[0:2 * n:2] - Jp[1:2 * n:2]) / (2 * hw)
        adj = np.array([gwp2[b, r - r0, c - c0] for r, c in cells])
        err = np.abs(adj - fdiff).max() / np.abs(gwp2[b]).max()
        print(f"member {b}: wp2 gradient at wp2 = 0 vs one-sided second-order FD on {n} cells: {err:.3e}")
        assert err <= G_BOUND


# ---- 6. host refusals ----------------------------------------------------------------------------------------------------

def _with(a, at, value):
    a = a.copy()
    a[at] = value
    return a


@pytest.mark.parametrize("change,match", [
    (dict(wp2=np.zeros((2, G_R, G_C - 1))), r"wp2 must have shape \(2, 64, 17\), got \(2, 64, 16\)"),
    (dict(wp2_at=((1, 30, 3), -1.0)), r"member 1: wp2 must be >= 0 and finite"),
    (dict(wp2_at=((0, 30, 3), np.inf)), r"member 0: wp2 must be >= 0 and finite"),
    (dict(wp2_at=((1, 5, 3), 1e20)), r"member 1: wp2 is non-zero at cell \(5, 3\), within 8 cells of an edge \(the 8-cell "
                                     r"PML layer\): only cells that take the plain update may carry a pole"),
    (dict(wp2_at=((0, 57, 0), 1e20)), r"member 0: wp2 is non-zero at cell \(57, 0\), within 8 cells"),
    (dict(wp2_at=((1, 50, 4), 1e20)), r"member 1: wp2 is non-zero at the probe cell \(50, 4\); the adjoint injection "
                                      r"there assumes conj\(g\) / D"),
    (dict(gamma=np.array([1e10, -1.0])), r"member 1: gamma must be >= 0 and finite"),
    (dict(omega0=np.array([np.nan, 1e11])), r"member 0: omega0 must be >= 0 and finite"),
    (dict(gamma=np.zeros(3)), r"gamma must be a scalar or have shape \(2,\), got \(3,\)"),
    (dict(boundary="mur"), r'boundary must be "pml" or "periodic", not \'mur\': a dispersive pole needs the PML layer or '
                           r"periodic columns"),
    (dict(boundary="none"), r'boundary must be "pml" or "periodic"'),
    (dict(sigma_at=((1, 5, 3), 0.1)), r"member 1: sigma is non-zero at cell \(5, 3\), within 8 cells"),
    (dict(design=(7, 0, 12, 16)), r"member 0 \(and every other\): design window .* must keep 8 rows"),
])
def test_dispersive_gradient_refuses_bad_arguments_on_the_host(fd, change, match):
    def boom(*a, **k):
        raise AssertionError("an engine was made")
    (eps, sigma), wp2 = g_materials(), d_wp2()
    change = dict(change)
    if "wp2_at" in change:
        at, v = change.pop("wp2_at")
        wp2 = _with(wp2, at, v)
    if "sigma_at" in change:
        at, v = change.pop("sigma_at")
        sigma = _with(sigma, at, v)
    wp2 = change.pop("wp2", wp2)
    gamma, omega0 = change.pop("gamma", D_GAMMA), change.pop("omega0", D_OMEGA0)
    for make in (lambda **kw: fd.batch_dispersive_gradient(eps, sigma, (wp2, gamma, omega0), objective=g_objective, **kw),
                 lambda **kw: fd.DispersiveAdjointSession(eps, dispersion=(wp2, gamma, omega0), sigma=sigma, **kw)):
        with pytest.raises(ValueError, match=match):
            make(**g_args(2, engine=boom, nsteps=400, **change))


def test_a_dispersion_that_is_no_triple_is_refused(fd):
    (eps, sigma), wp2 = g_materials(), d_wp2()
    for bad in ((wp2, D_GAMMA), None):
        with pytest.raises(ValueError, match=r"dispersion must be \(wp2, gamma, omega0\)"):
            fd.batch_dispersive_gradient(eps, sigma, bad, objective=g_objective, **g_args(2, engine=None, nsteps=400))


def test_a_bloch_engine_is_refused(fd):
    from fdtd2d_amd import _abi

    class Phased(DispersiveAdjointPeriodicOracle):
        _bloch = object()

    (eps, sigma), wp2 = g_materials(), d_wp2()
    for call in (lambda: d_gradient(fd, engine=Phased, nsteps=50),
                 lambda: fd.DispersiveAdjointSession(eps, dispersion=(wp2, D_GAMMA, D_OMEGA0),
                                                     **g_args(2, engine=Phased, nsteps=50))):
        with pytest.raises(fd.Fdtd2dError, match="Bloch phase") as ei:
            call()
        assert ei.value.code == _abi.E_STATE


def test_a_failed_design_update_leaves_the_session_unchanged(fd):
    """set_design_wp2 and set_design_eps: a host refusal (ValueError) and the engine's own refusal (the stability check:
    E_ARG from the library, an AssertionError from the stand-in) both leave the session's copies as they were."""
    from fdtd2d_amd import _abi
    (eps, sigma), wp2 = g_materials(), d_wp2()
    r0, c0, nr, nc = G_DESIGN

    class Refusing(DispersiveAdjointPeriodicOracle):
        refuse = False

        def set_eps_window(self, window, e):
            if self.refuse:
                raise fd.Fdtd2dError(_abi.E_ARG, "member 0: the pole at cell (24,0) breaks the stability bound")
            return DispersiveAdjointPeriodicOracle.set_eps_window(self, window, e)

    with fd.DispersiveAdjointSession(eps, dispersion=(wp2, D_GAMMA, D_OMEGA0), sigma=sigma,
                                     **g_args(2, engine=Refusing, nsteps=50)) as s:
        ok = wp2[:, r0:r0 + nr, c0:c0 + nc]
        for bad, match in ((_with(ok, (1, 2, 3), -1.0), "member 1: wp2 must be >= 0 and finite"),
                           (ok[:, :-1], r"wp2 must have shape \(2, 12, 16\)")):
            with pytest.raises(ValueError, match=match):
                s.set_design_wp2(bad)
        with pytest.raises(AssertionError, match="unstable"):          # dt^2 wp2 EPS0 / eps > 4
            s.set_design_wp2(_with(ok, (0, 2, 3), 1e27))
        assert np.array_equal(s.wp2, wp2) and np.array_equal(s.engine.wp2, wp2)
        e_ok = eps[:, r0:r0 + nr, c0:c0 + nc]
        with pytest.raises(ValueError, match="Courant"):
            s.set_design_eps(_with(e_ok, (0, 1, 1), 0.1 * EPS0))
        s.engine.refuse = True
        with pytest.raises(fd.Fdtd2dError, match="stability") as ei:
            s.set_design_eps(2 * e_ok)
        assert ei.value.code == _abi.E_ARG
        assert np.array_equal(s.eps, eps) and np.array_equal(s.engine.eps, eps)
        s.engine.refuse = False
        J, g, _, _ = s.value_and_grad(g_objective)     # and the session still runs
        assert np.all(np.isfinite(g))


def test_the_existing_helpers_still_refuse_a_dispersive_engine(fd):
    """An engine factory that sets a pole: batch_eps_gradient, batch_material_gradient and AdjointSession raise E_STATE
    before any run, with the new stand-in too, whose parents' hold_dft_window still raises."""
    from fdtd2d_amd import _abi

    class Dispersive(DispersiveAdjointPmlOracle):
        ran = False

        def __init__(self, *a, **k):
            DispersiveAdjointPmlOracle.__init__(self, *a, **k)
            self.wp2 = np.zeros((self.count, self.rows, self.cols))
            self.gamma = self.omega0 = np.zeros(self.count)

        def run(self, *a, **k):
            Dispersive.ran = True
            return DispersiveAdjointPmlOracle.run(self, *a, **k)

    eps = pcfg.design_eps(count=2)
    args = p_args(2, engine=Dispersive, nsteps=50)
    for call in (lambda: fd.batch_eps_gradient(eps, objective=pcfg.objective, **args),
                 lambda: fd.batch_material_gradient(eps, np.zeros(eps.shape), objective=pcfg.objective, **args),
                 lambda: fd.AdjointSession(eps, **args)):
        with pytest.raises(fd.Fdtd2dError, match="dispersive pole") as ei:
            call()
        assert ei.value.code == _abi.E_STATE
    assert not Dispersive.ran
    with pytest.raises(AssertionError):
        Dispersive(1, 23, 19).hold_dft_window()


def test_the_engine_refuses_the_new_calls_without_a_pole_before_the_library(fd):
    """BatchEngine's own refusals need no device: they are raised before the library is called."""
    from fdtd2d_amd import _abi
    E = fd.BatchEngine

    class Fake:
        _bloch = None
        dispersive = False
        _no_lattice = lambda self, what: None
        _no_bloch = E._no_bloch
        _need_dispersion = E._need_dispersion

    for call in (lambda: E.hold_dispersive_window(Fake()), lambda: E.dispersive_window_product(Fake(), np.ones((1, 2)))):
        with pytest.raises(fd.Fdtd2dError, match="needs a dispersive pole") as ei:
            call()
        assert ei.value.code == _abi.E_STATE
