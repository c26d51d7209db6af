"""CPU-only checks of lossy materials in the batched engine (fdtd2d_batch_lossy.h, batch.py, adjoint.py).

The surface: the two entry points are declared, exported and bound, the constant is named and its id free, the Python
surface has its shape, bad arguments are refused before any device is touched, and without a device nothing falls back.

The method: ``batch_material_gradient`` driven by the stand-in of tests/oracle_batch_lossy.py on the configuration of
test_batch_adjoint_cpu (48x48, 8-cell PML, 5000 steps, float64) with sigma random in [0, 0.5] S/m on the design window,
against central finite differences (h = 1e-4 eps0 and 1e-4 S/m) of the stand-in's own objective on that file's 8
FD_CELLS.  With loss and the PML the fields ring down (end-of-run residuals 2.6e-5 forward, 9.9e-8 adjoint), so the
adjoint is far closer to the finite differences than in the lossless case (1.6e-3).  Measured on these 8 cells, worst
error over max|gradient|:
    pml   eps 2.6e-7   sigma 2.2e-7     bound 1e-5 for both (the issue's: two decades over the finite-difference noise,
                                        four under what a wrong coefficient gives)
    mur   eps 6.2e-6   sigma 5.8e-6     bound 6e-4 for both, set the same way: two decades over the measurement (what
                                        the Mur frame reflects comes back into the sums; the frame also leaves a slowly
                                        growing near-static field behind, which the transforms at 25..55 GHz do not
                                        see but which makes info's residuals large, 0.14 and 21), and still two decades
                                        under a wrong coefficient (> 0.1).

The physics: a closed box rings down as ca^n (see test_closed_box_energy_follows_ca_to_the_n).

The session: ``AdjointSession.sigma_gradient`` against the helper's grad_sigma, 1e-9 of its maximum."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch_lossy import LossyOracle, lossy_coefficients
import test_batch_adjoint_cpu as cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_lossy.h")
NAMES = ["fdtd2d_batch_set_conductivity", "fdtd2d_batch_set_conductivity_window"]
EPS0, MU0 = cpu.EPS0, 4 * np.pi * 1e-7
R0, C0, NR, NC = cpu.DESIGN
FD_BOUND = {"pml": 1e-5, "mur": 6e-4}
H_EPS, H_SIGMA = 1e-4 * EPS0, 1e-4


def design_sigma(seed=100, count=1):
    sigma = np.zeros((count, cpu.R, cpu.C))
    for b in range(count):
        sigma[b, R0:R0 + NR, C0:C0 + NC] = 0.5 * np.random.default_rng(seed + b).random((NR, NC))
    return sigma


def gradient(fd, boundary, dtype=np.float64, eps=None, sigma=None, engine=LossyOracle, nsteps=cpu.NSTEPS, **kw):
    eps = cpu.design_eps() if eps is None else eps
    sigma = design_sigma(count=eps.shape[0]) if sigma is None else sigma
    B = eps.shape[0]
    args = dict(nsteps=nsteps, sources=np.tile(cpu.SOURCE, (B, 1)), probes=cpu.PROBES, omegas=cpu.OMEGAS,
                design=cpu.DESIGN, objective=cpu.objective, fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, dtype=dtype,
                boundary=boundary, pml_cells=cpu.LAYER, engine=engine)
    args.update(kw)
    return fd.batch_material_gradient(eps, sigma, **args)


def oracle_objective(boundary, eps, sigma):
    """J of every member from a forward run of the stand-in alone (no adjoint code involved)."""
    from fdtd2d_amd.adjoint import probe_spectra
    from fdtd2d_amd.api import ricker_amplitude
    B = eps.shape[0]
    amps = np.tile(np.array([ricker_amplitude(n * cpu.DT, cpu.FC) for n in range(cpu.NSTEPS)]), (B, 1))
    eng = LossyOracle(B, cpu.R, cpu.C, cpu.DT, cpu.DX, dtype=np.float64, boundary=boundary)
    eng.set_materials(eps, MU0)
    if boundary == "pml":
        eng.set_pml(cpu.LAYER, courant00=(1 / np.sqrt(EPS0 * MU0) * cpu.DT) / cpu.DX)
    eng.set_conductivity(sigma)
    eng.set_sources(np.tile(cpu.SOURCE, (B, 1))).set_probes(cpu.PROBES, cpu.NSTEPS)
    eng.run(cpu.NSTEPS, amps)
    return cpu.objective(probe_spectra(eng.read_probes(), np.tile(cpu.OMEGAS, (B, 1)), cpu.DT))[0]


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_batch_lossy_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_LOSSY_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_LOSSY_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_LOSSY_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "const void *": ctypes.c_void_p,
             "const int": ctypes.POINTER(ctypes.c_int)}
    for n, args in proto.items():
        got = []
        for a in args.split(","):
            a = " ".join(a.split())
            kind = re.match(r"(.*?[ *])\w+(\[4\])?$", a).group(1).strip()
            got.append(kinds[kind])
        assert got == _abi.BATCH_LOSSY_SIGNATURES[n][1], n


def test_batch_lossy_constant_is_named_and_its_id_free():
    from fdtd2d_amd import _abi
    pat = r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)"
    mine = dict(re.findall(pat, open(HEADER).read()))
    assert mine == {"BATCH_INFO_LOSSY": "14"} and _abi.BATCH_INFO_LOSSY == 14
    taken = {}
    for h in ("fdtd2d.h", "fdtd2d_batch_pml.h", "fdtd2d_batch_monitor.h", "fdtd2d_batch_adjoint.h",
              "fdtd2d_batch_design.h"):
        taken.update(re.findall(pat, open(os.path.join(ROOT, "include", h)).read()))
    assert max(int(v) for k, v in taken.items() if k.startswith("BATCH_INFO")) == 13
    assert "BATCH_INFO_LOSSY" not in taken


def test_batch_lossy_python_surface():
    import fdtd2d_amd as fd
    E, S = fd.BatchEngine, fd.AdjointSession
    assert list(inspect.signature(E.set_conductivity).parameters) == ["self", "sigma"]
    assert list(inspect.signature(E.set_conductivity_window).parameters) == ["self", "window", "sigma"]
    assert isinstance(E.lossy, property)
    p = inspect.signature(fd.batch_material_gradient).parameters
    q = inspect.signature(fd.batch_eps_gradient).parameters
    assert list(p) == ["eps", "sigma", "mu"] + [k for k in q if k not in ("eps", "mu")]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k not in ("eps", "sigma", "mu"))
    assert {k: p[k].default for k in q if k != "eps"} == {k: q[k].default for k in q if k != "eps"}
    assert "batch_material_gradient" in fd.__all__
    assert fd.batch_material_gradient is fd.adjoint.batch_material_gradient
    assert list(inspect.signature(S.set_conductivity).parameters) == ["self", "sigma"]
    assert list(inspect.signature(S.set_design_sigma).parameters) == ["self", "sigma_window"]
    assert list(inspect.signature(S.sigma_gradient).parameters) == ["self"]
    # what was there is as it was
    assert list(inspect.signature(S.set_design_eps).parameters) == ["self", "eps_window"]
    assert list(inspect.signature(E.set_eps_window).parameters) == ["self", "window", "eps"]
    for name in ("set_conductivity", "set_conductivity_window"):
        assert callable(getattr(LossyOracle, name))


def test_batch_lossy_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    w = np.array([1, 1, 2, 2], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_conductivity(None, d.ctypes.data, _abi.F64) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_conductivity_window(None, w, d.ctypes.data, _abi.F64) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_INFO_LOSSY) == _abi.E_ARG


def _sigma_with(value, at, member=1):
    s = design_sigma(count=2)
    s[(member,) + at] = value
    return s


@pytest.mark.parametrize("sigma,kwargs,match", [
    (_sigma_with(-1e-3, (20, 20)), {}, "member 1: sigma must be >= 0 and finite"),
    (_sigma_with(np.nan, (20, 20)), {}, "member 1: sigma must be >= 0 and finite"),
    (_sigma_with(np.inf, (20, 20), 0), {}, "member 0: sigma must be >= 0 and finite"),
    (-0.1, {}, "member 0: sigma must be >= 0 and finite"),
    (_sigma_with(0.1, (5, 20)), dict(boundary="mur"), r"member 1: sigma is non-zero at cell \(5, 20\), within 6 cells"),
    (_sigma_with(0.1, (20, 42)), dict(boundary="mur"), r"member 1: sigma is non-zero at cell \(20, 42\), within 6"),
    (_sigma_with(0.1, (7, 20)), {}, r"member 1: sigma is non-zero at cell \(7, 20\), within 8 cells.*PML"),
    (_sigma_with(0.1, (40, 20)), {}, r"member 1: sigma is non-zero at cell \(40, 20\), within 8 cells.*PML"),
    (_sigma_with(0.1, (22, 38)), {}, r"member 1: sigma is non-zero at the probe cell \(22, 38\)"),
    (np.zeros((2, 48, 47)), {}, r"sigma must have shape \(2, 48, 48\)"),
    (np.zeros((1, 48, 48)), {}, r"sigma must have shape \(2, 48, 48\)"),
    (design_sigma(count=2), dict(design=(5, 18, 16, 12), boundary="mur"), "6 cells from every edge"),
    (design_sigma(count=2), dict(boundary="none"), "rings down"),
])
def test_batch_material_gradient_refuses_bad_arguments_on_the_host(monkeypatch, sigma, kwargs, match):
    import fdtd2d_amd as fd

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    with pytest.raises(ValueError, match=match):
        kwargs = dict(kwargs)
        gradient(fd, kwargs.pop("boundary", "pml"), eps=cpu.design_eps(count=2), sigma=sigma, engine=None, nsteps=400,
                 **kwargs)


def test_batch_lossy_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 4, 40, 40, 5e-14, 1e-4, _abi.F32, _abi.BOUNDARY_MUR5, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        gradient(fd, "pml", np.float32, engine=None, nsteps=400)
    assert ei.value.code == _abi.E_NODEVICE
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.BatchEngine(2, 40, 40).set_conductivity(0.0)
    assert ei.value.code == _abi.E_NODEVICE


def test_zero_conductivity_leaves_the_stand_in_bit_identical():
    """ca = inv = 1 exactly, so the lossy update is the plain one; float32 and float64, Mur and PML."""
    for dtype in (np.float32, np.float64):
        ca, cb, ce = lossy_coefficients((EPS0 * np.linspace(1, 3, 7)).astype(dtype), np.zeros(7), cpu.DT, cpu.DX)
        assert np.all(ca == 1) and np.array_equal(cb, ce) and ca.dtype == cb.dtype == dtype
        for boundary in ("mur", "pml"):
            out = []
            for sigma in (None, 0.0):
                eng = LossyOracle(1, cpu.R, cpu.C, cpu.DT, cpu.DX, dtype=dtype, boundary=boundary)
                eng.set_materials(cpu.design_eps(), MU0)
                if boundary == "pml":
                    eng.set_pml(cpu.LAYER, courant00=(1 / np.sqrt(EPS0 * MU0) * cpu.DT) / cpu.DX)
                eng.set_conductivity(sigma)
                assert eng.lossy == (sigma is not None)
                eng.set_sources(np.array([cpu.SOURCE]))
                eng.run(200, np.sin(np.arange(200.0))[None])
                out.append(eng.download())
            for a, b in zip(*out):
                assert np.array_equal(a, b)


# ---- 2. the gradients against finite differences ------------------------------------------------------------------------

_cache = {}


def grad64(fd, boundary):
    if boundary not in _cache:
        _cache[boundary] = gradient(fd, boundary)
    return _cache[boundary]


@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_material_gradients_match_finite_differences_of_the_oracle(fd, boundary):
    """Measured: pml eps 2.6e-7, sigma 2.2e-7 (bound 1e-5); mur eps 6.2e-6, sigma 5.8e-6 (bound 6e-4, see the module
    docstring) of max|gradient|."""
    J, geps, gsig, spectra, info = grad64(fd, boundary)
    assert geps.shape == gsig.shape == (1, NR, NC) and spectra.shape == (1, 8, 3) and J.shape == (1,)
    n = len(cpu.FD_CELLS)
    eps, sigma = np.repeat(cpu.design_eps(), 4 * n, axis=0), np.repeat(design_sigma(), 4 * n, axis=0)
    for k, (r, c) in enumerate(cpu.FD_CELLS):
        eps[4 * k, r, c] += H_EPS
        eps[4 * k + 1, r, c] -= H_EPS
        sigma[4 * k + 2, r, c] += H_SIGMA
        sigma[4 * k + 3, r, c] -= H_SIGMA
    Jp = oracle_objective(boundary, eps, sigma)
    assert np.array_equal(oracle_objective(boundary, cpu.design_eps(), design_sigma()), J)
    at = lambda g: np.array([g[0, r - R0, c - C0] for r, c in cpu.FD_CELLS])
    err_eps = np.abs(at(geps) - (Jp[0::4] - Jp[1::4]) / (2 * H_EPS)).max() / np.abs(geps[0]).max()
    err_sig = np.abs(at(gsig) - (Jp[2::4] - Jp[3::4]) / (2 * H_SIGMA)).max() / np.abs(gsig[0]).max()
    print(f"{boundary}: adjoint vs central FD on {n} cells, worst / max|gradient|: eps {err_eps:.3e}, sigma "
          f"{err_sig:.3e}; residuals {info['residual_forward'][0]:.2e} {info['residual_adjoint'][0]:.2e}")
    assert err_eps <= FD_BOUND[boundary]
    assert err_sig <= FD_BOUND[boundary]


def test_a_wrong_coefficient_is_far_outside_the_bound(fd):
    """The eps coefficient used for sigma is off by more than 0.1 of max|gradient|."""
    from fdtd2d_amd.adjoint import gradient_coefficients, sigma_coefficients
    a, b = gradient_coefficients(cpu.OMEGAS, cpu.DT), sigma_coefficients(cpu.OMEGAS, cpu.DT)
    assert np.abs(a - b).max() / np.abs(b).max() > 0.1
    z = np.exp(1j * cpu.OMEGAS * cpu.DT)
    assert np.allclose(b * (z - 1), -(z - 1 / z), rtol=1e-12, atol=0)     # G's factor over the source's (z - 1)


# ---- 3. the physics ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_closed_box_energy_follows_ca_to_the_n(dtype):
    """Closed box, 40x40, uniform eps_r = 2, sigma = 0.05 S/m, dx = 1e-3, dt = 1.6e-12, from a Gaussian blob with zero
    edges.  Every underdamped mode of the lossy leapfrog has |z|^2 = ca exactly, so the leapfrog energy
    W_n = sum eps Ez_n^2 + mu sum H_(n-1/2) H_(n+1/2) follows ca^n; the bound is +-1 % at 500 and 1000 steps.
    The blob: a mode of angle theta per step leaves an oscillation of relative size s / theta in W_n / ca^n
    (s = sigma dt / (2 eps) = 2.3e-3 here), which is what the nearly static modes contribute.  A blob of standard
    deviation 1.5 cells has its spectrum around 0.67 rad per cell, theta = 0.23 per step at this Courant number (0.34),
    where s / theta is 1 %; the sum over modes averages well below that.  Measured W_n / W_0 over ca^n with it: 1.0009
    at step 500, 0.9972 at 1000, 1.0023 at 3000, the same in float32 and float64.  A blob of standard deviation 5 cells
    reaches 0.969 at step 1000: that is the slow modes' oscillation, not a wrong decay rate."""
    n, dx, dt, sigma = 40, 1e-3, 1.6e-12, 0.05
    eng = LossyOracle(1, n, n, dt, dx, dtype=dtype, boundary="none")
    eng.set_materials(2 * EPS0, MU0).set_conductivity(sigma)
    ii, jj = np.mgrid[0:n, 0:n]
    blob = np.exp(-((ii - 19.5) ** 2 + (jj - 19.5) ** 2) / (2 * 1.5 ** 2))
    blob[0, :] = blob[-1, :] = blob[:, 0] = blob[:, -1] = 0
    eng.upload(Ez=blob[None])
    eps, mu = 2 * EPS0, MU0
    s = sigma * dt / (2 * float(dtype(eps)))
    ca = float(dtype((1 - s) / (1 + s)))

    def energy():
        """W of the current Ez: H before and after the next H half-step (a scratch copy takes it)."""
        Ez, Hx, Hy = (a[0].astype(np.float64) for a in eng.download())
        ch = dt / (mu * dx)
        Hx2, Hy2 = Hx.copy(), Hy.copy()
        Hx2[:-1, :] -= ch * (Ez[1:, :-1] - Ez[:-1, :-1])
        Hy2[:, :-1] += ch * (Ez[:-1, 1:] - Ez[:-1, :-1])
        return eps * np.sum(Ez ** 2) + mu * (np.sum(Hx * Hx2) + np.sum(Hy * Hy2))
    W0 = energy()
    done = 0
    for step in (500, 1000, 3000):
        eng.run(step - done)
        done = step
        ratio = energy() / W0 / ca ** step
        print(f"{np.dtype(dtype).name}: W_{step} / W_0 over ca^{step} = {ratio:.4f}")
        assert step > 1000 or abs(ratio - 1) <= 0.01


# ---- 4. the session ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_session_sigma_gradient_is_the_helpers(fd, boundary):
    """sigma_gradient() equals the helper's grad_sigma to 1e-9 of its maximum before and after set_design_sigma and
    set_design_eps (and value_and_grad the helper's grad_eps, as the lossless session does)."""
    nsteps = 2500
    eps, sigma = cpu.design_eps(count=2), design_sigma(count=2)
    B = 2
    args = dict(nsteps=nsteps, sources=np.tile(cpu.SOURCE, (B, 1)), probes=cpu.PROBES, omegas=cpu.OMEGAS,
                design=cpu.DESIGN, fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, dtype=np.float64, boundary=boundary,
                pml_cells=cpu.LAYER, engine=LossyOracle)

    def agree(s, eps, sigma):
        want = gradient(fd, boundary, eps=eps, sigma=sigma, nsteps=nsteps)
        J, g, sp, _ = s.value_and_grad(cpu.objective)
        gs = s.sigma_gradient()
        assert gs.shape == want[2].shape and gs.dtype == np.float64
        for m in range(B):
            assert np.abs(gs[m] - want[2][m]).max() <= 1e-9 * np.abs(want[2][m]).max(), m
            assert np.abs(g[m] - want[1][m]).max() <= 1e-9 * np.abs(want[1][m]).max(), m
        assert np.allclose(J, want[0], rtol=1e-12, atol=0)
        assert np.array_equal(s.sigma_gradient(), gs)          # asking again changes nothing
        return gs

    with fd.AdjointSession(eps, **args) as s:
        with pytest.raises(RuntimeError, match="value_and_grad first"):
            s.sigma_gradient()
        assert s.sigma is None and s.set_conductivity(sigma) is s
        assert np.array_equal(s.sigma, sigma) and not s.sigma.flags.writeable and s.engine.lossy
        g0 = agree(s, eps, sigma)
        new = 0.5 * np.random.default_rng(5).random((B, NR, NC))
        assert s.set_design_sigma(new) is s
        sigma2 = sigma.copy()
        sigma2[:, R0:R0 + NR, C0:C0 + NC] = new
        assert np.array_equal(s.sigma, sigma2) and np.array_equal(sigma, design_sigma(count=2))
        g1 = agree(s, eps, sigma2)
        assert not np.allclose(g1, g0, rtol=1e-3)
        new_eps = EPS0 * (1 + 2 * np.random.default_rng(7).random((B, NR, NC)))
        s.set_design_eps(new_eps)
        eps2 = eps.copy()
        eps2[:, R0:R0 + NR, C0:C0 + NC] = new_eps
        agree(s, eps2, sigma2)
        # refusals leave the state
        bad = new.copy()
        bad[1, 2, 3] = -1.0
        with pytest.raises(ValueError, match="member 1: sigma must be >= 0"):
            s.set_design_sigma(bad)
        with pytest.raises(ValueError, match=r"shape \(2, 16, 12\)"):
            s.set_design_sigma(new[:, 1:])
        assert np.array_equal(s.sigma, sigma2) and np.array_equal(s.engine.sigma, sigma2)
        s.set_conductivity(None)
        assert s.sigma is None and not s.engine.lossy
