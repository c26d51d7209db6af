"""CPU-only checks of periodic columns in the batched engine (fdtd2d_batch_periodic.h, batch.py, adjoint.py).

The surface: the entry point is declared, exported and bound, the constant is named and its id free, the pinned
parameter lists are as they were, ``boundary="periodic"`` is accepted, bad arguments are refused on the host.

The stand-in (tests/oracle_batch_periodic.py) has three exact properties, float32 and float64 (64 rows, Q = 20, a
10-cell layer, dt 1.6e-13, dx 1e-4, Ricker 150 GHz, 400 steps, eps_r random in [1, 4] on rows 20..39):
a period-Q member equals both halves of a period-2Q member with two copies of materials and sources; shifting materials
and source cyclically by 7 columns shifts the fields; column-uniform materials under a full-width line source keep every
column equal to column 0 and Hy at zero.  All three with ``np.array_equal``.

The physics: the transmission of a 20-cell slab of index 2 under normal incidence against the Airy formula, at 40..80
GHz (240 x 9, 20-cell layer, 6000 steps).  Measured: worst error 0.0073 in float32 and float64 (the grid's numerical
dispersion at 15-30 cells per wavelength in the slab); the bound is 0.015, twice that, and covers only a differently
rounded restatement since the run is deterministic NumPy.  PEC side walls in place of the wrap are a parallel-plate
guide below cut-off for Ez constant across it: they miss the bound by far (asserted).

The gradients: ``batch_material_gradient(boundary="periodic")`` driven by the stand-in against central finite
differences of the stand-in's own objective J = sum_k |sum_p X[p, k]|^2 (B = 2, 64 x 17, 8-cell layer, dt 4e-13, dx
2.5e-4, eps_r in [1, 3] and sigma in [0.2, 0.7] S/m on the design window (24, 0, 12, 16), which spans the whole period,
sources (14, 0, 1, 16) and (14, 3, 1, 4), 16 probes on row 50, 25 / 40 / 55 GHz, 5000 steps, float64) on eight cells
that include columns 0 and 15.  Bound 1e-5 of max|gradient| for both, the project's lossy PML bound; the measured values
are printed and in the test's docstring.  The design region conducts because a lossless high-index periodic layer traps
guided modes that never reach the layer on the rows (see batch_eps_gradient's docstring).

The session: ``AdjointSession(boundary="periodic")`` against the helper, 1e-9 of max|gradient|."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch_periodic import PeriodicOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_periodic.h")
NAMES = ["fdtd2d_batch_set_periodic"]
EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7
C0 = 1 / np.sqrt(EPS0 * MU0)


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def ricker(nsteps, dt, fc):
    from fdtd2d_amd.api import ricker_amplitude
    return np.array([ricker_amplitude(n * dt, fc) for n in range(nsteps)])


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_batch_periodic_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_PERIODIC_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_PERIODIC_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_PERIODIC_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_PERIODIC_SIGNATURES[n][1], n


def test_batch_periodic_constant_is_named_and_its_id_free():
    from fdtd2d_amd import _abi
    pat = r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)"
    mine = dict(re.findall(pat, open(HEADER).read()))
    assert mine == {"BATCH_INFO_PERIODIC": "15"} and _abi.BATCH_INFO_PERIODIC == 15
    taken = {}
    for h in ("fdtd2d.h", "fdtd2d_batch_pml.h", "fdtd2d_batch_monitor.h", "fdtd2d_batch_adjoint.h",
              "fdtd2d_batch_design.h", "fdtd2d_batch_lossy.h"):
        taken.update(re.findall(pat, open(os.path.join(ROOT, "include", h)).read()))
    assert max(int(v) for k, v in taken.items() if k.startswith("BATCH_INFO")) == 14
    assert "BATCH_INFO_PERIODIC" not in taken


def test_pinned_parameter_lists_are_unchanged(fd):
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(fd.BatchEngine.__init__) == ["self", "count", "rows", "cols", "dt", "dx", "dtype", "boundary", "device"]
    assert sig(fd.BatchEngine.set_pml) == ["self", "L", "m", "R0", "courant00", "profiles"]
    grad = ["eps", "mu", "nsteps", "sources", "probes", "omegas", "design", "objective", "fc", "waveform", "dt", "dx",
            "dtype", "boundary", "pml_cells", "device", "engine"]
    assert sig(fd.batch_eps_gradient) == grad
    assert sig(fd.batch_material_gradient) == ["eps", "sigma"] + grad[1:]
    assert sig(fd.AdjointSession.__init__) == ["self"] + [k for k in grad if k != "objective"]
    assert isinstance(fd.BatchEngine.periodic, property)
    assert inspect.signature(fd.run_fdtd_batch).parameters["boundary"].default == "mur"


def test_boundary_periodic_is_accepted(fd):
    """BatchEngine takes boundary="periodic": with a device it is a periodic batch, without one the library's own
    refusal (there is no CPU path), never a ValueError for an unknown boundary."""
    from fdtd2d_amd import _abi
    try:
        eng = fd.BatchEngine(2, 40, 21, boundary="periodic")
    except fd.Fdtd2dError as e:
        assert e.code == _abi.E_NODEVICE
    else:
        with eng:
            assert eng.periodic and eng.boundary == "periodic"
    with pytest.raises(ValueError, match="unknown boundary"):
        fd.BatchEngine(2, 40, 21, boundary="bloch")
    with pytest.raises(ValueError, match="BatchEngine alone"):
        fd.Engine(64, 64, boundary="periodic")
    lib = _abi.load()
    assert lib.fdtd2d_batch_set_periodic(None, 1) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_INFO_PERIODIC) == _abi.E_ARG
    # the fit rule is one of rows alone: the 64 x 17 member of the gradient test takes an 8-cell layer
    assert not fd.batch.pml_fits(64, 17, 8) and fd.batch.pml_fits(64, 17, 8, periodic=True)
    assert fd.batch.pml_fits(64, 17, 30, periodic=True) and not fd.batch.pml_fits(64, 17, 31, periodic=True)


# ---- 2. exact properties of the stand-in ----------------------------------------------------------------------------

ROWS, Q, LAYER, DT, DX, FC, NSTEPS = 64, 20, 10, 1.6e-13, 1e-4, 150e9, 400


def slab_eps(seed=1):
    """(64, Q + 1): eps_r random in [1, 4] on rows 20..39, the image column equal to column 0."""
    eps = np.full((ROWS, Q + 1), EPS0)
    eps[20:40, :Q] = EPS0 * (1 + 3 * np.random.default_rng(seed).random((20, Q)))
    eps[:, Q] = eps[:, 0]
    return eps


def run_member(engine, dtype, eps, rect=None, points=None, nsteps=NSTEPS, layer=LAYER, **kw):
    """One member on `engine` (the stand-in, or the device engine in tests/test_gpu_batch_periodic.py)."""
    R, Cc = eps.shape
    with engine(1, R, Cc, DT, DX, dtype=dtype, boundary="periodic", **kw) as eng:
        eng.set_materials(eps[None], MU0)
        if layer:
            eng.set_pml(layer, courant00=C0 * DT / DX)
        amps = ricker(nsteps, DT, FC)
        if rect is not None:
            eng.set_sources(np.array([rect]))
        if points is not None:
            eng.set_point_sources(np.array(points), np.ones((len(points), 1)))
            eng.run(nsteps, amps[None] if rect is not None else None, amps[None])
        else:
            eng.run(nsteps, amps[None])
        return [a[0] for a in eng.download()]


def check_supercell(engine, dtype, **kw):
    eps = slab_eps()
    eps2 = np.concatenate([eps[:, :Q], eps[:, :Q], eps[:, :1]], axis=1)
    Ez, Hx, Hy = run_member(engine, dtype, eps, points=[(15, 5), (30, 0)], **kw)
    Ez2, Hx2, Hy2 = run_member(engine, dtype, eps2, points=[(15, 5), (30, 0), (15, 5 + Q), (30, Q)], **kw)
    assert np.abs(Ez).max() > 0 and np.abs(Hy[:, :Q]).max() > 0
    assert np.array_equal(Ez2[:, :Q + 1], Ez) and np.array_equal(Ez2[:, Q:], Ez)
    assert np.array_equal(Hy2[:, :Q], Hy[:, :Q]) and np.array_equal(Hy2[:, Q:2 * Q], Hy[:, :Q])
    assert np.array_equal(Hx2[:, :Q], Hx) and np.array_equal(Hx2[:, Q:], Hx)


def check_cyclic_shift(engine, dtype, **kw):
    eps = slab_eps()
    shifted = np.roll(eps[:, :Q], 7, axis=1)
    shifted = np.concatenate([shifted, shifted[:, :1]], axis=1)
    Ez, Hx, Hy = run_member(engine, dtype, eps, rect=(15, 5, 1, 3), **kw)
    Ez_s, Hx_s, Hy_s = run_member(engine, dtype, shifted, rect=(15, 12, 1, 3), **kw)
    assert np.abs(Ez).max() > 0
    assert np.array_equal(Ez_s[:, :Q], np.roll(Ez[:, :Q], 7, axis=1)) and np.array_equal(Ez_s[:, Q], Ez_s[:, 0])
    assert np.array_equal(Hy_s[:, :Q], np.roll(Hy[:, :Q], 7, axis=1))
    assert np.array_equal(Hx_s, np.roll(Hx, 7, axis=1))


def check_column_invariance(engine, dtype, **kw):
    eps = np.repeat(slab_eps()[:, :1], Q + 1, axis=1)
    Ez, Hx, Hy = run_member(engine, dtype, eps, rect=(15, 0, 1, Q), **kw)
    assert np.abs(Ez).max() > 0
    assert np.array_equal(Ez, np.repeat(Ez[:, :1], Q + 1, axis=1))
    assert not Hy.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_period_equals_both_halves_of_a_double_period(dtype):
    check_supercell(PeriodicOracle, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_cyclic_shift_of_materials_and_source_shifts_the_fields(dtype):
    check_cyclic_shift(PeriodicOracle, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_column_uniform_members_stay_column_uniform(dtype):
    check_column_invariance(PeriodicOracle, dtype)


def test_the_stand_in_without_conductivity_or_layer_is_the_plain_update():
    """ca = 1 and cb = ce without a conductivity, unit factors without a layer: away from the wrap the periodic step is
    the reference's own (oracle/fdtd_numpy), bit for bit, until the wrap's influence arrives."""
    from oracle import fdtd_numpy as onp
    eps = np.full((40, 41), EPS0)
    eps[10:20, 5:30] *= 3
    mu = np.full(eps.shape, MU0)
    with PeriodicOracle(1, 40, 41, DT, DX, dtype=np.float32) as eng:
        eng.set_materials(eps[None], MU0).set_sources(np.array([(20, 20, 1, 1)]))
        eng.run(12, ricker(12, DT, FC)[None])
        got = eng.download()[0][0]
    ref = onp.grid_zeros(40, 41, np.float32)
    for n in range(12):
        onp.update_h(*ref, mu.astype(np.float32), eps.astype(np.float32), DT, DX)
        ref[0][1:-1, 1:-1] += ((ref[2][1:, 1:-1] - ref[2][1:, :-2]) - (ref[1][1:-1, 1:] - ref[1][:-2, 1:])) * \
            (DT / (eps.astype(np.float32)[1:-1, 1:-1] * DX))
        ref[0][20, 20] = np.float32(np.float64(ref[0][20, 20]) + ricker(12, DT, FC)[n])
    assert np.abs(got).max() > 0 and np.array_equal(got[:, 1:-1], ref[0][:, 1:-1])


# ---- 3. the physics: a slab's transmission against the Airy formula --------------------------------------------------

AIRY_FREQS = np.array([40e9, 50e9, 60e9, 70e9, 80e9])
AIRY_BOUND = 0.015


def airy(f, d=20 * 1e-4, n=2.0):
    """|t| of a slab of index n and thickness d in vacuum under normal incidence."""
    r2 = ((n - 1) / (n + 1)) ** 2
    return (1 - r2) / np.abs(1 - r2 * np.exp(2j * (2 * np.pi * f / C0) * n * d))


def transmission(dtype, engine=PeriodicOracle):
    from fdtd2d_amd.adjoint import probe_spectra
    R, Cc, L, n = 240, 9, 20, 6000
    X = []
    for slab in (True, False):
        eps = np.full((1, R, Cc), EPS0)
        if slab:
            eps[:, 110:130] *= 4
        with engine(1, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as eng:
            eng.set_materials(eps, MU0).set_pml(L, courant00=C0 * DT / DX)
            eng.set_sources(np.array([(40, 0, 1, 8)])).set_probes(np.array([(200, 3)]), n)
            eng.run(n, ricker(n, DT, 80e9)[None])
            X.append(probe_spectra(eng.read_probes(), 2 * np.pi * AIRY_FREQS[None], DT)[0, 0])
    return np.abs(X[0] / X[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_slab_transmission_matches_the_airy_formula(dtype):
    """Measured: worst |T_fdtd - T_airy| 0.0073 over 40..80 GHz (at 80 GHz), float32 and float64; bound 0.015."""
    T = transmission(dtype)
    err = np.abs(T - airy(AIRY_FREQS))
    print(f"{np.dtype(dtype).name}: |T| {np.round(T, 4)} airy {np.round(airy(AIRY_FREQS), 4)} worst error {err.max():.4f}")
    assert err.max() <= AIRY_BOUND


def test_pec_side_walls_miss_the_airy_bound_by_far():
    """The same slab in a closed-sided member (the lossy PML stand-in with unit column factors: PEC columns 0 and C-1)."""
    from fdtd2d_amd.adjoint import probe_spectra
    from oracle_batch_lossy import LossyOracle
    from oracle_batch_periodic import row_profiles
    R, Cc, L, n = 240, 9, 20, 6000
    X = []
    for slab in (True, False):
        eps = np.full((1, R, Cc), EPS0)
        if slab:
            eps[:, 110:130] *= 4
        eng = LossyOracle(1, R, Cc, DT, DX, dtype=np.float64, boundary="pml")
        eng.set_materials(eps, MU0)
        P = row_profiles(R, C0 * DT / DX, L)
        one = np.ones(Cc)
        P.update(aec=one, bec=one, ahc=one, bhc=one, in_c=np.zeros(Cc, bool))
        eng.profiles = [P]
        eng.set_sources(np.array([(40, 1, 1, 7)])).set_probes(np.array([(200, 3)]), n)
        eng.run(n, ricker(n, DT, 80e9)[None])
        X.append(probe_spectra(eng.read_probes(), 2 * np.pi * AIRY_FREQS[None], DT)[0, 0])
    err = np.abs(np.abs(X[0] / X[1]) - airy(AIRY_FREQS)).max()
    print(f"PEC side walls: worst error {err:.3f}")
    assert err > 10 * AIRY_BOUND


# ---- 4. the gradients against finite differences ----------------------------------------------------------------------

G_R, G_C, G_L, G_DT, G_DX, G_FC, G_NSTEPS = 64, 17, 8, 4e-13, 2.5e-4, 40e9, 5000
G_DESIGN = (24, 0, 12, 16)
G_SOURCES = np.array([(14, 0, 1, 16), (14, 3, 1, 4)])
G_PROBES = np.array([(50, c) for c in range(16)])
G_OMEGAS = 2 * np.pi * np.array([25e9, 40e9, 55e9])
G_CELLS = [(24, 0), (35, 15), (24, 15), (35, 0), (28, 7), (30, 3), (26, 12), (33, 9)]
G_BOUND = 1e-5
H_EPS, H_SIGMA = 1e-4 * EPS0, 1e-4


def g_materials(count=2, seed=3):
    """eps_r in [1, 3] and sigma in [0.2, 0.7] S/m on the design window, the image column equal to column 0."""
    rng = np.random.default_rng(seed)
    r0, c0, nr, nc = G_DESIGN
    eps, sigma = np.full((count, G_R, G_C), EPS0), np.zeros((count, G_R, G_C))
    eps[:, r0:r0 + nr, c0:c0 + nc] = EPS0 * (1 + 2 * rng.random((count, nr, nc)))
    sigma[:, r0:r0 + nr, c0:c0 + nc] = 0.2 + 0.5 * rng.random((count, nr, nc))
    eps[:, :, -1], sigma[:, :, -1] = eps[:, :, 0], sigma[:, :, 0]
    return eps, sigma


def g_sources(count):
    return np.tile(G_SOURCES, ((count + 1) // 2, 1))[:count]


def g_objective(spectra):
    """J = sum_k |sum_p X[p, k]|^2 and its cotangent g = dJ/dRe + i dJ/dIm = 2 sum_p X[p, k] at every probe."""
    S = spectra.sum(axis=1)
    return (np.abs(S) ** 2).sum(axis=1), np.repeat(2 * S[:, None, :], spectra.shape[1], axis=1)


def g_args(count, engine=PeriodicOracle, nsteps=G_NSTEPS, dtype=np.float64, **kw):
    args = dict(nsteps=nsteps, sources=g_sources(count), probes=G_PROBES, omegas=G_OMEGAS, design=G_DESIGN, fc=G_FC,
                dt=G_DT, dx=G_DX, dtype=dtype, boundary="periodic", pml_cells=G_L, engine=engine)
    args.update(kw)
    return args


def g_gradient(fd, eps=None, sigma=None, **kw):
    e, s = g_materials()
    eps, sigma = e if eps is None else eps, s if sigma is None else sigma
    return fd.batch_material_gradient(eps, sigma, objective=g_objective, **g_args(eps.shape[0], **kw))


def g_forward_objective(eps, sigma, sources):
    """J of every member from a forward run of the stand-in alone (no adjoint code involved)."""
    from fdtd2d_amd.adjoint import probe_spectra
    B = eps.shape[0]
    eng = PeriodicOracle(B, G_R, G_C, G_DT, G_DX, dtype=np.float64)
    eng.set_materials(eps, MU0).set_pml(G_L, courant00=C0 * G_DT / G_DX)
    eng.set_conductivity(sigma)
    eng.set_sources(sources).set_probes(G_PROBES, G_NSTEPS)
    eng.run(G_NSTEPS, np.tile(ricker(G_NSTEPS, G_DT, G_FC), (B, 1)))
    return g_objective(probe_spectra(eng.read_probes(), np.tile(G_OMEGAS, (B, 1)), G_DT))[0]


def test_periodic_gradients_match_finite_differences_of_the_oracle(fd):
    """Adjoint against central finite differences on eight cells of both members, worst error over max|gradient|.
    Measured: eps 2.1e-7 and 1.4e-7, sigma 5.9e-9 and 6.2e-9 (members 0 and 1); residuals at most 4.6e-5 (forward) and
    1.4e-9 (adjoint); bound 1e-5 for both."""
    J, geps, gsig, spectra, info = g_gradient(fd)
    r0, c0, nr, nc = G_DESIGN
    assert geps.shape == gsig.shape == (2, nr, nc) and spectra.shape == (2, 16, 3) and J.shape == (2,)
    eps0, sigma0 = g_materials()
    assert np.array_equal(g_forward_objective(eps0, sigma0, G_SOURCES), J)
    for b in range(2):
        n = len(G_CELLS)
        eps, sigma = np.repeat(eps0[b:b + 1], 4 * n, axis=0), np.repeat(sigma0[b:b + 1], 4 * n, axis=0)
        for k, (r, c) in enumerate(G_CELLS):
            cols = [c, G_C - 1] if c == 0 else [c]          # column 0 and its image move together
            eps[4 * k, r, cols] += H_EPS
            eps[4 * k + 1, r, cols] -= H_EPS
            sigma[4 * k + 2, r, cols] += H_SIGMA
            sigma[4 * k + 3, r, cols] -= H_SIGMA
        Jp = g_forward_objective(eps, sigma, np.tile(G_SOURCES[b], (4 * n, 1)))
        at = lambda g: np.array([g[b, r - r0, c - c0] for r, c in G_CELLS])
        err_eps = np.abs(at(geps) - (Jp[0::4] - Jp[1::4]) / (2 * H_EPS)).max() / np.abs(geps[b]).max()
        err_sig = np.abs(at(gsig) - (Jp[2::4] - Jp[3::4]) / (2 * H_SIGMA)).max() / np.abs(gsig[b]).max()
        print(f"member {b}: adjoint vs central FD on {n} cells, worst / max|gradient|: eps {err_eps:.3e}, sigma "
              f"{err_sig:.3e}; residuals {info['residual_forward'][b]:.2e} {info['residual_adjoint'][b]:.2e}")
        assert err_eps <= G_BOUND
        assert err_sig <= G_BOUND


# ---- 5. the session ----------------------------------------------------------------------------------------------------

def test_periodic_session_is_the_helper(fd):
    """AdjointSession(boundary="periodic") against batch_material_gradient over two iterations with a set_design_eps
    and a set_design_sigma between them: 1e-9 of max|gradient| for both gradients."""
    nsteps = 2500
    eps, sigma = g_materials()
    r0, c0, nr, nc = G_DESIGN

    def agree(s, eps, sigma):
        want = g_gradient(fd, eps=eps, sigma=sigma, nsteps=nsteps)
        J, g, sp, _ = s.value_and_grad(g_objective)
        gs = s.sigma_gradient()
        for m in range(2):
            assert np.abs(g[m] - want[1][m]).max() <= 1e-9 * np.abs(want[1][m]).max(), m
            assert np.abs(gs[m] - want[2][m]).max() <= 1e-9 * np.abs(want[2][m]).max(), m
        assert np.allclose(J, want[0], rtol=1e-12, atol=0)
        return g

    with fd.AdjointSession(eps, **g_args(2, nsteps=nsteps)) as s:
        assert s.engine.periodic and s.set_conductivity(sigma) is s
        g0 = agree(s, eps, sigma)
        rng = np.random.default_rng(11)
        new_eps = EPS0 * (1 + 2 * rng.random((2, nr, nc)))
        new_sigma = 0.2 + 0.5 * rng.random((2, nr, nc))
        s.set_design_eps(new_eps)
        s.set_design_sigma(new_sigma)
        eps2, sigma2 = eps.copy(), sigma.copy()
        eps2[:, r0:r0 + nr, c0:c0 + nc] = new_eps
        sigma2[:, r0:r0 + nr, c0:c0 + nc] = new_sigma
        g1 = agree(s, eps2, sigma2)
        assert not np.allclose(g1, g0, rtol=1e-3)


# ---- 6. host refusals ----------------------------------------------------------------------------------------------------

def _with(a, at, value):
    a = a.copy()
    a[at] = value
    return a


@pytest.mark.parametrize("change,match", [
    (dict(sources=np.array([(14, 0, 1, 16), (14, 3, 1, 14)])), r"member 1: the source \(14, 3, 1, 14\) reaches column 16"),
    (dict(probes=np.array([(50, c) for c in range(1, 17)])), r"member 0: a probe cell lies in column 16"),
    (dict(design=(24, 0, 12, 17)), r"member 0 \(and every other\): design window \(24, 0, 12, 17\) must lie in columns"),
    (dict(design=(7, 0, 12, 16)), r"member 0 \(and every other\): design window .* must keep 8 rows"),
    (dict(sigma_at=((1, 5, 3), 0.1)), r"member 1: sigma is non-zero at cell \(5, 3\), within 8 cells"),
    (dict(sigma_at=((1, 57, 0), 0.1)), r"member 1: sigma is non-zero at cell \(57, 0\), within 8 cells"),
    (dict(pml_cells=31), r"member 0 \(and every other\): a 31-cell PML does not fit the rows"),
])
def test_periodic_gradient_refuses_bad_arguments_on_the_host(monkeypatch, fd, change, match):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    eps, sigma = g_materials()
    change = dict(change)
    if "sigma_at" in change:
        at, v = change.pop("sigma_at")
        sigma = _with(sigma, at, v)
    with pytest.raises(ValueError, match=match):
        g_gradient(fd, eps=eps, sigma=sigma, engine=None, nsteps=400, **change)


def test_sigma_in_the_image_column_and_over_the_whole_period_is_accepted(fd):
    """No column margin: a conductivity in columns 0 and C-2 passes the host check, and so does one in column C-1,
    which is never read."""
    from fdtd2d_amd.adjoint import _check_sigma, _plan
    eps, sigma = g_materials()
    a = g_args(2)
    p = _plan(eps, None, a["nsteps"], a["sources"], a["probes"], a["omegas"], a["design"], a["fc"], "ricker", a["dt"],
              a["dx"], "periodic", a["pml_cells"])
    assert p.periodic and p.margin == 8 and p.win == G_DESIGN
    s = _check_sigma(p, _with(sigma, (0, 30, 16), 0.4))
    assert s[0, 30, 16] == 0.4 and s[0, 30, 0] > 0 and s[0, 30, 15] > 0
    with pytest.raises(ValueError, match=r"member 0: sigma is non-zero at the probe cell \(50, 0\)"):
        _check_sigma(p, 0.3)            # a scalar fills every column of the rows outside the margin, row 50 included
