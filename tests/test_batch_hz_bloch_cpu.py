"""CPU-only checks of the Bloch phase of the Hz polarisation (fdtd2d_batch_hz_bloch.h, batch.py): the stand-in
(tests/oracle_batch_hz_bloch.py) against code that already exists, plus the surface and the host refusals.

1. Surface.  The header's symbols are declared, exported by both libraries and bound with the _abi signatures; the info
   id is named and was free; fdtd2d.h is untouched.
2. Supercells.  A complex field that repeats as F(x + Q) = F(x) e^{i phi} with phi = 2 pi m / N is periodic over N
   periods, and its parts are two real fields of an N-period supercell driven, period n, with cos(phi n) and sin(phi n)
   times the source.  So the Hz Bloch member (one period, a one-cell rectangle source) runs against ``HzPeriodicOracle``
   members of N periods with one unit-channel Hz point source per period.  rho = (1, 0), (-1, 0) and (0, 1) agree bit for
   bit, in both dtypes, over all eight fields (Hz, Ex, Ey, Hzx, Jx, Qx, Jy, Qy); N = 3 and 5 agree to rounding.
   Shapes: 40 rows, Q = 12, an 8-cell layer, dt 1.6e-13, dx 1e-4, Ricker 150 GHz, 300 steps; eps_r, mu_r random in
   [1, 4] and [1, 2], sigma random in [0, 2] S/m and wp2 random in [0, 4e25] on rows 16..23, gamma 1e12, omega0 2 pi 1e11.
3. Duality.  Without sigma and without a pole the stand-in equals ``BlochOracle`` with eps and mu exchanged and E negated
   (identity (b)); wp2 = 0 with zero state equals no pole (identity (c)).
4. Brewster's angle: a dielectric slab passes the in-plane polarisation at Brewster incidence and reflects the other.
5. Host refusals on an engine without a library.

``tests/test_gpu_batch_hz_bloch.py`` pins the device to the stand-in."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle_batch_bloch import BlochOracle
from oracle_batch_hz import HzPeriodicOracle
from oracle_batch_hz_bloch import HzBlochOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_hz_bloch.h")
NAMES = ["fdtd2d_batch_read_dft_window_hz_bloch", "fdtd2d_batch_read_probes_hz_bloch", "fdtd2d_batch_run_hz_bloch",
         "fdtd2d_batch_set_hz_bloch", "fdtd2d_batch_set_hz_bloch_source", "fdtd2d_batch_transfer_hz_bloch",
         "fdtd2d_batch_transfer_hz_bloch_dispersion"]
EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7
C0 = 1 / np.sqrt(EPS0 * MU0)
ROWS, Q, LAYER, DT, DX, FC, NSTEPS = 40, 12, 8, 1.6e-13, 1e-4, 150e9, 300
SRC = (12, 4)                 # the source cell of period 0
GAMMA, OMEGA0 = 1e12, 2 * np.pi * 1e11


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def ricker(nsteps, dt, fc):
    from fdtd2d_amd.api import ricker_amplitude
    return np.array([ricker_amplitude(n * dt, fc) for n in range(nsteps)])


def materials(seed=5, lossy=True):
    """(eps, mu, sigma, wp2) of one period, (ROWS, Q + 1), the image column equal to column 0."""
    rng = np.random.default_rng(seed)
    eps, mu = np.full((ROWS, Q + 1), EPS0), np.full((ROWS, Q + 1), MU0)
    sigma, wp2 = np.zeros((ROWS, Q + 1)), np.zeros((ROWS, Q + 1))
    eps[16:24, :Q] = EPS0 * (1 + 3 * rng.random((8, Q)))
    mu[16:24, :Q] = MU0 * (1 + rng.random((8, Q)))
    if lossy:
        sigma[16:24, :Q] = 2 * rng.random((8, Q))
        wp2[16:24, :Q] = 4e25 * rng.random((8, Q))
    for a in (eps, mu, sigma, wp2):
        a[:, Q] = a[:, 0]
    return eps, mu, sigma, wp2


def tiled(a, n):
    """n periods of a one-period array and the image column."""
    return np.concatenate([a[:, :Q]] * n + [a[:, :1]], axis=1)


def fields(eng):
    """The eight fields of member 0: Hz, Ex, Ey, Hzx, Jx, Qx, Jy, Qy."""
    return [a[0] for a in eng.download()] + [eng.download_ezx()[0]] + [a[0] for a in eng.download_dispersion()]


def run_bloch(engine, dtype, phi=None, rotation=None, nsteps=NSTEPS, **kw):
    """The Hz Bloch member on `engine` (the stand-in, or the device engine): the eight complex fields."""
    eps, mu, sigma, wp2 = materials()
    with engine(1, ROWS, Q + 1, DT, DX, dtype=dtype, boundary="periodic", **kw) as eng:
        if hasattr(eng, "set_polarization"):
            eng.set_polarization("hz")
        eng.set_materials(eps[None], mu[None])
        eng.set_pml(LAYER, courant00=C0 * DT / DX)
        eng.set_conductivity(sigma[None])
        eng.set_dispersion(wp2[None], GAMMA, OMEGA0)
        eng.set_sources(np.array([SRC]))
        eng.set_hz_bloch_phase(phi, rotation=rotation)
        eng.run(nsteps, ricker(nsteps, DT, FC)[None])
        return fields(eng)


def run_supercell(engine, dtype, weights, nsteps=NSTEPS, **kw):
    """len(weights) periods on a plain periodic Hz `engine`, one unit-channel Hz point source per period."""
    n = len(weights)
    eps, mu, sigma, wp2 = (tiled(a, n) for a in materials())
    with engine(1, ROWS, n * Q + 1, DT, DX, dtype=dtype, boundary="periodic", **kw) as eng:
        if hasattr(eng, "set_polarization"):
            eng.set_polarization("hz")
        eng.set_materials(eps[None], mu[None])
        eng.set_pml(LAYER, courant00=C0 * DT / DX)
        eng.set_conductivity(sigma[None])
        eng.set_dispersion(wp2[None], GAMMA, OMEGA0)
        eng.set_point_sources(np.array([(SRC[0], SRC[1] + k * Q) for k in range(n)]),
                              np.asarray(weights, dtype=np.float64)[:, None])
        eng.run(nsteps, None, ricker(nsteps, DT, FC)[None])
        return fields(eng)


def period(f, k):
    """Period k of a supercell's eight fields in a one-period member's shapes (Hz and Hzx with their image column)."""
    Hz, Ex, Ey, Hzx = f[:4]
    sl, sli = slice(k * Q, (k + 1) * Q), slice(k * Q, (k + 1) * Q + 1)
    return [Hz[:, sli], Ex[:, sl], Ey[:, sli], Hzx[:, sli]] + [a[:, sli] for a in f[4:]]


def same(a, b):
    """array_equal of a member's eight fields over columns 0..Q-1 (Ey and the state have no image: column C-1 is the
    supercell's next period there, a permanent zero here), and of Hz and Hzx with their image column."""
    return (all(np.array_equal(x[..., :Q], y[..., :Q]) for x, y in zip(a, b)) and np.array_equal(a[0], b[0])
            and np.array_equal(a[3], b[3]))


def alive(f):
    """Every one of the eight fields is non-zero: the pole and the layer are exercised."""
    return all(np.abs(a).max() > 0 for a in f)


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_hz_bloch_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_HZ_BLOCH_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_HZ_BLOCH_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_HZ_BLOCH_SIGNATURES[n][0]
    main = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    assert "hz_bloch" not in main.lower()                  # a companion header: fdtd2d.h declares none of it


def test_hz_bloch_info_id_is_named_and_was_free():
    """The id is written relative to FDTD2D_BATCH_INFO_FLUX_LDS (22), as fdtd2d_batch_flux_adjoint.h writes the line
    sources' 23: earlier tests pin the numbered #defines of the other headers."""
    from fdtd2d_amd import _abi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    mine = strip(open(HEADER).read())
    assert re.findall(r"FDTD2D_BATCH_INFO_\w+\s*=\s*([^,}]+)", mine) == ["FDTD2D_BATCH_INFO_FLUX_LDS + 2 "]
    assert not re.search(r"#define\s+FDTD2D_BATCH_(INFO|OPT)_", mine)
    assert _abi.BATCH_INFO_FLUX_LDS + 2 == _abi.BATCH_HZ_BLOCH_INFO == 24
    inc = os.path.join(ROOT, "include")
    for h in sorted(os.listdir(inc)):
        if h == os.path.basename(HEADER):
            continue
        txt = strip(open(os.path.join(inc, h)).read())
        ids = [int(v) for v in re.findall(r"FDTD2D_BATCH_INFO_\w+\s*(?:=\s*|\s+)(-?\d+)\b", txt)]
        ids += [22 + int(v) for v in re.findall(r"FDTD2D_BATCH_INFO_\w+\s*=\s*FDTD2D_BATCH_INFO_FLUX_LDS\s*\+\s*(\d+)", txt)]
        assert ids == [] or max(ids) < 24, h
    taken = [v for k, v in vars(_abi).items()
             if isinstance(v, int) and (k.startswith("BATCH_INFO_") or (k.startswith("BATCH_") and k.endswith("_INFO")))]
    assert taken.count(24) == 1 and max(taken) == 24 and _abi.BATCH_FLUX_LINE_SOURCES_INFO == 23
    lib = _abi.load()
    assert lib.fdtd2d_batch_set_hz_bloch(None, None, None) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_HZ_BLOCH_INFO) == _abi.E_ARG


# ---- 2. supercell identities of the stand-in, against the real HzPeriodicOracle ---------------------------------------

def check_unit_rotation(bloch_engine, periodic_engine, dtype, **kw):
    got = run_bloch(bloch_engine, dtype, rotation=(1, 0), **kw)
    want = run_supercell(periodic_engine, dtype, [1.0], **kw)
    assert alive(want)
    for g, w in zip(got, want):
        assert np.iscomplexobj(g) and np.array_equal(g.real, w) and not g.imag.any()


def check_half_turn(bloch_engine, periodic_engine, dtype, **kw):
    got = run_bloch(bloch_engine, dtype, rotation=(-1, 0), **kw)
    sup = run_supercell(periodic_engine, dtype, [1.0, -1.0], **kw)
    assert alive([g.real for g in got]) and not any(g.imag.any() for g in got)
    assert same([g.real for g in got], period(sup, 0))
    assert same([-g.real for g in got], period(sup, 1))


def check_quarter_turn(bloch_engine, periodic_engine, dtype, **kw):
    got = run_bloch(bloch_engine, dtype, rotation=(0, 1), **kw)
    re_ = run_supercell(periodic_engine, dtype, [1.0, 0.0, -1.0, 0.0], **kw)
    im_ = run_supercell(periodic_engine, dtype, [0.0, 1.0, 0.0, -1.0], **kw)
    assert alive([g.real for g in got]) and alive([g.imag for g in got])
    assert same([g.real for g in got], period(re_, 0))
    assert same([g.imag for g in got], period(im_, 0))
    assert same([g.imag for g in got], period(re_, 3))     # F(x + 3Q) = -i F(x)


def nth_root_difference(bloch_engine, periodic_engine, m, N, **kw):
    """max|difference| / max|field| between the Hz Bloch member at phi = 2 pi m / N and period 0 of the N-period
    supercells driven with cos(phi n) and sin(phi n), float64, over the eight fields."""
    phi = 2 * np.pi * m / N
    got = run_bloch(bloch_engine, np.float64, phi=phi, **kw)
    re_ = period(run_supercell(periodic_engine, np.float64, np.cos(phi * np.arange(N)), **kw), 0)
    im_ = period(run_supercell(periodic_engine, np.float64, np.sin(phi * np.arange(N)), **kw), 0)
    worst = 0.0
    for g, r, i in zip(got, re_, im_):
        scale = max(np.abs(r).max(), np.abs(i).max())
        assert scale > 0
        worst = max(worst, np.abs(g.real[..., :Q] - r[..., :Q]).max() / scale,
                    np.abs(g.imag[..., :Q] - i[..., :Q]).max() / scale)
    return worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_unit_rotation_is_the_periodic_hz_batch(dtype):
    check_unit_rotation(HzBlochOracle, HzPeriodicOracle, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_half_turn_is_a_two_period_supercell(dtype):
    check_half_turn(HzBlochOracle, HzPeriodicOracle, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_quarter_turn_is_two_four_period_supercells(dtype):
    check_quarter_turn(HzBlochOracle, HzPeriodicOracle, dtype)


# measured here (NumPy, float64): max|difference| / max|field| over the eight fields after 300 steps.  (The Ez stand-in
# measured 3.3e-15 and 5.9e-15 on Ez, Hx, Hy: here the pole state is compared too, and the pole feeds its rounding back.)
ROOT_MEASURED = {(1, 3): 8.9e-14, (2, 5): 1.3e-13}
ROOT_BOUND = {k: 10 * v for k, v in ROOT_MEASURED.items()}


@pytest.mark.parametrize("m,N", [(1, 3), (2, 5)])
def test_nth_root_phases_match_their_supercells_to_rounding(m, N):
    d = nth_root_difference(HzBlochOracle, HzPeriodicOracle, m, N)
    print(f"phi = 2 pi {m}/{N}: max|difference| / max|field| = {d:.3e} (bound {ROOT_BOUND[m, N]:.3e})")
    assert d <= ROOT_BOUND[m, N]


# ---- 3. duality with the Ez Bloch stand-in; a zero pole is no pole ------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lossless_run_is_the_ez_bloch_run_with_eps_and_mu_exchanged(dtype):
    """Identity (b): the Ez member takes the Hz member's mu as its eps and its eps as its mu, number for number."""
    eps, mu, _, _ = materials(lossy=False)
    out = []
    amps = (ricker(NSTEPS, DT, FC) * np.exp(0.3j))[None]
    for cls, e, m in ((HzBlochOracle, eps, mu), (BlochOracle, mu, eps)):
        with cls(1, ROWS, Q + 1, DT, DX, dtype=dtype, boundary="periodic") as eng:
            eng.set_materials(e[None], m[None])
            eng.set_pml(LAYER, courant00=C0 * DT / DX)
            eng.set_sources(np.array([(SRC[0], 0, 1, Q)]))
            if cls is HzBlochOracle:
                eng.set_hz_bloch_phase(0.7).set_hz_bloch_source("ramp")
            else:
                eng.set_bloch_phase(0.7).set_bloch_source("ramp")
            eng.run(NSTEPS, amps)
            out.append([a[0] for a in eng.download()] + [eng.download_ezx()[0]])
    (hz, ex, ey, hzx), (ez, hx, hy, ezx) = out
    assert np.abs(hz.real).max() > 0 and np.abs(hz.imag).max() > 0 and np.abs(hzx).max() > 0
    assert np.array_equal(hz, ez) and np.array_equal(hzx, ezx)
    assert np.array_equal(ex, -hx) and np.array_equal(ey, -hy)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_zero_pole_with_zero_state_is_no_pole(dtype):
    """Identity (c)."""
    eps, mu, _, _ = materials()
    amps = (ricker(NSTEPS, DT, FC) * np.exp(0.3j))[None]
    out = []
    for pole in (False, True):
        with HzBlochOracle(1, ROWS, Q + 1, DT, DX, dtype=dtype, boundary="periodic") as eng:
            eng.set_materials(eps[None], mu[None])
            eng.set_pml(LAYER, courant00=C0 * DT / DX)
            eng.set_sources(np.array([SRC]))
            if pole:
                eng.set_conductivity(np.zeros((1, ROWS, Q + 1)))
                eng.set_dispersion(np.zeros((1, ROWS, Q + 1)), GAMMA, OMEGA0)
            eng.set_hz_bloch_phase(-2.1)
            eng.run(NSTEPS, amps)
            out.append([a[0] for a in eng.download()] + [eng.download_ezx()[0]])
            if pole:
                assert not any(a.any() for a in eng.download_dispersion())
    assert np.abs(out[0][0].imag).max() > 0
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 4. Brewster's angle ------------------------------------------------------------------------------------------------

B_ROWS, B_Q, B_L, B_PHI, B_STEPS, B_TAIL, B_SRC_ROW = 160, 12, 20, 2.2495, 5000, 1500, 30
B_WINDOW = (110, 0, 10, 1)
B_FREQS = (100e9, 125e9)       # Brewster incidence (63.4 degrees) and 45.7 degrees at this k_x
# the Airy transmission of the 4-cell eps_r = 4 slab at these angles: the in-plane polarisation (Hz), the other (Ez)
B_AIRY = {("hz", 0): 1.0, ("hz", 1): 0.87185, ("ez", 0): 0.2223, ("ez", 1): 0.4686}
# measured here (NumPy, float64), over the window rows: Hz 100 GHz 0.9784..0.9792, 125 GHz 0.85198; Ez 100 GHz
# 0.2166..0.2168, 125 GHz 0.4557.  The worst deviation from Airy is 0.022; the bound 0.03 covers libm differences.
B_TOL = 0.03


def brewster_transmissions(pol):
    """T[f] (over the window rows) = |W_slab|^2 / |W_vacuum|^2 for the two frequencies: four members in one stand-in
    (slab and vacuum at each frequency), float64."""
    cls = HzBlochOracle if pol == "hz" else BlochOracle
    n = np.arange(B_STEPS)
    env = 1 - np.exp(-(n / 400.0) ** 2)
    w = 2 * np.pi * np.array([B_FREQS[0], B_FREQS[0], B_FREQS[1], B_FREQS[1]])
    amps = env[None, :] * np.exp(1j * w[:, None] * n[None, :] * DT)
    eps = np.full((4, B_ROWS, B_Q + 1), EPS0)
    eps[0::2, 70:74, :] = 4 * EPS0
    with cls(4, B_ROWS, B_Q + 1, DT, DX, dtype=np.float64, boundary="periodic") as eng:
        eng.set_materials(eps, np.full(eps.shape, MU0))
        eng.set_pml(B_L, courant00=C0 * DT / DX)
        eng.set_sources(np.array([(B_SRC_ROW, 0, 1, B_Q)] * 4))
        if pol == "hz":
            eng.set_hz_bloch_phase(B_PHI).set_hz_bloch_source("ramp")
        else:
            eng.set_bloch_phase(B_PHI).set_bloch_source("ramp")
        eng.run(B_STEPS - B_TAIL, amps[:, :B_STEPS - B_TAIL])
        eng.set_dft_window(B_WINDOW, w[:, None])
        eng.run(B_TAIL, amps[:, B_STEPS - B_TAIL:])
        W = eng.read_dft_window()[:, 0, :, 0]
    return [np.abs(W[2 * k]) ** 2 / np.abs(W[2 * k + 1]) ** 2 for k in range(2)]


@pytest.fixture(scope="module")
def brewster():
    return {pol: brewster_transmissions(pol) for pol in ("hz", "ez")}


def test_brewster_incidence_passes_the_in_plane_polarisation_alone(brewster):
    for pol in ("hz", "ez"):
        for k in range(2):
            t = brewster[pol][k]
            print(f"{pol} {B_FREQS[k] / 1e9:.0f} GHz: T = {t.min():.5f} .. {t.max():.5f} (Airy {B_AIRY[pol, k]})")
    assert brewster["hz"][0].min() >= 0.97
    assert brewster["ez"][0].max() <= 0.23


@pytest.mark.parametrize("pol,k", [("hz", 0), ("hz", 1), ("ez", 0), ("ez", 1)])
def test_slab_transmission_matches_airy(brewster, pol, k):
    t = brewster[pol][k]
    assert np.abs(t - B_AIRY[pol, k]).max() <= B_TOL, (t.min(), t.max())


# ---- 5. host refusals ------------------------------------------------------------------------------------------------

class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def host_engine(fd, phase=True, boundary="periodic", hz=True, count=3, rows=30, cols=13):
    """A BatchEngine without a handle, for the checks that never reach the library."""
    eng = object.__new__(fd.BatchEngine)
    eng._lib, eng._h = _NoLibrary(), ctypes.c_void_p()
    eng.count, eng.rows, eng.cols, eng.dt, eng.dx = count, rows, cols, DT, DX
    eng.dtype, eng.boundary = np.dtype(np.float32), boundary
    eng._pml_on, eng._pml_chosen, eng._pml_L = False, True, 0
    eng._win, eng._nprobe, eng._npoint = (1, 2, 2), 1, (1, 1)
    eng._flux, eng._bflux, eng._hzflux = None, False, False
    eng._hz, eng._hzb = hz, hz and phase
    eng._bloch = (np.ones(count), np.zeros(count)) if phase else None
    eng._phi = np.zeros(count) if phase else None
    return eng


@pytest.mark.parametrize("call,what", [
    (lambda e: e.set_dft(1e11), "the whole-grid transform"),
    (lambda e: e.set_point_sources(np.array([(5, 5)]), np.ones((1, 1))), "a point source"),
    (lambda e: e.run(4, None, np.zeros((1, 4))), "a run with channels"),
    (lambda e: e.set_hz_flux_lines([("row", 5, 0, 12)], [1e11]), "set_hz_flux_lines"),
    (lambda e: e.set_polarization("ez"), "a change of polarisation"),
])
def test_what_the_hz_phase_excludes_is_refused_on_the_host(fd, call, what):
    from fdtd2d_amd import _abi
    with pytest.raises(fd.Fdtd2dError, match="is not available while a Bloch phase is set") as ei:
        call(host_engine(fd))
    assert ei.value.code == _abi.E_STATE and what in str(ei.value)
    with pytest.raises(AssertionError, match="the library was called"):     # without a phase the call goes through
        call(host_engine(fd, phase=False))


def test_the_phase_is_refused_beside_hz_flux_lines_and_off_the_hz_polarisation(fd):
    from fdtd2d_amd import _abi
    eng = host_engine(fd, phase=False)
    eng._hzflux = True
    with pytest.raises(fd.Fdtd2dError, match="flux lines of the Hz polarisation") as ei:
        eng.set_hz_bloch_phase(0.3)
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(fd.Fdtd2dError, match="set_hz_bloch_phase needs the Hz polarisation") as ei:
        host_engine(fd, phase=False, hz=False).set_hz_bloch_phase(0.3)
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(fd.Fdtd2dError, match="a Bloch phase needs periodic columns") as ei:
        host_engine(fd, phase=False, boundary="pml").set_hz_bloch_phase(0.3)
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(fd.Fdtd2dError, match="Hz polarisation") as ei:      # the Ez phase stays refused
        host_engine(fd, phase=False).set_bloch_phase(0.3)
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(fd.Fdtd2dError, match="no Bloch phase of the Hz polarisation is set") as ei:
        host_engine(fd, phase=False).set_hz_bloch_source("ramp")
    assert ei.value.code == _abi.E_STATE
    with pytest.raises(AssertionError, match="the library was called"):
        host_engine(fd, phase=False).set_hz_bloch_phase(0.3)


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


def test_bad_phases_are_refused_on_the_host(fd):
    with pytest.raises(ValueError, match=r"phi must be a scalar or have shape \(3,\)"):
        host_engine(fd, phase=False).set_hz_bloch_phase(np.zeros(2))
    with pytest.raises(ValueError, match=r"c must be a scalar or have shape \(3,\)"):
        host_engine(fd, phase=False).set_hz_bloch_phase(None, rotation=(np.ones(4), 0.0))
    with pytest.raises(ValueError, match="rotation must be a pair"):
        host_engine(fd, phase=False).set_hz_bloch_phase(None, rotation=(1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="phi must be finite"):
        host_engine(fd, phase=False).set_hz_bloch_phase(np.array([0.1, np.nan, 0.2]))
    with pytest.raises(ValueError, match="s must be finite"):
        host_engine(fd, phase=False).set_hz_bloch_phase(None, rotation=(1.0, np.inf))
    with pytest.raises(ValueError, match=r"weights must have shape \(12,\) or \(3, 12\)"):
        host_engine(fd).set_hz_bloch_source(np.ones(13))
    with pytest.raises(ValueError, match="a complex pole state needs the phase"):
        host_engine(fd, phase=False).upload_hz_dispersion(Jx=np.zeros((3, 30, 13), complex))
    for call in (lambda e: e.upload(Ez=np.zeros((3, 30, 13), complex)), lambda e: e.run(4, np.zeros((3, 4), complex))):
        with pytest.raises(ValueError, match="need a Bloch phase"):
            call(host_engine(fd, phase=False))


def test_run_fdtd_batch_checks_its_hz_bloch_arguments_on_the_host(monkeypatch, fd):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    eps = np.full((2, 30, 13), EPS0)
    kw = dict(nsteps=10, sources=np.array([(5, 5), (5, 5)]), dt=DT, dx=DX)
    with pytest.raises(ValueError, match='hz_bloch_phase needs polarization="hz"'):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, hz_bloch_phase=0.2, **kw)
    with pytest.raises(ValueError, match='hz_bloch_phase needs boundary="periodic"'):
        fd.run_fdtd_batch(eps, boundary="pml", pml_cells=5, polarization="hz", hz_bloch_phase=0.2, **kw)
    with pytest.raises(ValueError, match="bloch_phase is not available with polarization"):    # the existing refusal stays
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", bloch_phase=0.2, **kw)
    with pytest.raises(ValueError, match=r"hz_bloch_phase must be a scalar or have shape \(2,\)"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", hz_bloch_phase=[0.1, 0.2, 0.3], **kw)
    with pytest.raises(ValueError, match="hz_bloch_phase must be finite"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", hz_bloch_phase=np.nan, **kw)
    with pytest.raises(ValueError, match="omega .* is not available with hz_bloch_phase"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", hz_bloch_phase=0.2, omega=1e11, **kw)
    with pytest.raises(ValueError, match="hz_flux_lines is not available with hz_bloch_phase"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", hz_bloch_phase=0.2,
                          hz_flux_lines=[("row", 20, 0, 12)], hz_flux_omegas=[1e11], **kw)
    with pytest.raises(ValueError, match="touches column 12"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", hz_bloch_phase=0.2,
                          dft_window=(3, 11, 2, 2), window_omegas=[1e11], **kw)
    with pytest.raises(ValueError, match="a probe lies in column 12"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", hz_bloch_phase=0.2, probes=[(3, 12)], **kw)
    with pytest.raises(ValueError, match="source_weights needs bloch_phase"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", source_weights="ramp", **kw)
    with pytest.raises(AssertionError, match="the device was touched"):
        fd.run_fdtd_batch(eps, boundary="periodic", pml_cells=5, polarization="hz", hz_bloch_phase=[0.2, 0.4],
                          source_weights="ramp", dft_window=(3, 10, 2, 2), window_omegas=[1e11], probes=[(3, 11)], **kw)
