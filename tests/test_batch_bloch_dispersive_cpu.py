"""CPU-only checks of the Drude-Lorentz pole of Bloch and lattice batches (fdtd2d_batch_bloch_dispersive.h, batch.py), on
the stand-in of tests/oracle_batch_bloch_dispersive.py.

The surface: the three entry points are declared, exported and bound, the header names no new id, the Python surface has
its shape, bad arguments are refused before any device is touched.

The arithmetic: with wp2 = 0 the stand-in equals the Bloch and the lattice stand-ins bit for bit; with a zero phase its
real part is the periodic dispersive stand-in's; a plane wave on a uniform lossless Drude lattice follows the three-term
recurrence with the plasma term; a unit cell equals its supercell, Jh and Q included; negated phases conjugate.

The physics: a periodic, column-uniform member (220 x 5, a 20-cell layer on the rows, dt = 5e-14, dx = 1e-4) with a 20-cell
Drude slab (wp = 2 pi 70 GHz, gamma = 1e11), a Ricker ramp line source at 60 GHz with the Bloch phase phi = 0.2 (transverse
wavenumber kx = phi / ((C-1) dx) = 500 rad/m: 36.6 degrees at 40 GHz, 17.4 degrees at 80 GHz) and 6000 steps; the probe
spectrum behind the slab over the same run without the slab, at 40, 50, 60, 70 and 80 GHz, against |T| of the analytic
s-polarised slab formula at that kx.  Worst error of the stand-in itself: 2.6e-3 in both dtypes; the bound is twice that,
the margin tests/test_batch_dispersive_cpu.py uses at normal incidence.  Without the pole the same check misses by 0.88
(the slab is opaque below its plasma frequency and the vacuum run transmits everything).

Stability: a lossless member whose cells sit at 3.9 on dt^2 (omega0^2 + wp2 EPS0 / eps) + 8 dt^2 / (eps mu dx^2) stays
bounded over 5000 steps."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch_bloch import BlochOracle
from oracle_batch_bloch_dispersive import BlochDispersiveOracle, LatticeDispersiveOracle
from oracle_batch_dispersive import DispersivePeriodicOracle, EPS0, stability
from oracle_batch_lattice import LatticeOracle
import test_batch_lattice_cpu as lcpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_bloch_dispersive.h")
NAMES = ["fdtd2d_batch_set_bloch_dispersion", "fdtd2d_batch_set_bloch_dispersion_window",
         "fdtd2d_batch_transfer_bloch_dispersion"]
MU0 = 4 * np.pi * 1e-7
DT, DX = 5e-14, 1e-4
COURANT0 = (1 / np.sqrt(EPS0 * MU0) * DT) / DX
WP2 = (2 * np.pi * 70e9) ** 2
EXACT = lcpu.EXACT


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


# ---- the surface ----------------------------------------------------------------------------------------------------

def test_batch_bloch_dispersive_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_BLOCH_DISPERSIVE_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_BLOCH_DISPERSIVE_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_BLOCH_DISPERSIVE_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "const void *": ctypes.c_void_p,
             "void *": ctypes.c_void_p, "const int": ctypes.POINTER(ctypes.c_int),
             "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = []
        for a in args.split(","):
            a = " ".join(a.split())
            got.append(kinds[re.match(r"(.*?[ *])\w+(\[4\])?$", a).group(1).strip()])
        assert got == _abi.BATCH_BLOCH_DISPERSIVE_SIGNATURES[n][1], n


def test_batch_bloch_dispersive_header_adds_no_info_or_option_id():
    """FDTD2D_BATCH_INFO_DISPERSIVE (19, fdtd2d_batch_dispersive.h) reports either pole."""
    from fdtd2d_amd import _abi
    assert not re.findall(r"#define\s+FDTD2D_BATCH_(?:INFO|OPT)_\w+", open(HEADER).read())
    assert _abi.BATCH_INFO_DISPERSIVE == 19


def test_batch_bloch_dispersive_python_surface(fd):
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_bloch_dispersion).parameters) == ["self", "wp2", "gamma", "omega0"]
    assert list(inspect.signature(E.set_bloch_dispersion_window).parameters) == ["self", "window", "wp2"]
    assert list(inspect.signature(E.download_bloch_dispersion).parameters) == ["self"]
    assert list(inspect.signature(E.upload_bloch_dispersion).parameters) == ["self", "Jh", "Q"]
    p = inspect.signature(fd.run_fdtd_batch).parameters
    assert p["bloch_dispersion"].default is None and p["bloch_dispersion"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (BlochDispersiveOracle, LatticeDispersiveOracle):
        for name in ("set_bloch_dispersion", "set_bloch_dispersion_window", "download_bloch_dispersion",
                     "upload_bloch_dispersion"):
            assert callable(getattr(cls, name))


def test_batch_bloch_dispersive_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    w = np.array([1, 1, 2, 2], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_bloch_dispersion(None, d.ctypes.data, _abi.F64, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_bloch_dispersion_window(None, w, d.ctypes.data, _abi.F64) == _abi.E_ARG
    assert lib.fdtd2d_batch_transfer_bloch_dispersion(None, d.ctypes.data, None, None, None, _abi.F64, 0) == _abi.E_ARG


def test_batch_bloch_dispersive_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 2, 17, 13, DT, DX, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, 17, 13), EPS0), nsteps=10, sources=np.array([[5, 5]] * 2), boundary="lattice",
                          bloch_phase=(0.3, 0.1), bloch_dispersion=(1e22, 1e11, 0.0))
    assert ei.value.code == _abi.E_NODEVICE


# ---- the members that the device tests share (tests/test_gpu_batch_bloch_dispersive.py) ---------------------------------

GAMMA = np.array([1e11, 0.0, 5e10, 2e11, 3e10])          # member 0 is a Drude pole, member 1 lossless, member 2 has wp2 = 0
OMEGA0 = np.array([0.0, 3e11, 2e11, 0.0, 4e11])


def members(engine, kind, dtype, R, C, n, layer=0, pole=True, seed=0, state=True, monitors=True, wp2_zero=False, B=5):
    """B members of a Bloch (kind "bloch": periodic columns, a `layer`-cell layer or PEC rows) or lattice batch with
    their own materials, phases and poles: random wp2 wherever it may be (columns 0, C-2 and C-1; on the lattice row 0,
    row R-2 and cell (0, 0) too), a conductivity, a ramp line source with complex amplitudes, a window, three probes
    (on the lattice one at (0, 0)) and a random complex state with Jh and Q (state "fields": Ez, Hx and Hy alone; the
    draws do not depend on the arguments).  Returns (engine, amps (5, n))."""
    rng = np.random.default_rng(seed)
    lattice = kind == "lattice"
    e = engine(B, R, C, DT, DX, dtype=dtype, boundary="lattice" if lattice else "periodic")
    e.set_materials((EPS0 * (1 + 2 * rng.random((B, R, C)))).astype(dtype), (MU0 * (1 + rng.random((B, R, C)))).astype(dtype))
    if layer:
        e.set_pml(layer, courant00=COURANT0)
    g = 0 if lattice else max(6, layer)
    phi = 0.3 + 2.7 * (np.arange(B) % 11) / 11 + 0.001 * np.arange(B)          # distinct
    if lattice:
        e.set_lattice_phase(phi, -2.8 + 5.5 * ((3 * np.arange(B) + 1) % 7) / 7)
    else:
        e.set_bloch_phase(phi)
    sigma, wp2 = np.zeros((B, R, C)), np.zeros((B, R, C))
    sigma[:, g:R - g, :] = np.where(rng.random((B, R - 2 * g, C)) < 0.3, 0.0, 5.0 * rng.random((B, R - 2 * g, C)))
    wp2[:, g:R - g, :] = 2e25 * rng.random((B, R - 2 * g, C))
    wp2[2::5] = 0
    if wp2_zero:
        wp2[...] = 0
    e.set_conductivity(sigma)
    e.set_sources(np.array([[g + 1 + (m % 3), 0, 1, C - 1] for m in range(B)]))
    e.set_bloch_source("ramp")
    if monitors:
        e.set_dft_window((g + 1, 0, 3, 4), 2 * np.pi * np.array([30e9, 55e9]), every=2)
        e.set_probes(np.array([(0, 0) if lattice else (g, 0), (g + 2, C - 2), (R - 2 - g, 3)]), n)
    if pole:
        assert wp2_zero or wp2[[0, 1, 3, 4]][:, g:R - g, [0, C - 2, C - 1]].all()
        e.set_bloch_dispersion(wp2, np.resize(GAMMA, B), np.resize(OMEGA0, B))
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(cdtype(dtype))
    st = [cplx(B, R, C), cplx(B, R, C - 1), cplx(B, R - 1, C), cplx(B, R, C), cplx(B, R, C)]
    if state:
        e.upload(*st[:3])
    if state is True and pole:
        e.upload_bloch_dispersion(st[3], st[4])
    amps = rng.standard_normal((B, n)) * np.exp(1j * (0.4 + 0.7 * np.arange(B)))[:, None]
    return e, amps


def outputs(e, kind, pole=True, monitors=True):
    out = dict(zip(("Ez", "Hx", "Hy"), e.download()))
    if kind == "bloch":
        out["Ezx"] = e.download_ezx()
    if pole:
        out["Jh"], out["Q"] = e.download_bloch_dispersion()
    if monitors:
        out["dft"], out["probes"] = e.read_dft_window(), e.read_probes()
    return out


def oracle_for(kind):
    return LatticeDispersiveOracle if kind == "lattice" else BlochDispersiveOracle


# ---- 1. wp2 = 0 is the stand-in without the pole ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["bloch", "lattice"])
def test_zero_strength_leaves_the_stand_in_bit_identical(kind, dtype):
    R, C, n = (23, 11, 40) if kind == "bloch" else (11, 13, 40)
    layer = 4 if kind == "bloch" else 0
    base_cls = LatticeOracle if kind == "lattice" else BlochOracle
    ref, amps = members(base_cls, kind, dtype, R, C, n, layer, pole=False, state="fields")
    ref.run(n, amps)
    eng, same = members(oracle_for(kind), kind, dtype, R, C, n, layer, wp2_zero=True, state="fields")
    assert eng.dispersive and not getattr(ref, "dispersive", False) and np.array_equal(amps, same)
    eng.run(n, amps)
    want, got = outputs(ref, kind, pole=False), outputs(eng, kind)
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    assert np.abs(got["Ez"].imag).max() > 0 and not np.any(got["Jh"]) and not np.any(got["Q"])


# ---- 2. a zero phase is the periodic dispersive stand-in ----------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_phase_is_the_real_periodic_pole(dtype):
    B, R, C, L, n = 2, 25, 9, 4, 60
    rng = np.random.default_rng(3)
    eps, mu = EPS0 * (1 + rng.random((B, R, C))), MU0 * (1 + rng.random((B, R, C)))
    wp2, sigma = np.zeros((B, R, C)), np.zeros((B, R, C))
    wp2[:, 6:R - 6] = 2e25 * rng.random((B, R - 12, C))
    sigma[:, 6:R - 6] = 0.5 * rng.random((B, R - 12, C))
    gam, om0 = np.array([1e11, 0.0]), np.array([0.0, 3e11])
    start = [rng.standard_normal(s) for s in ((B, R, C), (B, R, C - 1), (B, R - 1, C), (B, R, C), (B, R, C), (B, R, C))]
    amps = rng.standard_normal((B, n))
    out = []
    for cls in (DispersivePeriodicOracle, BlochDispersiveOracle):
        e = cls(B, R, C, DT, DX, dtype=dtype)
        e.set_materials(eps, mu).set_pml(L, courant00=COURANT0)
        e.set_conductivity(sigma)
        e.set_sources(np.array([[8, 0, 1, C - 1], [9, 2, 1, 3]]))
        e.set_probes(np.array([[8, 0], [12, 5]]), n)
        if cls is BlochDispersiveOracle:
            e.set_bloch_phase(None, rotation=(1.0, 0.0))          # unit weights are the default
            e.set_bloch_dispersion(wp2, gam, om0)
            e.upload(*start[:3]).upload_ezx(start[3]).upload_bloch_dispersion(start[4], start[5])
            e.run(n, amps)
            out.append(e.download() + (e.download_ezx(),) + e.download_bloch_dispersion() + (e.read_probes(),))
        else:
            e.set_dispersion(wp2, gam, om0)
            e.upload(*start[:3]).upload_ezx(start[3]).upload_dispersion(start[4], start[5])
            e.run(n, amps)
            out.append(e.download() + (e.download_ezx(),) + e.download_dispersion() + (e.read_probes(),))
    for name, a, b in zip(("Ez", "Hx", "Hy", "Ezx", "Jh", "Q", "probes"), *out):
        assert np.array_equal(a, b.real), name
        assert not np.any(b.imag), name
    assert np.any(out[0][4]) and np.any(out[0][5])


# ---- 3. the plane wave on a Drude lattice ---------------------------------------------------------------------------------

PW_QR, PW_QC, PW_STEPS, PW_BOUND = 6, 9, 300, 1e-10
PW_WP2 = (2 * np.pi * 100e9) ** 2       # a plasma period of 200 steps: after 300 the uniform field has changed its sign


def plane_wave(phi_r, phi_c, skip_pole=False):
    """(a_N of the recurrence, max|Ez - a_N start|) after PW_STEPS steps from Ez = exp(i (th_r i + th_c j)), H = J = 0."""
    R, Cc = PW_QR + 1, PW_QC + 1
    th_r, th_c = phi_r / PW_QR, phi_c / PW_QC
    start = np.exp(1j * (th_r * np.arange(R)[:, None] + th_c * np.arange(Cc)[None, :]))
    ref = LatticeDispersiveOracle(1, R, Cc, DT, DX, dtype=np.float64)
    ref.set_materials(EPS0, MU0).set_lattice_phase(phi_r, phi_c)
    ref.set_bloch_dispersion(PW_WP2, 0.0, 0.0)
    assert np.all(ref.wp2 == PW_WP2)
    ref.skip_pole = skip_pole
    ref.upload(Ez=start[None])
    ref.run(PW_STEPS)
    S = (DT / (EPS0 * DX)) * (DT / (MU0 * DX)) * (np.sin(th_r / 2) ** 2 + np.sin(th_c / 2) ** 2)
    K = DT * DT * PW_WP2                                         # cb * cj = dt^2 wp2 EPS0 / eps
    a0, a1 = 1.0, 1 - 4 * S - K
    for _ in range(PW_STEPS - 1):
        a0, a1 = a1, (2 - 4 * S - K) * a1 - a0
    return a1, np.abs(ref.download()[0][0] - a1 * start).max()


@pytest.mark.parametrize("phi_r,phi_c", [(0.0, 0.0), (0.7, -1.9)])
def test_plane_wave_on_a_drude_lattice_follows_its_recurrence(phi_r, phi_c):
    aN, err = plane_wave(phi_r, phi_c)
    print(f"phases ({phi_r:.3f}, {phi_c:.3f}): a_N = {aN:.6f}, max|Ez - a_N start| = {err:.3e} (bound {PW_BOUND:.0e})")
    assert abs(aN) > 0.05 and err <= PW_BOUND              # images and the corner included
    _, miss = plane_wave(phi_r, phi_c, skip_pole=True)
    print(f"    without the pole block: {miss:.3e}")
    assert miss > 1e7 * PW_BOUND            # seven decades over the bound; at (0, 0) the field then never moves: 2
    if (phi_r, phi_c) == (0.0, 0.0):          # the discrete plasma frequency: cos(th) = 1 - K / 2, th = w dt
        th = np.arccos(1 - DT * DT * PW_WP2 / 2)
        assert abs(aN - np.cos((PW_STEPS + 0.5) * th) / np.cos(th / 2)) < 1e-9
        assert abs(th / DT / np.sqrt(PW_WP2) - 1) < 1e-4


# ---- 4. supercells ----------------------------------------------------------------------------------------------------------

SUPER_BOUND = 1e-12
LATTICE_ROTS = [("half", "quarter"), ("quarter", "half"), ("one", "quarter"), ("quarter", "quarter")]
BLOCH_ROTS = ["half", "quarter", "one"]


def supercell_difference(engine, kind, dtype, R, Cc, rots=None, phases=None, nsteps=200, seed=11, layer=4):
    """A random-eps, lossy, dispersive unit cell against its supercell with phase-tiled start fields and state: a lattice
    cell of period (R-1) x (C-1) with (rho_r, rho_c) against 2 x 3 tiles with (rho_r^2, rho_c^3); a Bloch member of
    period C-1 (a `layer`-cell layer) with rho against 2 tiles with rho^2.  rots: per member EXACT keys (pairs on the
    lattice); phases: (phi_r (B,), phi_c (B,)) (phi_r is not read for a Bloch member).  Returns the worst
    max|supercell - tiled unit| / max|unit| over Ez, Hx, Hy, Jh and Q (and Ezx of a Bloch member), images included."""
    lattice = kind == "lattice"
    Qr, Qc = (R - 1, Cc - 1) if lattice else (R, Cc - 1)
    tr, tc = (2, 3) if lattice else (1, 2)
    SR, SC = (tr * Qr + 1 if lattice else R), tc * Qc + 1
    if not lattice and rots is not None:
        rots = [("one", k) for k in rots]
    B = len(rots) if rots is not None else len(phases[1])
    rng = np.random.default_rng(seed)
    g = 0 if lattice else max(6, layer)
    eps = (EPS0 * (1 + 3 * rng.random((B, R, Cc)))).astype(dtype)
    sigma, wp2 = np.zeros((B, R, Cc)), np.zeros((B, R, Cc))
    sigma[:, g:R - g] = np.where(rng.random((B, R - 2 * g, Cc)) < 0.5, 0.0, 5.0 * rng.random((B, R - 2 * g, Cc)))
    wp2[:, g:R - g] = 2e25 * rng.random((B, R - 2 * g, Cc))
    gam, om0 = 1e11 * rng.random(B), 3e11 * rng.random(B)
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(cdtype(dtype))
    start = [cplx(B, R, Cc), cplx(B, R, Cc - 1), cplx(B, R - 1, Cc), cplx(B, R, Cc), cplx(B, R, Cc), cplx(B, R, Cc)]
    if rots is not None:
        fr = np.array([complex(*EXACT[a]) for a, _ in rots])
        fc = np.array([complex(*EXACT[b]) for _, b in rots])
        pair = lambda zs: (np.array([z.real for z in zs]), np.array([z.imag for z in zs]))
        unit_rot = (pair(fr), pair(fc))
        super_rot = (pair([lcpu._unit_power(EXACT[a], tr) for a, _ in rots]),
                     pair([lcpu._unit_power(EXACT[b], tc) for _, b in rots]))
    else:
        fr = np.exp(1j * phases[0]) if lattice else np.ones(B, complex)
        fc = np.exp(1j * phases[1])
    tile = lambda F, shape: lcpu._tiled(F, Qr, Qc, shape, fr, fc)
    plain = lambda F, shape: lcpu._tiled(F, Qr, Qc, shape)
    out = []
    for rows, cols, big in ((R, Cc, False), (SR, SC, True)):
        with engine(B, rows, cols, DT, DX, dtype=dtype, boundary="lattice" if lattice else "periodic") as e:
            e.set_materials(plain(eps, (rows, cols)) if big else eps, MU0)
            if not lattice and layer:
                e.set_pml(layer, courant00=COURANT0)
            e.set_conductivity(plain(sigma, (rows, cols)) if big else sigma)
            rot = (super_rot if big else unit_rot) if rots is not None else None
            if lattice and rot is not None:
                e.set_lattice_phase(0, 0, rotation=rot)
            elif lattice:
                e.set_lattice_phase(*((tr * phases[0], tc * phases[1]) if big else phases))
            elif rot is not None:
                e.set_bloch_phase(None, rotation=rot[1])
            else:
                e.set_bloch_phase(tc * phases[1] if big else phases[1])
            e.set_bloch_dispersion(plain(wp2, (rows, cols)) if big else wp2, gam, om0)
            shapes = ((rows, cols), (rows, cols - 1), (rows - 1, cols), (rows, cols), (rows, cols), (rows, cols))
            s = [tile(F, sh) for F, sh in zip(start, shapes)] if big else start
            e.upload(*s[:3])
            if not lattice:
                e.upload_ezx(s[3])
            e.upload_bloch_dispersion(s[4], s[5])
            e.run(nsteps)
            out.append(e.download() + e.download_bloch_dispersion() + (() if lattice else (e.download_ezx(),)))
    unit, sup = out
    worst = 0.0
    # Hx: on the lattice row R-1 is never updated; Hy has R-1 rows and its column C-1 is never updated
    cuts = [(SR, SC), (SR - 1 if lattice else SR, SC - 1), (SR - 1, SC - 1), (SR, SC), (SR, SC), (SR, SC)]
    for name, F, G, cut in zip(("Ez", "Hx", "Hy", "Jh", "Q", "Ezx"), unit, sup, cuts):
        want = lcpu._tiled(F.astype(np.complex128), Qr, Qc, G.shape[1:], fr, fc)[:, :cut[0], :cut[1]]
        assert np.any(F), name
        worst = max(worst, np.abs(G[:, :cut[0], :cut[1]] - want).max() / np.abs(F).max())
    return worst


def check_supercell_exact(engine, kind, dtype, R, Cc, nsteps=60):
    rots = LATTICE_ROTS if kind == "lattice" else BLOCH_ROTS
    assert supercell_difference(engine, kind, dtype, R, Cc, rots=rots, nsteps=nsteps) == 0.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,R,Cc", [("lattice", 8, 6), ("bloch", 19, 8)])
def test_exact_rotations_match_their_supercell_bit_for_bit(kind, R, Cc, dtype):
    check_supercell_exact(oracle_for(kind), kind, dtype, R, Cc)


@pytest.mark.parametrize("kind,R,Cc", [("lattice", 8, 6), ("bloch", 19, 8)])
def test_general_phases_match_their_supercell_to_rounding(kind, R, Cc):
    phases = (np.array([0.7, np.pi, -2.2]), np.array([-1.9, 2.4, 0.3]))
    d = supercell_difference(oracle_for(kind), kind, np.float64, R, Cc, phases=phases, nsteps=200)
    print(f"{kind}: unit cell against its supercell after 200 steps, Jh and Q included: {d:.3e} (bound {SUPER_BOUND:.0e})")
    assert d <= SUPER_BOUND


# ---- 5. negated phases conjugate ----------------------------------------------------------------------------------------------

def check_conjugate(engine, kind, dtype, R, Cc, nsteps=60, layer=0):
    lattice = kind == "lattice"
    B = 3
    rng = np.random.default_rng(9)
    g = 0 if lattice else max(6, layer)
    eps = (EPS0 * (1 + 3 * rng.random((B, R, Cc)))).astype(dtype)
    sigma, wp2 = np.zeros((B, R, Cc)), np.zeros((B, R, Cc))
    sigma[:, g:R - g] = 5.0 * rng.random((B, R - 2 * g, Cc))
    wp2[:, g:R - g] = 2e25 * rng.random((B, R - 2 * g, Cc))
    (cr, sr), (cc, sc) = lcpu._rotations(B, dtype, seed=5)
    amps = rng.standard_normal((B, nsteps))
    res = []
    for sign in (1, -1):
        with engine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice" if lattice else "periodic") as e:
            e.set_materials(eps, MU0)
            if layer:
                e.set_pml(layer, courant00=COURANT0)
            e.set_conductivity(sigma).set_sources(np.array([(g, 0, 1, 1)] * B))
            if lattice:
                e.set_lattice_phase(0, 0, rotation=((cr, sign * sr), (cc, sign * sc)))
            else:
                e.set_bloch_phase(None, rotation=(cc, sign * sc))
            e.set_bloch_dispersion(wp2, np.array([1e11, 0.0, 4e10]), np.array([0.0, 3e11, 1e11]))
            e.run(nsteps, amps)
            res.append(e.download() + e.download_bloch_dispersion())
    a, b = res
    assert np.abs(a[0].imag).max() > 0 and np.abs(a[3].imag).max() > 0 and np.abs(a[4].imag).max() > 0
    for name, x, y in zip(("Ez", "Hx", "Hy", "Jh", "Q"), a, b):
        assert np.array_equal(y, np.conj(x)), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,R,Cc", [("lattice", 8, 6), ("bloch", 17, 6)])
def test_negated_phases_give_the_conjugate_bit_for_bit(kind, R, Cc, dtype):
    check_conjugate(oracle_for(kind), kind, dtype, R, Cc)


# ---- 6. oblique transmission through a Drude slab ------------------------------------------------------------------------------

SLAB_R, SLAB_C, SLAB_L, SLAB_SRC, SLAB_ROWS, SLAB_PROBE, SLAB_STEPS = 220, 5, 20, 40, (100, 120), 170, 6000
SLAB_PHI = 0.2
FREQS = np.array([40e9, 50e9, 60e9, 70e9, 80e9])
DRUDE = (WP2, 1e11, 0.0)
# Worst |T| error of the stand-in over FREQS, measured on the CPU (the test prints it): 2.581e-3 in float64 and in float32
# (the scheme's own dispersion error at 50 cells per wavelength, larger along an oblique path, and what the layer
# reflects at 17 to 37 degrees).  The bound is twice the measured value.  Without the pole the check misses by 0.88; the
# normal-incidence formula misses by 0.050.
OBLIQUE_MEASURED = {"float64": 2.6e-3, "float32": 2.6e-3}
OBLIQUE_BOUND = {k: 2 * v for k, v in OBLIQUE_MEASURED.items()}      # 5.2e-3


def oblique_spectrum(dtype, pole):
    """The complex probe spectrum at FREQS behind the slab (pole None: no slab)."""
    from fdtd2d_amd.api import ricker_amplitude
    R, C = SLAB_R, SLAB_C
    eng = BlochDispersiveOracle(1, R, C, DT, DX, dtype=dtype)
    eng.set_materials(np.full((1, R, C), EPS0), MU0)
    eng.set_pml(SLAB_L, courant00=COURANT0)
    eng.set_bloch_phase(SLAB_PHI)
    w = np.zeros((1, R, C))
    w[:, SLAB_ROWS[0]:SLAB_ROWS[1], :] = 0.0 if pole is None else pole[0]
    eng.set_bloch_dispersion(w, *((0.0, 0.0) if pole is None else pole[1:]))
    eng.set_sources(np.array([[SLAB_SRC, 0, 1, C - 1]])).set_bloch_source("ramp")
    eng.set_probes(np.array([[SLAB_PROBE, 1]]), SLAB_STEPS)
    eng.run(SLAB_STEPS, np.array([[ricker_amplitude(n * DT, 60e9) for n in range(SLAB_STEPS)]]))
    tr = eng.read_probes()[0, 0]
    t = (np.arange(SLAB_STEPS) + 1) * DT
    return np.array([np.sum(tr * np.exp(-2j * np.pi * f * t)) for f in FREQS])


def oblique_transmission(pole, phi):
    """|T| of a slab of thickness d in vacuum for s-polarisation (E along the invariant axis) at the transverse
    wavenumber kx = phi / ((C-1) dx): kz = sqrt(eps_r k0^2 - kx^2) on either side, eps_r(w) = 1 + wp2 / (omega0^2 - w^2 -
    i gamma w) in the slab, T = 4 k0z k1z e^{i k1z d} / ((k0z + k1z)^2 - (k0z - k1z)^2 e^{2 i k1z d})."""
    wp2, gamma, omega0 = pole
    w = 2 * np.pi * FREQS
    k0 = w * np.sqrt(EPS0 * MU0)
    kx = phi / ((SLAB_C - 1) * DX)
    er = (1 + wp2 / (omega0 ** 2 - w ** 2 - 1j * gamma * w)).astype(complex)
    k0z = np.sqrt((k0 ** 2 - kx ** 2).astype(complex))
    k1z = np.sqrt(er * k0 ** 2 - kx ** 2)
    k1z = np.where(k1z.imag < 0, -k1z, k1z)
    ph = np.exp(1j * k1z * (SLAB_ROWS[1] - SLAB_ROWS[0]) * DX)
    return np.abs(4 * k0z * k1z * ph / ((k0z + k1z) ** 2 - (k0z - k1z) ** 2 * ph ** 2))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oblique_slab_transmission_follows_the_analytic_formula(dtype):
    name = np.dtype(dtype).name
    T = np.abs(oblique_spectrum(dtype, DRUDE)) / np.abs(oblique_spectrum(dtype, None))
    want = oblique_transmission(DRUDE, SLAB_PHI)
    err = np.abs(T - want).max()
    print(f"{name}: |T| {np.round(T, 4)} want {np.round(want, 4)}: worst error {err:.3e} (bound {OBLIQUE_BOUND[name]})")
    assert np.all(2 * np.pi * FREQS * np.sqrt(EPS0 * MU0) > SLAB_PHI / ((SLAB_C - 1) * DX))      # all propagate
    assert err <= OBLIQUE_BOUND[name]
    # the run without the pole transmits everything: it cannot pass; nor can the formula at normal incidence
    assert np.abs(1.0 - want).max() > 0.3
    assert np.abs(oblique_transmission(DRUDE, 0.0) - want).max() > 4 * OBLIQUE_BOUND[name]


# ---- 7. the stability bound ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,pole", [("lattice", "drude"), ("bloch", "lorentz")])
def test_a_lossless_pole_at_3p9_stays_bounded(kind, pole):
    """gamma = 0, no conductivity, no layer: nothing leaves or damps.  Every cell that may carry the pole sits at 3.9 on
    the stability expression.  The bound is the real pole's (tests/test_batch_dispersive_cpu.py): the largest |Ez| of
    steps 1000..5000 is at most 10 times that of the first 1000."""
    N = 5000
    R, C = (9, 9) if kind == "lattice" else (30, 9)
    omega0 = 0.0 if pole == "drude" else 1.0 / DT
    courant = 8 * DT * DT / (EPS0 * MU0 * DX * DX)
    wp2 = (3.9 - courant - (DT * omega0) ** 2) / (DT * DT)
    assert abs(stability(wp2, omega0, EPS0, MU0, DT, DX) - 3.9) < 1e-12
    eng = oracle_for(kind)(1, R, C, DT, DX, dtype=np.float32)
    eng.set_materials(np.full((1, R, C), EPS0), MU0)
    if kind == "lattice":
        eng.set_lattice_phase(0.7, -1.9)
    else:
        eng.set_bloch_phase(1.3)
    eng.set_bloch_dispersion(wp2, 0.0, omega0)
    assert np.count_nonzero(eng.wp2) == (R * C if kind == "lattice" else (R - 12) * C)
    eng.set_sources(np.array([[3, 2, 1, 1]]))
    rows = (0, 2, 5, 7) if kind == "lattice" else (4, 10, 15, 20)
    eng.set_probes(np.array([[r, c] for r in rows for c in (1, 5)]), N)
    amps = np.zeros((1, N))
    amps[0, :200] = np.sin(2 * np.pi * 60e9 * DT * np.arange(200)) * np.hanning(200)
    eng.run(N, amps)
    tr = np.abs(eng.read_probes()[0])
    assert np.all(np.isfinite(eng.Ez)) and np.all(np.isfinite(eng.Q)) and np.all(np.isfinite(eng.Q_i))
    early, late = tr[:, :1000].max(), tr[:, 1000:].max()
    print(f"{kind} {pole}: early {early:.3e} late {late:.3e} ratio {late / early:.3f}")
    assert early > 0 and late <= 10 * early and np.abs(eng.Ez_i).max() > 0


# ---- 8. the host refusals -----------------------------------------------------------------------------------------------

def _snapshot(e):
    return [a.copy() for a in (e.wp2, e.gamma, e.omega0, e.Jh, e.Q, e.Jh_i, e.Q_i, e.Ez, e.Ez_i)]


@pytest.mark.parametrize("kind", ["bloch", "lattice"])
def test_the_stand_in_refuses_what_the_library_refuses(kind):
    R, C = (23, 11) if kind == "bloch" else (11, 13)
    eng, amps = members(oracle_for(kind), kind, np.float32, R, C, 10, layer=4 if kind == "bloch" else 0)
    eng.run(3, amps)
    before = _snapshot(eng)
    ok = eng.wp2.copy()
    bad_cells = [(-1.0, (1, 8, 3)), (np.nan, (0, 8, 3)), (np.inf, (0, 8, 3)), (20.0 / DT ** 2, (0, 8, 3))]     # eps is up to 3 EPS0
    if kind == "bloch":
        bad_cells += [(1e22, (1, 5, 3)), (1e22, (1, R - 6, 0))]          # the margin on the rows; columns are all allowed
    for bad, at in bad_cells:
        w = ok.copy()
        w[at] = bad
        with pytest.raises(AssertionError):
            eng.set_bloch_dispersion(w, GAMMA, OMEGA0)
    for gamma, omega0 in ((-1.0, 0.0), (np.nan, 0.0), (0.0, -1.0), (0.0, np.inf), (0.0, 2.0 / DT)):
        with pytest.raises(AssertionError):
            eng.set_bloch_dispersion(ok, gamma, omega0)
    with pytest.raises(AssertionError, match="use set_bloch_dispersion"):
        eng.set_dispersion(ok, 0.0, 0.0)
    for call in (lambda: eng.set_bloch_point_sources(np.array([(8, 3)]), np.ones((1, 1))),
                 lambda: eng.run_bloch_channels(4, None, np.zeros((1, 4))), lambda: eng.hold_bloch_window(),
                 lambda: eng.bloch_window_product(np.ones(2))):
        with pytest.raises(AssertionError):
            call()
    if kind == "bloch":
        with pytest.raises(AssertionError, match="turning the Bloch phase off"):
            eng.set_bloch_phase(None)
    for x, y in zip(before, _snapshot(eng)):
        assert np.array_equal(x, y, equal_nan=True)
    # without complex fields, and without the pole
    plain = BlochDispersiveOracle(2, 23, 11, DT, DX, dtype=np.float32)
    plain.set_materials(np.full((2, 23, 11), EPS0), MU0)
    with pytest.raises(AssertionError, match="needs a Bloch phase or the lattice mode"):
        plain.set_bloch_dispersion(0.0)
    plain.set_bloch_phase(0.3)
    for call in (lambda: plain.set_bloch_dispersion_window((8, 0, 2, 2), np.ones((2, 2, 2))),
                 lambda: plain.download_bloch_dispersion(), lambda: plain.upload_bloch_dispersion(np.zeros((2, 23, 11)))):
        with pytest.raises(AssertionError, match="no pole is set"):
            call()
    plain.set_dft_window((8, 0, 2, 2), np.array([1e11])).hold_bloch_window()
    with pytest.raises(AssertionError, match="exclude the pole"):
        plain.set_bloch_dispersion(0.0)
    # what keeps working: new rotations with the state kept, the window of strengths, removal
    eng.set_bloch_dispersion_window((8, 0, 2, 3), np.full((5, 2, 3), 1e24))
    assert np.all(eng.wp2[:, 8:10, 0:3] == 1e24)
    jh = eng.Jh.copy()
    if kind == "bloch":
        eng.set_bloch_phase(0.9)
    else:
        eng.set_lattice_phase(0.9, -0.4)
    assert np.array_equal(eng.Jh[:, :-1, :-1], jh[:, :-1, :-1]) and eng.dispersive
    eng.set_bloch_dispersion(None)
    assert not eng.dispersive and eng.Jh is None


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def test_the_python_wrappers_refuse_an_engine_without_complex_fields(fd):
    from fdtd2d_amd import _abi
    calls = [lambda e: e.set_bloch_dispersion(1e22, 1e11, 0.0), lambda e: e.set_bloch_dispersion(None),
             lambda e: e.set_bloch_dispersion_window((2, 2, 2, 2), np.zeros((3, 2, 2))),
             lambda e: e.download_bloch_dispersion(), lambda e: e.upload_bloch_dispersion(np.zeros((3, 17, 13)))]
    for boundary in ("periodic", "pml"):
        for call in calls:
            eng = lcpu.host_engine(fd, lattice=False, boundary=boundary)
            with pytest.raises(fd.Fdtd2dError, match="needs a Bloch phase or the lattice mode") as ei:
                call(eng)
            assert ei.value.code == _abi.E_STATE and "set_dispersion" in str(ei.value)
    # bad shapes are refused before the library sees them; good ones reach it
    eng = lcpu.host_engine(fd)
    with pytest.raises(ValueError, match=r"gamma must be a scalar or have shape \(3,\)"):
        eng.set_bloch_dispersion(1e22, np.zeros(2), 0.0)
    with pytest.raises(ValueError, match=r"omega0 must be a scalar or have shape \(3,\)"):
        eng.set_bloch_dispersion(1e22, 0.0, np.zeros(4))
    with pytest.raises(ValueError, match="wp2"):
        eng.set_bloch_dispersion(np.zeros((3, 17, 12)), 0.0, 0.0)
    with pytest.raises(ValueError, match="window must be 4 integers"):
        eng.set_bloch_dispersion_window((2, 2, 2), np.zeros((3, 2, 2)))
    with pytest.raises(ValueError, match="Jh"):
        eng.upload_bloch_dispersion(np.zeros((3, 17, 12)))
    with pytest.raises(AssertionError, match=r"the library was called \(fdtd2d_batch_set_bloch_dispersion\)"):
        eng.set_bloch_dispersion(1e22, 1e11, 0.0)
    with pytest.raises(AssertionError, match=r"the library was called \(fdtd2d_batch_transfer_bloch_dispersion\)"):
        eng.upload_bloch_dispersion(Q=np.zeros((3, 17, 13), complex))


@pytest.mark.parametrize("kwargs,match", [
    (dict(boundary="periodic"), "bloch_dispersion needs bloch_phase"),
    (dict(boundary="pml"), "bloch_dispersion needs bloch_phase"),
    (dict(boundary="mur", bloch_phase=0.3), 'bloch_phase needs boundary="periodic" or "lattice"'),
    (dict(boundary="periodic", bloch_phase=0.3, bloch_dispersion=(1e22, 1e11)),
     r"bloch_dispersion must be \(wp2, gamma, omega0\)"),
    (dict(boundary="periodic", bloch_phase=0.3, dispersion=(1e22, 1e11, 0.0)),
     "dispersion is not available with bloch_phase"),
    (dict(boundary="lattice", dispersion=(1e22, 1e11, 0.0)), 'dispersion is not available with boundary="lattice"'),
])
def test_run_fdtd_batch_refuses_bad_bloch_dispersion_on_the_host(monkeypatch, kwargs, match):
    import fdtd2d_amd as fd

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    base = dict(nsteps=10, sources=np.array([[8, 3]] * 2), pml_cells=4, bloch_dispersion=(1e22, 1e11, 0.0))
    with pytest.raises(ValueError, match=match):
        fd.run_fdtd_batch(np.full((2, 23, 13), EPS0), **dict(base, **kwargs))
    for good in (dict(boundary="periodic", bloch_phase=0.3), dict(boundary="lattice"),
                 dict(boundary="lattice", bloch_phase=(0.2, [0.1, 0.4]))):
        with pytest.raises(AssertionError, match="the device was touched"):
            fd.run_fdtd_batch(np.full((2, 23, 13), EPS0), **dict(base, **good))
