"""CPU-only checks of the lattice mode of the Hz polarisation (fdtd2d_batch_hz_lattice.h, batch.py): the stand-in
(tests/oracle_batch_hz_lattice.py) against code that already exists and against closed forms, plus the surface and the
host refusals.

1. Surface.  The header's symbols are declared with the header's signatures, exported by both libraries and bound; the
   info id 25 is named and was free.
2. Host refusals on an engine without a library, and run_fdtd_batch's checks before any engine exists.
3. Identities (a) to (e) of the header on the stand-in, in both dtypes on 11x13 and 23x19: (b) against ``LatticeOracle``
   with eps and mu exchanged, (c) against its own run without a pole, (d) and (e) bit for bit.
4. Supercells.  With the exact rotations (-1, 0) and (0, 1) a member equals its 2- or 4-cell supercell at zero phase bit
   for bit, along rows and along columns, fields and pole state; along columns the source is weighted per cell.
5. An eigenmode: a discrete plane wave of the vacuum cell keeps its shape and turns by exp(-i omega dt) per step.
6. The rods: a Drude rod in the cell has no cutoff in this polarisation (the lowest band starts at zero frequency) where
   the Ez polarisation has one.

``tests/test_gpu_batch_hz_lattice.py`` repeats the exact properties on the device through the ``check_*`` functions here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch_bloch_dispersive import LatticeDispersiveOracle
from oracle_batch_hz_lattice import HzLatticeOracle
from oracle_batch_lattice import LatticeOracle
from test_batch_lattice_cpu import EXACT, _tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_hz_lattice.h")
NAMES = ["fdtd2d_batch_is_hz_lattice", "fdtd2d_batch_set_hz_lattice"]
EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7
DT, DX = 5e-14, 1e-4
SHAPES = [(11, 13), (23, 19)]
WP2_TOP = (2 * np.pi * 300e9) ** 2


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def oracle(B, R, C, dtype):
    """The stand-in as a periodic engine in the Hz polarisation, as ``BatchEngine(...).set_polarization("hz")`` is."""
    return HzLatticeOracle(B, R, C, DT, DX, dtype=dtype)


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_hz_lattice_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_HZ_LATTICE_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_HZ_LATTICE_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_HZ_LATTICE_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "const fdtd2d_batch_t *": ctypes.c_void_p,
             "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_HZ_LATTICE_SIGNATURES[n][1], n
    every = [v for k, v in vars(_abi).items() if k.endswith("SIGNATURES") and k != "BATCH_HZ_LATTICE_SIGNATURES"]
    assert not any(set(_abi.BATCH_HZ_LATTICE_SIGNATURES) & set(s) for s in every)
    main = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    assert "hz_lattice" not in main.lower()                # a companion header: fdtd2d.h declares none of it


def test_hz_lattice_info_id_is_named_and_was_free():
    """The id is written relative to FDTD2D_BATCH_INFO_HZ_BLOCH (24): earlier tests pin that no other header writes a
    number, or an offset from FDTD2D_BATCH_INFO_FLUX_LDS, of 24 or more."""
    from fdtd2d_amd import _abi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    mine = strip(open(HEADER).read())
    assert re.findall(r"FDTD2D_BATCH_INFO_\w+\s*=\s*([^,}]+)", mine) == ["FDTD2D_BATCH_INFO_HZ_BLOCH + 1 "]
    assert not re.search(r"#define\s+FDTD2D_BATCH_(INFO|OPT)_", mine)
    assert _abi.BATCH_HZ_BLOCH_INFO + 1 == _abi.BATCH_HZ_LATTICE_INFO_ID == 25
    inc = os.path.join(ROOT, "include")
    for h in sorted(os.listdir(inc)):
        if h != os.path.basename(HEADER):
            assert "FDTD2D_BATCH_INFO_HZ_LATTICE" not in strip(open(os.path.join(inc, h)).read()), h
    ids = [v for k, v in vars(_abi).items() if isinstance(v, int) and "INFO" in k and k.startswith("BATCH_")]
    assert ids.count(25) == 1 and max(ids) == 25
    lib = _abi.load()
    assert lib.fdtd2d_batch_set_hz_lattice(None, None, None, None, None) == _abi.E_ARG
    assert lib.fdtd2d_batch_is_hz_lattice(None) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_HZ_LATTICE_INFO_ID) == _abi.E_ARG


def test_hz_lattice_python_surface(fd):
    E = fd.BatchEngine
    assert callable(E.set_hz_lattice_phase) and isinstance(E.hz_lattice, property) and E._hzlat is False
    assert list(inspect.signature(E.set_hz_lattice_phase).parameters) == ["self", "phi_rows", "phi_cols", "rotation"]
    assert inspect.signature(fd.run_fdtd_batch).parameters["hz_lattice_phase"].default is None
    assert "hz_lattice_phase" in inspect.getdoc(fd.run_fdtd_batch)
    for path in ("include/fdtd2d_batch_hz.h", "include/fdtd2d_batch_hz_bloch.h"):
        txt = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "Not available: the lattice mode" not in txt and "fdtd2d_batch_hz_lattice.h" in txt, path
    assert "set_hz_lattice_phase" in open(os.path.join(ROOT, "README.md")).read()


# ---- 2. host refusals ------------------------------------------------------------------------------------------------

class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def host_engine(fd, mode=True, boundary="periodic", hz=True, count=3, rows=17, cols=13):
    """A BatchEngine without a handle, for the checks that never reach the library."""
    eng = object.__new__(fd.BatchEngine)
    eng._lib, eng._h = _NoLibrary(), ctypes.c_void_p()
    eng.count, eng.rows, eng.cols, eng.dt, eng.dx = count, rows, cols, DT, DX
    eng.dtype, eng.boundary = np.dtype(np.float32), boundary
    eng._pml_on, eng._pml_chosen, eng._pml_L = False, True, 0
    eng._win, eng._nprobe, eng._npoint = (1, 2, 2), 1, (0, 0)
    eng._flux, eng._bflux, eng._hzflux, eng._hzbflux = None, False, False, False
    one, zero = np.ones(count), np.zeros(count)
    eng._hz = hz
    eng._hzb = eng._hzlat = hz and mode
    eng._lattice = ((one, zero), (one, zero)) if mode else None
    eng._bloch = (one, zero) if mode else None
    eng._phi = zero if mode else None
    return eng


@pytest.mark.parametrize("call,what", [
    (lambda e: e.set_pml(3), "a PML layer"),
    (lambda e: e.download_ezx(), "download_ezx"),
    (lambda e: e.upload_ezx(np.zeros((3, 17, 13))), "upload_ezx"),
    (lambda e: e.set_hz_bloch_phase(0.3), "set_hz_bloch_phase"),
    (lambda e: e.set_hz_bloch_phase(None), "set_hz_bloch_phase"),
    (lambda e: e.set_bloch_phase(0.3), "set_bloch_phase"),
    (lambda e: e.set_hz_flux_lines([("row", 5, 0, 12)], [1e11]), "set_hz_flux_lines"),
    (lambda e: e.set_hz_bloch_flux_lines([("row", 5, 0, 12)], [1e11]), "set_hz_bloch_flux_lines"),
    (lambda e: e.set_dft(1e11), "the whole-grid transform"),
    (lambda e: e.set_point_sources(np.array([(5, 5)]), np.ones((1, 1))), "a point source"),
    (lambda e: e.run(4, None, np.zeros((1, 4))), "a run with channels"),
    (lambda e: e.set_polarization("ez"), "a change of polarisation"),
    (lambda e: e.set_dispersion_window((2, 2, 2, 2), np.zeros((3, 2, 2))), "a dispersive pole"),
])
def test_what_the_hz_lattice_mode_excludes_is_refused_on_the_host(fd, call, what):
    from fdtd2d_amd import _abi
    with pytest.raises(fd.Fdtd2dError, match="is not available in the lattice mode") as ei:
        call(host_engine(fd))
    assert ei.value.code == _abi.E_STATE and what in str(ei.value)


def test_the_mode_keeps_the_materials_and_the_monitors_of_the_period(fd):
    """What the mode allows reaches the library: the pole and the conductivity anywhere in the period, windows and probes
    next to the images."""
    eng = host_engine(fd)
    assert eng.conductivity_margin == 0
    ok = eng._hz_allowed()
    assert ok[:, :16, :12].all() and not ok[:, 16, :].any() and not ok[:, :, 12].any()
    for call in (lambda e: e.set_dispersion(1e22, 1e11, 0.0), lambda e: e.set_conductivity(2.0),
                 lambda e: e.set_dft_window((13, 9, 3, 3), [1e11]), lambda e: e.set_probes([(0, 0), (15, 11)], 10),
                 lambda e: e.set_hz_lattice_phase(0.3, [0.1, 0.2, 0.3]), lambda e: e.set_hz_lattice_phase(None, None),
                 lambda e: e.set_hz_lattice_phase(0, 0, rotation=(EXACT["half"], EXACT["quarter"]))):
        with pytest.raises(AssertionError, match="the library was called"):
            call(host_engine(fd))
    assert host_engine(fd, mode=False).conductivity_margin == 6


def test_monitors_in_the_images_are_refused_on_the_host(fd):
    from fdtd2d_amd import _abi
    for call in (lambda e: e.set_dft_window((4, 10, 3, 3), [1e11]), lambda e: e.set_dft_window((14, 2, 3, 3), [1e11]),
                 lambda e: e.set_probes([(4, 2), (9, 12)], 10), lambda e: e.set_probes([(16, 2)], 10)):
        with pytest.raises(fd.Fdtd2dError, match="touches row 16 or column 12, the images of row 0 and column 0") as ei:
            call(host_engine(fd))
        assert ei.value.code == _abi.E_ARG


def test_bad_hz_lattice_arguments_are_refused_on_the_host(fd):
    from fdtd2d_amd import _abi
    new = lambda **kw: host_engine(fd, mode=False, **kw)
    with pytest.raises(ValueError, match=r"phi_rows must be a scalar or have shape \(3,\)"):
        new().set_hz_lattice_phase(np.zeros(2), 0.0)
    with pytest.raises(ValueError, match=r"phi_cols must be a scalar or have shape \(3,\)"):
        new().set_hz_lattice_phase(0.0, np.zeros(4))
    with pytest.raises(ValueError, match="phi_cols must be finite"):
        new().set_hz_lattice_phase(0.0, np.nan)
    with pytest.raises(ValueError, match="phi_rows and phi_cols must both be given"):
        new().set_hz_lattice_phase(0.3, None)
    with pytest.raises(ValueError, match=r"cc must be a scalar or have shape \(3,\)"):
        new().set_hz_lattice_phase(0, 0, rotation=((1.0, 0.0), (np.ones(4), 0.0)))
    with pytest.raises(ValueError, match="rotation must be two pairs"):
        new().set_hz_lattice_phase(0, 0, rotation=(1.0, 0.0))
    with pytest.raises(fd.Fdtd2dError, match="set_hz_lattice_phase needs the Hz polarisation") as ei:
        new(hz=False).set_hz_lattice_phase(0.3, 0.1)
    assert ei.value.code == _abi.E_STATE
    for boundary in ("pml", "lattice"):
        with pytest.raises(fd.Fdtd2dError, match="the lattice mode of the Hz polarisation needs periodic columns") as ei:
            new(boundary=boundary).set_hz_lattice_phase(0.3, 0.1)
        assert ei.value.code == _abi.E_STATE

    def beside(**attrs):
        e = new()
        for k, v in attrs.items():
            setattr(e, k, v)
        return e
    one = (np.ones(3), np.zeros(3))
    for eng, match in ((beside(_pml_on=True, _pml_L=4), "has no layer"),
                       (beside(_hzb=True, _bloch=one), "while a Bloch phase is set"),
                       (beside(_flux=(None, None), _hzflux=True), "while flux lines are set"),
                       (beside(_npoint=(1, 1)), "a point source")):
        with pytest.raises(fd.Fdtd2dError, match=match) as ei:
            eng.set_hz_lattice_phase(0.3, 0.1)
        assert ei.value.code == _abi.E_STATE and "lattice mode of the Hz polarisation" in str(ei.value)
    with pytest.raises(AssertionError, match=r"the library was called \(fdtd2d_batch_set_hz_lattice\)"):
        new().set_hz_lattice_phase(0.3, 0.1)
    # the Ez lattice mode stays closed to an Hz engine, whatever its mode
    for eng in (new(), host_engine(fd)):
        with pytest.raises(fd.Fdtd2dError, match='set_lattice_phase needs boundary="lattice"'):
            eng.set_lattice_phase(0.3, 0.1)
    with pytest.raises(fd.Fdtd2dError, match="Hz polarisation"):
        host_engine(fd, mode=False, boundary="lattice").set_lattice_phase(0.3, 0.1)
    with pytest.raises(fd.Fdtd2dError, match="no Bloch phase of the Hz polarisation is set"):
        new().set_hz_bloch_source("ramp")
    with pytest.raises(ValueError, match='weights="ramp" needs the phases'):
        e = host_engine(fd)
        e._phi = None
        e.set_hz_bloch_source("ramp")


def test_run_fdtd_batch_checks_its_hz_lattice_arguments_on_the_host(monkeypatch, fd):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    eps = np.full((2, 17, 13), EPS0)
    kw = dict(nsteps=10, sources=np.array([(5, 5), (5, 5)]), dt=DT, dx=DX, pml_cells=0)
    hz = dict(kw, polarization="hz", boundary="periodic")
    with pytest.raises(ValueError, match='hz_lattice_phase needs polarization="hz"'):
        fd.run_fdtd_batch(eps, boundary="periodic", hz_lattice_phase=(0.2, 0.1), **kw)
    with pytest.raises(ValueError, match='hz_lattice_phase needs boundary="periodic"'):
        fd.run_fdtd_batch(eps, boundary="pml", polarization="hz", hz_lattice_phase=(0.2, 0.1), **dict(kw, pml_cells=3))
    with pytest.raises(ValueError, match='polarization="hz" needs boundary="pml" or "periodic"'):     # stays refused
        fd.run_fdtd_batch(eps, boundary="lattice", polarization="hz", **kw)
    with pytest.raises(ValueError, match="hz_lattice_phase and hz_bloch_phase exclude each other"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), hz_bloch_phase=0.3, **hz)
    with pytest.raises(ValueError, match="hz_lattice_phase is not available with a layer"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), **dict(hz, pml_cells=3))
    with pytest.raises(ValueError, match=r"hz_lattice_phase must be \(phi_rows, phi_cols\)"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=0.2, **hz)
    with pytest.raises(ValueError, match=r"phi_cols must be a scalar or have shape \(2,\)"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, np.zeros(3)), **hz)
    with pytest.raises(ValueError, match="phi_rows must be finite"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(np.inf, 0.0), **hz)
    with pytest.raises(ValueError, match="omega .* is not available with hz_lattice_phase"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), omega=1e11, **hz)
    lines = dict(hz_flux_lines="hz_flux_omegas", hz_bloch_flux_lines="hz_bloch_flux_omegas")
    for name, om in lines.items():
        with pytest.raises(ValueError, match=f"{name} is not available with hz_lattice_phase"):
            fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), **{name: [("row", 8, 0, 12)], om: [1e11]}, **hz)
    with pytest.raises(ValueError, match="touches row 16 or column 12"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), dft_window=(3, 11, 2, 2), window_omegas=[1e11], **hz)
    with pytest.raises(ValueError, match="touches row 16 or column 12"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), dft_window=(15, 3, 2, 2), window_omegas=[1e11], **hz)
    with pytest.raises(ValueError, match="a probe lies in row 16 or column 12"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), probes=[(16, 3)], **hz)
    with pytest.raises(ValueError, match="a probe lies in row 16 or column 12"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, 0.1), probes=[(3, 12)], **hz)
    with pytest.raises(AssertionError, match="the device was touched"):
        fd.run_fdtd_batch(eps, hz_lattice_phase=(0.2, [0.1, 0.4]), source_weights="ramp", dispersion=(1e22, 1e11, 0.0),
                          conductivity=1.0, dft_window=(3, 10, 2, 2), window_omegas=[1e11], probes=[(0, 0), (15, 11)], **hz)


# ---- 3. the identities of the header (also run on the device: tests/test_gpu_batch_hz_lattice.py) ------------------------

def members(seed, B, R, C, dtype, metal=True):
    """eps, mu, and (metal) a conductivity and pole strengths that reach row 0, column 0, row R-2 and column C-2; a random
    complex start of the fields and of the pole state, of the batch dtype."""
    rng = np.random.default_rng(seed)
    eps = (EPS0 * (1 + 3 * rng.random((B, R, C)))).astype(dtype)
    mu = (MU0 * (1 + 0.5 * rng.random((B, R, C)))).astype(dtype)
    sigma, wp2 = np.zeros((B, R, C)), np.zeros((B, R, C))
    if metal:
        per = (B, R - 1, C - 1)
        sigma[:, :-1, :-1] = np.where(rng.random(per) < 0.4, 0.0, 5.0 * rng.random(per))
        wp2[:, :-1, :-1] = np.where(rng.random(per) < 0.3, 0.0, WP2_TOP * rng.random(per))
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(cdtype(dtype))
    fields = [cplx(B, R, C), cplx(B, R, C - 1), cplx(B, R - 1, C)]
    fields[1][:, -1, :] = 0                     # row R-1 of Ex and column C-1 of Ey are never written
    fields[2][:, :, -1] = 0
    state = [cplx(B, R, C) for _ in range(4)]
    for a in state:                             # the state lives on the period alone
        a[:, -1, :] = 0
        a[:, :, -1] = 0
    return dict(eps=eps, mu=mu, sigma=sigma, wp2=wp2, fields=fields, state=state,
                gamma=np.linspace(0.0, 1e11, B), omega0=2 * np.pi * np.linspace(0.0, 60e9, B))


def generic_rotations(B, dtype, seed=4):
    """Generic rotations, already rounded to the batch dtype: ((cr, sr), (cc, sc)), each (B,) float64."""
    ph = np.random.default_rng(seed).uniform(-np.pi, np.pi, (2, B))
    r = lambda v: v.astype(dtype).astype(np.float64)
    return (r(np.cos(ph[0])), r(np.sin(ph[0]))), (r(np.cos(ph[1])), r(np.sin(ph[1])))


def phased_run(new, dtype, m, rot, rect, amps, nsteps, pole=True, sigma=True, start=True, weights=None, prepare=None):
    """One run of the members m on the engine that new(B, R, C, dtype) makes: (Hz, Ex, Ey) and, with a pole,
    (Jx, Qx, Jy, Qy)."""
    B, R, C = m["eps"].shape
    with new(B, R, C, dtype) as e:
        e.set_materials(m["eps"], m["mu"]).set_sources(np.array([rect] * B))
        e.set_hz_lattice_phase(0, 0, rotation=rot)
        if sigma:
            e.set_conductivity(m["sigma"])
        if pole:
            e.set_dispersion(m["wp2"], m["gamma"], m["omega0"])
        if weights is not None:
            e.set_hz_bloch_source(weights)
        if start:
            e.upload(*m["fields"])
            if pole:
                e.upload_hz_dispersion(*m["state"])
        if prepare is not None:
            prepare(e)
        e.run(nsteps, amps)
        return tuple(e.download()) + (tuple(e.download_dispersion()) if pole else ())


def check_unit_rotations(new, dtype, R, C, nsteps=40, **kw):
    """(a): both rotations (1, 0), real amplitudes, unit weights, a real start: the imaginary parts stay zero."""
    B = 2
    m = members(3, B, R, C, dtype)
    m["fields"] = [a.real + 0j for a in m["fields"]]
    m["state"] = [a.real + 0j for a in m["state"]]
    one, zero = np.ones(B), np.zeros(B)
    amps = np.random.default_rng(1).standard_normal((B, nsteps))
    for F in phased_run(new, dtype, m, ((one, zero), (one, zero)), (3, 2, 2, 3), amps, nsteps, **kw):
        assert np.abs(F.real).max() > 0 and not F.imag.any()


def check_duality(new, new_ez, dtype, R, C, nsteps=40, **kw):
    """(b): without a conductivity and without a pole, the Ez lattice run with eps and mu exchanged, E negated."""
    B = 3
    m = members(5, B, R, C, dtype, metal=False)
    rot = generic_rotations(B, dtype)
    rng = np.random.default_rng(6)
    amps = rng.standard_normal((B, nsteps)) + 1j * rng.standard_normal((B, nsteps))
    w = np.exp(1j * rng.uniform(-3, 3, (B, C - 1)))
    hz, ex, ey = phased_run(new, dtype, m, rot, (R - 3, C - 4, 2, 3), amps, nsteps, pole=False, sigma=False, weights=w, **kw)
    with new_ez(B, R, C, dtype) as e:
        e.set_materials(m["mu"], m["eps"]).set_sources(np.array([(R - 3, C - 4, 2, 3)] * B))
        e.set_lattice_phase(0, 0, rotation=rot)
        e.set_bloch_source(w)
        e.upload(m["fields"][0], -m["fields"][1], -m["fields"][2])
        if kw.get("prepare") is not None:
            kw["prepare"](e)
        e.run(nsteps, amps)
        ez, hx, hy = e.download()
    assert np.abs(hz.imag).max() > 0 and np.abs(hz[:, -1, -1]).max() > 0
    assert np.array_equal(hz, ez) and np.array_equal(ex, -hx) and np.array_equal(ey, -hy)


def check_empty_pole(new, dtype, R, C, nsteps=40, **kw):
    """(c): sigma = 0, wp2 = 0 and zero state: the run without a pole, bit for bit, and the state stays zero."""
    B = 3
    m = members(7, B, R, C, dtype)
    m["sigma"][...] = 0
    m["wp2"][...] = 0
    m["state"] = [np.zeros_like(a) for a in m["state"]]
    rot = generic_rotations(B, dtype, seed=8)
    amps = np.random.default_rng(9).standard_normal((B, nsteps)) * np.exp(0.7j)
    a = phased_run(new, dtype, m, rot, (0, 0, 2, 2), amps, nsteps, **kw)
    b = phased_run(new, dtype, m, rot, (0, 0, 2, 2), amps, nsteps, pole=False, sigma=False, **kw)
    assert np.abs(a[0].imag).max() > 0
    for x, y in zip(a[:3], b):
        assert np.array_equal(x, y)
    assert not any(np.any(s) for s in a[3:])


def check_transpose(new, dtype, R, C, nsteps=40, **kw):
    """(d): the transposed member with its phases exchanged gives Hz^T, Ex = -Ey^T, Ey = -Ex^T, Jx = -Jy^T, Qx = -Qy^T,
    Jy = -Jx^T, Qy = -Qx^T bit for bit, with a conductivity, a pole and a complex start."""
    B = 3
    m = members(11, B, R, C, dtype)
    rot_r, rot_c = generic_rotations(B, dtype, seed=12)
    amps = np.random.default_rng(13).standard_normal((B, nsteps)) * np.exp(1j * np.array([0.3, 1.2, 2.5]))[:, None]
    t = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    hz, ex, ey, jx, qx, jy, qy = phased_run(new, dtype, m, (rot_r, rot_c), (2, C - 3, 2, 1), amps, nsteps, **kw)
    f, s = m["fields"], m["state"]
    mt = dict(eps=t(m["eps"]), mu=t(m["mu"]), sigma=t(m["sigma"]), wp2=t(m["wp2"]), gamma=m["gamma"], omega0=m["omega0"],
              fields=[t(f[0]), -t(f[2]), -t(f[1])], state=[-t(s[2]), -t(s[3]), -t(s[0]), -t(s[1])])
    hzt, ext, eyt, jxt, qxt, jyt, qyt = phased_run(new, dtype, mt, (rot_c, rot_r), (C - 3, 2, 1, 2), amps, nsteps, **kw)
    assert np.abs(hz.imag).max() > 0 and np.abs(hz[:, -1, -1]).max() > 0 and np.any(jx) and np.any(qy)
    assert np.array_equal(ext, -t(ey)) and np.array_equal(eyt, -t(ex))
    assert np.array_equal(jxt, -t(jy)) and np.array_equal(qxt, -t(qy))
    assert np.array_equal(jyt, -t(jx)) and np.array_equal(qyt, -t(qx))
    # Every cell of Hz but the corner image: that one is rho_r * (rho_c * Hz[0, 0]) here and rho_c * (rho_r * Hz[0, 0]) in
    # the transposed member (the column rotation comes first in both), two roundings in another order.  It is an output
    # of download alone; no step reads it.
    corner = np.zeros(hzt.shape, bool)
    corner[:, -1, -1] = True
    assert np.array_equal(hzt[~corner], t(hz)[~corner])
    assert np.abs(hzt[corner] - t(hz)[corner]).max() <= 4 * np.finfo(dtype).eps * np.abs(hz[:, 0, 0]).max()


def check_conjugate(new, dtype, R, C, nsteps=40, **kw):
    """(e): negated phases, conjugated start, real amplitudes and unit weights give the conjugate of every field."""
    B = 3
    m = members(15, B, R, C, dtype)
    (cr, sr), (cc, sc) = generic_rotations(B, dtype, seed=16)
    amps = np.random.default_rng(17).standard_normal((B, nsteps))
    a = phased_run(new, dtype, m, ((cr, sr), (cc, sc)), (0, 0, 1, 1), amps, nsteps, **kw)
    mc = dict(m, fields=[np.conj(x) for x in m["fields"]], state=[np.conj(x) for x in m["state"]])
    b = phased_run(new, dtype, mc, ((cr, -sr), (cc, -sc)), (0, 0, 1, 1), amps, nsteps, **kw)
    assert np.abs(a[0].imag).max() > 0 and len(a) == len(b) == 7
    for x, y in zip(a, b):
        assert np.array_equal(y, np.conj(x))


def ez_oracle(B, R, C, dtype):
    return LatticeOracle(B, R, C, DT, DX, dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("R,C", SHAPES)
def test_unit_rotations_keep_the_imaginary_parts_zero(R, C, dtype):
    check_unit_rotations(oracle, dtype, R, C)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("R,C", SHAPES)
def test_the_lossless_run_is_the_ez_lattice_run_with_exchanged_materials(R, C, dtype):
    check_duality(oracle, ez_oracle, dtype, R, C)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("R,C", SHAPES)
def test_an_empty_pole_is_no_pole(R, C, dtype):
    check_empty_pole(oracle, dtype, R, C)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("R,C", SHAPES)
def test_transposed_member_gives_the_transposed_fields_bit_for_bit(R, C, dtype):
    check_transpose(oracle, dtype, R, C)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("R,C", SHAPES)
def test_negated_phases_give_the_conjugate_bit_for_bit(R, C, dtype):
    check_conjugate(oracle, dtype, R, C)


# ---- 4. supercells with exact rotations ----------------------------------------------------------------------------------

SUPER_CASES = [("half", "one"), ("quarter", "one"), ("one", "half"), ("one", "quarter")]
ORDER = {"one": 1, "half": 2, "quarter": 4}


def check_supercell_exact(new, dtype, R, C, rot_r, rot_c, nsteps=40, seed=21, **kw):
    """A unit cell with the exact rotations (rot_r, rot_c) against its Nr x Nc-cell supercell at zero phase, N the order
    of the rotation: materials tiled, start fields and pole state tiled with the cell's power of the rotation.  Along
    columns a line source spans the supercell, cell n weighted with rho_c^n (the weights are per column); along rows
    there is no source, because the weights do not depend on the row.  Everything bit for bit, images included."""
    Qr, Qc, Nr, Nc = R - 1, C - 1, ORDER[rot_r], ORDER[rot_c]
    SR, SC = Nr * Qr + 1, Nc * Qc + 1
    m = members(seed, 1, R, C, dtype)
    m["gamma"], m["omega0"] = np.array([5e10]), np.array([2 * np.pi * 40e9])
    fr, fc = np.array([complex(*EXACT[rot_r])]), np.array([complex(*EXACT[rot_c])])
    rot = lambda a, b: ((np.array([EXACT[a][0]]), np.array([EXACT[a][1]])), (np.array([EXACT[b][0]]), np.array([EXACT[b][1]])))
    sourced = Nr == 1
    amps = np.random.default_rng(seed + 1).standard_normal((1, nsteps)) * np.exp(0.4j) if sourced else None
    base = np.exp(1j * np.random.default_rng(seed + 2).uniform(-3, 3, Qc))
    unit = phased_run(new, dtype, m, rot(rot_r, rot_c), (3, 0, 1, Qc) if sourced else (0, 0, 0, 0), amps, nsteps,
                      weights=base[None] if sourced else None, **kw)
    shapes = [(SR, SC), (SR, SC - 1), (SR - 1, SC)] + [(SR, SC)] * 4
    tile = lambda F, s: _tiled(F, Qr, Qc, s, fr, fc)
    plain = lambda F, s: _tiled(F, Qr, Qc, s)
    big = dict(eps=plain(m["eps"], shapes[0]), mu=plain(m["mu"], shapes[0]), sigma=plain(m["sigma"], shapes[0]),
               wp2=plain(m["wp2"], shapes[0]), gamma=m["gamma"], omega0=m["omega0"],
               fields=[tile(F, s) for F, s in zip(m["fields"], shapes)], state=[tile(F, s) for F, s in zip(m["state"], shapes[3:])])
    for a in (big["sigma"], big["wp2"]) + tuple(big["state"]):     # nothing in the supercell's own images
        a[:, -1, :] = 0
        a[:, :, -1] = 0
    big["fields"][1][:, -1, :] = 0
    big["fields"][2][:, :, -1] = 0
    wbig = (np.tile(base, Nc) * np.repeat(fc[0] ** np.arange(Nc), Qc))[None]
    sup = phased_run(new, dtype, big, rot("one", "one"), (3, 0, 1, Nc * Qc) if sourced else (0, 0, 0, 0), amps, nsteps,
                     weights=wbig if sourced else None, **kw)
    assert all(np.any(F.real) and np.any(F.imag) for F in unit)
    cuts = [(SR, SC), (SR - 1, SC - 1), (SR - 1, SC - 1)] + [(SR - 1, SC - 1)] * 4
    for F, G, cut in zip(unit, sup, cuts):
        want = _tiled(F, Qr, Qc, G.shape[1:], fr, fc)[:, :cut[0], :cut[1]]
        assert np.array_equal(G[:, :cut[0], :cut[1]], want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rot_r,rot_c", SUPER_CASES)
def test_exact_rotations_match_their_supercell_bit_for_bit(rot_r, rot_c, dtype):
    check_supercell_exact(oracle, dtype, 8, 6, rot_r, rot_c)


# ---- 5. an eigenmode of the vacuum cell ----------------------------------------------------------------------------------

EIG_QR, EIG_QC, EIG_PHASES, EIG_ORDER = 10, 12, (0.7, -2.1), (1, 0)
# measured on the stand-in (float64): the worst field's max|field - start * exp(-i omega N dt)| / amplitude
EIG_MEASURED = {200: 5.3e-15, 1000: 1.3e-14}


@pytest.mark.parametrize("nsteps", sorted(EIG_MEASURED))
def test_a_discrete_plane_wave_turns_by_its_yee_frequency(nsteps):
    """Vacuum, a period of 10 x 12, phases (0.7, -2.1), the harmonic (1, 0): Hz = exp(i (a i + b j)) with
    a = (phi_r + 2 pi) / 10, b = phi_c / 12, and Ex, Ey from the update equations half a step earlier.  With
    sin^2(omega dt / 2) = S^2 (sin^2(a/2) + sin^2(b/2)) every field after N steps is its start times exp(-i omega N dt).
    Measured on the stand-in, relative to each field's amplitude: 5.3e-15 at N = 200 and 1.3e-14 at N = 1000 (rounding
    alone; a sign error in either seam or either curl gives order 1).  The bound is ten times the measurement."""
    R, C = EIG_QR + 1, EIG_QC + 1
    a, b = (EIG_PHASES[0] + 2 * np.pi * EIG_ORDER[0]) / EIG_QR, (EIG_PHASES[1] + 2 * np.pi * EIG_ORDER[1]) / EIG_QC
    cb, ch = DT / (EPS0 * DX), DT / (MU0 * DX)
    half = np.arcsin(np.sqrt(cb * ch * (np.sin(a / 2) ** 2 + np.sin(b / 2) ** 2)))          # omega dt / 2
    pw = np.exp(1j * (a * np.arange(R)[:, None] + b * np.arange(C)[None, :]))
    X = cb * (np.exp(1j * a) - 1) / (-2j * np.sin(half))           # Ex = X pw exp(-i omega (n - 1/2) dt)
    Y = -cb * (np.exp(1j * b) - 1) / (-2j * np.sin(half))
    Hz, Ex, Ey = pw, (X * np.exp(1j * half) * pw)[:, :-1].copy(), (Y * np.exp(1j * half) * pw)[:-1, :].copy()
    Ex[-1, :] = 0
    Ey[:, -1] = 0
    ref = oracle(1, R, C, np.float64)
    ref.set_materials(EPS0, MU0).set_hz_lattice_phase(*EIG_PHASES)
    ref.upload(Hz[None], Ex[None], Ey[None])
    ref.run(nsteps)
    h, ex, ey = (f[0] for f in ref.download())
    turn = np.exp(-2j * half * nsteps)
    err = max(np.abs(h - turn * Hz).max(), np.abs(ex[:-1] - turn * Ex[:-1]).max() / abs(X),
              np.abs(ey[:, :-1] - turn * Ey[:, :-1]).max() / abs(Y))
    print(f"N = {nsteps}: omega = 2 pi {half / np.pi / DT / 1e9:.3f} GHz, worst relative error {err:.3e} "
          f"(measured {EIG_MEASURED[nsteps]:.1e}, bound ten times that)")
    assert err <= 10 * EIG_MEASURED[nsteps]


# ---- 6. the rods -----------------------------------------------------------------------------------------------------------

ROD_Q, ROD_STEPS, ROD_FC, ROD_SRC, ROD_PROBE = 16, 16384, 30e9, (2, 3), (13, 12)
ROD_WP2 = (2 * np.pi * 600e9) ** 2
ROD_PHASES = [(0.4, 0.0), (np.pi, 0.0)]
ROD_BIN = 1 / (ROD_STEPS * DT)                  # 1.22 GHz


def lowest_line(trace):
    """The frequency in Hz of the lowest spectral line of a complex probe trace.  The cells have no loss (gamma = 0), so
    a resonance is a line as narrow as the Hann window's main lobe, two bins to either side; the transient of the pulse
    itself is a broad bump under the pulse's own spectrum.  A line is a local maximum of the windowed spectrum above 5 %
    of the largest that falls to less than a quarter four bins away on both sides."""
    N = len(trace)
    spec = np.abs(np.fft.fft(trace * np.hanning(N)))[:N // 2]
    top = spec.max()
    for k in range(4, N // 2 - 4):
        if (spec[k] > 0.05 * top and spec[k] >= spec[k - 1] and spec[k] > spec[k + 1]
                and spec[k - 4] < 0.25 * spec[k] and spec[k + 4] < 0.25 * spec[k]):
            return k * ROD_BIN
    raise AssertionError("no line in the spectrum")


@pytest.fixture(scope="module")
def rod_lines(fd):
    """The lowest line per phase of the Hz member with the rod, of the Ez member with the rod and of the empty cell."""
    B, R = len(ROD_PHASES), ROD_Q + 1
    wp2 = np.zeros((B, R, R))
    wp2[:, 5:11, 5:11] = ROD_WP2                                  # a 6 x 6 Drude rod, gamma = 0
    pr, pc = (np.array(v) for v in zip(*ROD_PHASES))
    amps = np.tile([fd.ricker_amplitude(n * DT, ROD_FC) for n in range(ROD_STEPS)], (B, 1))
    src = np.array([ROD_SRC] * B)
    hz = oracle(B, R, R, np.float64)
    hz.set_materials(EPS0, MU0).set_sources(src).set_hz_lattice_phase(pr, pc).set_dispersion(wp2, 0.0, 0.0)
    ez = LatticeDispersiveOracle(B, R, R, DT, DX, dtype=np.float64)
    ez.set_materials(EPS0, MU0).set_sources(src).set_lattice_phase(pr, pc).set_bloch_dispersion(wp2, 0.0, 0.0)
    empty = oracle(B, R, R, np.float64)
    empty.set_materials(EPS0, MU0).set_sources(src).set_hz_lattice_phase(pr, pc)
    out = {}
    for name, e in (("hz", hz), ("ez", ez), ("empty", empty)):
        e.set_probes([ROD_PROBE], ROD_STEPS)
        e.run(ROD_STEPS, amps)
        out[name] = [lowest_line(t) for t in e.read_probes()[:, 0]]
    for b, ph in enumerate(ROD_PHASES):
        print(f"phases ({ph[0]:.3f}, {ph[1]:.3f}): lowest line Hz {out['hz'][b] / 1e9:.1f} GHz, Ez {out['ez'][b] / 1e9:.1f} GHz, "
              f"empty cell {out['empty'][b] / 1e9:.1f} GHz")
    return out


def test_the_rod_has_no_cutoff_in_the_hz_polarisation_near_gamma(rod_lines):
    """Phases (0.4, 0), a 16 x 16-cell period with a 6 x 6 Drude rod (wp = 2 pi 600 GHz, gamma = 0), float64, 16384 steps,
    one FFT bin = 1.22 GHz.  Measured on the stand-in: Hz 11.0 GHz, Ez 87.9 GHz, the empty cell 12.2 GHz.  With E across
    the rod the lowest band still starts at zero frequency, a little below the light line; with E along the rod it starts
    at the plasma-like cutoff."""
    hz, ez, empty = (rod_lines[k][0] for k in ("hz", "ez", "empty"))
    assert hz < empty + ROD_BIN
    assert ez > 3 * empty


def test_the_rod_lowers_the_hz_band_edge_and_raises_the_ez_one(rod_lines):
    """Phases (pi, 0).  Measured on the stand-in: Hz 72.0 GHz, Ez 108.6 GHz, the empty cell 94.0 GHz."""
    hz, ez, empty = (rod_lines[k][1] for k in ("hz", "ez", "empty"))
    assert abs(empty - 94e9) <= ROD_BIN
    assert hz < empty < ez
