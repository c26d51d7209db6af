"""CPU-only checks of the lattice mode of periodic batches (fdtd2d_batch_lattice.h, batch.py): the stand-in
(tests/oracle_batch_lattice.py) alone, plus the surface and the host refusals.

What pins the stand-in, and with it the definition:
  plane wave   on a uniform cell Ez = exp(i (theta_r i + theta_c j)) with H = 0 is an eigenvector of the step: after N steps
               Ez = a_N times the start, a_0 = 1, a_1 = 1 - 4S, a_{k+1} = (2 - 4S) a_k - a_{k-1},
               S = ce ch (sin^2(theta_r/2) + sin^2(theta_c/2)); both seams, both rotations and the corner enter
  supercell    a unit cell with the phases (phi_r, phi_c) is the 2 x 3-tile supercell with (2 phi_r, 3 phi_c); bit for bit
               with rotations that are exact in floating point
  transpose    (R, C, rho_r, rho_c, eps) and (C, R, rho_c, rho_r, eps^T) give Ez' = Ez^T, Hx' = -Hy^T, Hy' = -Hx^T bit for bit:
               every operation of the step maps to itself up to exact negations (the corner image, which download alone
               forms with the column rotation first, agrees to rounding)
  conjugate    negated phases with real amplitudes and unit weights give the complex conjugate bit for bit
  bands        the peaks of a probe spectrum of the empty lattice sit on the Yee frequencies of the folded plane waves

``tests/test_gpu_batch_lattice.py`` repeats the exact properties on the device through the ``check_*`` functions here."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle_batch_lattice import LatticeOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_lattice.h")
NAMES = ["fdtd2d_batch_is_lattice", "fdtd2d_batch_set_lattice"]
EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7
DT, DX = 5e-14, 1e-4
EXACT = {"one": (1.0, 0.0), "half": (-1.0, 0.0), "quarter": (0.0, 1.0)}      # rotations that are exact in any dtype


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_batch_lattice_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_LATTICE_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_LATTICE_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_LATTICE_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "const fdtd2d_batch_t *": ctypes.c_void_p,
             "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_LATTICE_SIGNATURES[n][1], n
    assert not set(_abi.BATCH_LATTICE_SIGNATURES) & set(_abi.SIGNATURES)
    main = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    assert "lattice" not in main.lower()                   # a companion header: fdtd2d.h declares none of it
    assert sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))) == \
        sorted(_abi.SIGNATURES)


def test_batch_lattice_header_adds_no_info_or_option_id():
    from fdtd2d_amd import _abi
    pat = r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)"
    assert re.findall(pat, open(HEADER).read()) == []
    lib = _abi.load()
    assert lib.fdtd2d_batch_set_lattice(None, None, None, None, None) == _abi.E_ARG
    assert lib.fdtd2d_batch_is_lattice(None) == _abi.E_ARG


def test_batch_lattice_python_surface(fd):
    E = fd.BatchEngine
    assert callable(E.set_lattice_phase) and isinstance(E.lattice, property) and E._lattice is None
    import inspect
    assert list(inspect.signature(E.set_lattice_phase).parameters) == ["self", "phi_rows", "phi_cols", "rotation"]
    assert "lattice" in inspect.getdoc(fd.run_fdtd_batch)


def test_the_no_periodic_rows_sentences_are_gone():
    for path, gone in (("README.md", "No periodic rows"), ("fdtd-2d_amd/batch.py", "There are no periodic rows"),
                       ("DESIGN.md", "there are no periodic rows")):
        assert gone not in " ".join(open(os.path.join(ROOT, path)).read().split()), path
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert 'boundary="lattice"' in readme and "bloch_phase=(" in readme      # the band-path sweep as one call


# ---- 2. host refusals ------------------------------------------------------------------------------------------------

class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def host_engine(fd, lattice=True, boundary="lattice", count=3, rows=17, cols=13):
    """A BatchEngine without a handle, for the checks that never reach the library."""
    eng = object.__new__(fd.BatchEngine)
    eng._lib, eng._h = _NoLibrary(), ctypes.c_void_p()
    eng.count, eng.rows, eng.cols, eng.dt, eng.dx = count, rows, cols, DT, DX
    eng.dtype, eng.boundary = np.dtype(np.float32), boundary
    eng._pml_on, eng._pml_chosen, eng._pml_L = False, True, 0
    eng._win, eng._nprobe, eng._npoint = (1, 2, 2), 1, (1, 1)
    one, zero = np.ones(count), np.zeros(count)
    eng._lattice = ((one, zero), (one, zero)) if lattice else None
    eng._bloch = (one, zero) if lattice else None
    eng._phi = zero if lattice else None
    return eng


@pytest.mark.parametrize("call,what", [
    (lambda e: e.set_pml(3), "a PML layer"),
    (lambda e: e.download_ezx(), "download_ezx"),
    (lambda e: e.upload_ezx(np.zeros((3, 17, 13))), "upload_ezx"),
    (lambda e: e.set_bloch_phase(0.3), "set_bloch_phase"),
    (lambda e: e.set_bloch_phase(None), "set_bloch_phase"),
    (lambda e: e.set_dispersion(1e22, 1e11, 0.0), "a dispersive pole"),
    (lambda e: e.set_dispersion_window((2, 2, 2, 2), np.zeros((3, 2, 2))), "a dispersive pole"),
    (lambda e: e.set_dft(1e11), "the whole-grid transform"),
    (lambda e: e.set_point_sources(np.array([(5, 5)]), np.ones((1, 1))), "a point source"),
    (lambda e: e.run(4, None, np.zeros((1, 4))), "a run with channels"),
    (lambda e: e.hold_dft_window(), "the held window"),
    (lambda e: e.dft_window_product(np.ones(1)), "the window product"),
    (lambda e: e.probe_spectra([1e11]), "fdtd2d_batch_probe_spectra"),
    (lambda e: e.field_absmax("Ez"), "fdtd2d_batch_field_absmax"),
    (lambda e: e.set_bloch_point_sources(np.array([(5, 5)]), np.ones((1, 1))), "a point source"),
    (lambda e: e.set_bloch_point_sources(None), "a point source"),
    (lambda e: e.run_bloch_channels(4, None, np.zeros((1, 4))), "a run with channels"),
    (lambda e: e.hold_bloch_window(), "the held window"),
    (lambda e: e.bloch_window_product(np.ones(1)), "the window product"),
])
def test_what_the_lattice_mode_excludes_is_refused_on_the_host(fd, call, what):
    from fdtd2d_amd import _abi
    with pytest.raises(fd.Fdtd2dError, match="is not available in the lattice mode") as ei:
        call(host_engine(fd))
    assert ei.value.code == _abi.E_STATE and what in str(ei.value)


def test_monitors_in_the_images_are_refused_on_the_host(fd):
    from fdtd2d_amd import _abi
    for call in (lambda e: e.set_dft_window((4, 10, 3, 3), [1e11]), lambda e: e.set_dft_window((14, 2, 3, 3), [1e11]),
                 lambda e: e.set_probes([(4, 2), (9, 12)], 10), lambda e: e.set_probes([(16, 2)], 10),
                 lambda e: e.set_probes(np.array([[(4, 2)], [(16, 12)], [(4, 3)]]), 10)):
        with pytest.raises(fd.Fdtd2dError, match="touches row 16 or column 12, the images of row 0 and column 0") as ei:
            call(host_engine(fd))
        assert ei.value.code == _abi.E_ARG
    for call in (lambda e: e.set_dft_window((13, 9, 3, 3), [1e11]), lambda e: e.set_probes([(0, 0), (15, 11)], 10)):
        with pytest.raises(AssertionError, match="the library was called"):
            call(host_engine(fd))


def test_bad_lattice_arguments_are_refused_on_the_host(fd):
    from fdtd2d_amd import _abi
    with pytest.raises(ValueError, match=r"phi_rows must be a scalar or have shape \(3,\)"):
        host_engine(fd).set_lattice_phase(np.zeros(2), 0.0)
    with pytest.raises(ValueError, match=r"phi_cols must be a scalar or have shape \(3,\)"):
        host_engine(fd).set_lattice_phase(0.0, np.zeros(4))
    with pytest.raises(ValueError, match=r"cc must be a scalar or have shape \(3,\)"):
        host_engine(fd).set_lattice_phase(0, 0, rotation=((1.0, 0.0), (np.ones(4), 0.0)))
    with pytest.raises(ValueError, match="rotation must be two pairs"):
        host_engine(fd).set_lattice_phase(0, 0, rotation=(1.0, 0.0))
    for boundary in ("periodic", "pml", "mur"):
        with pytest.raises(fd.Fdtd2dError, match='set_lattice_phase needs boundary="lattice"') as ei:
            host_engine(fd, lattice=False, boundary=boundary).set_lattice_phase(0.3, 0.1)
        assert ei.value.code == _abi.E_STATE
    with pytest.raises(AssertionError, match=r"the library was called \(fdtd2d_batch_set_lattice\)"):
        host_engine(fd).set_lattice_phase([0.1, 0.2, 0.3], 0.5)
    with pytest.raises(AssertionError, match=r"the library was called \(fdtd2d_batch_set_lattice\)"):
        host_engine(fd).set_lattice_phase(0, 0, rotation=(EXACT["half"], EXACT["quarter"]))
    assert host_engine(fd).conductivity_margin == 0
    with pytest.raises(ValueError, match="unknown boundary"):
        fd.BatchEngine(2, 40, 21, boundary="lattice2")


def test_run_fdtd_batch_checks_its_lattice_arguments_on_the_host(monkeypatch, fd):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)
    eps = np.full((2, 17, 13), EPS0)
    kw = dict(nsteps=10, sources=np.array([(5, 5), (5, 5)]), dt=DT, dx=DX, boundary="lattice")
    with pytest.raises(ValueError, match=r'boundary="lattice" takes bloch_phase=\(phi_rows, phi_cols\)'):
        fd.run_fdtd_batch(eps, bloch_phase=0.2, **kw)
    with pytest.raises(ValueError, match=r'boundary="lattice" takes bloch_phase=\(phi_rows, phi_cols\)'):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, 0.3, 0.4), **kw)
    with pytest.raises(ValueError, match=r"phi_cols must be a scalar or have shape \(2,\)"):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, np.zeros(3)), **kw)
    with pytest.raises(ValueError, match="omega .* is not available with bloch_phase"):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, 0.1), omega=1e11, **kw)
    with pytest.raises(ValueError, match='dispersion is not available with boundary="lattice"'):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, 0.1), dispersion=(1e22, 1e11, 0.0), **kw)
    with pytest.raises(ValueError, match="touches column 12"):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, 0.1), dft_window=(3, 11, 2, 2), window_omegas=[1e11], **kw)
    with pytest.raises(ValueError, match="touches row 16"):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, 0.1), dft_window=(15, 3, 2, 2), window_omegas=[1e11], **kw)
    with pytest.raises(ValueError, match="a probe lies in row 16"):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, 0.1), probes=[(16, 3)], **kw)
    with pytest.raises(ValueError, match="a probe lies in column 12"):
        fd.run_fdtd_batch(eps, bloch_phase=(0.2, 0.1), probes=[(3, 12)], **kw)
    with pytest.raises(ValueError, match='bloch_phase needs boundary="periodic" or "lattice"'):
        fd.run_fdtd_batch(eps, **dict(kw, boundary="mur"), bloch_phase=(0.2, 0.1))
    for phase in (None, (0.2, [0.1, 0.4])):
        with pytest.raises(AssertionError, match="the device was touched"):
            fd.run_fdtd_batch(eps, bloch_phase=phase, source_weights=None if phase is None else "ramp",
                              dft_window=(3, 10, 2, 2), window_omegas=[1e11], probes=[(0, 0), (15, 11)], **kw)


# ---- 3. the plane wave: an eigenvector of the step ---------------------------------------------------------------------

PW_QR, PW_QC, PW_STEPS, PW_BOUND = 6, 9, 300, 1e-10


@pytest.mark.parametrize("m,n", [(0, 0), (1, -1)])
@pytest.mark.parametrize("phi_r,phi_c", [(0.7, -1.9), (np.pi, 2.4)])
def test_plane_wave_follows_its_recurrence(phi_r, phi_c, m, n):
    R, Cc = PW_QR + 1, PW_QC + 1
    th_r, th_c = (phi_r + 2 * np.pi * m) / PW_QR, (phi_c + 2 * np.pi * n) / PW_QC
    start = np.exp(1j * (th_r * np.arange(R)[:, None] + th_c * np.arange(Cc)[None, :]))
    ref = LatticeOracle(1, R, Cc, DT, DX, dtype=np.float64)
    ref.set_materials(EPS0, MU0).set_lattice_phase(phi_r, phi_c)
    ref.upload(Ez=start[None])
    ref.run(PW_STEPS)
    S = (DT / (EPS0 * DX)) * (DT / (MU0 * DX)) * (np.sin(th_r / 2) ** 2 + np.sin(th_c / 2) ** 2)
    a0, a1 = 1.0, 1 - 4 * S
    for _ in range(PW_STEPS - 1):
        a0, a1 = a1, (2 - 4 * S) * a1 - a0
    Ez = ref.download()[0][0]
    err = np.abs(Ez - a1 * start).max()
    print(f"phases ({phi_r:.3f}, {phi_c:.3f}), order ({m}, {n}): a_N = {a1:.6f}, max|Ez - a_N start| = {err:.3e} "
          f"(bound {PW_BOUND:.0e})")
    assert abs(a1) > 0.05 and err <= PW_BOUND              # images and the corner included


# ---- 4. the exact properties (also run on the device: tests/test_gpu_batch_lattice.py) -----------------------------------

def random_members(seed, B, R, Cc, dtype):
    """eps with inclusions, a conductivity that reaches row 0 and column 0, complex start fields of the batch dtype."""
    rng = np.random.default_rng(seed)
    eps = (EPS0 * (1 + 3 * rng.random((B, R, Cc)))).astype(dtype)
    sigma = np.where(rng.random((B, R, Cc)) < 0.5, 0.0, 5.0 * rng.random((B, R, Cc)))
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(cdtype(dtype))
    return eps, sigma, (cplx(B, R, Cc), cplx(B, R, Cc - 1), cplx(B, R - 1, Cc))


def _unit_power(rot, k):
    """(c + i s)^k for an exact rotation, exactly."""
    z = complex(*rot) ** k
    return complex(round(z.real), round(z.imag))


def _powers(f, k):
    """f[b] ** k[t] by repeated multiplication (exact for the exact rotations): (B, len(k)) complex."""
    out = np.ones((len(f), len(k)), np.complex128)
    for t in range(int(k.max())):
        out = np.where(k[None, :] > t, out * f[:, None], out)
    return out


def _tiled(F, Qr, Qc, shape, fr=None, fc=None):
    """F's period (rows 0..Qr-1, columns 0..Qc-1) repeated over `shape`; with fr, fc: tile (a, b) times fr^a fc^b, per
    member."""
    i, j = np.arange(shape[0]), np.arange(shape[1])
    out = F[:, i % Qr][:, :, j % Qc]
    if fr is None:
        return np.ascontiguousarray(out)
    return (out * _powers(fr, i // Qr)[:, :, None] * _powers(fc, j // Qc)[:, None, :]).astype(F.dtype)


def supercell_difference(engine, dtype, R, Cc, rots=None, phases=None, nsteps=200, seed=11):
    """A unit cell of period (R-1) x (C-1) with (rho_r, rho_c) against its 2 x 3-tile supercell with (rho_r^2, rho_c^3) and
    phase-tiled start fields.  rots: per member a pair of EXACT keys; phases: (phi_r (B,), phi_c (B,)).  Returns the worst
    max|supercell - tiled unit| / max|unit| over Ez (images and corner included), Hx and Hy."""
    Qr, Qc = R - 1, Cc - 1
    SR, SC = 2 * Qr + 1, 3 * Qc + 1
    B = len(rots) if rots is not None else len(phases[0])
    eps, sigma, start = random_members(seed, B, R, Cc, dtype)
    if rots is not None:
        fr = np.array([complex(*EXACT[a]) for a, _ in rots])
        fc = np.array([complex(*EXACT[b]) for _, b in rots])
        unit_rot = (tuple(np.array(v) for v in zip(*(EXACT[a] for a, _ in rots))),
                    tuple(np.array(v) for v in zip(*(EXACT[b] for _, b in rots))))
        r2 = [_unit_power(EXACT[a], 2) for a, _ in rots]
        c3 = [_unit_power(EXACT[b], 3) for _, b in rots]
        super_rot = ((np.array([z.real for z in r2]), np.array([z.imag for z in r2])),
                     (np.array([z.real for z in c3]), np.array([z.imag for z in c3])))
    else:
        fr, fc = np.exp(1j * phases[0]), np.exp(1j * phases[1])
    tile = lambda F, shape: _tiled(F, Qr, Qc, shape, fr, fc)
    plain = lambda F, shape: _tiled(F, Qr, Qc, shape)
    out = []
    for rows, cols, scale in ((R, Cc, None), (SR, SC, (2, 3))):
        with engine(B, rows, cols, DT, DX, dtype=dtype, boundary="lattice") as e:
            big = scale is not None
            e.set_materials(plain(eps, (rows, cols)) if big else eps, MU0)
            e.set_conductivity(plain(sigma, (rows, cols)) if big else sigma)
            if rots is not None:
                e.set_lattice_phase(0, 0, rotation=super_rot if big else unit_rot)
            else:
                e.set_lattice_phase(*((2 * phases[0], 3 * phases[1]) if big else phases))
            shapes = ((rows, cols), (rows, cols - 1), (rows - 1, cols))
            e.upload(*(tile(F, s) for F, s in zip(start, shapes)) if big else start)
            e.run(nsteps)
            out.append(e.download())
    unit, sup = out
    worst = 0.0
    for F, G, cut in zip(unit, sup, ((SR, SC), (SR - 1, SC - 1), (SR - 1, SC - 1))):
        want = _tiled(F.astype(np.complex128), Qr, Qc, G.shape[1:], fr, fc)[:, :cut[0], :cut[1]]
        worst = max(worst, np.abs(G[:, :cut[0], :cut[1]] - want).max() / np.abs(F).max())
    return worst


SUPER_ROTS = [("half", "quarter"), ("quarter", "half"), ("one", "quarter"), ("quarter", "quarter")]
SUPER_BOUND = 1e-12


def check_supercell_exact(engine, dtype, R, Cc, nsteps=60):
    assert supercell_difference(engine, dtype, R, Cc, rots=SUPER_ROTS, nsteps=nsteps) == 0.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_rotations_match_their_supercell_bit_for_bit(dtype):
    check_supercell_exact(LatticeOracle, dtype, 8, 6)


def test_general_phases_match_their_supercell_to_rounding():
    phases = (np.array([0.7, np.pi, -2.2]), np.array([-1.9, 2.4, 0.3]))
    d = supercell_difference(LatticeOracle, np.float64, 8, 6, phases=phases, nsteps=200)
    print(f"unit cell against its 2 x 3 supercell after 200 steps: {d:.3e} relative (bound {SUPER_BOUND:.0e})")
    assert d <= SUPER_BOUND


def _phased_run(engine, dtype, R, Cc, eps, sigma, rot, src, amps, nsteps, weights=None):
    B = eps.shape[0]
    with engine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice") as e:
        e.set_materials(eps, MU0).set_conductivity(sigma).set_sources(np.array([src] * B))
        e.set_lattice_phase(0, 0, rotation=rot)
        e.run(nsteps, amps)
        return e.download()


def _rotations(B, dtype, seed=4):
    """Generic rotations, already rounded to the batch dtype: ((cr, sr), (cc, sc)), each (B,) float64."""
    ph = np.random.default_rng(seed).uniform(-np.pi, np.pi, (2, B))
    r = lambda v: v.astype(dtype).astype(np.float64)
    return (r(np.cos(ph[0])), r(np.sin(ph[0]))), (r(np.cos(ph[1])), r(np.sin(ph[1])))


def check_transpose(engine, dtype, R, Cc, nsteps=60):
    B = 3
    eps, sigma, _ = random_members(7, B, R, Cc, dtype)
    rot_r, rot_c = _rotations(B, dtype)
    amps = np.random.default_rng(8).standard_normal((B, nsteps)) * np.exp(1j * np.array([0.3, 1.2, 2.5]))[:, None]
    Ez, Hx, Hy = _phased_run(engine, dtype, R, Cc, eps, sigma, (rot_r, rot_c), (2, Cc - 2), amps, nsteps)
    t = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    Et, Hxt, Hyt = _phased_run(engine, dtype, Cc, R, t(eps), t(sigma), (rot_c, rot_r), (Cc - 2, 2), amps, nsteps)
    assert np.abs(Ez.imag).max() > 0 and np.abs(Ez[:, -1, -1]).max() > 0
    assert np.array_equal(Hxt, -t(Hy)) and np.array_equal(Hyt, -t(Hx))
    # Every cell of Ez but the corner image: that one is rho_r * (rho_c * Ez[0, 0]) here and rho_c * (rho_r * Ez[0, 0]) in
    # the transposed member (the column rotation comes first in both), two roundings in another order.  It is an output
    # of download alone; no step reads it.
    corner = np.zeros(Et.shape, bool)
    corner[:, -1, -1] = True
    assert np.array_equal(Et[~corner], t(Ez)[~corner])
    eps_t = np.finfo(dtype).eps
    assert np.abs(Et[corner] - t(Ez)[corner]).max() <= 4 * eps_t * np.abs(Ez[:, 0, 0]).max()


def check_conjugate(engine, dtype, R, Cc, nsteps=60):
    B = 3
    eps, sigma, _ = random_members(9, B, R, Cc, dtype)
    (cr, sr), (cc, sc) = _rotations(B, dtype, seed=5)
    amps = np.random.default_rng(10).standard_normal((B, nsteps))
    a = _phased_run(engine, dtype, R, Cc, eps, sigma, ((cr, sr), (cc, sc)), (0, 0), amps, nsteps)
    b = _phased_run(engine, dtype, R, Cc, eps, sigma, ((cr, -sr), (cc, -sc)), (0, 0), amps, nsteps)
    assert np.abs(a[0].imag).max() > 0
    for x, y in zip(a, b):
        assert np.array_equal(y, np.conj(x))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_transposed_member_gives_the_transposed_fields_bit_for_bit(dtype):
    check_transpose(LatticeOracle, dtype, 8, 6)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_negated_phases_give_the_conjugate_bit_for_bit(dtype):
    check_conjugate(LatticeOracle, dtype, 8, 6)


def test_unit_rotations_keep_the_imaginary_part_zero():
    eps, sigma, _ = random_members(3, 2, 9, 7, np.float32)
    amps = np.random.default_rng(1).standard_normal((2, 50))
    one, zero = np.ones(2), np.zeros(2)
    for F in _phased_run(LatticeOracle, np.float32, 9, 7, eps, sigma, ((one, zero), (one, zero)), (3, 2), amps, 50):
        assert np.abs(F.real).max() > 0 and not F.imag.any()


# ---- 5. the bands of the empty lattice ----------------------------------------------------------------------------------

BAND_Q, BAND_STEPS, BAND_FC, BAND_SRC, BAND_PROBE = 16, 4096, 80e9, (3, 5), (9, 2)
BAND_PHASES = [(2.0, 0.0), (1.1, 2.6), (np.pi, np.pi)]


def band_peaks(trace):
    """Angular frequencies (>= 0) of the peaks of the Hann-windowed spectrum of a complex trace that exceed 5 % of the
    largest, each refined by a parabola through the logarithms of the three bins around it, in units of rad/s."""
    N = len(trace)
    spec = np.abs(np.fft.fft(trace * np.hanning(N)))
    top = spec.max()
    w = []
    for k in range(N):
        a, b, c = spec[k - 1], spec[k], spec[(k + 1) % N]
        if b > 0.05 * top and b >= a and b > c:
            la, lb, lc = np.log(a), np.log(b), np.log(c)
            shift = 0.5 * (la - lc) / (la - 2 * lb + lc)
            f = (k + shift) / N
            w.append(abs(2 * np.pi * (f if f < 0.5 else f - 1) / DT))
    return np.array(w)


def yee_bands(phi_r, phi_c, Q):
    """omega = (2 / dt) asin(sqrt(S)) of the folded plane waves (m, n) of the empty lattice."""
    m = np.arange(-Q // 2, Q // 2 + 1)
    th_r, th_c = (phi_r + 2 * np.pi * m) / Q, (phi_c + 2 * np.pi * m) / Q
    S = (DT / (EPS0 * DX)) * (DT / (MU0 * DX)) * (np.sin(th_r / 2)[:, None] ** 2 + np.sin(th_c / 2)[None, :] ** 2)
    return np.sort((2 / DT * np.arcsin(np.sqrt(S))).ravel())


def test_probe_spectrum_peaks_sit_on_the_yee_bands_of_the_empty_lattice(fd):
    B, R = len(BAND_PHASES), BAND_Q + 1
    ref = LatticeOracle(B, R, R, DT, DX, dtype=np.float64)
    ref.set_materials(EPS0, MU0).set_sources(np.array([BAND_SRC] * B))
    ref.set_lattice_phase(*(np.array(v) for v in zip(*BAND_PHASES)))
    ref.set_probes([BAND_PROBE], BAND_STEPS)
    amp = np.array([fd.ricker_amplitude(n * DT, BAND_FC) for n in range(BAND_STEPS)])
    ref.run(BAND_STEPS, np.tile(amp, (B, 1)))
    traces = ref.read_probes()[:, 0]
    spacing = 2 * np.pi / (BAND_STEPS * DT)
    for b, (phi_r, phi_c) in enumerate(BAND_PHASES):
        bands, peaks = yee_bands(phi_r, phi_c, BAND_Q), band_peaks(traces[b])
        off = np.array([np.abs(bands - p).min() for p in peaks]) / spacing
        print(f"phases ({phi_r:.3f}, {phi_c:.3f}): {len(peaks)} peaks, worst distance from a Yee band {off.max():.3f} "
              f"of the bin spacing (bound 0.5); lowest band {bands[0] / 2e9 / np.pi:.2f} GHz")
        assert len(peaks) >= 2 and off.max() <= 0.5              # at least +w and -w of one band
        assert np.abs(peaks - bands[0]).min() <= 0.5 * spacing      # the lowest analytic band is among the peaks
