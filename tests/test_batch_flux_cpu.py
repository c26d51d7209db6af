"""CPU-only checks of the flux lines of the batched engine (fdtd2d_batch_flux.h, batch.py), on the stand-in of
tests/oracle_batch_flux.py.

The surface: the three entry points are declared, exported and bound, the constants and ids are named and are the next
free numbers, the Python surface has its shape, bad arguments are refused before any device is touched, and without a
device nothing falls back.

The stand-in: lines never change a field or another monitor; `every`, the step count and reset follow the window's rule.

The physics, on the stand-in: a periodic vacuum member of 120 x 9 cells (period 8), dx = 1e-4, dt = 1.6e-13 (Courant
0.48), a 12-row layer top and bottom, a Ricker line source over the period on row 40 with fc = c / (20 dx), 1600 steps in
float64, whole-period row lines at rows 25, 50, 56 and 75, wavelengths of 30, 20 and 12 cells.

The pulse is the library's Ricker wavelet delayed by 2 / fc instead of 1 / fc, so that its first sample is 6e-16 of
its peak and not 1e-3.  With the 1 / fc delay the run starts with a step of 1e-3, whose grid-scale content the layer does
not absorb: the field is still 3e-5 after 1600 steps (and 1e-5 after 6400), the transforms are those of a truncated
record, and the flux through two lines then differs by 3.5e-7, 1.1e-6 and 1.0e-6 at the three frequencies whatever the
definition of the flux.  With the 2 / fc delay the field ends at 1e-16 and the measured values are:

    1. conservation   |P50 - P75| / P50 = 7.8e-16, 1.9e-15, 5.2e-15      bound 1e-9 (any mistake of centring: > 1e-3)
                      |P25 / P50 + 1|   = 3.2e-5, 1.4e-5, 9.9e-6        bound 1e-3
    2. the half step  |Im / Re| of sum E conj(H): <= 2.9e-5 with the factor (bound tan(w dt / 2) / 4 = 0.0126, 0.0189,
                      0.0316); 0.0503, 0.0755, 0.1263 raw, within 4.5e-4 of tan(w dt / 2) (bound 1 %)
    3. absorption     sigma = 20 S/m on rows 60..65: |P50 - P56| / P50 = 5e-16 .. 4e-15 (bound 1e-9),
                      P75 / P56 = 0.0680, 0.0416, 0.0223 (bound: 0 < . < 0.1)
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle import fdtd_numpy as onp
from oracle_batch_flux import (FluxDispersivePeriodicOracle, FluxDispersivePmlOracle, FluxLossyOracle,
                               FluxPeriodicOracle, flux_oracle_for)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_flux.h")
NAMES = ["fdtd2d_batch_flux", "fdtd2d_batch_read_flux_lines", "fdtd2d_batch_set_flux_lines"]
EPS0, MU0 = onp.EPS0, onp.MU0
C0 = 1 / np.sqrt(EPS0 * MU0)


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- the surface ----------------------------------------------------------------------------------------------------

def test_batch_flux_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_FLUX_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_FLUX_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_FLUX_SIGNATURES[n][0]
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "const int *": ctypes.POINTER(ctypes.c_int),
             "double *": ctypes.POINTER(ctypes.c_double), "const double *": ctypes.POINTER(ctypes.c_double)}
    for n, args in proto.items():
        got = [kinds[re.match(r"(.*?[ *])\w+$", " ".join(a.split())).group(1).strip()] for a in args.split(",")]
        assert got == _abi.BATCH_FLUX_SIGNATURES[n][1], n
    # nothing was added to the fixed surfaces
    for h in ("fdtd2d.h", "fdtd2d_batch_monitor.h"):
        assert "flux" not in open(os.path.join(ROOT, "include", h)).read()


def test_batch_flux_constants_and_ids_are_named_and_the_next_free():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+FDTD2D_BATCH_MAX_FLUX_LINES\s+4\b", txt) and _abi.BATCH_MAX_FLUX_LINES == 4
    assert re.search(r"#define\s+FDTD2D_BATCH_MAX_FLUX_FREQS\s+16\b", txt) and _abi.BATCH_MAX_FLUX_FREQS == 16
    assert re.search(r"#define\s+FDTD2D_BATCH_OPT_FLUX_LDS\s+3\b", txt) and _abi.BATCH_OPT_FLUX_LDS == 3
    # the info ids are written relative to the last one taken, which every other header's ids stay below
    last = "FDTD2D_BATCH_INFO_HELD_DISPERSIVE_WINDOW"
    assert re.search(rf"FDTD2D_BATCH_INFO_FLUX_LINES\s*=\s*{last}\s*\+\s*1\b", txt)
    assert re.search(rf"FDTD2D_BATCH_INFO_FLUX_LDS\s*=\s*{last}\s*\+\s*2\b", txt)
    info, opt = {}, {}
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != os.path.basename(HEADER):
            other = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            info.update(re.findall(r"FDTD2D_(BATCH_INFO_\w+)\s*(?:=\s*|\s+)(-?\d+)\b", other))
            opt.update(re.findall(r"FDTD2D_(BATCH_OPT_\w+)\s*(?:=\s*|\s+)(-?\d+)\b", other))
    assert max(info.values(), key=int) == info["BATCH_INFO_HELD_DISPERSIVE_WINDOW"] == "20"
    assert sorted(int(v) for v in info.values()) == list(range(21))
    assert sorted(int(v) for v in opt.values()) == [0, 1, 2]
    assert (_abi.BATCH_INFO_FLUX_LINES, _abi.BATCH_INFO_FLUX_LDS) == (21, 22)
    names = [k for k in dir(_abi) if k.startswith("BATCH_INFO_")]
    assert len({getattr(_abi, k) for k in names}) == len(names)
    names = [k for k in dir(_abi) if k.startswith("BATCH_OPT_")]
    assert len({getattr(_abi, k) for k in names}) == len(names)


def test_batch_flux_python_surface(fd):
    E = fd.BatchEngine
    assert list(inspect.signature(E.set_flux_lines).parameters) == ["self", "lines", "omegas", "every"]
    assert inspect.signature(E.set_flux_lines).parameters["every"].default == 1
    assert list(inspect.signature(E.read_flux_lines).parameters) == ["self", "raw"]
    assert inspect.signature(E.read_flux_lines).parameters["raw"].default is False
    assert list(inspect.signature(E.flux).parameters) == ["self"]
    assert isinstance(E.flux_lines_in_lds, property)
    p = inspect.signature(fd.run_fdtd_batch).parameters
    for name in ("flux_lines", "flux_omegas"):
        assert p[name].default is None and p[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[-2:] == ["flux_lines", "flux_omegas"]
    for cls in (FluxLossyOracle, FluxPeriodicOracle, FluxDispersivePmlOracle, FluxDispersivePeriodicOracle):
        for name in ("set_flux_lines", "read_flux_lines", "flux"):
            assert callable(getattr(cls, name))


def test_batch_flux_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ln = np.array([0, 5, 0, 4], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_flux_lines(None, 1, ln, 1, dp, 1) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_flux_lines(None, dp, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_flux(None, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_INFO_FLUX_LINES) == _abi.E_ARG
    assert lib.fdtd2d_batch_info(None, _abi.BATCH_INFO_FLUX_LDS) == _abi.E_ARG


R0, C0_ = 40, 17
BAD = [
    ("pml", [("row", 5 + k, 0, 4) for k in range(5)], [1e11], 1, "1..4 lines"),
    ("pml", [("row", 5, 0, 4)], np.linspace(1e11, 2e11, 17), 1, "1..16 frequencies"),
    ("pml", [("row", 0, 0, 4)], [1e11], 1, "row 0 outside"),
    ("pml", [("row", R0 - 1, 0, 4)], [1e11], 1, f"row {R0 - 1} outside"),
    ("periodic", [("col", C0_ - 1, 0, 4)], [1e11], 1, "image of column 0"),
    ("pml", [("col", 0, 0, 4)], [1e11], 1, "column 0 outside"),
    ("pml", [("col", C0_ - 1, 0, 4)], [1e11], 1, f"column {C0_ - 1} outside"),
    ("pml", [("row", 5, 10, C0_ - 9)], [1e11], 1, "run past"),
    ("periodic", [("row", 5, 0, C0_)], [1e11], 1, "run past"),
    ("pml", [("col", 5, R0 - 3, 4)], [1e11], 1, "run past"),
    ("pml", [("row", 5, 0, 0)], [1e11], 1, "empty"),
    ("pml", [("row", 5, 0, 4)], [1e11], 0, "every must be >= 1"),
    ("pml", [("diag", 5, 0, 4)], [1e11], 1, '"row"'),
    ("mur", [("row", 5, 0, 4)], [1e11], 1, 'needs boundary="pml" or "periodic"'),
]


@pytest.mark.parametrize("boundary,lines,omegas,every,msg", BAD, ids=[f"{b[0]}-{b[4]}" for b in BAD])
def test_bad_flux_arguments_are_refused_before_a_device_is_touched(fd, boundary, lines, omegas, every, msg):
    """run_fdtd_batch raises ValueError before it creates an engine, so this passes with and without a device."""
    with pytest.raises(ValueError, match=re.escape(msg)):
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), nsteps=5, sources=np.array([[20, 8]] * 2), boundary=boundary,
                          pml_cells=6, dft_every=every, flux_lines=lines, flux_omegas=omegas)


def test_flux_arguments_come_together_and_not_with_a_bloch_phase(fd):
    kw = dict(nsteps=5, sources=np.array([[20, 8]] * 2), boundary="periodic", pml_cells=6)
    with pytest.raises(ValueError, match="together"):
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), flux_lines=[("row", 5, 0, 4)], **kw)
    with pytest.raises(ValueError, match="bloch_phase"):
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), flux_lines=[("row", 5, 0, 4)], flux_omegas=[1e11],
                          bloch_phase=0.3, **kw)


def test_batch_flux_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 2, R0, C0_, 5e-14, 1e-4, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, R0, C0_), EPS0), nsteps=10, sources=np.array([[20, 8]] * 2), boundary="periodic",
                          pml_cells=6, flux_lines=[("row", 12, 0, C0_ - 1)], flux_omegas=[2e11])
    assert ei.value.code == _abi.E_NODEVICE


# ---- the stand-in -----------------------------------------------------------------------------------------------------

def _member(boundary, dispersive, dtype=np.float32, R=24, C=13, seed=3):
    rng = np.random.default_rng(seed)
    eng = flux_oracle_for(boundary, dispersive)(2, R, C, 5e-14, 1e-4, dtype=dtype, boundary=boundary)
    eng.set_materials(EPS0 * (1 + rng.random((2, R, C))), MU0 * (1 + rng.random((2, R, C))))
    eng.set_pml(4, courant00=(C0 * 5e-14) / 1e-4)
    if dispersive:
        g = eng.margin()
        wp2 = np.zeros((2, R, C))
        wp2[:, g:R - g, (0 if boundary == "periodic" else g):(C if boundary == "periodic" else C - g)] = 4e22
        eng.set_dispersion(wp2, np.array([1e11, 0.0]), np.array([0.0, 3e11]))
    eng.set_sources(np.array([[9, 3, 2, 2], [10, 4, 1, 3]]))
    eng.set_dft_window((7, 2, 5, 6), 2 * np.pi * np.array([30e9, 55e9]), every=2)
    eng.set_probes(np.array([[8, 0], [11, C - 2], [12, 5]]), 40)
    return eng


@pytest.mark.parametrize("dispersive", [False, True])
@pytest.mark.parametrize("boundary", ["pml", "periodic"])
def test_lines_never_change_a_field_or_another_monitor(boundary, dispersive):
    amps = np.random.default_rng(5).standard_normal((2, 30))
    col = 0 if boundary == "periodic" else 1
    lines = [("row", 9, 0, 12), ("col", col, 2, 20), ("col", 11, 7, 5), ("row", 2, 3, 4)]
    out = []
    for with_lines in (False, True):
        eng = _member(boundary, dispersive)
        if with_lines:
            eng.set_flux_lines(lines, 2 * np.pi * np.array([[30e9, 55e9, 80e9], [20e9, 45e9, 70e9]]), every=3)
        eng.run(30, amps)
        out.append(eng.download() + (eng.Ezx.copy(), eng.read_dft_window(), eng.read_probes()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    E, H = eng.read_flux_lines(raw=True)
    assert E.shape == H.shape == (2, 3, 41) and np.all(np.abs(E).max(axis=(1, 2)) > 0) and np.abs(H).max() > 0
    # the cell (9, col) lies on the row line (its cell `col`) and on the column line (its cell 9 - 2): one Ez, two H
    assert np.array_equal(E[:, :, col], E[:, :, 12 + 7])
    assert not np.array_equal(H[:, :, col], H[:, :, 12 + 7])


def test_sampling_follows_the_window_rule_and_reset_zeroes():
    om = 2 * np.pi * np.array([40e9, 70e9])
    amps = np.random.default_rng(6).standard_normal((2, 40))
    eng = _member("periodic", False)
    eng.run(7, amps[:, :7])
    eng.set_dft_window((9, 0, 1, 12), om, every=3)       # the same cells, frequencies and rule as the line's Ez
    eng.set_flux_lines([("row", 9, 0, 12)], om, every=3)
    eng.run(33, amps[:, 7:])
    E, _ = eng.read_flux_lines(raw=True)
    assert np.array_equal(E, eng.read_dft_window()[:, :, 0, :])
    # one run or two, the same sums
    one = _member("periodic", False)
    one.run(7, amps[:, :7])
    one.set_flux_lines([("row", 9, 0, 12)], om, every=3)
    one.run(20, amps[:, 7:27])
    one.run(13, amps[:, 27:])
    for a, b in zip(one.read_flux_lines(), eng.read_flux_lines()):
        assert np.array_equal(a, b)
    assert np.array_equal(one.flux(), eng.flux())
    eng.reset()
    assert not np.any(eng.read_flux_lines()[0]) and not np.any(eng.read_flux_lines()[1]) and not np.any(eng.flux())
    eng.run(3, amps[:, :3])                              # the count restarts: step 3 is sampled
    assert np.any(eng.read_flux_lines()[0])


# ---- the physics -----------------------------------------------------------------------------------------------------

PR, PC, PDX, PDT, PSTEPS, PL, PSRC = 120, 9, 1e-4, 1.6e-13, 1600, 12, 40
PLINES = (25, 50, 56, 75)
POMEGA = 2 * np.pi * C0 / (np.array([30.0, 20.0, 12.0]) * PDX)
PFC = C0 / (20 * PDX)


def _physics(sigma=None):
    # the library's Ricker wavelet, delayed by 2 / fc (the module docstring says why)
    amps = np.array([onp.ricker_amplitude(i * PDT - 1 / PFC, PFC) for i in range(PSTEPS)])
    assert abs(amps[0]) < 1e-15 and abs(amps).max() > 0.99
    eng = FluxPeriodicOracle(1, PR, PC, PDT, PDX, dtype=np.float64)
    eng.set_materials(np.full((1, PR, PC), EPS0), np.full((1, PR, PC), MU0))
    eng.set_pml(PL, courant00=(C0 * PDT) / PDX)
    if sigma is not None:
        s = np.zeros((1, PR, PC))
        s[:, 60:66, :] = sigma
        eng.set_conductivity(s)
    eng.set_sources(np.array([[PSRC, 0, 1, PC - 1]]))
    eng.set_flux_lines([("row", r, 0, PC - 1) for r in PLINES], POMEGA)
    eng.run(PSTEPS, amps[None])
    assert np.abs(eng.Ez).max() < 1e-12                  # measured 1.1e-16: the record is complete
    return eng


@pytest.fixture(scope="module")
def lossless():
    return _physics()


def test_flux_is_conserved_between_lines_and_reverses_behind_the_source(lossless):
    P = lossless.flux()[0]                               # (line, frequency)
    assert np.all(P[1] > 0)
    cons = np.abs(P[1] - P[3]) / P[1]
    print("conservation |P50 - P75| / P50:", cons)       # measured 7.8e-16, 1.9e-15, 5.2e-15
    assert np.all(cons <= 1e-9)
    up = np.abs(P[0] / P[1] + 1)
    print("upstream |P25 / P50 + 1|:", up)                # measured 3.2e-5, 1.4e-5, 9.9e-6
    assert np.all(up <= 1e-3)


def test_half_step_factor_makes_the_flux_real(lossless):
    tan = np.tan(POMEGA * PDT / 2)
    n = PC - 1
    for raw in (False, True):
        E, H = lossless.read_flux_lines(raw=raw)
        z = (E[0] * np.conj(H[0])).reshape(3, len(PLINES), n).sum(axis=2)     # (frequency, line)
        ratio = np.abs(z.imag / z.real)
        print("raw" if raw else "with the factor", "|Im / Re|:", ratio.max(axis=1))
        if raw:
            assert np.all(np.abs(ratio / tan[:, None] - 1) <= 0.01)            # measured: within 4.5e-4
        else:
            assert np.all(ratio <= 0.25 * tan[:, None])                        # measured <= 2.9e-5


def test_a_conducting_slab_absorbs_what_the_lines_miss(lossless):
    P = _physics(sigma=20.0).flux()[0]
    same = np.abs(P[1] - P[2]) / P[1]
    print("|P50 - P56| / P50:", same, " P75 / P56:", P[3] / P[2])              # measured <= 4e-15; 0.0680, 0.0416, 0.0223
    assert np.all(same <= 1e-9)
    assert np.all(P[3] > 0) and np.all(P[3] < 0.1 * P[2])
    # and the slab reflects: less net power reaches line 50 than without it
    assert np.all(P[1] < lossless.flux()[0][1])
