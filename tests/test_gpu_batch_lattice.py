"""GPU: the lattice mode of periodic batches (fdtd2d_batch_lattice.h, kernels_batch_lattice.hpp).

Complex fields and probe traces equal the stand-in of tests/oracle_batch_lattice.py bit for bit (exact build), window DFTs to
1e-12 (the device's float64 cos and sin are not NumPy's, the project's bound for every window DFT): both dtypes, resident
and streamed, whole runs and 7 steps per launch, 5 members with distinct phase pairs, complex amplitudes, ramp weights, a
conductivity that reaches row 0 and column 0, a window and probes that include (0, 0), (0, C-2) and (R-2, 0).  The shapes:
11 x 13 (the smallest member, 64 threads), 23 x 19 (128 threads, 128 % 19 = 14: the cell walk carries) and 37 x 31 (1147
cells on 320 threads: 4 cells per thread).  The largest member the capacity rule admits runs resident (float32: 5 cells per
thread, the second instance of the resident kernel), one row more streams.  The exact properties of
tests/test_batch_lattice_cpu.py hold on the device.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_BOUND."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_lattice import LatticeOracle
import test_batch_lattice_cpu as lcpu

pytestmark = pytest.mark.gpu

ROOT = lcpu.ROOT
DT, DX, LDS_LIMIT = 5e-14, 1e-4, 163840
E_ARG, E_STATE = -1, -4
SHAPES = {"11x13": (11, 13), "23x19": (23, 19), "37x31": (37, 31)}
# The fused build evaluates the multiply-add pairs of the step and the seams' rotations as one fma each
# (batch_lattice_hx, batch_periodic_plain, batch_lossy_e, batch_bloch_rot, _unrot, _source), so its results differ from the
# exact build's by rounding.  The quantity is: complex Ez after 300 steps, 5 members of 37 x 31 with the conductivity,
# complex amplitudes and ramp weights, worst member, max|fused - exact| / max|exact|.
# FUSED_MEASURED is what test_fused_build_within_its_bounds printed on its first MI355X run; the bounds are ten times
# that, as for the periodic and the Bloch batch (tests/test_gpu_batch_periodic.py, tests/test_gpu_batch_bloch.py).
NSTEPS_FIELD = 300
FUSED_MEASURED = {"f32": 1.054e-06, "f64": 1.666e-15}
FUSED_BOUND = {k: 10 * v for k, v in FUSED_MEASURED.items()}      # 1.1e-5, 1.7e-14


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _threads(cells):
    return min(1024, -(-(-(-cells // 4)) // 64) * 64)


def _cfg(fd, seed, B, R, Cc, dtype, n):
    """Members with their own materials, phase pairs and line sources (one spans the whole period in row 0, one starts in
    column 0, one ends in column C-2 of row R-2), complex amplitudes, a conductivity anywhere in the period (row 0 and
    column 0 included), a window that stops short of the images and four probes, three of them on the seams."""
    rng = np.random.default_rng(seed)
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(dtype)
    mu = (fd.MU0 * np.where(rng.random((B, R, Cc)) < 0.1, 1.5, 1.0)).astype(dtype)
    spans = [(0, 0, Cc - 1), (R // 2, 0, 4), (R - 2, Cc - 5, 4), (3, 2, Cc - 5)]
    rects = np.array([[spans[m % 4][0], spans[m % 4][1], 1, spans[m % 4][2]] for m in range(B)])
    amps = np.stack([[fd.ricker_amplitude(k * DT, 30e9 * (1 + 0.1 * (m % 7))) for k in range(n)] for m in range(B)])
    amps = amps * np.exp(1j * (0.4 + 0.7 * np.arange(B)))[:, None]
    phi_r = 0.3 + 2.9 * (np.arange(B) % 11) / 11 + 0.001 * np.arange(B)      # distinct, up to about pi
    phi_c = -2.8 + 5.5 * ((3 * np.arange(B) + 1) % 7) / 7 - 0.002 * np.arange(B)
    sigma = np.where(rng.random((B, R, Cc)) < 0.3, 0.0, 20.0 * rng.random((B, R, Cc)))
    omegas = (2 * np.pi * np.array([20e9, 45e9, 80e9]))[None, :] * (1 + 0.01 * np.arange(B))[:, None]
    probes = np.array([(0, 0), (0, Cc - 2), (R - 2, 0), (R // 2, 4)])
    return dict(eps=eps, mu=mu, rects=rects, amps=amps, phi_r=phi_r, phi_c=phi_c, sigma=sigma, omegas=omegas,
                probes=probes, window=(0, 0, 4, Cc - 3), n=n)


def _drive(b, cfg, monitors=True):
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    b.set_conductivity(cfg["sigma"])
    b.set_lattice_phase(cfg["phi_r"], cfg["phi_c"]).set_bloch_source("ramp")
    if monitors:
        b.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
    return b


def _expect_path(b, nf, window_cells, never=False, lds_allowed=True):
    """The capacity rule, restated: 9 arrays, 16 (C-1) bytes of source weights beside the phasor table, and twice the
    accumulators."""
    esz, R, Cc = b.dtype.itemsize, b.rows, b.cols
    fields = 9 * _seg(R * Cc, esz)
    table, acc = 16 * nf + 16 * (Cc - 1), 2 * 16 * nf * window_cells
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = bool(nf) and lds_allowed and fields + table + acc <= LDS_LIMIT
    assert b.lattice and b.periodic and not b.bloch
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - table) // 9 // 16 * 16 // esz
    assert b.resident == resident
    assert b.window_in_lds == (in_lds and resident)
    return resident


def _device_run(fd, dtype, R, Cc, cfg, splits, monitors=True, resident=None, spl=None, lds=True):
    B = cfg["eps"].shape[0]
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice") as b:
        _drive(b, cfg, monitors)
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        w = cfg["window"]
        path = _expect_path(b, cfg["omegas"].shape[1] if monitors else 0, w[2] * w[3], never=resident == 0,
                            lds_allowed=lds)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, cfg["amps"][:, done:done + k])
            done += k
        if path:      # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * sum(splits)
        out = dict(fields=b.download(), path=path, in_lds=b.window_in_lds)
        if monitors:
            out.update(dft=b.read_dft_window(), probes=b.read_probes(),
                       spectra=b.bloch_probe_spectra(cfg["omegas"], peak=True), absmax=b.bloch_field_absmax("Ez"))
        return out


def _stand_in(dtype, R, Cc, cfg, monitors=True):
    B = cfg["eps"].shape[0]
    ref = _drive(LatticeOracle(B, R, Cc, DT, DX, dtype=dtype), cfg, monitors)
    ref.run(cfg["n"], cfg["amps"])
    out = dict(fields=ref.download())
    if monitors:
        out.update(dft=ref.read_dft_window(), probes=ref.read_probes(),
                   spectra=ref.bloch_probe_spectra(cfg["omegas"], peak=True), absmax=ref.bloch_field_absmax("Ez"))
    return out


def _same(a, b):
    ok = all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"]))
    if "dft" in a:
        ok = ok and np.array_equal(a["dft"], b["dft"]) and np.array_equal(a["probes"], b["probes"])
    return ok


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_within_its_bounds")


def _agrees(got, ref, cfg):
    """Fields and probes bit for bit, the window DFT to 1e-12; both parts and both seams saw the field."""
    for name, a, w in zip(("Ez", "Hx", "Hy"), got["fields"], ref["fields"]):
        assert np.iscomplexobj(a) and np.array_equal(a, w), name
    Ez = got["fields"][0]
    assert np.abs(Ez.real).max() > 0 and np.abs(Ez.imag).max() > 0
    assert np.abs(Ez[:, :, 0]).max() > 0 and np.abs(Ez[:, 0, :]).max() > 0
    rr, rc = np.exp(1j * cfg["phi_r"])[:, None], np.exp(1j * cfg["phi_c"])[:, None]
    tol = 1e-6 * np.abs(Ez).max()
    assert np.abs(Ez[:, :-1, -1] - rc * Ez[:, :-1, 0]).max() <= tol       # the images, and the corner
    assert np.abs(Ez[:, -1, :-1] - rr * Ez[:, 0, :-1]).max() <= tol
    assert np.abs(Ez[:, -1, -1] - (rr * rc)[:, 0] * Ez[:, 0, 0]).max() <= tol
    if "dft" in ref:
        assert np.array_equal(got["probes"], ref["probes"]) and np.abs(got["probes"][:, 0].imag).max() > 0
        assert np.abs(got["dft"] - ref["dft"]).max() <= 1e-12 * np.abs(ref["dft"]).max()
        assert np.abs(got["spectra"][0] - ref["spectra"][0]).max() <= 1e-12 * np.abs(ref["spectra"][0]).max()
        assert np.array_equal(got["spectra"][1], ref["spectra"][1]) and np.array_equal(got["absmax"], ref["absmax"])


# ---- 1. against the stand-in ------------------------------------------------------------------------------------------------

N_STEPS = 50


@functools.lru_cache(maxsize=None)
def _reference(fd, dtype, shape):
    R, Cc = SHAPES[shape]
    cfg = _cfg(fd, R, 5, R, Cc, dtype, N_STEPS)
    return cfg, _stand_in(dtype, R, Cc, cfg)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("where", ["resident", "resident_spl7", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_lattice_runs_match_the_stand_in(fd, dtype, where, shape):
    _exact_only(fd)
    R, Cc = SHAPES[shape]
    cells, threads = R * Cc, _threads(R * Cc)
    assert {"11x13": threads == 64, "23x19": threads % Cc != 0, "37x31": -(-cells // threads) == 4}[shape]
    cfg, ref = _reference(fd, dtype, shape)
    got = _device_run(fd, dtype, R, Cc, cfg, (27, 23), resident=0 if where == "streamed" else None,
                      spl=7 if where == "resident_spl7" else 0)
    assert got["path"] == (where != "streamed")
    _agrees(got, ref, cfg)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_lattice_runs_are_bit_identical_on_every_path(fd, dtype):
    """In either build: streamed, split runs, steps per launch and the accumulators' place change no bit."""
    R, Cc = SHAPES["23x19"]
    cfg = _cfg(fd, 5, 6, R, Cc, dtype, 60)
    base = _device_run(fd, dtype, R, Cc, cfg, (60,))
    assert base["path"] and base["in_lds"]
    variants = dict(streamed=dict(resident=0), spl=dict(spl=7), split=dict(splits=(1, 32, 27)),
                    global_acc=dict(lds=False))
    for name, kw in variants.items():
        splits = kw.pop("splits", (60,))
        got = _device_run(fd, dtype, R, Cc, cfg, splits, **kw)
        assert got["path"] == (name != "streamed"), name
        assert _same(base, got), name


# ---- 2. the capacity rule ----------------------------------------------------------------------------------------------------

def _largest_rows(fd, dtype, Cc):
    """The most rows of a Cc-column member that the rule admits without monitors: restated here, then checked against
    the library's own figure, read at run time."""
    esz = np.dtype(dtype).itemsize
    fits = lambda R: R * Cc <= (LDS_LIMIT - 16 * (Cc - 1)) // 9 // 16 * 16 // esz
    R = max(r for r in range(11, 400) if fits(r))
    for rows, want in ((R, True), (R + 1, False)):
        with fd.BatchEngine(1, rows, Cc, DT, DX, dtype=dtype, boundary="lattice") as b:
            assert (rows * Cc <= b.resident_max_cells) == want and b.resident == want
    return R


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_largest_member_is_resident_and_one_row_more_streams(fd, dtype):
    _exact_only(fd)
    Cc, B, n = 61, 3, 10
    R = _largest_rows(fd, dtype, Cc)
    assert R * Cc > (4400 if dtype == np.float32 else 2200)           # about 4500 float32 / 2270 float64 cells
    assert -(-R * Cc // _threads(R * Cc)) == (5 if dtype == np.float32 else 4)      # cells per thread
    for rows, resident in ((R, True), (R + 1, False)):
        cfg = _cfg(fd, rows, B, rows, Cc, dtype, n)
        got = _device_run(fd, dtype, rows, Cc, cfg, (n,), monitors=False)
        assert got["path"] == resident, rows
        _agrees(got, _stand_in(dtype, rows, Cc, cfg, monitors=False), cfg)


def test_more_members_than_one_round_of_workgroups(fd):
    dtype, (R, Cc), B, n = np.float32, (40, 41), 600, 6
    cfg = _cfg(fd, 9, B, R, Cc, dtype, n)
    a = _device_run(fd, dtype, R, Cc, cfg, (n,), monitors=False)
    b = _device_run(fd, dtype, R, Cc, cfg, (n,), monitors=False, resident=0)
    assert a["path"] and not b["path"] and _same(a, b)
    Ez = a["fields"][0]
    assert len({Ez[m].tobytes() for m in range(B)}) == B
    if fd.ARITHMETIC == "exact":                                      # three of them against the stand-in
        pick = [0, 301, 599]
        sub = {k: (v[pick] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in cfg.items()}
        ref = _stand_in(dtype, R, Cc, sub, monitors=False)
        for x, y in zip(a["fields"], ref["fields"]):
            assert np.array_equal(x[pick], y)


# ---- 3. the exact properties on the device --------------------------------------------------------------------------------------

def _engine(fd, resident):
    def make(*a, **k):
        return fd.BatchEngine(*a, **k).set_option(resident=resident)
    return make


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_transposed_member_gives_the_transposed_fields_on_the_device(fd, dtype, resident):
    lcpu.check_transpose(_engine(fd, resident), dtype, 11, 13)        # engines of 11 x 13 and 13 x 11


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_negated_phases_give_the_conjugate_on_the_device(fd, dtype, resident):
    lcpu.check_conjugate(_engine(fd, resident), dtype, 11, 13)
    lcpu.check_conjugate(_engine(fd, resident), dtype, 13, 11)


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_exact_rotations_match_their_supercell_on_the_device(fd, dtype, resident):
    lcpu.check_supercell_exact(_engine(fd, resident), dtype, 11, 13)  # against 21 x 37
    lcpu.check_supercell_exact(_engine(fd, resident), dtype, 13, 11)  # against 25 x 31


# ---- 4. state -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_complex_fields_round_trip_with_the_images_rotated(fd, dtype):
    B, (R, Cc) = 3, SHAPES["23x19"]
    rng = np.random.default_rng(3)
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(lcpu.cdtype(dtype))
    Ez, Hx, Hy = cplx(B, R, Cc), cplx(B, R, Cc - 1), cplx(B, R - 1, Cc)
    rot = ((np.array([0.0, -1.0, 0.6]), np.array([1.0, 0.0, 0.8])), (np.array([-1.0, 0.0, 0.28]), np.array([0.0, 1.0, 0.96])))
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice") as b:
        assert b.lattice and b.periodic and not b.bloch
        assert not any(np.any(a) for a in b.download())
        b.set_lattice_phase(0, 0, rotation=rot)
        b.upload(Ez, Hx, Hy)
        ref = LatticeOracle(B, R, Cc, DT, DX, dtype=dtype).set_lattice_phase(0, 0, rotation=rot)
        ref.upload(Ez, Hx, Hy)
        got = b.download()
        for name, a, given, w in zip(("Ez", "Hx", "Hy"), got, (Ez, Hx, Hy), ref.download()):
            # members 0 and 1 have exact rotations; member 2's images are rounded once per product in the exact build
            # and once per fma in the fused one
            assert np.array_equal(a[:2], w[:2]), name
            if fd.ARITHMETIC == "exact":
                assert np.array_equal(a[2], w[2]), name
            else:
                assert np.abs(a[2] - w[2]).max() <= 4 * np.finfo(dtype).eps * np.abs(w[2]).max(), name
            assert np.array_equal(a[:, :R - 1, :Cc - 1], given[:, :R - 1, :Cc - 1]), name
        E = got[0]
        # member 0: rho_r = i, rho_c = -1; member 1: rho_r = -1, rho_c = i: the images and the corner, exactly
        assert np.array_equal(E[0, :-1, -1], -Ez[0, :-1, 0]) and np.array_equal(E[0, -1, :-1], 1j * Ez[0, 0, :-1])
        assert np.array_equal(E[1, :-1, -1], 1j * Ez[1, :-1, 0]) and np.array_equal(E[1, -1, :-1], -Ez[1, 0, :-1])
        assert E[0, -1, -1] == -1j * Ez[0, 0, 0] and E[1, -1, -1] == -1j * Ez[1, 0, 0]
        # a real upload has a zero imaginary part; download(dtype) converts both parts
        b.upload(Ez=Ez.real)
        assert not b.download()[0][:, :R - 1, :Cc - 1].imag.any()
        assert b.download(np.float64)[0].dtype == np.complex128
        b.reset()
        assert not any(np.any(a) for a in b.download()) and b.step_count == 0


def test_turning_the_mode_off_and_on_again(fd):
    _exact_only(fd)
    import ctypes as C
    dtype, (R, Cc), B, n = np.float32, SHAPES["23x19"], 4, 30
    cfg = _cfg(fd, 21, B, R, Cc, dtype, 2 * n)
    cfg["sigma"][:, :6, :] = 0          # what a plain periodic batch allows: no conductivity near its PEC rows
    cfg["sigma"][:, R - 6:, :] = 0
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice") as b:
        lib, h = b._lib, b._h
        _drive(b, cfg, monitors=False)
        b.run(n, cfg["amps"][:, :n])
        Ez, Hx, Hy = b.download()
        assert lib.fdtd2d_batch_set_lattice(h, None, None, None, None) == 0
        assert not b.lattice and b.periodic and lib.fdtd2d_batch_is_lattice(h) == 0
        assert b.lds_bytes == 7 * _seg(R * Cc, 4) + _seg(4 * R, 4) + _seg(4 * Cc, 4)      # the periodic rule again
        real = [np.empty(s, dtype) for s in ((B, R, Cc), (B, R, Cc - 1), (B, R - 1, Cc))]
        assert lib.fdtd2d_batch_download(h, *(a.ctypes.data for a in real), 0 if dtype == np.float32 else 1) == 0
        for a, w in zip(real, (Ez, Hx, Hy)):
            assert np.array_equal(a[:, :R - 1, :Cc - 1], w.real[:, :R - 1, :Cc - 1])
        assert lib.fdtd2d_batch_set_lattice(h, None, None, None, None) == 0            # off twice is no error
        # and on again: the imaginary parts start from zero, the real parts are as they were, the run continues
        b.set_lattice_phase(cfg["phi_r"], cfg["phi_c"]).set_bloch_source("ramp")
        assert b.lattice
        again = b.download()
        for a, w in zip(again, (Ez, Hx, Hy)):
            assert np.array_equal(a.real[:, :R - 1, :Cc - 1], w.real[:, :R - 1, :Cc - 1]) and not a.imag[:, :R - 1, :Cc - 1].any()
        b.run(n, cfg["amps"][:, n:])
        ref = _drive(LatticeOracle(B, R, Cc, DT, DX, dtype=dtype), cfg, monitors=False)
        ref.upload(*(a.real for a in again))
        ref.step = n
        ref.run(n, cfg["amps"][:, n:])
        for a, w in zip(b.download(), ref.download()):
            assert np.array_equal(a, w)
        # periodic off turns the mode off too
        assert lib.fdtd2d_batch_set_periodic(h, 0) == 0 and not b.lattice and not b.periodic


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

def test_the_library_refuses_what_the_lattice_mode_excludes(fd):
    _exact_only(fd)
    from fdtd2d_amd import _abi
    import ctypes as C
    dtype, B, (R, Cc), n = np.float32, 2, SHAPES["23x19"], 12
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    one, zero, w = np.ones(B), np.zeros(B), np.full(B, 1e11)
    on = lambda lib, h: lib.fdtd2d_batch_set_lattice(h, dp(one), dp(zero), dp(one), dp(zero))
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="none") as b:        # needs periodic columns
        b.set_materials(None, None)
        assert on(b._lib, b._h) == E_STATE and "needs periodic columns" in b._lib.fdtd2d_batch_last_error(b._h).decode()
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="periodic") as b:
        lib, h = b._lib, b._h
        err = lambda: lib.fdtd2d_batch_last_error(h).decode()
        assert on(lib, h) == E_STATE and "materials not set" in err()
        b.set_materials(None, None)
        assert lib.fdtd2d_batch_set_lattice(h, dp(one), None, dp(one), dp(zero)) == E_ARG and "all be given" in err()
        assert lib.fdtd2d_batch_set_lattice(h, dp(one), dp(zero), dp(np.array([1.0, np.inf])), dp(zero)) == E_ARG
        assert "member 1" in err()
        # what is already there
        b.set_pml(4)
        assert on(lib, h) == E_STATE and "no layer" in err()
        b.clear_pml().set_bloch_phase(0.3)
        assert on(lib, h) == E_STATE and "fdtd2d_batch_set_bloch" in err()
        b.set_bloch_phase(None).set_dispersion(1e22, 1e11, 0.0)
        assert on(lib, h) == E_STATE and "dispersive pole" in err()
        b.set_dispersion(None).set_dft(1e11)
        assert on(lib, h) == E_STATE and "whole-grid transform" in err()
        b.set_dft(None).set_point_sources([(8, 6)], np.ones((1, 1)))
        assert on(lib, h) == E_STATE and "point source" in err()
        b.set_point_sources(None).set_dft_window((3, 2, 2, 3), [1e11]).hold_dft_window()
        assert on(lib, h) == E_STATE and "held window" in err()
        b.set_dft_window((R - 3, 2, 3, 3), [1e11])
        assert on(lib, h) == E_ARG and f"touches row {R - 1} or column {Cc - 1}" in err()
        b.set_dft_window((3, Cc - 3, 2, 3), [1e11])
        assert on(lib, h) == E_ARG and f"touches row {R - 1} or column {Cc - 1}" in err()
        b.set_dft_window((3, 2, 2, 3), [1e11]).set_probes(np.array([[(4, 2)], [(R - 1, 3)]]), 8)
        assert on(lib, h) == E_ARG and "member 1 probe 0" in err()
        b.set_probes([(0, 0)], n).set_sources(np.array([(R - 2, 3, 2, 2), (4, 4, 1, 1)]))
        assert on(lib, h) == E_ARG and f"member 0: source ({R - 2},3)+2x2 reaches row {R - 1}" in err()
        assert not b.lattice and lib.fdtd2d_batch_is_lattice(h) == 0 and b.lds_bytes == \
            7 * _seg(R * Cc, 4) + _seg(4 * R, 4) + _seg(4 * Cc, 4) + 16 + 96     # nothing changed: the periodic rule
        b.set_sources(np.array([(0, 0, 1, Cc - 1), (4, 4, 1, 1)]))
        assert on(lib, h) == 0 and b.lattice and b.info(_abi.BATCH_INFO_BLOCH) == 0
    # while the mode is on: the library's own refusals (the Python wrappers refuse earlier: tests/test_batch_lattice_cpu.py)
    cfg = _cfg(fd, 2, B, R, Cc, dtype, n)
    cfg["probes"], cfg["window"] = np.array([(0, 0)]), (3, 2, 2, 3)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice") as b:
        lib, h = b._lib, b._h
        err = lambda: lib.fdtd2d_batch_last_error(h).decode()
        _drive(b, cfg)
        b.run(5, cfg["amps"][:, :5])
        state = b.download() + (b.read_dft_window(), b.read_probes(), b.lds_bytes)
        cells, wts, chan = np.array([[6, 6]] * B, dtype=np.int32), np.ones((B, 1)), np.zeros((1, 4))
        out, f32 = np.zeros(4 * B * R * Cc), np.zeros((B, R, Cc), np.float32)
        rowf, colf = np.ones((B, 4 * R), np.float32), np.ones((B, 4 * Cc), np.float32)
        refused = [
            lambda: lib.fdtd2d_batch_set_pml(h, rowf.ctypes.data, colf.ctypes.data, 0, 3),
            lambda: lib.fdtd2d_batch_transfer_ezx(h, f32.ctypes.data, 0, 0),
            lambda: lib.fdtd2d_batch_transfer_ezx(h, f32.ctypes.data, 0, 1),
            lambda: lib.fdtd2d_batch_set_bloch(h, dp(one), dp(zero)),
            lambda: lib.fdtd2d_batch_set_bloch(h, None, None),
            lambda: lib.fdtd2d_batch_set_dispersion(h, f32.ctypes.data, 0, dp(w), dp(zero)),
            lambda: lib.fdtd2d_batch_set_dft(h, dp(w), 1),
            lambda: lib.fdtd2d_batch_set_point_sources(h, 1, ip(cells), 1, dp(wts)),
            lambda: lib.fdtd2d_batch_run_channels(h, 4, None, dp(chan), 0),
            lambda: lib.fdtd2d_batch_hold_dft_window(h),
            lambda: lib.fdtd2d_batch_dft_window_product(h, dp(one), dp(zero), dp(out)),
            lambda: lib.fdtd2d_batch_probe_spectra(h, 1, dp(w), 0, 0, dp(out), dp(out), None),
            lambda: lib.fdtd2d_batch_field_absmax(h, 0, dp(out)),
            lambda: lib.fdtd2d_batch_set_bloch_point_sources(h, 1, ip(cells), 1, dp(wts)),
            lambda: lib.fdtd2d_batch_run_bloch_channels(h, 4, None, None, dp(chan), 0, 0),
            lambda: lib.fdtd2d_batch_hold_bloch_window(h),
            lambda: lib.fdtd2d_batch_bloch_window_product(h, dp(one), dp(zero), dp(out)),
            lambda: lib.fdtd2d_batch_transfer_bloch(h, None, None, None, f32.ctypes.data, 0, 0),
        ]
        for k, call in enumerate(refused):
            assert call() == E_STATE and "is not available in the lattice mode" in err(), k
        win = np.array([1e11] * B)
        assert lib.fdtd2d_batch_set_dft_window(h, R - 3, 2, 3, 3, 1, dp(win), 1) == E_ARG and f"touches row {R - 1}" in err()
        assert lib.fdtd2d_batch_set_dft_window(h, 3, Cc - 3, 2, 3, 1, dp(win), 1) == E_ARG and f"touches column {Cc - 1}" in err()
        bad = np.array([[4, 2], [R - 1, 2]], dtype=np.int32)
        assert lib.fdtd2d_batch_set_probes(h, 1, ip(bad), 8) == E_ARG and "member 1 probe 0" in err()
        bad = np.array([[4, 2], [4, Cc - 1]], dtype=np.int32)
        assert lib.fdtd2d_batch_set_probes(h, 1, ip(bad), 8) == E_ARG and "member 1 probe 0" in err()
        rect = np.array([(R - 2, 3, 2, 2), (4, 4, 1, 1)], dtype=np.int32)
        assert lib.fdtd2d_batch_set_sources(h, ip(rect)) == E_ARG and f"reaches row {R - 1}" in err()
        rect = np.array([(3, Cc - 2, 1, 2), (4, 4, 1, 1)], dtype=np.int32)
        assert lib.fdtd2d_batch_set_sources(h, ip(rect)) == E_ARG and f"reaches column {Cc - 1}" in err()
        nan = np.array([1.0, np.nan])
        assert lib.fdtd2d_batch_set_lattice(h, dp(one), dp(zero), dp(one), dp(nan)) == E_ARG and "member 1" in err()
        assert lib.fdtd2d_batch_set_lattice(h, dp(one), dp(zero), None, dp(zero)) == E_ARG
        # turning the mode off is refused while a conductivity sits where a periodic batch allows none
        assert cfg["sigma"][:, :6, :Cc - 1].any()
        assert lib.fdtd2d_batch_set_lattice(h, None, None, None, None) == E_ARG and "sigma is non-zero" in err()
        assert lib.fdtd2d_batch_set_periodic(h, 0) == E_ARG and "sigma is non-zero" in err()
        # nothing changed: the state is as it was, and the run goes on as the stand-in's
        assert b.lattice and lib.fdtd2d_batch_set_pml(h, None, None, 0, 0) == 0
        now = b.download() + (b.read_dft_window(), b.read_probes(), b.lds_bytes)
        assert all(np.array_equal(x, y) for x, y in zip(state, now))
        # what keeps working: materials, windows of eps and sigma, options, a conductivity in row 0 and column 0
        b.set_conductivity_window((0, 0, 2, 3), np.full((B, 2, 3), 2.0))
        b.set_eps_window((0, 1, 2, 3), np.full((B, 2, 3), 3 * fd.EPS0, np.float32))
        b.set_option(steps_per_launch=5)
        b.run(n - 5, cfg["amps"][:, 5:])
        ref = _drive(LatticeOracle(B, R, Cc, DT, DX, dtype=dtype), cfg)
        ref.run(5, cfg["amps"][:, :5])
        ref.set_conductivity_window((0, 0, 2, 3), np.full((B, 2, 3), 2.0))
        eps = cfg["eps"].copy()
        eps[:, 0:2, 1:4] = np.float32(3 * fd.EPS0)
        ref.set_materials(eps, cfg["mu"])
        ref.run(n - 5, cfg["amps"][:, 5:])
        for a, w2 in zip(b.download() + (b.read_probes(),), ref.download() + (ref.read_probes(),)):
            assert np.array_equal(a, w2)
        assert np.abs(b.read_dft_window() - ref.read_dft_window()).max() <= 1e-12 * np.abs(ref.read_dft_window()).max()


# ---- 6. the run helper ------------------------------------------------------------------------------------------------------------

def test_run_fdtd_batch_takes_a_lattice(fd):
    _exact_only(fd)
    dtype, (R, Cc), B, n = np.float64, SHAPES["23x19"], 3, 40
    eps = np.full((B, R, Cc), fd.EPS0)
    eps[:, 8:14, 5:11] *= 8.9                                         # a rod in the unit cell
    phi_r, phi_c = np.array([0.0, np.pi, np.pi]), np.array([0.0, 0.0, np.pi])      # Gamma, X, M
    kw = dict(nsteps=n, sources=np.array([(3, 0, 1, Cc - 1)] * B), fc=60e9, dt=DT, dx=DX, dtype=dtype, boundary="lattice",
              dft_window=(16, 0, 3, 5), window_omegas=[2 * np.pi * 60e9], probes=[(0, 0), (20, 5)])
    Ez, Hx, Hy, W, tr = fd.run_fdtd_batch(eps, bloch_phase=(phi_r, phi_c), source_weights="ramp", **kw)
    amps = np.tile([fd.ricker_amplitude(i * DT, 60e9) for i in range(n)], (B, 1))
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice") as b:      # the engine driven by hand
        b.set_materials(eps, fd.MU0).set_sources(kw["sources"]).set_lattice_phase(phi_r, phi_c).set_bloch_source("ramp")
        b.set_dft_window(kw["dft_window"], kw["window_omegas"]).set_probes(kw["probes"], n)
        b.run(n, amps)
        for a, w in zip((Ez, Hx, Hy, W, tr), b.download() + (b.read_dft_window(), b.read_probes())):
            assert np.iscomplexobj(a) and np.array_equal(a, w)
    ref = LatticeOracle(B, R, Cc, DT, DX, dtype=dtype)
    ref.set_materials(eps, fd.MU0).set_sources(kw["sources"]).set_lattice_phase(phi_r, phi_c).set_bloch_source("ramp")
    ref.set_dft_window(kw["dft_window"], kw["window_omegas"]).set_probes(kw["probes"], n)
    ref.run(n, amps)
    for a, w in zip((Ez, Hx, Hy, tr), ref.download() + (ref.read_probes(),)):
        assert np.array_equal(a, w)
    assert np.abs(W - ref.read_dft_window()).max() <= 1e-12 * np.abs(W).max()
    assert np.abs(Ez[1:].imag).max() > 0 and not Ez[0].imag.any()    # Gamma stays real


# ---- 7. the fused build ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_lattice as t
out = {"arithmetic": fd.ARITHMETIC, "paths": True}
R, Cc = t.SHAPES["37x31"]
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    cfg = t._cfg(fd, 23, 5, R, Cc, dtype, t.NSTEPS_FIELD)
    got = t._device_run(fd, dtype, R, Cc, cfg, (t.NSTEPS_FIELD,))
    np.save(f"{OUT}/field_{name}.npy", got["fields"][0])
    b = t._device_run(fd, dtype, R, Cc, cfg, (t.NSTEPS_FIELD,), resident=0)      # resident against streamed, in this build
    out["paths"] = out["paths"] and t._same(got, b)
print("LATTICE_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's complex fields against the exact build's (which the stand-in pins), both on the device, each in a
    process of its own; in both builds the resident and the streamed path agree bit for bit."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("LATTICE_RESULT ")][-1][15:])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"field_{k}.npy").astype(np.complex128) for k in FUSED_BOUND}
    worst = {}
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m] - e[m]).max() / np.abs(e[m]).max() for m in range(e.shape[0]))
        print(f"fused vs exact, complex Ez {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
