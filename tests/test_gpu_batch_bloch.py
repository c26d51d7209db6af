"""GPU: the Bloch phase of periodic batches (fdtd2d_batch_bloch.h, kernels_batch_bloch.hpp).

Complex fields, Ezx and probe traces equal the stand-in of tests/oracle_batch_bloch.py bit for bit (exact build), window
DFTs to 1e-12 (the device's float64 cos and sin are not NumPy's, the project's bound for every window DFT): both dtypes,
resident and streamed, whole runs and 7 steps per launch, with a 4-cell layer and with PEC rows, 5 members with distinct
phases, complex amplitudes, ramp weights, a conductivity, a window and three probes (one in column 0).  The shapes are
23 x 11 and 29 x 13: 64 and 128 threads, 64 % 11 = 9 and 128 % 13 = 11, so the cell walk carries in both.  (A 23 x 9 member cannot
exist: the library's minimum is 11 x 11, include/fdtd2d.h; the test asserts that refusal.)  The three exact properties of
tests/test_batch_bloch_cpu.py hold on the device against the plain periodic BatchEngine.  Every path gives the same bits in
both builds.  The largest member the capacity rule admits runs resident, one row more streams.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_BOUND."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_bloch import BlochOracle
from oracle_batch_periodic import PeriodicOracle
import test_batch_bloch_cpu as bcpu

pytestmark = pytest.mark.gpu

ROOT = bcpu.ROOT
DT, DX, LAYER, LDS_LIMIT = 5e-14, 1e-4, 4, 163840
E_ARG, E_STATE = -1, -4
SHAPES = {"23x11": (23, 11), "29x13": (29, 13)}
# The fused build evaluates the multiply-add pairs of the step and the seam's rotations as one fma each
# (batch_periodic_split, _plain, batch_lossy_e, batch_bloch_rot, _unrot, _source), so its results differ from the exact
# build's by rounding.  The quantity is: complex Ez after 300 steps, 5 members of 29 x 13 with the layer, conductivity,
# complex amplitudes and ramp weights, worst member, max|fused - exact| / max|exact|.
# FUSED_MEASURED is what test_fused_build_within_its_bounds printed on its first MI355X run; the bounds are ten times
# that, as for the periodic batch (tests/test_gpu_batch_periodic.py).
NSTEPS_FIELD = 300
FUSED_MEASURED = {"f32": 8.996e-07, "f64": 1.502e-15}
FUSED_BOUND = {k: 10 * v for k, v in FUSED_MEASURED.items()}      # 9.0e-6, 1.5e-14


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _cfg(fd, seed, B, R, Cc, dtype, n):
    """Members with their own materials, phases and line sources (one spans the whole period, one starts in column 0,
    one ends in column C-2), complex amplitudes, a conductivity on the rows that may conduct, a window that stops short of
    column C-1 and three probes, one of them in column 0."""
    rng = np.random.default_rng(seed)
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(dtype)
    mu = (fd.MU0 * np.where(rng.random((B, R, Cc)) < 0.1, 1.5, 1.0)).astype(dtype)
    spans = [(0, Cc - 1), (0, 4), (Cc - 5, 4), (2, Cc - 5)]
    rects = np.array([[R // 2 + (m % 3) - 1, spans[m % 4][0], 1, spans[m % 4][1]] for m in range(B)])
    amps = np.stack([[fd.ricker_amplitude(k * DT, 30e9 * (1 + 0.1 * (m % 7))) for k in range(n)] for m in range(B)])
    amps = amps * np.exp(1j * (0.4 + 0.7 * np.arange(B)))[:, None]
    phis = 0.3 + 2.9 * (np.arange(B) % 11) / 11 + 0.001 * np.arange(B)       # distinct, up to about pi
    sigma = np.zeros((B, R, Cc))
    inner = 20.0 * rng.random((B, R - 12, Cc))
    sigma[:, 6:R - 6, :] = np.where(rng.random(inner.shape) < 0.3, 0.0, inner)
    omegas = (2 * np.pi * np.array([20e9, 45e9, 80e9]))[None, :] * (1 + 0.01 * np.arange(B))[:, None]
    probes = np.array([(R // 2 + 1, 0), (7, Cc - 2), (R - 3, 4)])
    return dict(eps=eps, mu=mu, rects=rects, amps=amps, phis=phis, sigma=sigma, omegas=omegas, probes=probes,
                window=(R // 2 - 2, 1, 4, Cc - 3), n=n)


def _drive(b, cfg, layer, monitors=True):
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    if layer:
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
        b.set_pml(layer, courant00=np.array(c00))
    else:
        b.clear_pml()
    b.set_conductivity(cfg["sigma"])
    b.set_bloch_phase(cfg["phis"]).set_bloch_source("ramp")
    if monitors:
        b.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
    return b


def _expect_path(b, nf, window_cells, never=False, lds_allowed=True):
    """The capacity rule, restated: 11 arrays, the 4R row factors, 16 (C-1) bytes of source weights beside the phasor
    table, and twice the accumulators."""
    esz, R, Cc = b.dtype.itemsize, b.rows, b.cols
    seg = _seg(R * Cc, esz)
    fields = 11 * seg + _seg(4 * R, esz)
    table, acc = 16 * nf + 16 * (Cc - 1), 2 * 16 * nf * window_cells
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = bool(nf) and lds_allowed and fields + table + acc <= LDS_LIMIT
    assert b.bloch and b.periodic
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - _seg(4 * R, esz) - table) // 11 // 16 * 16 // esz
    assert b.resident == resident
    assert b.window_in_lds == (in_lds and resident)
    return resident


def _device_run(fd, dtype, R, Cc, cfg, splits, layer=LAYER, monitors=True, resident=None, spl=None, lds=True):
    B = cfg["eps"].shape[0]
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        _drive(b, cfg, layer, monitors)
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
        out = dict(fields=b.download() + (b.download_ezx(),), path=path, in_lds=b.window_in_lds)
        if monitors:
            out.update(dft=b.read_dft_window(), probes=b.read_probes())
        return out


def _stand_in(dtype, R, Cc, cfg, layer=LAYER, monitors=True):
    B = cfg["eps"].shape[0]
    ref = _drive(BlochOracle(B, R, Cc, DT, DX, dtype=dtype), cfg, layer, monitors)
    ref.run(cfg["n"], cfg["amps"])
    out = dict(fields=ref.download() + (ref.download_ezx(),))
    if monitors:
        out.update(dft=ref.read_dft_window(), probes=ref.read_probes())
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
    """Fields, Ezx and probes bit for bit, the window DFT to 1e-12; both parts and the seam saw the field."""
    for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx"), got["fields"], ref["fields"]):
        assert np.iscomplexobj(a) and np.array_equal(a, w), name
    Ez = got["fields"][0]
    assert np.abs(Ez.real).max() > 0 and np.abs(Ez.imag).max() > 0 and np.abs(Ez[:, :, 0]).max() > 0
    rho = np.exp(1j * cfg["phis"])[:, None]
    assert np.abs(Ez[:, :, -1] - rho * Ez[:, :, 0]).max() <= 1e-6 * np.abs(Ez).max()    # the image is rho * column 0
    if "dft" in ref:
        assert np.array_equal(got["probes"], ref["probes"]) and np.abs(got["probes"][:, 0].imag).max() > 0
        assert np.abs(got["dft"] - ref["dft"]).max() <= 1e-12 * np.abs(ref["dft"]).max()


# ---- 1. against the stand-in ------------------------------------------------------------------------------------------------

N_STEPS = 50


@functools.lru_cache(maxsize=None)
def _reference(fd, dtype, shape, layer):
    R, Cc = SHAPES[shape]
    cfg = _cfg(fd, R + layer, 5, R, Cc, dtype, N_STEPS)
    return cfg, _stand_in(dtype, R, Cc, cfg, layer)


@pytest.mark.parametrize("layer", [LAYER, 0], ids=["layer4", "pec"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("where", ["resident", "resident_spl7", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bloch_runs_match_the_stand_in(fd, dtype, where, shape, layer):
    _exact_only(fd)
    R, Cc = SHAPES[shape]
    assert min(1024, -(-(-(-R * Cc // 4)) // 64) * 64) % Cc != 0        # 64 or 128 threads: the walk carries
    cfg, ref = _reference(fd, dtype, shape, layer)
    got = _device_run(fd, dtype, R, Cc, cfg, (27, 23), layer, resident=0 if where == "streamed" else None,
                      spl=7 if where == "resident_spl7" else 0)
    assert got["path"] == (where != "streamed")
    _agrees(got, ref, cfg)
    assert (np.abs(got["fields"][3]).max() > 0) == bool(layer)


def test_a_member_below_the_minimum_is_refused(fd):
    with pytest.raises(fd.Fdtd2dError, match="11x11") as ei:
        fd.BatchEngine(5, 23, 9, DT, DX, boundary="periodic")
    assert ei.value.code == E_ARG


# ---- 2. the exact properties on the device, against the plain periodic engine -------------------------------------------------

def _engine(fd, resident):
    def make(*a, **k):
        return fd.BatchEngine(*a, **k).set_option(resident=resident)
    return make


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_unit_rotation_is_the_periodic_batch_on_the_device(fd, dtype, resident):
    bcpu.check_unit_rotation(_engine(fd, resident), _engine(fd, resident), dtype)


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_half_turn_is_a_two_period_supercell_on_the_device(fd, dtype, resident):
    bcpu.check_half_turn(_engine(fd, resident), _engine(fd, resident), dtype)


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_quarter_turn_is_two_four_period_supercells_on_the_device(fd, dtype, resident):
    bcpu.check_quarter_turn(_engine(fd, resident), _engine(fd, resident), dtype)


# ---- 3. bit-identical whatever the path, in both builds -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bloch_runs_are_bit_identical_on_every_path(fd, dtype):
    R, Cc = SHAPES["29x13"]
    cfg = _cfg(fd, 5, 6, R, Cc, dtype, 60)
    base = _device_run(fd, dtype, R, Cc, cfg, (60,))
    assert base["path"] and base["in_lds"]
    variants = dict(streamed=dict(resident=0), spl=dict(spl=7), split=dict(splits=(1, 32, 27)),
                    global_acc=dict(lds=False), split_spl=dict(splits=(33, 27), spl=10, lds=False))
    for name, kw in variants.items():
        splits = kw.pop("splits", (60,))
        got = _device_run(fd, dtype, R, Cc, cfg, splits, **kw)
        assert got["path"] == (name != "streamed"), name
        assert got["in_lds"] == (name in ("spl", "split")), name
        assert _same(base, got), name


# ---- 4. the capacity rule ----------------------------------------------------------------------------------------------------

def _largest_rows(fd, dtype, Cc):
    """The most rows of a Cc-column member that the rule admits without monitors: restated here, then checked against
    the library's own figure, read at run time."""
    esz = np.dtype(dtype).itemsize
    fits = lambda R: R * Cc <= (LDS_LIMIT - _seg(4 * R, esz) - 16 * (Cc - 1)) // 11 // 16 * 16 // esz
    R = max(r for r in range(11, 400) if fits(r))
    for rows, want in ((R, True), (R + 1, False)):
        with fd.BatchEngine(1, rows, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
            b.set_materials(None, None).set_bloch_phase(0.5)
            assert (rows * Cc <= b.resident_max_cells) == want and b.resident == want
    return R


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_largest_member_is_resident_and_one_row_more_streams(fd, dtype):
    _exact_only(fd)
    Cc, B, n = 41, 3, 12
    R = _largest_rows(fd, dtype, Cc)
    assert R * Cc > (3400 if dtype == np.float32 else 1700)           # about 3700 float32 / 1850 float64 cells
    assert -(-R * Cc // min(1024, -(-(-(-R * Cc // 4)) // 64) * 64)) <= 4     # at most 4 cells per thread
    for rows, resident in ((R, True), (R + 1, False)):
        cfg = _cfg(fd, rows, B, rows, Cc, dtype, n)
        got = _device_run(fd, dtype, rows, Cc, cfg, (n,), monitors=False)
        assert got["path"] == resident, rows
        _agrees(got, _stand_in(dtype, rows, Cc, cfg, monitors=False), cfg)


def test_more_members_than_one_round_of_workgroups(fd):
    dtype, Cc, B, n = np.float32, 41, 300, 6
    R = _largest_rows(fd, dtype, Cc)
    cfg = _cfg(fd, 9, B, R, Cc, dtype, n)
    a = _device_run(fd, dtype, R, Cc, cfg, (n,), monitors=False)
    b = _device_run(fd, dtype, R, Cc, cfg, (n,), monitors=False, resident=0)
    assert a["path"] and not b["path"] and _same(a, b)
    Ez = a["fields"][0]
    assert all(np.abs(Ez[m].real).max() > 0 and np.abs(Ez[m].imag).max() > 0 for m in range(B))
    assert len({Ez[m].tobytes() for m in range(B)}) == B
    if fd.ARITHMETIC == "exact":                                      # three of them against the stand-in
        pick = [0, 151, 299]
        sub = {k: (v[pick] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in cfg.items()}
        ref = _stand_in(dtype, R, Cc, sub, monitors=False)
        for x, y in zip(a["fields"], ref["fields"]):
            assert np.array_equal(x[pick], y)


# ---- 5. transfers, switching the phase off, refusals ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_complex_fields_round_trip_with_the_image_rotated(fd, dtype):
    B, (R, Cc) = 3, SHAPES["29x13"]
    rng = np.random.default_rng(3)
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64 if dtype == np.float32
                                                                                  else np.complex128)
    Ez, Hx, Hy, Ezx = cplx(B, R, Cc), cplx(B, R, Cc - 1), cplx(B, R - 1, Cc), cplx(B, R, Cc)
    rot = (np.array([0.0, -1.0, 0.6]), np.array([1.0, 0.0, 0.8]))
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        b.set_materials(None, None).set_pml(LAYER).set_bloch_phase(None, rotation=rot)
        assert b.bloch
        b.upload(Ez, Hx, Hy).upload_ezx(Ezx)
        ref = BlochOracle(B, R, Cc, DT, DX, dtype=dtype).set_bloch_phase(None, rotation=rot)
        ref.upload(Ez, Hx, Hy).upload_ezx(Ezx)
        got = b.download() + (b.download_ezx(),)
        for name, a, given, w in zip(("Ez", "Hx", "Hy", "Ezx"), got, (Ez, Hx, Hy, Ezx), ref.download() + (ref.download_ezx(),)):
            assert np.array_equal(a, w), name
            assert np.array_equal(a[..., :Cc - 1], given[..., :Cc - 1]), name
        assert np.array_equal(got[0][1, :, -1], -Ez[1, :, 0]) and np.array_equal(got[0][0, :, -1], 1j * Ez[0, :, 0])
        assert np.array_equal(got[3][0, :, -1], 1j * Ezx[0, :, 0])
        # a real upload has a zero imaginary part; download(dtype) converts both parts
        b.upload(Ez=Ez.real)
        assert not b.download()[0][..., :Cc - 1].imag.any()
        assert b.download(np.float64)[0].dtype == np.complex128
        b.reset()
        assert not any(np.any(a) for a in b.download() + (b.download_ezx(),))


def test_switching_the_phase_off_returns_the_batch_to_the_periodic_kernels(fd):
    _exact_only(fd)
    dtype, (R, Cc), B, n = np.float32, SHAPES["29x13"], 4, 30
    cfg = _cfg(fd, 21, B, R, Cc, dtype, 2 * n)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        _drive(b, cfg, LAYER, monitors=False)
        b.run(n, cfg["amps"][:, :n])
        Ez, Hx, Hy = b.download()
        Ezx = b.download_ezx()
        assert b.set_bloch_phase(None) is b and not b.bloch and b.periodic
        assert b.lds_bytes == 7 * _seg(R * Cc, 4) + _seg(4 * R, 4) + _seg(4 * Cc, 4)      # the periodic rule again
        got = b.download() + (b.download_ezx(),)
        for a, w in zip(got, (Ez, Hx, Hy, Ezx)):
            assert a.dtype == dtype and np.array_equal(a[..., :Cc - 1], w.real[..., :Cc - 1])
        assert np.array_equal(got[0][:, :, -1], got[0][:, :, 0]) and np.array_equal(got[3][:, :, -1], got[3][:, :, 0])
        amps = cfg["amps"][:, n:].real
        b.run(n, amps)
        ref = PeriodicOracle(B, R, Cc, DT, DX, dtype=dtype)
        ref.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
        ref.set_pml(LAYER, courant00=np.array([(1 / np.sqrt(float(e) * float(u)) * DT) / DX
                                               for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]))
        ref.set_conductivity(cfg["sigma"])
        ref.upload(*got[:3]).upload_ezx(got[3])
        ref.run(n, amps)
        for a, w in zip(b.download() + (b.download_ezx(),), ref.download() + (ref.download_ezx(),)):
            assert np.array_equal(a, w)
        # and on again: the imaginary parts start from zero
        b.set_bloch_phase(cfg["phis"])
        assert b.bloch and not any(a.imag[..., :Cc - 1].any() for a in b.download())


def test_the_library_refuses_what_a_bloch_phase_excludes(fd):
    from fdtd2d_amd import _abi
    import ctypes as C
    B, (R, Cc) = 2, SHAPES["29x13"]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    one, zero, w = np.ones(B), np.zeros(B), np.full(B, 1e11)
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="none") as b:        # needs periodic columns
        assert b._lib.fdtd2d_batch_set_bloch(b._h, dp(one), dp(zero)) == E_STATE
        assert "needs periodic columns" in b._lib.fdtd2d_batch_last_error(b._h).decode()
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="periodic") as b:
        lib, h = b._lib, b._h
        err = lambda: lib.fdtd2d_batch_last_error(h).decode()
        b.set_materials(None, None)
        assert lib.fdtd2d_batch_set_bloch_source(h, None, None) == E_STATE and "no Bloch phase is set" in err()
        assert lib.fdtd2d_batch_run_bloch(h, 3, None, None) == E_STATE
        assert lib.fdtd2d_batch_set_bloch(h, dp(one), None) == E_ARG
        assert lib.fdtd2d_batch_set_bloch(h, dp(np.array([1.0, np.nan])), dp(zero)) == E_ARG and "member 1" in err()
        # monitors that are already there
        b.set_dft_window((3, Cc - 3, 2, 3), [1e11])
        assert lib.fdtd2d_batch_set_bloch(h, dp(one), dp(zero)) == E_ARG and "touches column 12" in err()
        b.set_dft_window((3, 2, 2, 3), [1e11]).set_probes(np.array([[(4, 2)], [(5, Cc - 1)]]), 8)
        assert lib.fdtd2d_batch_set_bloch(h, dp(one), dp(zero)) == E_ARG and "member 1 probe 0" in err()
        b.set_probes([(4, 2)], 8).set_dft(1e11)
        assert lib.fdtd2d_batch_set_bloch(h, dp(one), dp(zero)) == E_STATE and "whole-grid transform" in err()
        b.set_dft(None).set_point_sources([(6, 6)], np.ones((1, 1)))
        assert lib.fdtd2d_batch_set_bloch(h, dp(one), dp(zero)) == E_STATE and "point source" in err()
        b.set_point_sources(None).hold_dft_window()
        assert lib.fdtd2d_batch_set_bloch(h, dp(one), dp(zero)) == E_STATE and "held window" in err()
        assert not b.bloch
        b.set_dft_window((3, 2, 2, 3), [1e11])
        b.set_bloch_phase([0.4, 1.1])
        assert b.bloch and b.info(_abi.BATCH_INFO_BLOCH) == 1
        # while the phase is set, the library's own refusals (the Python wrappers refuse earlier: tests/test_batch_bloch_cpu.py)
        cells, wts, chan = np.array([[6, 6]] * B, dtype=np.int32), np.ones((B, 1)), np.zeros((1, 4))
        out = np.zeros(4 * B * R * Cc)
        assert lib.fdtd2d_batch_set_dft(h, dp(w), 1) == E_STATE and "is not available while a Bloch phase is set" in err()
        assert lib.fdtd2d_batch_set_point_sources(h, 1, ip(cells), 1, dp(wts)) == E_STATE
        assert lib.fdtd2d_batch_run_channels(h, 4, None, dp(chan), 0) == E_STATE
        assert lib.fdtd2d_batch_hold_dft_window(h) == E_STATE
        assert lib.fdtd2d_batch_dft_window_product(h, dp(one), dp(zero), dp(out)) == E_STATE
        assert lib.fdtd2d_batch_probe_spectra(h, 1, dp(w), 0, 0, dp(out), dp(out), None) == E_STATE
        assert lib.fdtd2d_batch_field_absmax(h, 0, dp(out)) == E_STATE
        win = np.array([1e11] * B)
        assert lib.fdtd2d_batch_set_dft_window(h, 3, Cc - 3, 2, 3, 1, dp(win), 1) == E_ARG and "touches column 12" in err()
        bad = np.array([[4, 2], [4, Cc - 1]], dtype=np.int32)
        assert lib.fdtd2d_batch_set_probes(h, 1, ip(bad), 8) == E_ARG and "member 1 probe 0" in err()
        assert lib.fdtd2d_batch_run_bloch(h, 3, None, dp(out)) == E_ARG
        assert lib.fdtd2d_batch_set_bloch_source(h, dp(out), None) == E_ARG
        wbad = np.ones((B, Cc - 1))
        wbad[1, 3] = np.inf
        assert lib.fdtd2d_batch_set_bloch_source(h, dp(wbad), dp(np.zeros((B, Cc - 1)))) == E_ARG and "member 1" in err()
        # nothing changed: the monitors that were set still record both parts, what keeps working still works
        b.set_sources(np.array([(10, 3), (11, 0)]))
        b.set_conductivity(0.5).set_conductivity_window((10, 2, 3, 4), np.full((B, 3, 4), 2.0))
        b.set_eps_window((12, 1, 2, 3), np.full((B, 2, 3), 3 * fd.EPS0, np.float32))
        b.set_pml(LAYER).set_option(steps_per_launch=5)
        b.run(12, np.ones((B, 12)) * (1 + 1j))
        assert b.step_count == 12 and np.abs(b.read_dft_window().imag).max() > 0
        assert b.read_probes().shape == (B, 1, 8) and np.iscomplexobj(b.read_probes())
        b.clear_pml()
        # periodic off turns the phase off too
        assert lib.fdtd2d_batch_set_periodic(h, 0) == 0 and not b.bloch and not b.periodic


def test_run_fdtd_batch_takes_a_bloch_phase(fd):
    _exact_only(fd)
    dtype, (R, Cc), B, n = np.float64, SHAPES["29x13"], 3, 40
    eps = np.full((B, R, Cc), fd.EPS0)
    eps[:, 12:16, :] *= 2.5
    phis = np.array([0.2, 0.9, 2.0])
    kw = dict(nsteps=n, sources=np.array([(8, 0, 1, Cc - 1)] * B), fc=60e9, dt=DT, dx=DX, dtype=dtype, boundary="periodic",
              pml_cells=LAYER, dft_window=(18, 0, 3, 5), window_omegas=[2 * np.pi * 60e9], probes=[(20, 0), (20, 5)])
    Ez, Hx, Hy, W, tr = fd.run_fdtd_batch(eps, bloch_phase=phis, source_weights="ramp", **kw)
    ref = BlochOracle(B, R, Cc, DT, DX, dtype=dtype)
    ref.set_materials(eps, fd.MU0).set_pml(LAYER, courant00=bcpu.C0 * DT / DX).set_sources(kw["sources"])
    ref.set_bloch_phase(phis).set_bloch_source("ramp")
    ref.set_dft_window(kw["dft_window"], kw["window_omegas"]).set_probes(kw["probes"], n)
    ref.run(n, np.tile([fd.ricker_amplitude(i * DT, 60e9) for i in range(n)], (B, 1)))
    for a, w in zip((Ez, Hx, Hy, tr), ref.download() + (ref.read_probes(),)):
        assert np.iscomplexobj(a) and np.array_equal(a, w)
    assert np.abs(W - ref.read_dft_window()).max() <= 1e-12 * np.abs(W).max() and np.abs(Ez.imag).max() > 0


# ---- 6. the fused build ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_bloch as t
out = {"arithmetic": fd.ARITHMETIC, "paths": True}
R, Cc = t.SHAPES["29x13"]
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    cfg = t._cfg(fd, 23, 5, R, Cc, dtype, t.NSTEPS_FIELD)
    got = t._device_run(fd, dtype, R, Cc, cfg, (t.NSTEPS_FIELD,))
    np.save(f"{OUT}/field_{name}.npy", got["fields"][0])
    b = t._device_run(fd, dtype, R, Cc, cfg, (t.NSTEPS_FIELD,), resident=0)      # resident against streamed, in this build
    out["paths"] = out["paths"] and t._same(got, b)
print("BLOCH_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's complex fields against the exact build's, both on the device, each in a process of its own; in
    both builds the resident and the streamed path agree bit for bit."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("BLOCH_RESULT ")][-1][13:])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"field_{k}.npy").astype(np.complex128) for k in FUSED_BOUND}
    worst = {}
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m] - e[m]).max() / np.abs(e[m]).max() for m in range(e.shape[0]))
        print(f"fused vs exact, complex Ez {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
