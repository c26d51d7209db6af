"""GPU: a Bloch phase in the Hz polarisation (fdtd2d_batch_hz_bloch.h, kernels_batch_hz_bloch.hpp).

The eight complex fields (Hz, Ex, Ey, Hzx, Jx, Qx, Jy, Qy) and the probe traces equal the stand-in of
tests/oracle_batch_hz_bloch.py bit for bit (exact build), window DFTs to 1e-12: both dtypes, resident with and without the
pole, 7 steps per launch (a run cut in three), streamed, and resident continued streamed, on the periodic shapes of
tests/test_gpu_batch_hz.py (23x11 with a 4-cell layer, 29x13 with PEC rows: the smallest at which the cell walk carries
and the seam is exercised).  Five members with distinct eps, mu, sigma, wp2, gamma and omega0 (a Drude one, a lossless one
and one with wp2 = 0) and the phases 0, pi, 0.7, -2.1, 3.0; wp2 and sigma on every cell that may carry them, columns 0 and
C-2 included; sources in columns 0 and C-2 with complex amplitudes and ramp weights; a window next to the seam, probes in
columns 0 and C-2 and a random uploaded complex state that includes the pole's.  Every case asserts the path it took and
its launch count.

Device against device: the lossless run equals the Ez Bloch kernels' with eps and mu exchanged and E negated; at phi = 0
the real parts equal the real Hz periodic kernels' run and the imaginary parts are zero.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_MEASURED."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_hz_bloch import HzBlochOracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, LDS_LIMIT = 5e-14, 1e-4, 163840
E_ARG, E_STATE = -1, -4
B, NSTEPS = 5, 21
PHI = np.array([0.0, np.pi, 0.7, -2.1, 3.0])
GAMMA = np.array([1e11, 0.0, 5e10, 8e10, 2e10])
OMEGA0 = 2 * np.pi * np.array([0.0, 50e9, 60e9, 40e9, 0.0])      # member 0 Drude, 1 lossless, 4 has wp2 = 0
WP2_TOP = (2 * np.pi * 70e9) ** 2
# (rows, cols, layer): layer 0 = PEC rows
CASES = {"per23x11": (23, 11, 4), "per29x13pec": (29, 13, 0)}
# The fused build evaluates the rotations, the pole, the layer's and Hz's updates as the fma that fdtd2d_batch_hz_bloch.h
# and fdtd2d_batch_hz.h write out, so its results differ from the exact build's by rounding.  Measured on an MI355X (the
# child processes of test_fused_build_within_its_bounds): both parts of Hz after 300 steps of the members of both cases
# from rest, worst member's max|fused - exact| / max|exact|.  The bound is ten times the measured value.
NSTEPS_FUSED = 300
FUSED_CASES = ("per23x11", "per29x13pec")
FUSED_MEASURED = {"f32": 8.6e-7, "f64": 1.8e-15}
FUSED_BOUND = {k: 10 * v for k, v in FUSED_MEASURED.items()}
NAMES = ("Hz", "Ex", "Ey", "Hzx", "Jx", "Qx", "Jy", "Qy")


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_within_its_bounds")


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _cfg(case, dtype, n=NSTEPS, seed=11, state=True):
    """The five members of a case: materials, conductivity, strengths, phases, sources, monitors and (state) a random
    complex state."""
    from fdtd2d_amd.api import EPS0, MU0, ricker_amplitude
    R, C, layer = CASES[case]
    rng = np.random.default_rng(seed)
    g = max(6, layer)
    rows = slice(g, R - 1 - g)                                     # rows g .. R-2-g
    shape = (B, R - 1 - 2 * g, C)                                  # the period and its never-read image
    wp2, sigma = np.zeros((B, R, C)), np.zeros((B, R, C))
    wp2[:, rows, :] = WP2_TOP * (0.05 + rng.random(shape))         # every allowed cell: the metal touches the seam
    wp2[4] = 0.0
    sigma[:, rows, :] = np.where(rng.random(shape) < 0.3, 0.0, 5.0 * rng.random(shape))
    real = np.stack([[ricker_amplitude(k * DT, 40e9 * (1 + 0.1 * m)) for k in range(n)] for m in range(B)])
    cfg = dict(case=case, R=R, C=C, layer=layer, dtype=dtype, n=n, wp2=wp2, sigma=sigma, phi=PHI,
               eps=(EPS0 * (1 + 3 * rng.random((B, R, C)))).astype(dtype),
               mu=(MU0 * (1 + 0.5 * rng.random((B, R, C)))).astype(dtype),
               rects=np.array([[R // 2 + m % 2, (0, 2, C - 4, 1, 3)[m], 1, (C - 1, 3, 3, 1, 4)[m]] for m in range(B)]),
               amps=real * np.exp(1j * (0.4 * np.arange(B) - 0.3))[:, None], weights="ramp",
               omegas=2 * np.pi * np.array([45e9, 65e9]), window=(5, C - 6, 8, 5),
               probes=np.array([[8, 0], [10, C - 2], [R - 3, 4]]), gamma=GAMMA, omega0=OMEGA0)
    if state:                                                      # Hz, Ex, Ey, Hzx, Jx, Qx, Jy, Qy
        shapes = ((B, R, C), (B, R, C - 1), (B, R - 1, C)) + ((B, R, C),) * 5
        cfg["state"] = [rng.standard_normal(s) + 1j * rng.standard_normal(s) for s in shapes]
    return cfg


def _engine(fd, count, cfg, polarization="hz"):
    b = fd.BatchEngine(count, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic")
    return b.set_polarization(polarization)


def _drive(b, cfg, pole=True, sigma=True, phase=True):
    """The same calls on a BatchEngine and on the stand-in."""
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    if cfg["layer"]:
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
        b.set_pml(cfg["layer"], courant00=np.array(c00))
    else:
        b.clear_pml()
    if sigma:
        b.set_conductivity(cfg["sigma"])
    if pole:
        b.set_dispersion(cfg["wp2"], cfg["gamma"], cfg["omega0"])
    b.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
    if phase:
        b.set_hz_bloch_phase(cfg["phi"]).set_hz_bloch_source(cfg["weights"])
    if "state" in cfg:
        s = cfg["state"] if phase else [a.real for a in cfg["state"]]
        b.upload(s[0], s[1], s[2])
        b.upload_ezx(s[3])
        if pole:
            b.upload_hz_dispersion(*s[4:8])
    return b


def _results(b, pole=True):
    return dict(fields=tuple(b.download()) + (b.download_ezx(),) + (tuple(b.download_dispersion()) if pole else ()),
                dft=b.read_dft_window(), probes=b.read_probes())


_refs = {}


def _stand_in(case, dtype, pole=True, **kw):
    """The stand-in's results of a case, computed once."""
    key = (case, np.dtype(dtype).name, pole) + tuple(sorted(kw.items()))
    if key not in _refs:
        _refs[key] = _oracle_run(_cfg(case, dtype, **kw), pole)
    return _refs[key]


def _oracle_run(cfg, pole=True, sigma=True):
    ref = _drive(HzBlochOracle(len(cfg["eps"]), cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"]), cfg, pole, sigma)
    ref.run(cfg["n"], cfg["amps"])
    return _results(ref, pole)


def _expect_path(b, cfg, never=False, pole=True):
    """The capacity rule, restated: twenty arrays with the pole, eleven without, the 4R row factors, the 2 (C-1) float64
    source weights with the phasor table, and the accumulators of both parts when they fit."""
    esz, R, C = b.dtype.itemsize, b.rows, b.cols
    arrays = 20 if pole else 11
    seg = _seg(R * C, esz)
    fields = arrays * seg + _seg(4 * R, esz)
    nf = len(cfg["omegas"])
    table, acc = 16 * nf + 16 * (C - 1), 2 * 16 * nf * cfg["window"][2] * cfg["window"][3]
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = fields + table + acc <= LDS_LIMIT
    assert b.polarization == "hz" and b.dispersive == pole and b.hz_bloch and not b.bloch
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - _seg(4 * R, esz) - table) // arrays // 16 * 16 // esz
    assert b.resident == resident
    return resident


def _device_run(fd, cfg, splits=None, resident=None, spl=None, pole=True, sigma=True, then_streamed=False):
    """then_streamed: the second of two runs is streamed."""
    with _engine(fd, len(cfg["eps"]), cfg) as b:
        _drive(b, cfg, pole, sigma)
        b.set_option(resident=resident, steps_per_launch=spl)
        path = _expect_path(b, cfg, never=resident == 0, pole=pole)
        done = 0
        for k in splits or (cfg["n"],):
            if then_streamed and done:
                b.set_option(resident=0)
                path = False
            launches = b.launches
            b.run(k, cfg["amps"][:, done:done + k])
            done += k
            # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert b.launches - launches == ((-(-k // spl) if spl else 1) if path else 2 * k)
        out = _results(b, pole)
        out["path"] = path
        return out


def _same(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"])) and np.array_equal(a["dft"], b["dft"])
            and np.array_equal(a["probes"], b["probes"]))


def _matches(got, want):
    for name, a, w in zip(NAMES, got["fields"], want["fields"]):
        assert np.iscomplexobj(a) and a.dtype == w.dtype and np.array_equal(a, w), name
    assert len(got["fields"]) == len(want["fields"])
    assert np.iscomplexobj(got["probes"]) and np.array_equal(got["probes"], want["probes"])
    assert np.abs(got["dft"] - want["dft"]).max() <= 1e-12 * np.abs(want["dft"]).max()


# ---- 1. against the stand-in, whatever the path ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_hz_bloch_runs_match_the_stand_in_on_every_path(fd, case, dtype):
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    want = _stand_in(case, dtype)
    assert all(np.any(a.real) and np.any(a.imag) for a in want["fields"])
    runs = {"resident": _device_run(fd, cfg),
            "split7": _device_run(fd, cfg, spl=7),
            "then_streamed": _device_run(fd, cfg, splits=(8, 13), then_streamed=True),
            "streamed": _device_run(fd, cfg, resident=0)}
    for name, got in runs.items():
        assert got["path"] == (name in ("resident", "split7")), name
        _matches(got, want)
    for name, got in runs.items():
        assert _same(got, runs["resident"]), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_hz_bloch_runs_without_a_pole_match_the_stand_in(fd, case, dtype):
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    want = _stand_in(case, dtype, pole=False)
    for kw in (dict(), dict(spl=7), dict(resident=0)):
        got = _device_run(fd, cfg, pole=False, **kw)
        assert got["path"] == (kw.get("resident") != 0)
        _matches(got, want)


# ---- 2. two cells per thread, and the first shape that no longer fits ---------------------------------------------------------

def _plain_cfg(R, C, layer, dtype, n, seed=3):
    """One shape of any size: the members of _cfg with their state."""
    CASES["tmp"] = (R, C, layer)
    try:
        return _cfg("tmp", dtype, n=n, seed=seed)
    finally:
        del CASES["tmp"]


def test_a_pole_member_of_two_cells_per_thread_is_resident_and_the_next_size_is_streamed(fd):
    """61 x 31 float32 with the pole: 1891 cells on 1024 threads, no multiple of 31, so the walk wraps; then the first
    row count above the reported resident_max_cells, which runs streamed."""
    _exact_only(fd)
    cfg = _plain_cfg(61, 31, 6, np.float32, 9)
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg)
        most = b.resident_max_cells
    assert 1891 <= most < 2048
    got = _device_run(fd, cfg)
    assert got["path"] is True
    _matches(got, _oracle_run(cfg))
    rows = most // 31 + 1
    big = _plain_cfg(rows, 31, 6, np.float32, 5)
    got = _device_run(fd, big)
    assert rows * 31 > most and got["path"] is False
    _matches(got, _oracle_run(big))


# ---- 3. device against device ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_the_lossless_run_is_the_ez_bloch_run_with_exchanged_materials(fd, case, dtype, where):
    """Hz = Ez, Ex = -Hx, Ey = -Hy, Hzx = Ezx, bit for bit, against k_batch_resident_bloch and its streamed pair, without
    the stand-in."""
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    never = 0 if where == "streamed" else None
    hz = _device_run(fd, cfg, resident=never, pole=False, sigma=False)
    s = cfg["state"]
    with _engine(fd, B, cfg, "ez") as b:
        b.set_materials(cfg["mu"], cfg["eps"]).set_sources(cfg["rects"])
        if cfg["layer"]:
            c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
            b.set_pml(cfg["layer"], courant00=np.array(c00))
        else:
            b.clear_pml()
        b.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
        b.set_bloch_phase(cfg["phi"]).set_bloch_source("ramp")
        b.upload(s[0], -s[1], -s[2]).upload_ezx(s[3])
        b.set_option(resident=never)
        assert b.polarization == "ez" and b.bloch and not b.hz_bloch and b.resident == (where == "resident")
        b.run(cfg["n"], cfg["amps"])
        ez = _results(b, pole=False)
    for name, a, w, sign in zip(NAMES, hz["fields"], ez["fields"], (1, -1, -1, 1)):
        assert np.any(a.imag) and np.array_equal(a, sign * w), name
    assert np.array_equal(hz["dft"], ez["dft"]) and np.array_equal(hz["probes"], ez["probes"])


@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_zero_phase_is_the_real_hz_periodic_run(fd, dtype, where):
    """c = 1, s = 0, real amplitudes, unit weights and a real state: the real parts equal the kernels of batch_hz.hip on
    the same members, pole and sigma included, and the imaginary parts are zero."""
    _exact_only(fd)
    cfg = _cfg("per23x11", dtype)
    cfg.update(amps=cfg["amps"].real.copy(), weights=None, state=[a.real + 0j for a in cfg["state"]])
    never = 0 if where == "streamed" else None
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg, phase=False)
        b.set_hz_bloch_phase(None, rotation=(1.0, 0.0))
        b.set_option(resident=never)
        assert b.hz_bloch and b.resident == (where == "resident")
        b.run(cfg["n"], cfg["amps"])
        got = _results(b)
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg, phase=False)
        b.set_option(resident=never)
        assert not b.hz_bloch and b.resident == (where == "resident")
        b.run(cfg["n"], cfg["amps"])
        want = _results(b)
    for name, a, w in zip(NAMES, got["fields"], want["fields"]):
        assert np.iscomplexobj(a) and not np.iscomplexobj(w) and np.any(w), name
        assert np.array_equal(a.real, w) and not a.imag.any(), name
    assert np.array_equal(got["probes"].real, want["probes"]) and not got["probes"].imag.any()
    assert np.abs(got["dft"] - want["dft"]).max() <= 1e-12 * np.abs(want["dft"]).max()


def test_new_phases_keep_the_pole_state_and_turning_the_phase_off_keeps_the_real_parts(fd):
    cfg = _cfg("per23x11", np.float32)
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg)
        b.run(5, cfg["amps"])
        before = _results(b)
        b.set_hz_bloch_phase(PHI[::-1].copy())
        after = _results(b)
        for name, a, w in zip(NAMES, after["fields"], before["fields"]):
            if name in ("Hz", "Hzx"):                              # the image column is delivered rotated by the new phase
                a, w = a[..., :-1], w[..., :-1]
            assert np.array_equal(a, w), name
        assert np.array_equal(after["dft"], before["dft"]) and np.array_equal(after["probes"], before["probes"])
        b.set_hz_bloch_phase(None)
        assert not b.hz_bloch and not b.bloch and b.dispersive and b.polarization == "hz"
        off = _results(b)
        for name, a, w in zip(NAMES, off["fields"], before["fields"]):
            assert not np.iscomplexobj(a), name
            if name in ("Hz", "Hzx"):
                assert np.array_equal(a[..., -1], a[..., 0]), name     # a plain periodic batch: the image is column 0
                a, w = a[..., :-1], w[..., :-1]
            assert np.array_equal(a, w.real), name
        b.run(3, cfg["amps"].real)                                 # and it runs on the real Hz kernels again
        b.set_hz_bloch_phase(0.5)                                  # a phase set again starts with zero imaginary parts
        hz, ex, ey = b.download()                                  # (Hz's image column is delivered rotated: sin(0.5) * Hz[:, 0])
        parts = (hz[..., :-1], ex, ey, b.download_ezx()[..., :-1]) + b.download_dispersion()
        assert b.hz_bloch and np.any(hz.real) and not any(np.any(a.imag) for a in parts)


# ---- 4. refusals leave the batch as it was ----------------------------------------------------------------------------------

def _raises(fd, code, match, call):
    with pytest.raises(fd.Fdtd2dError, match=match) as ei:
        call()
    assert ei.value.code == code


def test_refusals_leave_an_hz_bloch_batch_as_it_was(fd):
    _exact_only(fd)
    cfg = _cfg("per23x11", np.float32)
    R, C = cfg["R"], cfg["C"]
    want = _stand_in("per23x11", np.float32)
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg)
        lds = b.lds_bytes
        _raises(fd, E_ARG, "touches column 10", lambda: b.set_dft_window((5, C - 5, 8, 5), cfg["omegas"]))
        _raises(fd, E_ARG, "touches column 10", lambda: b.set_probes([(8, 0), (10, C - 1)], 10))
        for call, match in ((lambda: b.set_dft(3e11), "Bloch phase"),
                            (lambda: b.set_point_sources(np.array([[8, 1]]), np.ones((1, 1))), "Bloch phase"),
                            (lambda: b.run(2, None, np.zeros((1, 2))), "Bloch phase"),
                            (lambda: b.set_hz_flux_lines([("row", 10, 0, C - 1)], [3e11]), "Bloch phase"),
                            (lambda: b.set_polarization("ez"), "Bloch phase"),
                            (lambda: b.set_bloch_phase(0.5), "Hz polarisation"),
                            (lambda: b.set_bloch_phase(None), "Hz polarisation"),
                            (lambda: b.set_bloch_flux_lines([("row", 10, 0, C - 1)], [3e11]), "Hz polarisation"),
                            (lambda: b.set_bloch_point_sources(np.array([[8, 1]]), np.ones((1, 1))), "Hz polarisation"),
                            (lambda: b.set_bloch_dispersion(cfg["wp2"], GAMMA, OMEGA0), "Hz polarisation"),
                            (b.hold_dft_window, "Hz polarisation"), (b.hold_bloch_window, "Hz polarisation"),
                            (lambda: b.set_flux_lines([("row", 10, 0, C - 1)], [3e11]), "Hz polarisation"),
                            (lambda: b.set_conductivity_window((10, 8, 1, 1), np.zeros((B, 1, 1))), "Hz polarisation")):
            _raises(fd, E_STATE, match, call)
        L = b._lib
        one = np.ones(B * R * C)
        dp = one.ctypes.data_as(L.fdtd2d_batch_set_bloch.argtypes[1])
        ip = np.array([8, 1], np.int32).ctypes.data_as(L.fdtd2d_batch_set_point_sources.argtypes[2])
        line = np.array([0, 10, 0, C - 1], np.int32).ctypes.data_as(L.fdtd2d_batch_set_hz_flux_lines.argtypes[2])
        win = (np.array([10, 8, 1, 1], np.int32)).ctypes.data_as(L.fdtd2d_batch_set_dispersion_window.argtypes[1])
        for rc in (L.fdtd2d_batch_set_dft(b._h, dp, 1), L.fdtd2d_batch_set_point_sources(b._h, 1, ip, 1, dp),
                   L.fdtd2d_batch_run_channels(b._h, 2, None, dp, 0),
                   L.fdtd2d_batch_set_hz_flux_lines(b._h, 1, line, 1, dp, 1),
                   L.fdtd2d_batch_set_polarization(b._h, 0), L.fdtd2d_batch_set_periodic(b._h, 0),
                   L.fdtd2d_batch_set_bloch(b._h, dp, dp), L.fdtd2d_batch_set_bloch(b._h, None, None),
                   L.fdtd2d_batch_set_bloch_source(b._h, None, None), L.fdtd2d_batch_run_bloch(b._h, 1, None, None),
                   L.fdtd2d_batch_transfer_bloch(b._h, one.ctypes.data, None, None, None, 1, 0),
                   L.fdtd2d_batch_read_dft_window_bloch(b._h, dp, dp), L.fdtd2d_batch_read_probes_bloch(b._h, dp, 0, 1),
                   L.fdtd2d_batch_set_bloch_point_sources(b._h, 1, ip, 1, dp), L.fdtd2d_batch_hold_bloch_window(b._h),
                   L.fdtd2d_batch_set_bloch_dispersion(b._h, one.ctypes.data, 1, dp, dp),
                   L.fdtd2d_batch_set_bloch_flux_lines(b._h, 1, line, 1, dp, 1),
                   L.fdtd2d_batch_set_lattice(b._h, dp, dp, dp, dp), L.fdtd2d_batch_hold_dft_window(b._h),
                   L.fdtd2d_batch_set_dispersion(b._h, one.ctypes.data, 1, dp, dp),
                   L.fdtd2d_batch_set_dispersion_window(b._h, win, one.ctypes.data, 1),
                   L.fdtd2d_batch_set_conductivity(b._h, one.ctypes.data, 1)):
            assert rc == E_STATE
        assert L.fdtd2d_batch_set_polarization(b._h, 1) == 0          # the polarisation it has: nothing to do
        nan = np.full(B, np.nan)
        assert L.fdtd2d_batch_set_hz_bloch(b._h, nan.ctypes.data_as(type(dp)), dp) == E_ARG
        assert L.fdtd2d_batch_set_hz_bloch(b._h, dp, None) == E_ARG
        assert b.dispersive and b.polarization == "hz" and b.lds_bytes == lds and b.hz_bloch and not b.bloch
        b.run(cfg["n"], cfg["amps"])
        _matches(_results(b), want)
    with _engine(fd, B, cfg) as b:                                 # the phase beside Hz flux lines, and off the polarisation
        _drive(b, cfg, phase=False)
        b.set_hz_flux_lines([("row", 10, 0, C - 1)], [3e11])
        c = np.ones(B)
        cp = c.ctypes.data_as(b._lib.fdtd2d_batch_set_hz_bloch.argtypes[1])
        assert b._lib.fdtd2d_batch_set_hz_bloch(b._h, cp, cp) == E_STATE and not b.hz_bloch
        _raises(fd, E_STATE, "flux lines", lambda: b.set_hz_bloch_phase(0.3))
    with fd.BatchEngine(B, R, C, DT, DX, boundary="periodic") as b:
        assert b._lib.fdtd2d_batch_set_hz_bloch(b._h, cp, cp) == E_STATE and not b.hz_bloch and not b.bloch
        _raises(fd, E_STATE, "needs the Hz polarisation", lambda: b.set_hz_bloch_phase(0.3))
    with fd.BatchEngine(B, R, 19, DT, DX, boundary="pml") as b:
        b.set_polarization("hz")
        assert b._lib.fdtd2d_batch_set_hz_bloch(b._h, cp, cp) == E_STATE and not b.hz_bloch


def test_the_pole_may_come_before_or_after_the_phase_and_reset_zeroes_both_parts(fd):
    _exact_only(fd)
    cfg = _cfg("per29x13pec", np.float64)
    want = _stand_in("per29x13pec", np.float64)
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg, pole=False, sigma=False)                   # the phase first, then sigma and the pole
        b.set_conductivity(cfg["sigma"]).set_dispersion(cfg["wp2"], cfg["gamma"], cfg["omega0"])
        assert not any(np.any(a) for a in b.download_dispersion())
        b.upload_hz_dispersion(*cfg["state"][4:8])
        _expect_path(b, cfg)
        b.run(cfg["n"], cfg["amps"])
        _matches(_results(b), want)
        b.reset()
        got = _results(b)
        assert not any(np.any(a) for a in got["fields"]) and not np.any(got["dft"]) and b.step_count == 0


def test_run_fdtd_batch_takes_the_hz_bloch_phase(fd):
    _exact_only(fd)
    from fdtd2d_amd.api import MU0
    cfg = _cfg("per23x11", np.float64, n=30, state=False)
    eps = cfg["eps"].astype(np.float64)
    out = fd.run_fdtd_batch(eps, nsteps=30, sources=cfg["rects"], fc=35e9, dtype=np.float64, boundary="periodic", pml_cells=4,
                            polarization="hz", hz_bloch_phase=PHI, source_weights="ramp",
                            dispersion=(cfg["wp2"], GAMMA, OMEGA0), conductivity=cfg["sigma"], probes=cfg["probes"])
    ref = HzBlochOracle(B, cfg["R"], cfg["C"], DT, DX, dtype=np.float64)
    c00 = [(1 / np.sqrt(float(e) * MU0) * DT) / DX for e in eps[:, 0, 0]]
    ref.set_materials(eps, MU0).set_pml(4, courant00=np.array(c00)).set_sources(cfg["rects"])
    ref.set_conductivity(cfg["sigma"]).set_dispersion(cfg["wp2"], GAMMA, OMEGA0)
    ref.set_hz_bloch_phase(PHI).set_hz_bloch_source("ramp").set_probes(cfg["probes"], 30)
    ref.run(30, np.tile([fd.ricker_amplitude(i * DT, 35e9) for i in range(30)], (B, 1)))
    assert len(out) == 4
    for a, w in zip(out, ref.download() + (ref.read_probes(),)):
        assert np.iscomplexobj(a) and np.array_equal(a, w)
    assert np.any(ref.Jx_i) and np.any(ref.Jy_i)


# ---- 5. the fused build -----------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_hz_bloch as t
out = {"arithmetic": fd.ARITHMETIC, "paths": True, "differs": []}
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    hz = []
    for case in t.FUSED_CASES:
        cfg = t._cfg(case, dtype, n=t.NSTEPS_FUSED, state=False)
        got = t._device_run(fd, cfg)
        streamed = t._device_run(fd, cfg, resident=0)      # resident against streamed, in this build
        assert got["path"] is True and streamed["path"] is False
        if not t._same(got, streamed):
            out["paths"] = False
            out["differs"].append(f"{name} {case}")
        hz.append(got["fields"][0].reshape(t.B, -1))
    np.save(f"{OUT}/hz_{name}.npy", np.concatenate(hz, axis=1))
print("HZ_BLOCH_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's complex Hz after 300 steps against the exact build's, both on the device, each in a process of
    its own; in both builds the resident and the streamed path agree bit for bit."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("HZ_BLOCH_RESULT ")][-1][16:])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"hz_{k}.npy").astype(np.complex128) for k in FUSED_BOUND}
    worst = {}
    n1 = CASES[FUSED_CASES[0]][0] * CASES[FUSED_CASES[0]][1]      # the two cases' cells lie side by side in a row
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m, s] - e[m, s]).max() / np.abs(e[m, s]).max()
                       for m in range(B) for s in (slice(0, n1), slice(n1, None)))
        print(f"fused vs exact, Hz {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
