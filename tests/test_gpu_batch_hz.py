"""GPU: the Hz polarisation of PML and periodic batches (fdtd2d_batch_hz.h, kernels_batch_hz.hpp).

Hz, Ex, Ey, Hzx, Jx, Qx, Jy, Qy and the probe traces equal the stand-in of tests/oracle_batch_hz.py bit for bit (exact
build), window DFTs to 1e-12: both dtypes, resident with and without the pole, 7 steps per launch (a run cut in three),
streamed, and resident continued streamed, on the smallest shapes at which the cell walk carries (PML 23x19 and 29x21: 128
and 192 threads, no multiple of C) and the seam is exercised (periodic 23x11 with a 4-cell layer, 29x13 with PEC rows).
Five members with distinct eps, sigma, wp2, gamma and omega0: a Drude one, a lossless one and one with wp2 = 0; a random
wp2 and sigma over every cell that may carry them (rows g and R-2-g, columns 0 and C-2 of the period and the never-read
C-1 included), a source in columns 0 and C-2 next to the seam, a window, three probes, a driven point source in column 0
and a random uploaded state that includes the pole's.  Every case asserts the path it took and its launch count.

The pole-free run equals the Ez kernels' run with eps and mu exchanged and E negated, device against device.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_MEASURED."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_hz import HzPeriodicOracle, HzPmlOracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, LDS_LIMIT = 5e-14, 1e-4, 163840
E_ARG, E_STATE = -1, -4
B, NSTEPS = 5, 21
GAMMA = np.array([1e11, 0.0, 5e10, 8e10, 2e10])
OMEGA0 = 2 * np.pi * np.array([0.0, 50e9, 60e9, 40e9, 0.0])      # member 0 Drude, 1 lossless, 4 has wp2 = 0
WP2_TOP = (2 * np.pi * 70e9) ** 2
# (boundary, rows, cols, layer): layer 0 = PEC rows (periodic alone)
CASES = {"pml23x19": ("pml", 23, 19, 4), "pml29x21": ("pml", 29, 21, 4), "per23x11": ("periodic", 23, 11, 4),
         "per29x13pec": ("periodic", 29, 13, 0)}
# The fused build evaluates jx = fma(a, Jx, fma(cj, Ex, -(ck Qx))), Ex = fma(dxi - jx, cb, ca Ex), the layer's and Hz's
# updates as the fma that fdtd2d_batch_hz.h writes out, so its results differ from the exact build's by rounding.
# Measured on an MI355X (the child processes of test_fused_build_within_its_bounds): Hz after 300 steps of the members of
# pml29x21 and per23x11 from rest, worst member's max|fused - exact| / max|exact|.  The bound is ten times the measured
# value, as tests/test_gpu_batch_dispersive.py derives its own.
NSTEPS_FUSED = 300
FUSED_CASES = ("pml29x21", "per23x11")
FUSED_MEASURED = {"f32": 9.8e-7, "f64": 2.5e-15}
FUSED_BOUND = {k: 10 * v for k, v in FUSED_MEASURED.items()}


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
    """The five members of a case: materials, conductivity, strengths, sources, monitors and (state) a random state."""
    from fdtd2d_amd.api import EPS0, MU0, ricker_amplitude
    boundary, R, C, layer = CASES[case]
    periodic = boundary == "periodic"
    rng = np.random.default_rng(seed)
    g = max(6, layer)
    rows = slice(g, R - 1 - g)                                     # rows g .. R-2-g
    cols = slice(0, C) if periodic else slice(g, C - 1 - g)        # the period and its image, or columns g .. C-2-g
    shape = (B, R - 1 - 2 * g, C if periodic else C - 1 - 2 * g)
    wp2, sigma = np.zeros((B, R, C)), np.zeros((B, R, C))
    wp2[:, rows, cols] = WP2_TOP * (0.05 + rng.random(shape))      # every allowed cell: the metal touches each edge
    wp2[4] = 0.0
    sigma[:, rows, cols] = np.where(rng.random(shape) < 0.3, 0.0, 5.0 * rng.random(shape))
    cfg = dict(case=case, boundary=boundary, R=R, C=C, layer=layer, dtype=dtype, n=n, wp2=wp2, sigma=sigma,
               eps=(EPS0 * (1 + 3 * rng.random((B, R, C)))).astype(dtype),
               mu=(MU0 * (1 + 0.5 * rng.random((B, R, C)))).astype(dtype),
               rects=np.array([[R // 2 + m % 2, (0, 2, C - 4, 1, 3)[m], 1, (C - 1, 3, 3, 1, 4)[m]] for m in range(B)]),
               amps=np.stack([[ricker_amplitude(k * DT, 40e9 * (1 + 0.1 * m)) for k in range(n)] for m in range(B)]),
               omegas=2 * np.pi * np.array([45e9, 65e9]),
               window=(5, C - 5, 8, 5) if periodic else (4, 3, 9, 8),
               probes=np.array([[8, 0], [10, C - 1], [R - 3, 4]] if periodic else [[9, 7], [2, 3], [12, C - 2]]),
               points=np.array([[8, 0]] if periodic else [[9, 7]]),
               weights=rng.standard_normal((B, 1, 2)), gamma=GAMMA, omega0=OMEGA0)
    t = np.arange(n) * DT
    cfg["chan"] = np.stack([np.sin(2 * np.pi * 30e9 * (1 + c) * t + c) for c in range(2)])
    if state:                                                      # Hz, Ex, Ey, Hzx, Jx, Qx, Jy, Qy
        cfg["state"] = [rng.standard_normal(s) for s in ((B, R, C), (B, R, C - 1), (B, R - 1, C)) + ((B, R, C),) * 5]
    return cfg


def _engine(fd, count, cfg, polarization="hz"):
    b = fd.BatchEngine(count, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"])
    return b.set_polarization(polarization)


def _drive(b, cfg, pole=True, sigma=True):
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
    b.set_point_sources(cfg["points"], cfg["weights"])
    if "state" in cfg:
        s = cfg["state"]
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
        cfg = _cfg(case, dtype, **kw)
        _refs[key] = _oracle_run(cfg, pole)
    return _refs[key]


def _oracle_run(cfg, pole=True):
    cls = HzPeriodicOracle if cfg["boundary"] == "periodic" else HzPmlOracle
    ref = _drive(cls(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"]), cfg, pole)
    ref.run(cfg["n"], cfg["amps"], cfg["chan"])
    return _results(ref, pole)


def _expect_path(b, cfg, never=False, pole=True):
    """The capacity rule, restated: twelve arrays with the pole, seven without, and the 4R + 4C factors, the phasor
    table, the point-source sums (one more for the image of a point in column 0) and the accumulators when they fit."""
    esz, R, C = b.dtype.itemsize, b.rows, b.cols
    arrays = 12 if pole else 7
    seg = _seg(R * C, esz)
    fields = arrays * seg + _seg(4 * R, esz) + _seg(4 * C, esz)
    nf, ntab = len(cfg["omegas"]), 1 + int(cfg["boundary"] == "periodic")
    table, acc = 16 * nf + 8 * ntab, 16 * nf * cfg["window"][2] * cfg["window"][3]
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = fields + table + acc <= LDS_LIMIT
    assert b.polarization == "hz" and b.dispersive == pole
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - (fields - arrays * seg) - table) // arrays // 16 * 16 // esz
    assert b.resident == resident
    return resident


def _device_run(fd, cfg, splits=None, resident=None, spl=None, pole=True, sigma=True, count=1, then_streamed=False):
    """count > 1: the five members repeated count times.  then_streamed: the second of two runs is streamed."""
    c = cfg
    if count > 1:
        c = dict(cfg)
        for k in ("eps", "mu", "wp2", "sigma", "rects", "amps", "weights", "gamma", "omega0"):
            c[k] = np.concatenate([cfg[k]] * count)
        c["state"] = [np.concatenate([a] * count) for a in cfg["state"]]
    with _engine(fd, B * count, c) as b:
        _drive(b, c, pole, sigma)
        b.set_option(resident=resident, steps_per_launch=spl)
        path = _expect_path(b, c, never=resident == 0, pole=pole)
        done, want = 0, 0
        for k in splits or (c["n"],):
            if then_streamed and done:
                b.set_option(resident=0)
                path = False
            launches = b.launches
            b.run(k, c["amps"][:, done:done + k], c["chan"][..., done:done + k])
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
    for name, a, w in zip(("Hz", "Ex", "Ey", "Hzx", "Jx", "Qx", "Jy", "Qy"), got["fields"], want["fields"]):
        assert a.dtype == w.dtype and np.array_equal(a, w), name
    assert len(got["fields"]) == len(want["fields"])
    assert np.array_equal(got["probes"], want["probes"])
    assert np.abs(got["dft"] - want["dft"]).max() <= 1e-12 * np.abs(want["dft"]).max()


# ---- 1. against the stand-in, whatever the path ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_hz_runs_match_the_stand_in_on_every_path(fd, case, dtype):
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    want = _stand_in(case, dtype)
    assert all(np.any(a) for a in want["fields"][4:8])
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
def test_hz_runs_without_a_pole_match_the_stand_in(fd, case, dtype):
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    want = _stand_in(case, dtype, pole=False)
    for kw in (dict(), dict(spl=7), dict(resident=0)):
        got = _device_run(fd, cfg, pole=False, **kw)
        assert got["path"] == (kw.get("resident") != 0)
        _matches(got, want)


def test_the_pole_state_round_trips_and_reset_zeroes_it(fd):
    cfg = _cfg("per23x11", np.float32)
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg)
        for got, sent in zip(b.download_dispersion(), cfg["state"][4:8]):
            assert np.array_equal(got, sent.astype(np.float32))          # the image column as given: the state has none
        b.upload_dispersion(None, (None, 2 * cfg["state"][7]))           # Qy alone: the others stay
        again = b.download_dispersion()
        assert np.array_equal(again[3], (2 * cfg["state"][7]).astype(np.float32))
        assert all(np.array_equal(again[k], cfg["state"][4 + k].astype(np.float32)) for k in range(3))
        b.reset()
        assert not any(np.any(a) for a in b.download_dispersion())


# ---- 2. duality, device against device --------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ["pml23x19", "per23x11", "per29x13pec"])
def test_the_pole_free_hz_run_is_the_ez_run_with_exchanged_materials(fd, case, dtype, where):
    """Hz = Ez, Ex = -Hx, Ey = -Hy, Hzx = Ezx, bit for bit, against the Ez kernels (periodic: k_batch_resident_periodic
    and the streamed pair; PML: the point-source kernels), without the stand-in."""
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    never = 0 if where == "streamed" else None
    hz = _device_run(fd, cfg, resident=never, pole=False, sigma=False)
    dual = dict(cfg, eps=cfg["mu"], mu=cfg["eps"])
    dual["state"] = [cfg["state"][0], -cfg["state"][1], -cfg["state"][2], cfg["state"][3]]
    with _engine(fd, B, dual, "ez") as b:
        _drive(b, dual, pole=False, sigma=False)
        b.set_option(resident=never)
        assert b.polarization == "ez" and b.resident == (where == "resident")
        b.run(cfg["n"], cfg["amps"], cfg["chan"])
        ez = _results(b, pole=False)
    for name, a, w, sign in zip(("Hz", "Ex", "Ey", "Hzx"), hz["fields"], ez["fields"], (1, -1, -1, 1)):
        assert np.array_equal(a, sign * w), name
    assert np.array_equal(hz["dft"], ez["dft"]) and np.array_equal(hz["probes"], ez["probes"])


@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("case", ["pml29x21", "per23x11"])
def test_zero_strength_is_bit_identical_to_no_pole(fd, case, where):
    never = 0 if where == "streamed" else None
    for dtype in (np.float32, np.float64):
        cfg = _cfg(case, dtype)
        cfg["wp2"] = np.zeros_like(cfg["wp2"])
        cfg["sigma"] = np.zeros_like(cfg["sigma"])
        for a in cfg["state"][4:8]:
            a[...] = 0
        with_pole = _device_run(fd, cfg, resident=never)
        without = _device_run(fd, cfg, resident=never, pole=False, sigma=False)
        assert not any(np.any(a) for a in with_pole["fields"][4:8])
        with_pole["fields"] = with_pole["fields"][:4]
        assert _same(with_pole, without)


# ---- 3. capacity ------------------------------------------------------------------------------------------------------------

def _plain_cfg(R, C, layer, dtype, n, seed=3):
    """One shape of any size: the members of _cfg without the state, from rest."""
    CASES["tmp"] = ("pml", R, C, layer)
    try:
        return _cfg("tmp", dtype, n=n, seed=seed, state=False)
    finally:
        del CASES["tmp"]


@pytest.mark.parametrize("pole", [True, False], ids=["12arrays", "7arrays"])
@pytest.mark.parametrize("dtype,C", [(np.float32, 60), (np.float64, 45)], ids=["f32", "f64"])
def test_the_largest_member_the_rule_admits_is_resident_and_one_row_more_is_not(fd, dtype, C, pole):
    _exact_only(fd)
    esz, arrays = np.dtype(dtype).itemsize, 12 if pole else 7

    def fits(R):
        return arrays * _seg(R * C, esz) + _seg(4 * R, esz) + _seg(4 * C, esz) + 16 * 2 + 8 <= LDS_LIMIT
    R = max(r for r in range(20, 200) if fits(r))
    assert fits(R) and not fits(R + 1)
    if not pole and esz == 4:
        assert R * C > 4096                                        # the 8-cells-per-thread instance
    for rows, resident in ((R, True), (R + 1, False)):
        cfg = _plain_cfg(rows, C, 6, dtype, 3)
        got = _device_run(fd, cfg, pole=pole)
        assert got["path"] is resident
        _matches(got, _oracle_run(cfg, pole))


def test_300_members_take_more_than_one_round_of_workgroups(fd):
    _exact_only(fd)
    cfg = _cfg("per23x11", np.float32)
    want = _stand_in("per23x11", np.float32)
    got = _device_run(fd, cfg, count=60)
    assert got["path"] is True
    for a, w in zip(got["fields"] + (got["dft"], got["probes"]), want["fields"] + (want["dft"], want["probes"])):
        assert a.shape[0] == 300
        for k in range(60):
            if a.dtype.kind == "c":
                assert np.abs(a[5 * k:5 * k + 5] - w).max() <= 1e-12 * np.abs(w).max()
            else:
                assert np.array_equal(a[5 * k:5 * k + 5], w), k


@pytest.mark.parametrize("case", ["pml23x19", "per23x11"])
def test_removing_the_pole_returns_the_batch_to_the_seven_array_kernels(fd, case):
    cfg = _cfg(case, np.float32)
    want = _device_run(fd, cfg, pole=False)
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg)
        assert b.dispersive and b.polarization == "hz"
        b.run(3, cfg["amps"], cfg["chan"])
        b.set_dispersion(None)
        assert not b.dispersive
        _expect_path(b, cfg, pole=False)
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.download_dispersion()
        assert ei.value.code == E_STATE
        b.reset()
        b.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
        s = cfg["state"]
        b.upload(s[0], s[1], s[2]).upload_ezx(s[3])
        b.run(cfg["n"], cfg["amps"], cfg["chan"])
        assert _same(_results(b, pole=False), want)
        b.set_dispersion(None)                                    # twice is nothing


# ---- 4. run_fdtd_batch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["pml", "periodic"])
def test_run_fdtd_batch_takes_the_polarization(fd, boundary):
    _exact_only(fd)
    from fdtd2d_amd.api import MU0
    case = "pml23x19" if boundary == "pml" else "per23x11"
    cfg = _cfg(case, np.float64, n=30, state=False)
    eps = cfg["eps"].astype(np.float64)
    out = fd.run_fdtd_batch(eps, nsteps=30, sources=cfg["rects"], fc=35e9, dtype=np.float64, boundary=boundary, pml_cells=4,
                            polarization="hz", dispersion=(cfg["wp2"], GAMMA, OMEGA0), conductivity=cfg["sigma"],
                            probes=cfg["probes"])
    ref = (HzPmlOracle if boundary == "pml" else HzPeriodicOracle)(B, cfg["R"], cfg["C"], DT, DX, dtype=np.float64,
                                                                   boundary=boundary)
    c00 = [(1 / np.sqrt(float(e) * MU0) * DT) / DX for e in eps[:, 0, 0]]
    ref.set_materials(eps, MU0).set_pml(4, courant00=np.array(c00)).set_sources(cfg["rects"])
    ref.set_conductivity(cfg["sigma"]).set_dispersion(cfg["wp2"], GAMMA, OMEGA0).set_probes(cfg["probes"], 30)
    ref.run(30, np.tile([fd.ricker_amplitude(i * DT, 35e9) for i in range(30)], (B, 1)))
    assert len(out) == 4
    for a, w in zip(out, ref.download() + (ref.read_probes(),)):
        assert np.array_equal(a, w)
    assert np.any(ref.Jx) and np.any(ref.Jy)


# ---- 5. the surface on the device -------------------------------------------------------------------------------------------

def _raises(fd, code, match, call):
    with pytest.raises(fd.Fdtd2dError, match=match) as ei:
        call()
    assert ei.value.code == code


def test_batches_that_cannot_change_polarization_refuse_it(fd):
    from fdtd2d_amd.api import EPS0
    for boundary in ("mur", "none", "lattice"):
        with fd.BatchEngine(2, 23, 19, DT, DX, boundary=boundary) as b:
            _raises(fd, E_STATE, "Hz polarisation", lambda: b.set_polarization("hz"))
            assert b.polarization == "ez"
    with fd.BatchEngine(2, 23, 19, DT, DX, boundary="mur") as b:              # the library's own refusal
        assert b._lib.fdtd2d_batch_set_polarization(b._h, 1) == E_STATE
        assert b._lib.fdtd2d_batch_set_polarization(b._h, 2) == E_ARG
        assert b._lib.fdtd2d_batch_polarization(b._h) == 0
    ok = np.zeros((2, 23, 19))
    ok[:, 8:14, 8:11] = 1.0
    with fd.BatchEngine(2, 23, 19, DT, DX, boundary="periodic") as b:
        b.set_materials(EPS0).set_bloch_phase(0.3)
        _raises(fd, E_STATE, "Bloch phase", lambda: b.set_polarization("hz"))
        assert b._lib.fdtd2d_batch_set_polarization(b._h, 1) == E_STATE and b.bloch
        b.set_bloch_phase(None)
        for setup, match, undo in ((lambda: b.set_conductivity(ok), "conductivity of the other", lambda: b.set_conductivity(None)),
                                   (lambda: b.set_dispersion(ok * WP2_TOP, 1e11, 0.0), "pole of the other",
                                    lambda: b.set_dispersion(None)),
                                   (lambda: b.set_flux_lines([("row", 10, 0, 18)], [3e11]), "flux lines",
                                    lambda: b.set_flux_lines(None, None)),
                                   (lambda: b.set_dft_window((8, 2, 3, 3), [3e11]).hold_dft_window(), "held window",
                                    lambda: b.set_dft_window((8, 2, 3, 3), [3e11]))):
            setup()
            _raises(fd, E_STATE, match, lambda: b.set_polarization("hz"))
            assert b.polarization == "ez" and b._lib.fdtd2d_batch_polarization(b._h) == 0
            undo()
        b.set_polarization("hz")
        assert b.polarization == "hz" and not b.lossy and not b.dispersive
        b.set_conductivity(ok)
        _raises(fd, E_STATE, "conductivity of the other", lambda: b.set_polarization("ez"))
        b.set_conductivity(None).set_dispersion(ok * WP2_TOP, 1e11, 0.0)
        _raises(fd, E_STATE, "pole of the other", lambda: b.set_polarization("ez"))
        b.set_dispersion(None).set_polarization("ez")
        assert b.polarization == "ez" and not b.lossy
    with fd.BatchEngine(2, 23, 19, DT, DX, boundary="pml") as b:   # a "pml" batch before set_pml: a plain box
        b.set_polarization("hz").set_materials(EPS0)
        _raises(fd, E_STATE, "plain box", lambda: b.set_dispersion(ok * WP2_TOP, 1e11, 0.0))
        b._pml_chosen = True
        _raises(fd, E_STATE, "plain box", lambda: b.run(1))


@pytest.mark.parametrize("case", ["pml23x19", "per23x11"])
def test_refusals_leave_an_hz_batch_as_it_was(fd, case):
    _exact_only(fd)
    cfg = _cfg(case, np.float32)
    R, C, periodic = cfg["R"], cfg["C"], cfg["boundary"] == "periodic"
    g = 6
    want = _stand_in(case, np.float32)

    def with_(a, value, at):
        w = a.copy()
        w[at] = value
        return w
    with _engine(fd, B, cfg) as b:
        _drive(b, cfg)
        lds = b.lds_bytes
        assert b.conductivity_margin == g
        # the allowed set is exact: row R-2-g is accepted (cfg has it non-zero), row R-1-g and column C-1-g are not
        assert np.all(cfg["wp2"][:4, R - 2 - g, 0 if periodic else g:C - 1 - g] > 0)
        for name, arr, setter in (("wp2", cfg["wp2"], lambda w: b.set_dispersion(w, GAMMA, OMEGA0)),
                                  ("sigma", cfg["sigma"], b.set_conductivity)):
            top = WP2_TOP if name == "wp2" else 1.0
            _raises(fd, E_ARG, rf"member 1: {name} is non-zero at cell \({R - 1 - g},8\)",
                    lambda: setter(with_(arr, top, (1, R - 1 - g, 8))))
            _raises(fd, E_ARG, rf"member 2: {name} is non-zero at cell \({g - 1},8\)",
                    lambda: setter(with_(arr, top, (2, g - 1, 8))))
            _raises(fd, E_ARG, f"member 3: {name} must be >= 0 and finite", lambda: setter(with_(arr, -1.0, (3, 10, 8))))
            if periodic:
                setter(with_(arr, top, (0, 10, C - 1)))            # the never-read image column is accepted
                setter(arr)
            else:
                _raises(fd, E_ARG, rf"member 0: {name} is non-zero at cell \(10,{C - 1 - g}\)",
                        lambda: setter(with_(arr, top, (0, 10, C - 1 - g))))
                _raises(fd, E_ARG, rf"member 0: {name} is non-zero at cell \(10,{g - 1}\)",
                        lambda: setter(with_(arr, top, (0, 10, g - 1))))
        _raises(fd, E_ARG, r"member 3: the pole at cell \(10,8\) is unstable",
                lambda: b.set_dispersion(with_(cfg["wp2"], 4.1 / DT ** 2 * 4, (3, 10, 8)), GAMMA, OMEGA0))
        # what the Hz polarisation does not have, in Python and in the library
        for call in (b.hold_dft_window, lambda: b.dft_window_product(np.ones(2)), b.hold_dispersive_window,
                     lambda: b.dispersive_window_product(np.ones((1, 2))),
                     lambda: b.set_flux_lines([("row", 10, 0, C - 1)], [3e11]),
                     lambda: b.set_conductivity_window((10, 8, 1, 1), np.zeros((B, 1, 1))),
                     lambda: b.set_dispersion_window((10, 8, 1, 1), np.zeros((B, 1, 1))),
                     lambda: b.set_bloch_phase(0.5), lambda: b.set_bloch_flux_lines([("row", 10, 0, C - 1)], [3e11]),
                     lambda: b.set_bloch_point_sources(np.array([[8, 1]]), np.ones((1, 1)))):
            _raises(fd, E_STATE, "Hz polarisation", call)
        L = b._lib
        one = np.ones(B * R * C)
        dp = one.ctypes.data_as(L.fdtd2d_batch_set_bloch.argtypes[1])
        win = (np.array([10, 8, 1, 1], np.int32)).ctypes.data_as(L.fdtd2d_batch_set_dispersion_window.argtypes[1])
        line = np.array([0, 10, 0, C - 1], np.int32).ctypes.data_as(L.fdtd2d_batch_set_flux_lines.argtypes[2])
        for rc in (L.fdtd2d_batch_hold_dft_window(b._h), L.fdtd2d_batch_dft_window_product(b._h, dp, dp, dp),
                   L.fdtd2d_batch_hold_dispersive_window(b._h),
                   L.fdtd2d_batch_dispersive_window_product(b._h, 1, dp, dp, dp, dp),
                   L.fdtd2d_batch_set_conductivity(b._h, one.ctypes.data, 1),
                   L.fdtd2d_batch_set_conductivity_window(b._h, win, one.ctypes.data, 1),
                   L.fdtd2d_batch_set_dispersion(b._h, one.ctypes.data, 1, dp, dp),
                   L.fdtd2d_batch_set_dispersion_window(b._h, win, one.ctypes.data, 1),
                   L.fdtd2d_batch_transfer_dispersion(b._h, one.ctypes.data, None, 1, 0),
                   L.fdtd2d_batch_set_bloch(b._h, dp, dp), L.fdtd2d_batch_set_lattice(b._h, dp, dp, dp, dp),
                   L.fdtd2d_batch_set_flux_lines(b._h, 1, line, 1, dp, 1),
                   L.fdtd2d_batch_set_bloch_flux_lines(b._h, 1, line, 1, dp, 1),
                   L.fdtd2d_batch_set_flux_line_sources(b._h, 2, dp, dp)):
            assert rc == E_STATE
        if not periodic:
            _raises(fd, E_STATE, "dispersive pole", b.clear_pml)
            assert b.pml
        assert b.dispersive and b.polarization == "hz" and b.lds_bytes == lds and not b.bloch
        b.run(cfg["n"], cfg["amps"], cfg["chan"])
        _matches(_results(b), want)


def test_the_adjoint_helpers_refuse_an_hz_engine_on_the_device(fd):
    import test_batch_adjoint_cpu as cpu
    eps = cpu.design_eps(count=2)
    args = dict(nsteps=50, sources=np.tile(cpu.SOURCE, (2, 1)), probes=cpu.PROBES, omegas=cpu.OMEGAS, design=cpu.DESIGN,
                fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, dtype=np.float64, boundary="pml", pml_cells=cpu.LAYER)
    with fd.AdjointSession(eps, **args) as s:
        s.engine.set_polarization("hz")
        _raises(fd, E_STATE, "Hz polarisation", lambda: s.value_and_grad(cpu.objective))
        s.engine.set_polarization("ez")
        s.value_and_grad(cpu.objective)


# ---- 6. the fused build -----------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_hz as t
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
print("HZ_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's Hz after 300 steps against the exact build's, both on the device, each in a process of its own;
    in both builds the resident and the streamed path agree bit for bit."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("HZ_RESULT ")][-1][10:])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"hz_{k}.npy").astype(np.float64) for k in FUSED_BOUND}
    worst = {}
    n1 = CASES[FUSED_CASES[0]][1] * CASES[FUSED_CASES[0]][2]      # the two cases' cells lie side by side in a row
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m, s] - e[m, s]).max() / np.abs(e[m, s]).max()
                       for m in range(B) for s in (slice(0, n1), slice(n1, None)))
        print(f"fused vs exact, Hz {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
