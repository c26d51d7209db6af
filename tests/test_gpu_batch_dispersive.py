"""GPU: dispersive (Drude-Lorentz) materials in the batched engine (fdtd2d_batch_dispersive.h,
kernels_batch_dispersive.hpp).

Ez, Hx, Hy, Ezx, Jh, Q and the probe traces equal the stand-in of tests/oracle_batch_dispersive.py bit for bit (exact
build), window DFTs to 1e-12: both dtypes, resident, 7 steps per launch and streamed, on the smallest shapes at which the
cell walk carries (PML 23x19 and 29x21: 128 and 192 threads, no multiple of C) and the seam is exercised (periodic 23x11
and 29x13, with a 4-cell layer and with PEC rows).  Five members with distinct (gamma, omega0): a Drude one, a lossless
one and one with wp2 = 0; a random wp2 over everything outside the margin (columns 0, C-2 and the never-read C-1 of the
periodic members included), a conductivity, a window, three probes, a driven point source and a random uploaded state
that includes Jh and Q.  Results are bit-identical whatever the path, the launch split and the accumulators' placement.
Every case asserts the path it took and its launch count.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_MEASURED."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_dispersive import DispersivePeriodicOracle, DispersivePmlOracle

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
         "per23x11pec": ("periodic", 23, 11, 0), "per29x13": ("periodic", 29, 13, 4),
         "per29x13pec": ("periodic", 29, 13, 0)}
# The fused build evaluates jn = fma(a, Jh, fma(cj, e, -(ck Q))) and e = fma((dhy - dhx) - jn, cb, ca e), so its results
# differ from the exact build's by rounding.  Measured on an MI355X (the child processes of
# test_fused_build_within_its_bounds): Ez after 300 steps of the members of pml29x21 and per29x13 from rest, worst
# member's max|fused - exact| / max|exact|.  The bound is ten times the measured value.
NSTEPS_FUSED = 300
FUSED_MEASURED = {"f32": 2.9e-6, "f64": 3.1e-15}
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


def _cfg(case, dtype, n=NSTEPS, seed=7, state=True):
    """The five members of a case: materials, conductivity, strengths, sources, monitors and (state) a random state."""
    from fdtd2d_amd.api import EPS0, MU0, ricker_amplitude
    boundary, R, C, layer = CASES[case]
    periodic = boundary == "periodic"
    rng = np.random.default_rng(seed)
    g = max(6, layer)
    rows = slice(g, R - g)
    cols = slice(0, C) if periodic else slice(g, C - g)
    shape = (B, R - 2 * g, C if periodic else C - 2 * g)
    wp2, sigma = np.zeros((B, R, C)), np.zeros((B, R, C))
    wp2[:, rows, cols] = WP2_TOP * rng.random(shape)
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
    if state:
        cfg["state"] = [rng.standard_normal(s) for s in ((B, R, C), (B, R, C - 1), (B, R - 1, C), (B, R, C), (B, R, C),
                                                         (B, R, C))]      # Ez, Hx, Hy, Ezx, Jh, Q
    return cfg


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
            b.upload_dispersion(s[4], s[5])
    return b


def _results(b, pole=True):
    out = dict(fields=tuple(b.download()) + (b.download_ezx(),) + (tuple(b.download_dispersion()) if pole else ()),
               dft=b.read_dft_window(), probes=b.read_probes())
    return out


_refs = {}


def _stand_in(case, dtype, **kw):
    """The stand-in's results of a case, computed once."""
    key = (case, np.dtype(dtype).name) + tuple(sorted(kw.items()))
    if key not in _refs:
        cfg = _cfg(case, dtype, **kw)
        cls = DispersivePeriodicOracle if cfg["boundary"] == "periodic" else DispersivePmlOracle
        ref = _drive(cls(B, cfg["R"], cfg["C"], DT, DX, dtype=dtype, boundary=cfg["boundary"]), cfg)
        ref.run(cfg["n"], cfg["amps"], cfg["chan"])
        _refs[key] = _results(ref)
    return _refs[key]


def _expect_path(b, cfg, never=False, lds_allowed=True, pole=True, sigma=True):
    """The capacity rule, restated: ten arrays (without the pole seven, six for a lossless PML batch) and the 4R + 4C
    factors, the phasor table, the point-source sums (one more for the image of a point in column 0) and the
    accumulators when they fit."""
    esz, R, C = b.dtype.itemsize, b.rows, b.cols
    arrays = 10 if pole else 7 if sigma or cfg["boundary"] == "periodic" else 6
    seg = _seg(R * C, esz)
    fields = arrays * seg + _seg(4 * R, esz) + _seg(4 * C, esz)
    nf, ntab = len(cfg["omegas"]), 1 + int(cfg["boundary"] == "periodic")
    table, acc = 16 * nf + 8 * ntab, 16 * nf * cfg["window"][2] * cfg["window"][3]
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = lds_allowed and fields + table + acc <= LDS_LIMIT
    assert b.dispersive == pole
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - (fields - arrays * seg) - table) // arrays // 16 * 16 // esz
    assert b.resident == resident
    assert b.window_in_lds == (in_lds and resident)
    return resident


def _device_run(fd, cfg, splits=None, resident=None, spl=None, lds=True, pole=True, sigma=True, count=1):
    """count > 1: the five members repeated count times."""
    c = cfg
    if count > 1:
        c = dict(cfg)
        for k in ("eps", "mu", "wp2", "sigma", "rects", "amps", "weights", "gamma", "omega0"):
            c[k] = np.concatenate([cfg[k]] * count)
        c["state"] = [np.concatenate([a] * count) for a in cfg["state"]]
    with fd.BatchEngine(B * count, c["R"], c["C"], DT, DX, dtype=c["dtype"], boundary=c["boundary"]) as b:
        _drive(b, c, pole, sigma)
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        path = _expect_path(b, c, never=resident == 0, lds_allowed=lds, pole=pole, sigma=sigma)
        done, launches = 0, b.launches
        for k in splits or (c["n"],):
            b.run(k, c["amps"][:, done:done + k], c["chan"][..., done:done + k])
            done += k
        if path:      # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits or (c["n"],))
        else:
            assert b.launches - launches == 2 * done
        out = _results(b, pole)
        out["path"] = path
        return out


def _same(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"])) and np.array_equal(a["dft"], b["dft"])
            and np.array_equal(a["probes"], b["probes"]))


def _matches(got, want, periodic):
    for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx", "Jh", "Q"), got["fields"], want["fields"]):
        assert a.dtype == w.dtype and np.array_equal(a, w), name
    assert np.array_equal(got["probes"], want["probes"])
    assert np.abs(got["dft"] - want["dft"]).max() <= 1e-12 * np.abs(want["dft"]).max()
    if periodic:      # the image slots repeat column 0
        for a in got["fields"][4:6]:
            assert np.array_equal(a[:, :, -1], a[:, :, 0])


# ---- 1. against the stand-in, whatever the path ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_dispersive_runs_match_the_stand_in_on_every_path(fd, case, dtype):
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    want = _stand_in(case, dtype)
    assert np.any(want["fields"][4]) and np.any(want["fields"][5])
    runs = {"resident": _device_run(fd, cfg),
            "split7": _device_run(fd, cfg, spl=7),
            "two_runs": _device_run(fd, cfg, splits=(8, 13)),
            "global_acc": _device_run(fd, cfg, lds=False),
            "streamed": _device_run(fd, cfg, resident=0)}
    for name, got in runs.items():
        assert got["path"] == (name != "streamed"), name
        _matches(got, want, cfg["boundary"] == "periodic")
    for name, got in runs.items():
        assert _same(got, runs["resident"]), name


@pytest.mark.parametrize("case", ["pml23x19", "per23x11"])
def test_an_upload_with_a_wrong_image_takes_column_0(fd, case):
    cfg = _cfg(case, np.float32)
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=np.float32, boundary=cfg["boundary"]) as b:
        _drive(b, cfg)
        jh, q = b.download_dispersion()
        for got, sent in ((jh, cfg["state"][4]), (q, cfg["state"][5])):
            want = sent.astype(np.float32)
            if cfg["boundary"] == "periodic":
                assert not np.array_equal(want[:, :, -1], want[:, :, 0])
                want[:, :, -1] = want[:, :, 0]
            assert np.array_equal(got, want)
        b.upload_dispersion(None, 2 * cfg["state"][5])            # one alone: the other stays
        jh2, q2 = b.download_dispersion()
        assert np.array_equal(jh2, jh) and np.array_equal(q2, 2 * q)
        b.reset()
        assert not any(np.any(a) for a in b.download_dispersion())


# ---- 2. capacity ------------------------------------------------------------------------------------------------------------

def _plain_cfg(R, C, layer, dtype, n, seed=3):
    """One shape of any size: the members of _cfg without the state, from rest."""
    CASES["tmp"] = ("pml", R, C, layer)
    try:
        return _cfg("tmp", dtype, n=n, seed=seed, state=False)
    finally:
        del CASES["tmp"]


def _oracle_run(cfg):
    ref = _drive(DispersivePmlOracle(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"]), cfg)
    ref.run(cfg["n"], cfg["amps"], cfg["chan"])
    return _results(ref)


def test_a_70x70_member_is_resident_before_the_pole_and_streamed_after(fd):
    _exact_only(fd)
    cfg = _plain_cfg(70, 70, 8, np.float32, 5)
    with fd.BatchEngine(B, 70, 70, DT, DX, dtype=np.float32, boundary="pml") as b:
        _drive(b, cfg, pole=False)
        assert _expect_path(b, cfg, pole=False) is True and b.resident_max_cells >= 4900
        b.set_dispersion(cfg["wp2"], GAMMA, OMEGA0)
        assert _expect_path(b, cfg) is False and b.resident_max_cells < 4096
        launches = b.launches
        b.run(5, cfg["amps"], cfg["chan"])
        assert b.launches - launches == 10
        _matches(_results(b), _oracle_run(cfg), False)


@pytest.mark.parametrize("dtype,C", [(np.float32, 60), (np.float64, 45)], ids=["f32", "f64"])
def test_the_largest_member_the_rule_admits_is_resident_and_one_row_more_is_not(fd, dtype, C):
    _exact_only(fd)
    esz = np.dtype(dtype).itemsize

    def fits(R):
        return 10 * _seg(R * C, esz) + _seg(4 * R, esz) + _seg(4 * C, esz) + 16 * 2 + 8 <= LDS_LIMIT
    R = max(r for r in range(20, 200) if fits(r))
    assert fits(R) and not fits(R + 1) and R * C < (4096 if esz == 4 else 2048)
    for rows, resident in ((R, True), (R + 1, False)):
        cfg = _plain_cfg(rows, C, 6, dtype, 3)
        got = _device_run(fd, cfg)
        assert got["path"] is resident
        _matches(got, _oracle_run(cfg), False)


def test_300_members_take_more_than_one_round_of_workgroups(fd):
    _exact_only(fd)
    cfg = _cfg("pml23x19", np.float32)
    want = _stand_in("pml23x19", np.float32)
    got = _device_run(fd, cfg, count=60)
    assert got["path"] is True
    for a, w in zip(got["fields"] + (got["dft"], got["probes"]), want["fields"] + (want["dft"], want["probes"])):
        assert a.shape[0] == 300
        for k in range(60):
            if a.dtype.kind == "c":
                assert np.abs(a[5 * k:5 * k + 5] - w).max() <= 1e-12 * np.abs(w).max()
            else:
                assert np.array_equal(a[5 * k:5 * k + 5], w), k


# ---- 3. the pole that is not there ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("case", ["pml29x21", "per23x11", "per29x13pec"])
def test_zero_strength_is_bit_identical_to_no_pole(fd, case, where):
    never = 0 if where == "streamed" else None
    for dtype in (np.float32, np.float64):
        cfg = _cfg(case, dtype)
        cfg["wp2"] = np.zeros_like(cfg["wp2"])
        cfg["state"][4][...] = 0
        cfg["state"][5][...] = 0
        with_pole = _device_run(fd, cfg, resident=never)
        without = _device_run(fd, cfg, resident=never, pole=False)
        assert not np.any(with_pole["fields"][4]) and not np.any(with_pole["fields"][5])
        with_pole["fields"] = with_pole["fields"][:4]
        assert _same(with_pole, without)


@pytest.mark.parametrize("sigma", [True, False], ids=["lossy", "lossless"])
@pytest.mark.parametrize("case", ["pml23x19", "per23x11"])
def test_removing_the_pole_returns_the_batch_to_its_other_kernels(fd, case, sigma):
    cfg = _cfg(case, np.float32)
    want = _device_run(fd, cfg, pole=False, sigma=sigma)
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=np.float32, boundary=cfg["boundary"]) as b:
        _drive(b, cfg, sigma=sigma)
        assert b.dispersive and b.lossy == sigma
        b.run(3, cfg["amps"], cfg["chan"])
        b.set_dispersion(None)
        assert not b.dispersive and b.lossy == sigma
        _expect_path(b, cfg, pole=False, sigma=sigma)
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


def test_run_fdtd_batch_takes_a_dispersion(fd):
    _exact_only(fd)
    from fdtd2d_amd.api import MU0
    cfg = _plain_cfg(23, 19, 4, np.float64, 30)
    eps = cfg["eps"].astype(np.float64)
    out = fd.run_fdtd_batch(eps, nsteps=30, sources=cfg["rects"], fc=35e9, dtype=np.float64, boundary="pml", pml_cells=4,
                            dispersion=(cfg["wp2"], GAMMA, OMEGA0))
    ref = DispersivePmlOracle(B, 23, 19, DT, DX, dtype=np.float64)
    c00 = [(1 / np.sqrt(float(e) * MU0) * DT) / DX for e in eps[:, 0, 0]]
    ref.set_materials(eps, MU0).set_pml(4, courant00=np.array(c00)).set_sources(cfg["rects"])
    ref.set_dispersion(cfg["wp2"], GAMMA, OMEGA0)
    ref.run(30, np.tile([fd.ricker_amplitude(i * DT, 35e9) for i in range(30)], (B, 1)))
    for a, w in zip(out, ref.download()):
        assert np.array_equal(a, w)
    assert np.any(ref.Jh)


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------

def _raises(fd, code, match, call):
    with pytest.raises(fd.Fdtd2dError, match=match) as ei:
        call()
    assert ei.value.code == code


def test_batches_that_cannot_carry_a_pole_refuse_it(fd):
    from fdtd2d_amd.api import EPS0
    ok = np.zeros((2, 23, 19))
    ok[:, 8:14, 8:11] = WP2_TOP
    for boundary in ("mur", "none", "pml"):                       # "pml" before set_pml: no layer yet
        with fd.BatchEngine(2, 23, 19, DT, DX, boundary=boundary) as b:
            b.set_materials(EPS0)
            _raises(fd, E_STATE, "Mur frame" if boundary == "mur" else "plain box", lambda: b.set_dispersion(ok, 1e11, 0.0))
            assert not b.dispersive and not b.lossy
            _raises(fd, E_STATE, "no pole is set", lambda: b.set_dispersion_window((8, 8, 2, 2), np.ones((2, 2, 2))))
            _raises(fd, E_STATE, "no pole is set", lambda: b.download_dispersion())
    with fd.BatchEngine(2, 23, 19, DT, DX, boundary="periodic") as b:
        b.set_materials(EPS0).set_bloch_phase(0.3)
        _raises(fd, E_STATE, "Bloch phase", lambda: b.set_dispersion(ok, 1e11, 0.0))
        assert not b.dispersive and b.bloch
        b.set_bloch_phase(None)
        b.set_dispersion(ok, 1e11, 0.0)
        _raises(fd, E_STATE, "dispersive pole", lambda: b.set_bloch_phase(0.3))
        assert b.dispersive and not b.bloch
    with fd.BatchEngine(2, 23, 19, DT, DX, boundary="pml") as b:   # no materials
        b.set_pml(4)
        _raises(fd, E_STATE, "materials not set", lambda: b.set_dispersion(ok, 1e11, 0.0))


@pytest.mark.parametrize("case", ["pml23x19", "per23x11"])
def test_refusals_leave_a_dispersive_batch_as_it_was(fd, case):
    _exact_only(fd)
    from fdtd2d_amd.api import EPS0
    cfg = _cfg(case, np.float32)
    R, C, periodic = cfg["R"], cfg["C"], cfg["boundary"] == "periodic"
    want = _stand_in(case, np.float32)

    def wp2_with(value, at):
        w = cfg["wp2"].copy()
        w[at] = value
        return w
    with fd.BatchEngine(B, R, C, DT, DX, dtype=np.float32, boundary=cfg["boundary"]) as b:
        _drive(b, cfg)
        lds = b.lds_bytes
        for value, at, match in ((-1.0, (2, 10, 8), "member 2: wp2 must be >= 0 and finite"),
                                 (np.nan, (1, 10, 8), "member 1: wp2 must be >= 0 and finite"),
                                 (np.inf, (3, 10, 8), "member 3: wp2 must be >= 0 and finite"),
                                 (WP2_TOP, (1, 5, 8), r"member 1: wp2 is non-zero at cell \(5,8\), within 6 cells"),
                                 (WP2_TOP, (2, R - 6, 8), r"member 2: wp2 is non-zero at cell"),
                                 (4.1 / DT ** 2 * 4, (3, 10, 8), r"member 3: the pole at cell \(10,8\) is unstable")):
            _raises(fd, E_ARG, match, lambda: b.set_dispersion(wp2_with(value, at), GAMMA, OMEGA0))
            patch = np.full((B, 1, 1), 0.0)
            patch[at[0]] = value
            _raises(fd, E_ARG, match, lambda: b.set_dispersion_window((at[1], at[2], 1, 1), patch))
        if not periodic:
            _raises(fd, E_ARG, r"member 0: wp2 is non-zero at cell \(10,5\)",
                    lambda: b.set_dispersion(wp2_with(WP2_TOP, (0, 10, 5)), GAMMA, OMEGA0))
        for gam, om0, match in ((-GAMMA - 1, OMEGA0, "member 0: gamma"), (GAMMA * np.nan, OMEGA0, "member 0: gamma"),
                                (GAMMA, np.where(np.arange(B) == 2, np.inf, OMEGA0), "member 2: omega0"),
                                (GAMMA, np.where(np.arange(B) == 3, -1.0, OMEGA0), "member 3: omega0"),
                                (GAMMA, np.where(np.arange(B) == 1, 2.1 / DT, OMEGA0), "member 1: the pole at cell")):
            _raises(fd, E_ARG, match, lambda: b.set_dispersion(cfg["wp2"], gam, om0))
        _raises(fd, E_ARG, "window", lambda: b.set_dispersion_window((R - 1, 0, 2, 2), np.zeros((B, 2, 2))))
        # the materials: a permittivity that breaks the pole's bound (8 dt^2 / (eps mu dx^2) = 4.5 at 0.04 EPS0, whose
        # Courant number 0.75 is allowed) is refused by set_materials and set_eps_window alike
        thin = cfg["eps"].copy()
        thin[1, 10, 8] = 0.04 * EPS0
        _raises(fd, E_ARG, r"member 1: the pole at cell \(10,8\) is unstable", lambda: b.set_materials(thin, cfg["mu"]))
        _raises(fd, E_ARG, r"member 1: the pole at cell \(10,8\) is unstable",
                lambda: b.set_eps_window((10, 8, 1, 1), thin[:, 10:11, 8:9]))
        # the adjoint tools, a Bloch phase and a plain box
        _raises(fd, E_STATE, "dispersive pole", b.hold_dft_window)
        _raises(fd, E_STATE, "dispersive pole", lambda: b.dft_window_product(np.ones(2)))
        rc = b._lib.fdtd2d_batch_hold_dft_window(b._h)
        assert rc == E_STATE
        if periodic:
            _raises(fd, E_STATE, "dispersive pole", lambda: b.set_bloch_phase(0.5))
        else:
            _raises(fd, E_STATE, "dispersive pole", b.clear_pml)
            assert b.pml
        assert b.dispersive and b.lds_bytes == lds and b.info(13) == 0      # FDTD2D_BATCH_INFO_HELD_WINDOW
        courant = b.courant()
        b.run(cfg["n"], cfg["amps"], cfg["chan"])
        assert np.array_equal(courant, b.courant())
        _matches(_results(b), want, periodic)


def test_the_adjoint_helpers_refuse_a_dispersive_engine_on_the_device(fd):
    import test_batch_adjoint_cpu as cpu
    eps = cpu.design_eps(count=2)
    args = dict(nsteps=50, sources=np.tile(cpu.SOURCE, (2, 1)), probes=cpu.PROBES, omegas=cpu.OMEGAS, design=cpu.DESIGN,
                fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, dtype=np.float64, boundary="pml", pml_cells=cpu.LAYER)
    with fd.AdjointSession(eps, **args) as s:
        s.engine.set_dispersion(WP2_TOP, 1e11, 0.0)
        _raises(fd, E_STATE, "dispersive pole", lambda: s.value_and_grad(cpu.objective))
        s.engine.set_dispersion(None)
        s.value_and_grad(cpu.objective)


# ---- 5. the fused build -----------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_dispersive as t
out = {"arithmetic": fd.ARITHMETIC, "paths": True, "differs": []}
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    ez = []
    for case in ("pml29x21", "per29x13"):
        cfg = t._cfg(case, dtype, n=t.NSTEPS_FUSED, state=False)
        got = t._device_run(fd, cfg)
        streamed = t._device_run(fd, cfg, resident=0)      # resident against streamed, in this build
        assert got["path"] is True and streamed["path"] is False
        if not t._same(got, streamed):
            out["paths"] = False
            out["differs"].append(f"{name} {case}")
        ez.append(got["fields"][0].reshape(t.B, -1))
    np.save(f"{OUT}/ez_{name}.npy", np.concatenate(ez, axis=1))
print("DISPERSIVE_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's Ez after 300 steps against the exact build's, both on the device, each in a process of its own;
    in both builds the resident and the streamed path agree bit for bit."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("DISPERSIVE_RESULT ")][-1][18:])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"ez_{k}.npy").astype(np.float64) for k in FUSED_BOUND}
    worst = {}
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        # per member and case: the two cases' cells lie side by side in a row
        n1 = 29 * 21
        worst[k] = max(np.abs(f[m, s] - e[m, s]).max() / np.abs(e[m, s]).max()
                       for m in range(B) for s in (slice(0, n1), slice(n1, None)))
        print(f"fused vs exact, Ez {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
