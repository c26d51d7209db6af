"""GPU: lossy materials in the batched engine (fdtd2d_batch_lossy.h, kernels_batch_lossy.hpp).

With sigma = 0 everywhere a lossy batch is bit-identical to the same batch without conductivity.  With sigma > 0 fields
and probe traces equal the stand-in of tests/oracle_batch_lossy.py bit for bit (exact build), window DFTs to 1e-12, and
everything is bit-identical whatever the path (resident or streamed), the launch split and the accumulators' placement;
every case asserts the path it took and its launch count.  The coefficients after any order of set_eps_window,
set_conductivity_window and set_materials are those of a fresh engine.  batch_material_gradient and the session's
sigma_gradient are checked against the stand-in and against each other.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_BOUND."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_lossy import LossyOracle
import test_batch_adjoint_cpu as cpu
import test_batch_lossy_cpu as lcpu
import test_gpu_batch_adjoint as adj

pytestmark = pytest.mark.gpu

ROOT = adj.ROOT
DT, DX, LAYER, LDS_LIMIT = adj.DT, adj.DX, adj.LAYER, adj.LDS_LIMIT
# The fused build evaluates the lossy update as fma(dhy - dhx, cb, ca * e), so its results differ from the exact
# build's by rounding.  Measured on an MI355X (the child processes of test_fused_build_within_its_bounds), worst member:
#   Ez after 300 steps with monitors and point sources, 6 members of 60x60 (48x48 in float64), max|fused - exact| /
#   max|exact|:   float32 mur 8.1e-7, pml 1.4e-7;   float64 mur 7.2e-16, pml 2.4e-16
#   both gradients of batch_material_gradient (4 members, 1500 steps), of max|gradient| over the design window:
#       float32 mur eps 6.9e-7 sigma 4.9e-7, pml eps 6.7e-7 sigma 4.1e-7
#       float64 mur eps 2.4e-15 sigma 1.4e-15, pml eps 1.3e-15 sigma 1.2e-15
# The bounds are ten times the measured values.
FUSED_BOUND = {
    ("field", "mur", "f32"): 8.1e-6, ("field", "pml", "f32"): 1.4e-6,
    ("field", "mur", "f64"): 7.2e-15, ("field", "pml", "f64"): 2.4e-15,
    ("eps", "mur", "f32"): 6.9e-6, ("sigma", "mur", "f32"): 4.9e-6,
    ("eps", "pml", "f32"): 6.7e-6, ("sigma", "pml", "f32"): 4.1e-6,
    ("eps", "mur", "f64"): 2.4e-14, ("sigma", "mur", "f64"): 1.4e-14,
    ("eps", "pml", "f64"): 1.3e-14, ("sigma", "pml", "f64"): 1.2e-14,
}


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _shape(dtype, where):
    if where == "streamed":
        return (72, 72) if dtype == np.float64 else (100, 120)
    return (48, 48) if dtype == np.float64 else (60, 60)


def _margin(boundary):
    return {"mur": 6, "pml": LAYER, "none": 1}[boundary]


def _sigma(rng, B, R, Cc, boundary, top=20.0):
    """Random conductivity up to `top` S/m (s up to 0.056 at this dt) on the cells that may conduct, zero on 30 %."""
    g = _margin(boundary)
    s = np.zeros((B, R, Cc))
    inner = top * rng.random((B, R - 2 * g, Cc - 2 * g))
    s[:, g:R - g, g:Cc - g] = np.where(rng.random(inner.shape) < 0.3, 0.0, inner)
    return s


def _expect_path(b, nf, window_cells, ncell, lossy, never=False, lds_allowed=True):
    """The capacity rule, restated: arrays = 6 (Mur) or 7 (PML) while a conductivity is set."""
    esz, R, Cc = b.dtype.itemsize, b.rows, b.cols
    seg = adj._seg(R * Cc, esz)
    arrays = (7 if b.pml else 6) if lossy else (6 if b.pml else 5)
    fields = arrays * seg + (adj._seg(4 * R, esz) + adj._seg(4 * Cc, esz) if b.pml else 0)
    table, acc = 16 * nf + 8 * ncell, 16 * nf * window_cells
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = bool(nf) and lds_allowed and fields + table + acc <= LDS_LIMIT
    assert b.lossy == lossy
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - (fields - arrays * seg) - table) // arrays // 16 * 16 // esz
    assert b.resident == resident
    assert b.window_in_lds == (in_lds and resident)
    return resident


def _drive(b, boundary, cfg, window, n, monitors=True, layer=LAYER):
    eps, mu, rects, amps, omegas, cells, weights, chan = cfg
    b.set_materials(eps, mu).set_sources(rects)
    if boundary == "pml":
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(eps[:, 0, 0], mu[:, 0, 0])]
        b.set_pml(layer, courant00=np.array(c00))
    if monitors:
        b.set_dft_window(window, omegas).set_probes(cells, n).set_point_sources(cells, weights)


def _device_run(fd, boundary, dtype, R, Cc, cfg, window, splits, sigma, monitors=True, resident=None, spl=None,
                lds=True, layer=LAYER):
    """sigma None: no conductivity.  Returns fields (+ monitors) and the path."""
    B, n = cfg[0].shape[0], sum(splits)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        _drive(b, boundary, cfg, window, n, monitors, layer)
        if sigma is not None:
            b.set_conductivity(sigma)
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        path = _expect_path(b, cfg[4].shape[1] if monitors else 0, window[2] * window[3],
                            cfg[5].shape[1] if monitors else 0, sigma is not None, never=resident == 0, lds_allowed=lds)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, cfg[3][:, done:done + k], cfg[7][..., done:done + k] if monitors else None)
            done += k
        if path:      # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * n
        out = dict(fields=b.download(), path=path, in_lds=b.window_in_lds)
        if boundary == "pml":
            out["fields"] += (b.download_ezx(),)
        if monitors:
            out.update(dft=b.read_dft_window(), probes=b.read_probes())
        return out


def _same(a, b):
    ok = all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"]))
    if "dft" in a:
        ok = ok and np.array_equal(a["dft"], b["dft"]) and np.array_equal(a["probes"], b["probes"])
    return ok


def _window(R, dtype):
    return (R // 2 - 6, 8, 12, 20) if dtype == np.float32 else (R // 2 - 2, 8, 3, 6)


# ---- 1. sigma = 0 is the lossless batch, bit for bit ---------------------------------------------------------------------

@pytest.mark.parametrize("monitors", [False, True], ids=["plain", "monitored"])
@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_zero_conductivity_is_bit_identical_to_no_conductivity(fd, boundary, dtype, where, monitors):
    R, Cc = _shape(dtype, where)
    B, n = 4, 40
    window = _window(R, dtype)
    cfg = adj._setup(fd, np.random.default_rng(R + 1), B, R, Cc, dtype, 6, n)
    want = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (23, 17), None, monitors)
    for sigma in (0.0, np.zeros((B, R, Cc), np.float32)):
        got = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (23, 17), sigma, monitors)
        assert got["path"] == (where == "resident")
        assert np.abs(got["fields"][0]).max() > 0 and _same(want, got)


# ---- 2. against the stand-in ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml", "none"])
def test_lossy_runs_match_the_stand_in(fd, boundary, dtype, where):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_within_its_bounds")
    R, Cc = _shape(dtype, where)
    B, n = 4, 40
    window = _window(R, dtype)
    rng = np.random.default_rng(R + 2)
    cfg = adj._setup(fd, rng, B, R, Cc, dtype, 6, n)
    sigma = _sigma(rng, B, R, Cc, boundary)
    got = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (23, 17), sigma)
    assert got["path"] == (where == "resident")
    ref = LossyOracle(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary)
    _drive(ref, boundary, cfg, window, n)
    ref.set_conductivity(sigma)
    ref.run(n, cfg[3], cfg[7])
    for name, a, w in zip(("Ez", "Hx", "Hy"), got["fields"], ref.download()):
        assert np.array_equal(a, w), name
    assert np.array_equal(got["probes"], ref.read_probes())
    want = ref.read_dft_window()
    assert np.abs(got["dft"] - want).max() <= 1e-12 * np.abs(want).max()
    # the conductivity changed the fields
    lossless = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (n,), None)
    assert not np.array_equal(lossless["fields"][0], got["fields"][0])


# ---- 3. bit-identical whatever the path -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_lossy_runs_are_bit_identical_on_every_path(fd, boundary, dtype):
    R, Cc = _shape(dtype, "resident")
    window = _window(R, dtype)
    rng = np.random.default_rng(5)
    cfg = adj._setup(fd, rng, 6, R, Cc, dtype, 6, 60)
    sigma = _sigma(rng, 6, R, Cc, boundary)
    base = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (60,), sigma)
    assert base["path"]
    variants = dict(streamed=dict(resident=0), spl=dict(spl=7), split=dict(splits=(1, 32, 27)),
                    global_acc=dict(lds=False), split_spl=dict(splits=(33, 27), spl=10, lds=False))
    seen_lds = {base["in_lds"]}
    for name, kw in variants.items():
        splits = kw.pop("splits", (60,))
        got = _device_run(fd, boundary, dtype, R, Cc, cfg, window, splits, sigma, **kw)
        assert got["path"] == (name != "streamed"), name
        seen_lds.add(got["in_lds"])
        assert _same(base, got), name
    assert seen_lds == {True, False}
    # no monitors, no point sources: the same family with them silent, the same fields
    plain = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (60,), sigma, monitors=False)
    quiet = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (60,), sigma, monitors=False, resident=0)
    assert plain["path"] and not quiet["path"] and _same(plain, quiet)


# ---- 4. members are independent; more members than one round of workgroups ------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
def test_lossy_members_are_independent(fd, where):
    boundary, dtype = "mur", np.float32
    R, Cc = _shape(dtype, where)
    window = _window(R, dtype)
    rng = np.random.default_rng(11)
    cfg = adj._setup(fd, rng, 6, R, Cc, dtype, 6, 40)
    sigma = _sigma(rng, 6, R, Cc, boundary)
    a = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (40,), sigma)
    sigma2 = sigma.copy()
    sigma2[2] *= 0.5
    b = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (40,), sigma2)
    for m in range(6):
        same = (all(np.array_equal(x[m], y[m]) for x, y in zip(a["fields"], b["fields"])) and
                np.array_equal(a["dft"][m], b["dft"][m]) and np.array_equal(a["probes"][m], b["probes"][m]))
        assert same == (m != 2), m


@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_264_lossy_members_beyond_one_round_of_workgroups(fd, boundary):
    dtype = np.float32
    R, Cc = _shape(dtype, "resident")
    window = _window(R, dtype)
    rng = np.random.default_rng(13)
    small = adj._setup(fd, rng, 8, R, Cc, dtype, 6, 40)
    sig8 = _sigma(rng, 8, R, Cc, boundary)
    want = _device_run(fd, boundary, dtype, R, Cc, small, window, (40,), sig8)
    B = 264
    big = tuple(np.concatenate([x] * (B // 8)) if x.shape[0] == 8 else x for x in small)
    with fd.BatchEngine(2, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        b.set_materials(small[0][:2], small[1][:2])
        if boundary == "pml":
            b.set_pml(LAYER)
        b.set_conductivity(0.0)
        assert b.resident and (LDS_LIMIT // b.lds_bytes) * 256 < B      # one workgroup per CU, 256 CUs: two rounds
    got = _device_run(fd, boundary, dtype, R, Cc, big, window, (40,), np.concatenate([sig8] * (B // 8)))
    assert got["path"]
    for k in ("dft", "probes"):
        assert np.array_equal(got[k], np.concatenate([want[k]] * (B // 8))), k
    for a, w in zip(got["fields"], want["fields"]):
        assert np.array_equal(a, np.concatenate([w] * (B // 8)))


# ---- 5. the coefficients are those of a fresh engine ------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["eps_sigma", "sigma_eps", "sigma_materials", "window_first", "uniform"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_coefficients_are_consistent_in_every_order(fd, boundary, order):
    dtype = np.float32
    R, Cc, B, n = 60, 60, 3, 300
    rng = np.random.default_rng(17)
    cfg = adj._setup(fd, rng, B, R, Cc, dtype, 6, n)
    eps, mu = cfg[0], cfg[1]
    uniform = order == "uniform"
    if uniform:
        eps = np.full((B, R, Cc), 2 * fd.EPS0).astype(dtype)
    sig0, sig1 = _sigma(rng, B, R, Cc, boundary), _sigma(rng, B, R, Cc, boundary)
    win = (14, 12, 20, 30)
    r0, c0, nr, nc = win
    eps_w = (fd.EPS0 * (1 + 2 * rng.random((B, nr, nc)))).astype(dtype)
    eps_full, sig_full = eps.copy(), sig0.copy()
    eps_full[:, r0:r0 + nr, c0:c0 + nc] = eps_w
    sig_full[:, r0:r0 + nr, c0:c0 + nc] = sig1[:, r0:r0 + nr, c0:c0 + nc]
    if order == "window_first":
        sig_full = np.zeros_like(sig0)
        sig_full[:, r0:r0 + nr, c0:c0 + nc] = sig1[:, r0:r0 + nr, c0:c0 + nc]
    if order == "sigma_materials":
        sig_full = sig0

    def prepare(b, first_eps):
        if uniform and first_eps is eps:
            b.set_materials(2 * fd.EPS0, fd.MU0)
        else:
            b.set_materials(first_eps, mu)
        b.set_sources(cfg[2])
        if boundary == "pml":
            b.set_pml(LAYER)

    def finish(b):
        assert b.lossy and b.resident
        launches = b.launches
        b.run(n, cfg[3])
        assert b.launches - launches == 1
        return b.courant(), b.download()

    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        prepare(b, eps_full)
        b.set_conductivity(sig_full)
        want = finish(b)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        prepare(b, eps)
        sw = sig1[:, r0:r0 + nr, c0:c0 + nc]
        if order == "eps_sigma":
            b.set_conductivity(sig0).set_eps_window(win, eps_w).set_conductivity_window(win, sw)
        elif order == "sigma_eps":
            b.set_conductivity(sig0).set_conductivity_window(win, sw).set_eps_window(win, eps_w)
        elif order == "sigma_materials":
            b.set_conductivity(sig0).set_materials(eps_full, mu)
        elif order == "window_first":
            b.set_conductivity_window(win, sw).set_eps_window(win, eps_w)
        else:
            b.set_conductivity(sig0)               # materialises the uniform batch's coefficient arrays
            assert b.lossy
            b.set_eps_window(win, eps_w).set_conductivity_window(win, sw)
        got = finish(b)
    assert np.array_equal(got[0], want[0])
    assert np.abs(want[1][0]).max() > 0
    for a, w in zip(got[1], want[1]):
        assert np.array_equal(a, w)


def test_removing_the_conductivity_returns_to_the_other_kernels(fd):
    dtype, boundary = np.float32, "mur"
    R, Cc, B, n = 60, 60, 3, 40
    rng = np.random.default_rng(19)
    cfg = adj._setup(fd, rng, B, R, Cc, dtype, 6, n)
    want = _device_run(fd, boundary, dtype, R, Cc, cfg, _window(R, dtype), (n,), None, monitors=False)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        b.set_materials(cfg[0], cfg[1]).set_sources(cfg[2])
        lds = b.lds_bytes
        b.set_conductivity(_sigma(rng, B, R, Cc, boundary))
        assert b.lossy and b.lds_bytes == lds // 5 * 6
        b.run(n, cfg[3])
        assert not np.array_equal(b.download()[0], want["fields"][0])
        b.set_conductivity(None)
        assert not b.lossy and b.lds_bytes == lds
        b.reset().run(n, cfg[3])
        for a, w in zip(b.download(), want["fields"]):
            assert np.array_equal(a, w)


def test_the_capacity_rule_counts_one_more_array(fd):
    """float32 60x60 and 64x64 stay resident with both boundaries; 80x80 stays resident with Mur and becomes streamed
    with the layer."""
    for (R, boundary), resident in {(60, "mur"): True, (60, "pml"): True, (64, "mur"): True, (64, "pml"): True,
                                    (80, "mur"): True, (80, "pml"): False}.items():
        with fd.BatchEngine(2, R, R, DT, DX, dtype=np.float32, boundary=boundary) as b:
            b.set_materials(np.full((2, R, R), fd.EPS0), fd.MU0)
            if boundary == "pml":
                b.set_pml(LAYER)
            assert b.resident
            b.set_conductivity(0.0)
            assert _expect_path(b, 0, 0, 0, True) == resident, (R, boundary)


def test_conductivity_arguments_are_checked(fd):
    E_ARG, E_STATE = fd._abi.E_ARG, fd._abi.E_STATE
    R = Cc = 40
    ok = np.zeros((3, R, Cc))
    ok[:, 10:30, 10:30] = 1.0

    def refused(b, call, code, match):
        with pytest.raises(fd.Fdtd2dError, match=match) as ei:
            call()
        assert ei.value.code == code
    for boundary, margin in (("mur", 6), ("pml", 10), ("none", 1)):
        with fd.BatchEngine(3, R, Cc, DT, DX, boundary=boundary) as b:
            refused(b, lambda: b.set_conductivity(ok), E_STATE, "materials not set")
            b.set_materials()
            if boundary == "pml":
                b.set_pml(LAYER)
            assert b.conductivity_margin == margin and not b.lossy
            for value, match in ((-1.0, "member 1: sigma must be >= 0"), (np.nan, "member 1: sigma must"),
                                 (np.inf, "member 1: sigma must")):
                bad = ok.copy()
                bad[1, 20, 20] = value
                refused(b, lambda: b.set_conductivity(bad), E_ARG, match)
            for cell in ((margin - 1, 20), (20, Cc - margin), (R - margin, 20), (20, margin - 1)):
                bad = ok.copy()
                bad[2][cell] = 0.5
                refused(b, lambda: b.set_conductivity(bad), E_ARG,
                        rf"member 2: sigma is non-zero at cell \({cell[0]},{cell[1]}\), within {margin} cells")
                refused(b, lambda: b.set_conductivity_window((cell[0], cell[1], 1, 1), np.full((3, 1, 1), 0.5)), E_ARG,
                        "member 0: sigma is non-zero")
            assert not b.lossy
            for win in ((0, 0, 0, 4), (30, 30, 11, 4), (-1, 3, 2, 2)):
                refused(b, lambda: b.set_conductivity_window(win, np.zeros((3, max(win[2], 0), win[3]))), E_ARG, "window")
            with pytest.raises(ValueError, match="sigma must have shape"):
                b.set_conductivity(ok[:2])
            b.set_conductivity(ok)
            assert b.lossy
            edge = ok.copy()
            edge[:, margin, margin] = 2.0                      # the first cell that may conduct
            b.set_conductivity(edge)
            b.set_conductivity(None)
            assert not b.lossy
    # a layer may not be laid over conducting cells
    with fd.BatchEngine(3, R, Cc, DT, DX, boundary="pml") as b:
        b.set_materials().clear_pml()
        s = np.zeros((3, R, Cc))
        s[1, 3, 20] = 1.0
        b.set_conductivity(s)
        with pytest.raises(fd.Fdtd2dError, match="member 1: sigma is non-zero within 10 cells") as ei:
            b.set_pml(LAYER)
        assert ei.value.code == E_ARG


# ---- 6. the gradients ----------------------------------------------------------------------------------------------------------

NSTEPS_G, MEMBERS_G = 1500, 4
_stand_in = {}


def _materials():
    return cpu.design_eps(count=MEMBERS_G), lcpu.design_sigma(count=MEMBERS_G)


def _reference(fd, boundary, dtype):
    key = (boundary, np.dtype(dtype).name)
    if key not in _stand_in:
        eps, sigma = _materials()
        _stand_in[key] = lcpu.gradient(fd, boundary, dtype, eps=eps, sigma=sigma, nsteps=NSTEPS_G)
    return _stand_in[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_batch_material_gradient_matches_the_stand_in(fd, boundary, dtype):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_within_its_bounds")
    Jr, ger, gsr, sr, ir = _reference(fd, boundary, dtype)
    eps, sigma = _materials()
    J, ge, gs, s, info = lcpu.gradient(fd, boundary, dtype, eps=eps, sigma=sigma, nsteps=NSTEPS_G, engine=None)
    assert ge.shape == gs.shape == (MEMBERS_G, 16, 12) and gs.dtype == np.float64 and s.shape == (MEMBERS_G, 8, 3)
    assert np.array_equal(s, sr) and np.array_equal(J, Jr)          # the probe traces are the stand-in's bit for bit
    for m in range(MEMBERS_G):
        for g, w in ((ge, ger), (gs, gsr)):
            gmax = np.abs(w[m]).max()
            assert gmax > 0 and np.abs(g[m] - w[m]).max() <= 1e-9 * gmax, m
    assert np.allclose(info["residual_forward"], ir["residual_forward"], rtol=1e-12)
    assert len({gsr[m].tobytes() for m in range(MEMBERS_G)}) == MEMBERS_G


@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_session_agrees_with_the_helper_over_three_iterations(fd, boundary):
    dtype = np.float64
    eps, sigma = _materials()
    B = MEMBERS_G
    r0, c0, nr, nc = cpu.DESIGN
    args = dict(nsteps=NSTEPS_G, sources=np.tile(cpu.SOURCE, (B, 1)), probes=cpu.PROBES, omegas=cpu.OMEGAS,
                design=cpu.DESIGN, fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, dtype=dtype, boundary=boundary,
                pml_cells=cpu.LAYER)
    with fd.AdjointSession(eps, **args) as s:
        s.set_conductivity(sigma)
        assert s.engine.lossy and s.engine.resident
        for it in range(3):
            launches = s.engine.launches
            J, ge, sp, info = s.value_and_grad(cpu.objective)
            gs = s.sigma_gradient()
            assert s.engine.launches - launches == 2 + 2 + 2 + 1 + 1      # runs, spectra, maxima, two products
            want = lcpu.gradient(fd, boundary, dtype, eps=np.array(s.eps), sigma=np.array(s.sigma), nsteps=NSTEPS_G,
                                 engine=None)
            for m in range(B):
                for g, w in ((ge, want[1]), (gs, want[2])):
                    assert np.abs(g[m] - w[m]).max() <= 1e-9 * np.abs(w[m]).max(), (it, m)
                assert np.abs(sp[m] - want[3][m]).max() <= 1e-12 * np.abs(want[3][m]).max(), (it, m)
            assert np.allclose(J, want[0], rtol=1e-12, atol=0)
            # a step of ascent in both materials
            e = s.eps[:, r0:r0 + nr, c0:c0 + nc] + 0.05 * cpu.EPS0 * ge / np.abs(ge).max(axis=(1, 2), keepdims=True)
            g = s.sigma[:, r0:r0 + nr, c0:c0 + nc] + 0.02 * gs / np.abs(gs).max(axis=(1, 2), keepdims=True)
            s.set_design_eps(np.clip(e, cpu.EPS0, 3 * cpu.EPS0)).set_design_sigma(np.clip(g, 0.0, 0.5))


# ---- 7. the fused build ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_lossy as t
out = {"arithmetic": fd.ARITHMETIC, "zero": True}
for boundary in ("mur", "pml"):
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        R, Cc = t._shape(dtype, "resident")
        rng = np.random.default_rng(23)
        cfg = t.adj._setup(fd, rng, 6, R, Cc, dtype, 6, 300)
        sigma = t._sigma(rng, 6, R, Cc, boundary)
        got = t._device_run(fd, boundary, dtype, R, Cc, cfg, t._window(R, dtype), (300,), sigma)
        np.save(f"{OUT}/field_{boundary}_{name}.npy", got["fields"][0])
        # sigma = 0 against no conductivity, in this build
        a = t._device_run(fd, boundary, dtype, R, Cc, cfg, t._window(R, dtype), (300,), None)
        for where in (None, 0):
            b = t._device_run(fd, boundary, dtype, R, Cc, cfg, t._window(R, dtype), (300,), 0.0, resident=where)
            out["zero"] = out["zero"] and t._same(a, b)
        eps, sig = t._materials()
        g = t.lcpu.gradient(fd, boundary, dtype, eps=eps, sigma=sig, nsteps=t.NSTEPS_G, engine=None)
        np.save(f"{OUT}/eps_{boundary}_{name}.npy", g[1])
        np.save(f"{OUT}/sigma_{boundary}_{name}.npy", g[2])
print("LOSSY_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's lossy fields and gradients against the exact build's, both on the device, each in a process
    of its own; in both builds sigma = 0 is bit-identical to no conductivity."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=900, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("LOSSY_RESULT ")][-1][13:])
        assert r["arithmetic"] == arith and r["zero"] is True
        res[arith] = {k: np.load(out / f"{k[0]}_{k[1]}_{k[2]}.npy").astype(np.float64) for k in FUSED_BOUND}
    worst = {}
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m] - e[m]).max() / np.abs(e[m]).max() for m in range(e.shape[0]))
        print(f"fused vs exact, {k[0]} {k[1]} {k[2]}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
