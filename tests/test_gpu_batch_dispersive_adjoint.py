"""GPU: the adjoint of dispersive batches (fdtd2d_batch_dispersive_adjoint.h, k_batch_window_product_multi, adjoint.py).

Shapes are those of tests/test_gpu_batch_dispersive.py: PML 23x19 and periodic 23x11 with a 4-cell layer, four members
with distinct (gamma, omega0), the last with wp2 = 0, 60 steps, two frequencies, three probes, float32 and float64;
dt = 1.6e-13 and a 1 THz source so that 60 steps tell the two frequencies apart (the channel system's condition number is
asserted).  Such a run has not rung down, so its gradients mean nothing physically: the device is compared with the
stand-in of tests/oracle_batch_dispersive_adjoint.py driven by the same helper, which holds whatever the fields do.  The
physics is checked on the stand-in in tests/test_batch_dispersive_adjoint_cpu.py.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_MEASURED."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch import window_product
from oracle_batch_dispersive_adjoint import oracle_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, FC, LAYER, LDS_LIMIT = 1.6e-13, 1e-4, 1e12, 4, 163840
E_ARG, E_STATE = -1, -4
INFO_HELD_WINDOW, INFO_HELD_DISPERSIVE_WINDOW = 13, 20
B, NSTEPS = 4, 60
GAMMA = np.array([1e11, 0.0, 5e10, 2e10])
OMEGA0 = 2 * np.pi * np.array([0.0, 0.5e12, 0.6e12, 0.0])        # member 0 Drude, 1 lossless, 3 has wp2 = 0
WP2_TOP = (2 * np.pi * 0.5e12) ** 2
OMEGAS = 2 * np.pi * np.array([0.4e12, 0.9e12])
# (boundary, rows, cols): the design window, the forward sources and the three probes
CASES = {"pml23x19": ("pml", 23, 19), "per23x11": ("periodic", 23, 11)}
DESIGN = {"pml": (8, 7, 6, 5), "periodic": (8, 0, 6, 10)}
SOURCES = {"pml": np.array([(15, 8, 1, 3), (16, 9, 1, 1), (15, 6, 2, 2), (14, 10, 1, 2)]),
           "periodic": np.array([(15, 2, 1, 3), (16, 0, 1, 10), (15, 6, 2, 2), (14, 8, 1, 2)])}
PROBES = {"pml": np.array([(6, 6), (15, 13), (10, 14)]), "periodic": np.array([(6, 0), (16, 9), (7, 5)])}
# The fused build contracts the step's multiply-add pairs and the product's (tr, ti and the term), so its gradients differ
# from the exact build's by rounding.  Measured on an MI355X (the child processes of test_fused_build_within_its_bounds):
# batch_dispersive_gradient on the members of both cases, worst member's max|fused - exact| / max|exact| per gradient.
# The bound is ten times the measured value.
FUSED_MEASURED = {("eps", "f32"): 9.8e-7, ("sigma", "f32"): 9.1e-7, ("wp2", "f32"): 1.2e-6,
                  ("eps", "f64"): 4.3e-15, ("sigma", "f64"): 5.9e-15, ("wp2", "f64"): 3.9e-15}
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


def objective(spectra):
    """J = sum_k |sum_p X[p, k]|^2 and its cotangent g = dJ/dRe + i dJ/dIm = 2 sum_p X[p, k] at every probe."""
    S = spectra.sum(axis=1)
    return (np.abs(S) ** 2).sum(axis=1), np.repeat(2 * S[:, None, :], spectra.shape[1], axis=1)


def _materials(boundary, R, C, dtype, seed=7, count=B):
    """eps everywhere; sigma and wp2 on the design window (the last member of every four: wp2 = 0)."""
    from fdtd2d_amd.api import EPS0
    rng = np.random.default_rng(seed)
    r0, c0, nr, nc = DESIGN[boundary]
    eps = EPS0 * (1 + 2 * rng.random((count, R, C)))
    sigma, wp2 = np.zeros((count, R, C)), np.zeros((count, R, C))
    sigma[:, r0:r0 + nr, c0:c0 + nc] = 5.0 * rng.random((count, nr, nc))
    wp2[:, r0:r0 + nr, c0:c0 + nc] = WP2_TOP * (0.2 + rng.random((count, nr, nc)))
    wp2[3::4] = 0.0
    if boundary == "periodic":
        for a in (eps, sigma, wp2):
            a[:, :, -1] = a[:, :, 0]
    return eps.astype(dtype), sigma, wp2


def _args(boundary, dtype, engine=None, nsteps=NSTEPS, count=B):
    tile = lambda a: np.concatenate([a] * (count // B)) if count > B else a[:count]
    return dict(nsteps=nsteps, sources=tile(SOURCES[boundary]), probes=PROBES[boundary], omegas=OMEGAS,
                design=DESIGN[boundary], fc=FC, dt=DT, dx=DX, dtype=dtype, boundary=boundary, pml_cells=LAYER,
                engine=engine)


def _pole(count=B):
    return np.resize(GAMMA, count), np.resize(OMEGA0, count)


_refs = {}


def _reference(fd, case, dtype):
    """batch_dispersive_gradient on the stand-in, computed once per case and dtype."""
    key = (case, np.dtype(dtype).name)
    if key not in _refs:
        boundary, R, C = CASES[case]
        eps, sigma, wp2 = _materials(boundary, R, C, dtype)
        _refs[key] = fd.batch_dispersive_gradient(eps, sigma, (wp2,) + _pole(), objective=objective,
                                                  **_args(boundary, dtype, engine=oracle_for(boundary)))
    return _refs[key]


def _close(got, want, tol):
    for m in range(want.shape[0]):
        top = np.abs(want[m]).max()
        assert top > 0 and np.abs(got[m] - want[m]).max() <= tol * top, m


# ---- 1. the held window and the product -------------------------------------------------------------------------------------

def _sequence(b, boundary, R, C, dtype, rng_seed=3):
    """A forward run, the hold, reset, point sources and a channel run, on an engine or the stand-in.  Returns the window
    at hold time, the current window, the three-set product and the one-set product."""
    from fdtd2d_amd.adjoint import channel_system
    from fdtd2d_amd.api import MU0, ricker_amplitude
    eps, sigma, wp2 = _materials(boundary, R, C, dtype)
    rng = np.random.default_rng(rng_seed)
    b.set_materials(eps, MU0)
    b.set_pml(LAYER, courant00=np.array([(1 / np.sqrt(float(e) * MU0) * DT) / DX for e in eps[:, 0, 0]]))
    b.set_sources(SOURCES[boundary]).set_conductivity(sigma).set_dispersion(wp2, GAMMA, OMEGA0)
    b.set_dft_window(DESIGN[boundary], OMEGAS).set_probes(PROBES[boundary], NSTEPS)
    amps = np.tile([ricker_amplitude(k * DT, FC) for k in range(NSTEPS)], (B, 1))
    b.run(NSTEPS, amps)
    at_hold = b.read_dft_window().copy()
    b.hold_dispersive_window()
    chan, A = channel_system(OMEGAS, NSTEPS, DT, FC)
    assert np.linalg.cond(A) < 1e4
    b.reset()
    b.set_point_sources(PROBES[boundary], rng.standard_normal((B, 3, 4)))
    b.run(NSTEPS, None, chan)
    cur = b.read_dft_window().copy()
    coefs = rng.standard_normal((3, B, 2)) + 1j * rng.standard_normal((3, B, 2))
    scales = rng.standard_normal((B, 3))
    return dict(at_hold=at_hold, cur=cur, coefs=coefs, scales=scales, multi=b.dispersive_window_product(coefs, scales),
                one=b.dispersive_window_product(coefs[:1])[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_the_held_window_and_the_product_match_the_stand_in_on_every_path(fd, case, dtype):
    _exact_only(fd)
    boundary, R, C = CASES[case]
    want = _sequence(oracle_for(boundary)(B, R, C, DT, DX, dtype=dtype, boundary=boundary), boundary, R, C, dtype)
    runs = {}
    for name, opts in (("resident", {}), ("split7", dict(steps_per_launch=7)), ("streamed", dict(resident=0))):
        with fd.BatchEngine(B, R, C, DT, DX, dtype=dtype, boundary=boundary) as b:
            b.set_option(**opts)
            got = runs[name] = _sequence(b, boundary, R, C, dtype)
            assert b.resident == (name != "streamed")
            assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 1 and b.info(INFO_HELD_WINDOW) == 0
            # the one-set product against the existing product of a pole-free lossy engine on the same two buffers: hold the
            # current window in both buffers, take the new product, remove the pole, take the old one
            b.hold_dispersive_window()
            new = b.dispersive_window_product(got["coefs"][:1])[0]
            b.set_dispersion(None)
            assert not b.dispersive and b.lossy and b.info(INFO_HELD_DISPERSIVE_WINDOW) == 0
            b.hold_dft_window()
            assert b.info(INFO_HELD_WINDOW) == 1
            assert np.array_equal(new, b.dft_window_product(got["coefs"][0])) and np.any(new)
        top = np.abs(want["cur"]).max()
        for k in ("at_hold", "cur"):
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), (name, k)
        assert np.abs(got["multi"] - want["multi"]).max() <= 1e-12 * np.abs(want["multi"]).max(), name
        assert np.abs(got["one"] - want["one"]).max() <= 1e-12 * np.abs(want["one"]).max(), name
        # the held window is the window at hold time: it survived reset, set_point_sources and the channel run
        for c in range(3):
            host = np.stack([got["scales"][m, c] * window_product(got["coefs"][c, m], got["at_hold"][m], got["cur"][m])
                             for m in range(B)])
            assert np.array_equal(got["multi"][c], host), (name, c)
        assert np.array_equal(got["one"], np.stack([window_product(got["coefs"][0, m], got["at_hold"][m], got["cur"][m])
                                                    for m in range(B)]))
        assert top > 0 and not np.array_equal(got["at_hold"], got["cur"])
    for name, got in runs.items():
        for k in ("at_hold", "cur", "multi", "one"):
            assert np.array_equal(got[k], runs["resident"][k]), (name, k)


# ---- 2. the gradients against the stand-in ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_dispersive_gradients_match_the_stand_in(fd, case, dtype):
    _exact_only(fd)
    boundary, R, C = CASES[case]
    Jr, ger, gsr, gwr, sr, ir = _reference(fd, case, dtype)
    eps, sigma, wp2 = _materials(boundary, R, C, dtype)
    J, ge, gs, gw, s, info = fd.batch_dispersive_gradient(eps, sigma, (wp2,) + _pole(), objective=objective,
                                                          **_args(boundary, dtype))
    nr, nc = DESIGN[boundary][2:]
    assert ge.shape == gs.shape == gw.shape == (B, nr, nc) and s.shape == (B, 3, 2) and J.shape == (B,)
    assert np.abs(s - sr).max() <= 1e-12 * np.abs(sr).max() and np.allclose(J, Jr, rtol=1e-12, atol=0)
    for g, w in ((ge, ger), (gs, gsr), (gw, gwr)):
        _close(g, w, 1e-9)
    assert np.any(gw[3]) and not np.any(wp2[3])      # the member without a pole has a wp2 gradient too
    assert np.allclose(info["residual_forward"], ir["residual_forward"], rtol=1e-9)


# ---- 3. the session against the helper ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_dispersive_session_matches_the_helper(fd, case, dtype):
    _exact_only(fd)
    boundary, R, C = CASES[case]
    eps, sigma, wp2 = _materials(boundary, R, C, dtype)
    r0, c0, nr, nc = DESIGN[boundary]
    with fd.DispersiveAdjointSession(eps, dispersion=(wp2,) + _pole(), sigma=sigma, **_args(boundary, dtype)) as s:
        assert s.engine.dispersive and s.engine.lossy and s.engine.resident
        launches = s.engine.launches
        J, ge, sp, info = s.value_and_grad(objective)
        gs, gw = s.sigma_gradient(), s.wp2_gradient()
        assert s.engine.launches - launches == 2 + 2 + 2 + 1            # runs, spectra, maxima, one product
        want = _reference(fd, case, dtype)
        for g, w in ((ge, want[1]), (gs, want[2]), (gw, want[3])):
            _close(g, w, 1e-9)
        assert np.abs(sp - want[4]).max() <= 1e-12 * np.abs(want[4]).max() and np.allclose(J, want[0], rtol=1e-12, atol=0)
        # across a set_design_wp2
        new = WP2_TOP * (0.1 + np.random.default_rng(19).random((B, nr, nc)))
        new[3] = 0.0
        assert s.set_design_wp2(new) is s
        wp22 = wp2.copy()
        wp22[:, r0:r0 + nr, c0:c0 + nc] = new
        if boundary == "periodic":
            wp22[:, :, -1] = wp22[:, :, 0]
        J2, ge2, sp2, _ = s.value_and_grad(objective)
        got2 = (ge2, s.sigma_gradient(), s.wp2_gradient())
        # the library's stability refusal leaves the engine and the session as they were
        bad = new.copy()
        bad[1, 2, 2] = 4.1 / DT ** 2 * 4
        with pytest.raises(fd.Fdtd2dError, match=r"member 1: the pole at cell") as ei:
            s.set_design_wp2(bad)
        assert ei.value.code == E_ARG and np.array_equal(s.wp2[:, r0:r0 + nr, c0:c0 + nc], new)
        from fdtd2d_amd.api import EPS0
        thin = np.array(s.eps[:, r0:r0 + nr, c0:c0 + nc])
        thin[0, 1, 1] = 0.2 * EPS0                 # Courant 0.48 / sqrt(0.2) > 1: the host refuses
        with pytest.raises(ValueError, match="Courant"):
            s.set_design_eps(thin)
        assert np.array_equal(s.eps, eps)
    want2 = fd.batch_dispersive_gradient(eps, sigma, (wp22,) + _pole(), objective=objective,
                                         **_args(boundary, dtype, engine=oracle_for(boundary)))
    for g, w in zip(got2, want2[1:4]):
        _close(g, w, 1e-9)
    assert np.allclose(J2, want2[0], rtol=1e-12, atol=0) and not np.allclose(J2, J, rtol=1e-6, atol=0)


# ---- 4. the largest resident member -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,R,C,resident", [(np.float32, 67, 60, True), (np.float64, 44, 45, True),
                                                (np.float32, 70, 70, False)], ids=["f32_67x60", "f64_44x45", "f32_70x70"])
def test_the_largest_resident_member_and_a_streamed_one(fd, dtype, R, C, resident):
    """67x60 float32 and 44x45 float64 are the largest members the ten-array rule admits with two frequencies and three
    point cells (one row more does not fit: asserted); 70x70 is streamed.  Two members, 30 steps."""
    _exact_only(fd)
    esz, n, count = np.dtype(dtype).itemsize, 30, 2

    def fits(rows):
        return 10 * _seg(rows * C, esz) + _seg(4 * rows, esz) + _seg(4 * C, esz) + 16 * 2 + 8 * 3 <= LDS_LIMIT
    assert fits(R) == resident and (not resident or not fits(R + 1))
    eps, sigma, wp2 = _materials("pml", R, C, dtype, count=count)
    gamma, omega0 = _pole(count)
    args = _args("pml", dtype, nsteps=n, count=count)
    args.update(fc=2e12)                           # 30 steps: a shorter envelope (condition number 7)
    with fd.DispersiveAdjointSession(eps, dispersion=(wp2, gamma, omega0), sigma=sigma, **args) as s:
        assert s.engine.resident == resident
        launches = s.engine.launches
        J, ge, sp, info = s.value_and_grad(objective)
        got = (ge, s.sigma_gradient(), s.wp2_gradient())
        assert s.engine.launches - launches == (2 if resident else 4 * n) + 2 + 2 + 1
    args["engine"] = oracle_for("pml")
    want = fd.batch_dispersive_gradient(eps, sigma, (wp2, gamma, omega0), objective=objective, **args)
    for g, w in zip(got, want[1:4]):
        _close(g, w, 1e-9)
    assert np.abs(sp - want[4]).max() <= 1e-12 * np.abs(want[4]).max()


# ---- 5. the C refusals ----------------------------------------------------------------------------------------------------------

def _raises(fd, code, match, call):
    with pytest.raises(fd.Fdtd2dError, match=match) as ei:
        call()
    assert ei.value.code == code


def _err(b):
    return b._lib.fdtd2d_batch_last_error(b._h).decode()


@pytest.mark.parametrize("case", list(CASES))
def test_refusals_leave_the_batch_as_it_was(fd, case):
    from fdtd2d_amd.api import EPS0, MU0
    boundary, R, C = CASES[case]
    eps, sigma, wp2 = _materials(boundary, R, C, np.float32)
    d = np.ones(3 * B * 2 + 3 * B)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(3 * B * 6 * 10)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with fd.BatchEngine(B, R, C, DT, DX, dtype=np.float32, boundary=boundary) as b:
        lib, h = b._lib, b._h
        b.set_materials(eps, MU0).set_pml(LAYER).set_conductivity(sigma)
        b.set_dft_window(DESIGN[boundary], OMEGAS)
        # without a pole: the raw calls and the engine's own check
        assert lib.fdtd2d_batch_hold_dispersive_window(h) == E_STATE and "fdtd2d_batch_hold_dft_window" in _err(b)
        assert lib.fdtd2d_batch_dispersive_window_product(h, 1, dp, dp, dp, op) == E_STATE
        assert "fdtd2d_batch_dft_window_product" in _err(b)
        _raises(fd, E_STATE, "needs a dispersive pole", b.hold_dispersive_window)
        assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 0 and not b.dispersive
        b.set_dispersion(wp2, GAMMA, OMEGA0)
        # with the pole: the product without a held window, bad arguments, the existing hold
        assert lib.fdtd2d_batch_dispersive_window_product(h, 3, dp, dp, dp, op) == E_STATE
        assert "no held dispersive window" in _err(b)
        _raises(fd, E_STATE, "no held dispersive window", lambda: b.dispersive_window_product(np.ones((1, 2))))
        assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 0
        b.hold_dispersive_window()
        assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 1 and b.info(INFO_HELD_WINDOW) == 0
        for n in (0, 4, -1):
            assert lib.fdtd2d_batch_dispersive_window_product(h, n, dp, dp, dp, op) == E_ARG and "ncoef" in _err(b)
        for args in ((None, dp, dp, op), (dp, None, dp, op), (dp, dp, None, op), (dp, dp, dp, None)):
            assert lib.fdtd2d_batch_dispersive_window_product(h, 1, *args) == E_ARG and "NULL" in _err(b)
        with pytest.raises(ValueError, match="coefs must have shape"):
            b.dispersive_window_product(np.ones((4, 2)))
        with pytest.raises(ValueError, match="scales must have shape"):
            b.dispersive_window_product(np.ones((2, 2)), np.ones(3))
        assert lib.fdtd2d_batch_hold_dft_window(h) == E_STATE and "dispersive pole" in _err(b)
        _raises(fd, E_STATE, "dispersive pole", b.hold_dft_window)
        _raises(fd, E_STATE, "dispersive pole", lambda: b.dft_window_product(np.ones(2)))
        assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 1 and b.info(INFO_HELD_WINDOW) == 0 and b.dispersive
        assert not np.any(b.dispersive_window_product(np.ones((2, 2))))        # windows of zeros: zeros, and it runs
        # the held window goes with the window
        b.set_dft_window(DESIGN[boundary], OMEGAS)
        assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 0 and b.info(INFO_HELD_WINDOW) == 0
        assert lib.fdtd2d_batch_dispersive_window_product(h, 1, dp, dp, dp, op) == E_STATE
        # without a window
        assert lib.fdtd2d_batch_set_dft_window(h, 0, 0, 0, 0, 0, None, 1) == 0
        assert lib.fdtd2d_batch_hold_dispersive_window(h) == E_STATE and "no window DFT" in _err(b)
        assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 0 and b.dispersive and b.lossy
    if boundary == "periodic":                      # complex fields: the pole of a Bloch batch is refused
        with fd.BatchEngine(B, R, C, DT, DX, dtype=np.float32, boundary="periodic") as b:
            b.set_materials(eps, MU0).set_pml(LAYER).set_bloch_phase(0.4)
            b.set_dft_window((8, 0, 6, 10), OMEGAS)
            b.set_bloch_dispersion(wp2, GAMMA, OMEGA0)
            assert b._lib.fdtd2d_batch_hold_dispersive_window(b._h) == E_STATE and "Bloch phase" in _err(b)
            assert b._lib.fdtd2d_batch_dispersive_window_product(b._h, 1, dp, dp, dp, op) == E_STATE
            _raises(fd, E_STATE, "Bloch phase", b.hold_dispersive_window)
            assert b.info(INFO_HELD_DISPERSIVE_WINDOW) == 0 and b.info(INFO_HELD_WINDOW) == 0 and b.dispersive


# ---- 6. the fused build ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_dispersive_adjoint as t
out = {"arithmetic": fd.ARITHMETIC}
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    grads = []
    for case, (boundary, R, C) in t.CASES.items():
        eps, sigma, wp2 = t._materials(boundary, R, C, dtype)
        g = fd.batch_dispersive_gradient(eps, sigma, (wp2,) + t._pole(), objective=t.objective, **t._args(boundary, dtype))
        grads.append(np.stack(g[1:4]).reshape(3, t.B, -1))
    np.save(f"{OUT}/grads_{name}.npy", np.concatenate(grads, axis=2))
print("DISPERSIVE_ADJOINT_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's three gradients against the exact build's, both on the device, each in a process of its own."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("DISPERSIVE_ADJOINT_RESULT ")][-1][26:])
        assert r["arithmetic"] == arith, r
        res[arith] = {k: np.load(out / f"grads_{k}.npy") for k in ("f32", "f64")}
    n1 = 6 * 5                                      # per member: the cells of the PML case, then the periodic case's
    worst = {}
    for (which, k) in FUSED_BOUND:
        i = ("eps", "sigma", "wp2").index(which)
        e, f = res["exact"][k][i], res["fused"][k][i]
        worst[which, k] = max(np.abs(f[m, s] - e[m, s]).max() / np.abs(e[m, s]).max()
                              for m in range(B) for s in (slice(0, n1), slice(n1, None)))
        print(f"fused vs exact, {which} gradient {k}: worst member {worst[which, k]:.3e} "
              f"(bound {FUSED_BOUND[which, k]:.1e})")
    for key in FUSED_BOUND:
        assert worst[key] <= FUSED_BOUND[key], key
