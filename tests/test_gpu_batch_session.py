"""GPU: probe spectra, field maxima and the permittivity window on the device (fdtd2d_batch_design.h) and
AdjointSession on them (adjoint.py).  In the exact build a probe's spectrum is the window DFT's accumulator at its cell
bit for bit, set_eps_window leaves the engine as set_materials with the full updated arrays would, and the session
agrees with batch_eps_gradient on the device and with the session driven by the stand-in of
tests/test_batch_session_cpu.py.  Every case asserts the path it took (resident or streamed)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_batch_adjoint_cpu as cpu
import test_batch_session_cpu as ses
import test_gpu_batch_adjoint as adj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, LAYER = adj.DT, adj.DX, adj.LAYER
# launches of one value_and_grad on the resident path: forward run, spectra, max|Ez|, adjoint run, peak, max|Ez|, product
LAUNCHES_PER_ITERATION = 7


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked in test_fused_build_probe_spectra_within_the_bound")


def _window(R):
    return (R // 2 - 6, 8, 12, 20)


def _members(fd, rng, B, R, Cc, dtype, n, P, F):
    """Members with their own materials, line sources, amplitudes and frequencies.  Probes: the corner, an edge cell, a
    frame / layer cell, a cell of the rectangle source, up to 12 cells inside the window, the others anywhere."""
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(dtype)
    mu = np.full((B, R, Cc), fd.MU0).astype(dtype)
    rects = np.array([[R // 2 + (m % 3) - 1, 3, 1, Cc - 6] for m in range(B)])
    amps = np.stack([[fd.ricker_amplitude(k * DT, 30e9 * (1 + 0.1 * (m % 7))) for k in range(n)] for m in range(B)])
    omegas = 2 * np.pi * np.linspace(10e9, 100e9, F)[None, :] * (1 + 0.001 * np.arange(B))[:, None]
    r0, c0, nr, nc = _window(R)
    cells = np.empty((B, P, 2), int)
    for m in range(B):
        special = [r0 * Cc + c0 + 1] if P == 1 else [0, (R - 1) * Cc + 5, (2 + m % 2) * Cc + Cc // 3,
                                                      int(rects[m, 0]) * Cc + Cc // 2]
        inside = [(r0 + int(i)) * Cc + c0 + int(j) for i, j in zip(rng.permutation(nr)[:P // 3], rng.permutation(nc))]
        chosen = list(dict.fromkeys(special + inside))[:P]
        rest = np.setdiff1d(rng.permutation(R * Cc)[:4 * P], chosen)
        chosen += [int(v) for v in rng.permutation(rest)[:P - len(chosen)]]
        cells[m] = np.array(divmod(np.array(chosen), Cc)).T
    return eps, mu, rects, amps, omegas, cells


def _engine(fd, boundary, dtype, R, Cc, cfg, n, where, monitors=True):
    eps, mu, rects, amps, omegas, cells = cfg
    b = fd.BatchEngine(eps.shape[0], R, Cc, DT, DX, dtype=dtype, boundary=boundary)
    b.set_materials(eps, mu).set_sources(rects)
    if boundary == "pml":
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(eps[:, 0, 0], mu[:, 0, 0])]
        b.set_pml(LAYER, courant00=np.array(c00))
    if monitors:
        b.set_dft_window(_window(R), omegas).set_probes(cells, n)
        path = adj._expect_path(b, omegas.shape[1], _window(R)[2] * _window(R)[3], 0)
    else:
        path = b.resident
    assert path == (where == "resident")
    return b


def _host_spectra(fd, traces, omegas, first=0, count=None):
    tr = np.zeros_like(traces)
    last = traces.shape[2] if count is None else first + count
    tr[:, :, first:last] = traces[:, :, first:last]
    return fd.adjoint.probe_spectra(tr, omegas, DT)


def _in_window(cells, R):
    r0, c0, nr, nc = _window(R)
    wi, wj = cells[..., 0] - r0, cells[..., 1] - c0
    return (wi >= 0) & (wi < nr) & (wj >= 0) & (wj < nc), wi, wj


def spectra_case(fd, boundary, dtype, where, B, P, F, n, splits):
    """One device run; returns what the checks below compare."""
    R, Cc = adj._shape(boundary, dtype, where)
    cfg = _members(fd, np.random.default_rng(R + P + F), B, R, Cc, dtype, n, P, F)
    out = {}
    with _engine(fd, boundary, dtype, R, Cc, cfg, n, where) as b:
        done = 0
        for k in splits:
            b.run(k, cfg[3][:, done:done + k])
            done += k
        assert b.probe_samples == n
        launches = b.launches
        out["X"], out["peak"] = b.probe_spectra(cfg[4], peak=True)
        out["sub"], out["sub_peak"] = b.probe_spectra(cfg[4], 13 % n, max(1, n - 60), peak=True)
        _, out["only_peak"] = b.probe_spectra(np.empty((B, 0)), peak=True)
        out["absmax"] = [b.field_absmax(f) for f in ("Ez", "Hx", "Hy")]
        assert b.launches - launches == 6
        out["traces"], out["window"], out["fields"] = b.read_probes(), b.read_dft_window(), b.download()
        assert np.array_equal(b.probe_spectra(cfg[4]), out["X"])         # nothing was changed by the calls above
    out["cfg"], out["R"] = cfg, R
    return out


# ---- 6. probe spectra and field maxima ------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_probe_spectra_are_the_window_dft_at_the_probe_cells(fd, boundary, dtype, where):
    _exact_only(fd)
    B, P, F, n = 264, 64, 16, 137          # more members than compute units; 137 samples: no multiple of a chunk
    got = spectra_case(fd, boundary, dtype, where, B, P, F, n, (n,))
    omegas, cells = got["cfg"][4], got["cfg"][5]
    X, traces = got["X"], got["traces"]
    assert X.shape == (B, P, F) and X.dtype == np.complex128 and np.abs(X).max() > 0
    inside, wi, wj = _in_window(cells, got["R"])
    assert inside.sum() >= B * 12 and (~inside).sum() >= B * 4
    for m in range(B):
        for p in np.nonzero(inside[m])[0]:
            assert np.array_equal(X[m, p], got["window"][m, :, wi[m, p], wj[m, p]]), (m, p)
    # the same steps split over several runs
    split = spectra_case(fd, boundary, dtype, where, B, P, F, n, (50, 1, 86))
    assert np.array_equal(split["X"], X) and np.array_equal(split["sub"], got["sub"])
    # the host transform of the traces read back (another summation order)
    want = _host_spectra(fd, traces, omegas)
    assert np.abs(X - want).max() <= 1e-12 * np.abs(want).max()
    want = _host_spectra(fd, traces, omegas, 13, n - 60)
    assert np.abs(want).max() > 0 and np.abs(got["sub"] - want).max() <= 1e-12 * np.abs(want).max()
    # maxima are exact
    assert np.array_equal(got["peak"], np.abs(traces).max(axis=(1, 2)))
    assert np.array_equal(got["only_peak"], got["peak"])
    assert np.array_equal(got["sub_peak"], np.abs(traces[:, :, 13:13 + n - 60]).max(axis=(1, 2)))
    for a, f in zip(got["absmax"], got["fields"]):
        assert a.dtype == np.float64 and np.array_equal(a, np.abs(f.astype(np.float64)).reshape(B, -1).max(axis=1))
    assert len(set(got["peak"].tolist())) > B // 2             # the members differ


@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_probe_spectra_of_one_probe_at_one_frequency(fd, boundary, where):
    _exact_only(fd)
    B, n = 5, 33
    got = spectra_case(fd, boundary, np.float32, where, B, 1, 1, n, (n,))
    inside, wi, wj = _in_window(got["cfg"][5], got["R"])
    assert inside.all() and got["X"].shape == (B, 1, 1) and np.abs(got["X"]).min() > 0
    for m in range(B):
        assert got["X"][m, 0, 0] == got["window"][m, 0, wi[m, 0], wj[m, 0]]
    want = _host_spectra(fd, got["traces"], got["cfg"][4])
    assert np.abs(got["X"] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(got["peak"], np.abs(got["traces"]).max(axis=(1, 2)))


def test_probe_spectra_follow_the_probes_step_of_origin(fd):
    """Probes and window set after some steps: sample n belongs to step step0 + n + 1, as the window DFT counts."""
    _exact_only(fd)
    boundary, dtype, where = "mur", np.float32, "resident"
    R, Cc = adj._shape(boundary, dtype, where)
    B, P, F, n = 6, 8, 3, 70
    cfg = _members(fd, np.random.default_rng(1), B, R, Cc, dtype, 20 + n, P, F)
    with _engine(fd, boundary, dtype, R, Cc, cfg, n, where, monitors=False) as b:
        b.run(20, cfg[3][:, :20])
        b.set_dft_window(_window(R), cfg[4]).set_probes(cfg[5], n)
        b.run(n - 10, cfg[3][:, 20:10 + n])
        assert b.probe_samples == n - 10
        X, W = b.probe_spectra(cfg[4]), b.read_dft_window()
        inside, wi, wj = _in_window(cfg[5], R)
        for m in range(B):
            for p in np.nonzero(inside[m])[0]:
                assert np.array_equal(X[m, p], W[m, :, wi[m, p], wj[m, p]]), (m, p)
        assert inside.any() and np.abs(X).max() > 0
        # the range must lie in the samples recorded so far, not in the capacity
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.probe_spectra(cfg[4], 0, n - 9)
        assert ei.value.code == fd._abi.E_ARG


def test_probe_spectra_and_field_absmax_arguments_are_checked(fd):
    E_ARG, E_STATE = fd._abi.E_ARG, fd._abi.E_STATE
    om = 2 * np.pi * np.array([20e9, 30e9])
    with fd.BatchEngine(3, 40, 40, DT, DX) as b:
        b.set_materials().set_sources(np.array([[20, 20]] * 3))
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.probe_spectra(om)
        assert ei.value.code == E_STATE
        b.set_probes(np.array([[20, 22], [5, 5]]), 30)
        b.run_waveform(20)
        traces = b.read_probes()
        bad = [dict(omegas=np.array([1e11, np.nan])), dict(omegas=np.array([np.inf, 1e11])),
               dict(omegas=np.ones(17)), dict(omegas=om, first=-1, count=3), dict(omegas=om, first=0, count=21),
               dict(omegas=om, first=21, count=0), dict(omegas=om, first=5, count=-1), dict(omegas=np.empty(0))]
        for kw in bad:
            with pytest.raises(fd.Fdtd2dError) as ei:
                b.probe_spectra(**kw)
            assert ei.value.code == E_ARG, kw
        dp = np.zeros(64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        wp = np.ascontiguousarray(np.broadcast_to(om, (3, 2))).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert b._lib.fdtd2d_batch_probe_spectra(b._h, 2, None, 0, 20, dp, dp, None) == E_ARG
        assert b._lib.fdtd2d_batch_probe_spectra(b._h, 2, wp, 0, 20, None, dp, None) == E_ARG
        assert b._lib.fdtd2d_batch_probe_spectra(b._h, 2, wp, 0, 20, dp, None, None) == E_ARG
        assert b._lib.fdtd2d_batch_field_absmax(b._h, 0, None) == E_ARG
        assert b._lib.fdtd2d_batch_field_absmax(b._h, 3, dp) == E_ARG
        with pytest.raises(ValueError, match="Ez"):
            b.field_absmax("Ezx")
        assert np.array_equal(b.read_probes(), traces) and b.probe_samples == 20
        X, peak = b.probe_spectra(om, 20, 0, peak=True)          # an empty range: zeros
        assert not X.any() and not peak.any()
        assert np.array_equal(b.field_absmax(), np.abs(b.download()[0].astype(np.float64)).reshape(3, -1).max(axis=1))
        # a NaN in the field gives NaN for its member alone
        Ez = b.download()[0]
        Ez[1, 7, 9] = np.nan
        b.upload(Ez)
        got = b.field_absmax("Ez")
        assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all()


CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_session as t
out = {"arithmetic": fd.ARITHMETIC}
for boundary in ("mur", "pml"):
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        for where in ("resident", "streamed"):
            got = t.spectra_case(fd, boundary, dtype, where, 40, 64, 16, 137, (50, 87))
            want = t._host_spectra(fd, got["traces"], got["cfg"][4])
            sub = t._host_spectra(fd, got["traces"], got["cfg"][4], 13, 77)
            out[f"{boundary} {name} {where}"] = [
                float(np.abs(got["X"] - want).max() / np.abs(want).max()),
                float(np.abs(got["sub"] - sub).max() / np.abs(sub).max()),
                bool(np.array_equal(got["peak"], np.abs(got["traces"]).max(axis=(1, 2)))),
                bool(all(np.array_equal(a, np.abs(f.astype(np.float64)).reshape(40, -1).max(axis=1))
                         for a, f in zip(got["absmax"], got["fields"])))]
print("SPECTRA_RESULT " + json.dumps(out))
"""


def test_fused_build_probe_spectra_within_the_bound(fd):
    """The fused build's device spectra against the host transform of its own traces, in a process of its own."""
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, FDTD2D_ARITHMETIC="fused"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("SPECTRA_RESULT ")][-1][15:])
    assert res.pop("arithmetic") == "fused" and len(res) == 8
    for k, (err, sub, peak, absmax) in res.items():
        print(f"fused build, {k}: device spectra vs host transform {err:.2e}, sub-range {sub:.2e} of max|X|")
        assert err <= 1e-12 and sub <= 1e-12 and peak and absmax, k


# ---- 7. the permittivity window ---------------------------------------------------------------------------------------

def _collect(b, amps, n):
    b.run(n, amps[:, :n])
    return dict(fields=b.download(), dft=b.read_dft_window(), probes=b.read_probes(), courant=b.courant())


@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_set_eps_window_equals_set_materials_with_the_updated_arrays(fd, boundary, dtype, where):
    R, Cc = adj._shape(boundary, dtype, where)
    B, n, P, F = 6, 300, 8, 4
    rng = np.random.default_rng(R + 17)
    cfg = list(_members(fd, rng, B, R, Cc, dtype, n, P, F))
    win = (R // 2 - 5, Cc // 2 - 4, 9, 11)
    sl = (slice(None), slice(win[0], win[0] + win[2]), slice(win[1], win[1] + win[3]))
    eps = cfg[0].astype(np.float64)
    eps[1] = 4 * fd.EPS0                       # member 1: the window holds the minimum before, not after
    eps[1][sl[1:]] = fd.EPS0
    cfg[0] = eps.astype(dtype)
    eps = cfg[0].astype(np.float64)            # the values the engine holds, so that a fresh engine grades the same PML
    first = fd.EPS0 * (0.5 + 2.5 * rng.random((B, win[2], win[3])))          # member 0 and others: a new minimum
    first[1] = fd.EPS0 * (2 + rng.random(win[2:]))
    second = fd.EPS0 * (1.5 + rng.random((B, win[2], win[3])))
    other = (12, 13, 3, 2)
    third = fd.EPS0 * (0.7 + rng.random((B, 3, 2)))

    def fresh(full):
        c = list(cfg)
        c[0] = full
        return _engine(fd, boundary, dtype, R, Cc, c, n, where)

    full = eps.copy()
    with _engine(fd, boundary, dtype, R, Cc, cfg, n, where) as b:
        before = b.courant()
        for window, new in ((win, first), (win, second), (other, third)):
            launches = b.launches
            assert b.set_eps_window(window, new.astype(np.float32) if window == other else new) is b
            assert b.launches - launches == 1
            full[:, window[0]:window[0] + window[2], window[1]:window[1] + window[3]] = \
                new.astype(np.float32) if window == other else new
            with fresh(full) as ref:
                assert np.array_equal(b.courant(), ref.courant()), window
            if new is first:
                assert not np.array_equal(b.courant(), before)
                assert b.courant()[1] < before[1]              # member 1's minimum rose from eps0 to at least 2 eps0
        assert b.resident == (where == "resident")
        got = _collect(b, cfg[3], n)
    with fresh(full) as ref:
        want = _collect(ref, cfg[3], n)
    for name, a, w in zip(("Ez", "Hx", "Hy"), got["fields"], want["fields"]):
        assert np.array_equal(a, w), name
    assert np.abs(want["fields"][0]).max() > 0 and np.abs(want["dft"]).max() > 0
    assert np.array_equal(got["dft"], want["dft"]) and np.array_equal(got["probes"], want["probes"])
    assert np.array_equal(got["courant"], want["courant"])
    with fresh(eps) as old:                                                  # the window mattered
        assert not np.array_equal(_collect(old, cfg[3], n)["fields"][0], want["fields"][0])


@pytest.mark.parametrize("where", ["resident", "streamed"])
def test_set_eps_window_refusals_leave_the_engine_unchanged(fd, where):
    boundary, dtype = "pml", np.float32
    E_ARG, E_STATE = fd._abi.E_ARG, fd._abi.E_STATE
    R, Cc = adj._shape(boundary, dtype, where)
    B, n = 4, 60
    cfg = _members(fd, np.random.default_rng(2), B, R, Cc, dtype, n, 8, 3)
    ok = np.full((B, 4, 5), 2 * fd.EPS0)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype) as u:
        with pytest.raises(fd.Fdtd2dError) as ei:
            u.set_eps_window((10, 10, 4, 5), ok)                 # before any materials
        assert ei.value.code == E_STATE
        u.set_materials(2 * fd.EPS0, fd.MU0)
        with pytest.raises(fd.Fdtd2dError) as ei:
            u.set_eps_window((10, 10, 4, 5), ok)                 # a uniform batch has no arrays to patch
        assert ei.value.code == E_STATE
    with _engine(fd, boundary, dtype, R, Cc, cfg, n, where) as b, _engine(fd, boundary, dtype, R, Cc, cfg, n, where) as ref:
        b.run(20, cfg[3][:, :20])
        ref.run(20, cfg[3][:, :20])
        courant, launches = b.courant(), b.launches
        bad = [((10, 10, 0, 5), np.empty((B, 0, 5))), ((10, 10, 4, 0), np.empty((B, 4, 0))), ((-1, 10, 4, 5), ok),
               ((10, -2, 4, 5), ok), ((R - 3, 10, 4, 5), ok), ((10, Cc - 4, 4, 5), ok), ((0, 0, 4, 5), ok)]
        for value in (0.0, -fd.EPS0, np.nan, np.inf, 1e-60):     # 1e-60 rounds to zero in float32
            w = ok.copy()
            w[B - 1, 3, 4] = value
            bad.append(((10, 10, 4, 5), w))
        for window, w in bad:
            with pytest.raises(fd.Fdtd2dError) as ei:
                b.set_eps_window(window, w)
            assert ei.value.code == E_ARG, (window, w[-1, -1, -1] if w.size else None)
        assert b._lib.fdtd2d_batch_set_eps_window(b._h, 10, 10, 4, 5, None, fd._abi.F64) == E_ARG
        assert b._lib.fdtd2d_batch_set_eps_window(b._h, 10, 10, 4, 5, ok.ctypes.data, 7) == E_ARG
        with pytest.raises(ValueError, match="shape"):
            b.set_eps_window((10, 10, 4, 5), ok[:, :3])
        assert b.launches == launches and np.array_equal(b.courant(), courant)
        # fields, monitors and the PML are left alone by a window that is accepted
        state = (b.download(), b.download_ezx(), b.read_dft_window(), b.read_probes())
        b.set_eps_window((0, 1, 1, 1), np.full((B, 1, 1), float(cfg[0][0, 0, 1])))
        for a, w in zip(state[0] + state[1:], b.download() + (b.download_ezx(), b.read_dft_window(), b.read_probes())):
            assert np.array_equal(a, w)
        b.set_eps_window((0, 1, 1, 1), cfg[0][:, :1, 1:2])       # back to what it was
        got, want = _collect(b, cfg[3][:, 20:], n - 20), _collect(ref, cfg[3][:, 20:], n - 20)
        for a, w in zip(got["fields"], want["fields"]):
            assert np.array_equal(a, w)
        assert np.array_equal(got["dft"], want["dft"]) and np.array_equal(got["probes"], want["probes"])
        assert np.array_equal(got["courant"], want["courant"])


# ---- 8. the session on the device ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_session_on_the_device_matches_the_helper_and_the_stand_in(fd, boundary, dtype):
    _exact_only(fd)
    B, nsteps = 8, 2500
    eps = cpu.design_eps(count=B)
    r0, c0, nr, nc = cpu.DESIGN
    with ses.session(fd, boundary, dtype, eps=eps, engine=None, nsteps=nsteps) as dev, \
            ses.session(fd, boundary, dtype, eps=eps, nsteps=nsteps) as ref:
        assert isinstance(dev.engine, fd.BatchEngine) and dev.engine.resident
        for it in range(3):
            launches = dev.engine.launches
            J, g, s, info = dev.value_and_grad(cpu.objective)
            assert dev.engine.launches - launches == LAUNCHES_PER_ITERATION
            Jr, gr, sr, infor = ref.value_and_grad(cpu.objective)
            Jh, gh, sh, infoh = cpu.gradient(fd, boundary, dtype, eps=np.array(dev.eps), engine=None, nsteps=nsteps)
            # the traces are the stand-in's bit for bit and both sessions sum them in the same order; the device's
            # sin / cos and NumPy's differ by rounding
            assert np.abs(s - sr).max() <= 1e-12 * np.abs(sr).max() and np.allclose(J, Jr, rtol=1e-12, atol=0)
            assert np.abs(s - sh).max() <= 1e-12 * np.abs(sh).max() and np.allclose(J, Jh, rtol=1e-12, atol=0)
            for m in range(B):
                for name, w in (("stand-in", gr), ("helper", gh)):
                    gmax = np.abs(w[m]).max()
                    assert gmax > 0 and np.abs(g[m] - w[m]).max() <= 1e-9 * gmax, (it, m, name)
            assert np.array_equal(info["residual_forward"], infoh["residual_forward"])     # the same run, exact maxima
            assert np.array_equal(info["residual_forward"], infor["residual_forward"])
            for k in ("residual_forward", "residual_adjoint"):           # see the docstring of test_batch_session_cpu
                assert np.allclose(info[k], infoh[k], rtol=1e-12) and np.allclose(info[k], infor[k], rtol=1e-12), k
            assert info["condition"] == infoh["condition"] and info["channels_shared"] is True
            assert len({g[m].tobytes() for m in range(B)}) == B
            w = ref.eps[:, r0:r0 + nr, c0:c0 + nc] + 0.2 * cpu.EPS0 * gr / np.abs(gr).max(axis=(1, 2), keepdims=True)
            launches = dev.engine.launches
            dev.set_design_eps(np.clip(w, cpu.EPS0, 3 * cpu.EPS0))
            assert dev.engine.launches - launches == 1
            ref.set_design_eps(np.clip(w, cpu.EPS0, 3 * cpu.EPS0))
            assert np.array_equal(dev.eps, ref.eps)


# ---- 9. the loop climbs on the device ----------------------------------------------------------------------------------

def test_a_gradient_ascent_loop_climbs_on_the_device(fd):
    with ses.session(fd, "pml", np.float32, eps=cpu.design_eps(0, 8), engine=None, nsteps=2500) as s:
        assert s.engine.resident
        Js = ses.climb(s)
    print("J per iteration:", np.array2string(Js.T, precision=3))
    assert Js.shape == (6, 8) and np.all(np.diff(Js, axis=0) > 0)
