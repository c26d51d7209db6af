"""CPU-only checks of the standing adjoint session of the batched engine (fdtd2d_batch_design.h, adjoint.py).

The surface: the three design-loop entry points are declared, exported and bound, the Python surface has its shape, and
without a device nothing falls back.

The method: ``AdjointSession`` driven by ``SessionOracle`` -- the oracle-backed stand-in of tests/oracle_batch.py plus
the three new methods restated in NumPy -- against ``batch_eps_gradient`` driven by the plain stand-in, on the
configuration of test_batch_adjoint_cpu.  The only difference between the two is the summation order of the spectra
(the session sums in ascending step order, the helper's host transform as a matrix product does).  Measured with a
sequential-sum transform given to the helper: spectra move by 3.7e-15 / 8.3e-15 of their maximum (PML / Mur), J by
1e-15, the gradient by at most 3.4e-15 of its maximum; the bounds are the project's 1e-12 for DFT sums and 1e-9 of
max|gradient| for gradients.  The residuals of ``info`` are compared with the expression the project uses for them
(tests/test_gpu_batch_adjoint.py: ``np.allclose(..., rtol=1e-12)``, NumPy's default atol of 1e-8 included).  Measured
here: residual_forward is identical (the same run); residual_adjoint, the end-of-run max|Ez| of the adjoint run over its
largest probe sample (1.1e-5 / 1.6e-5 on this configuration), moves by 7.7e-14 (PML) and 5.3e-11 (Mur) of its own value,
which is 8.5e-16 of the run's peak: the remnant field at the end of the run is a difference of much larger terms and
follows the rounding of the weights, so a purely relative 1e-12 would not hold for it."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle_batch import OracleBatch
import test_batch_adjoint_cpu as cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_design.h")
NAMES = ["fdtd2d_batch_field_absmax", "fdtd2d_batch_probe_spectra", "fdtd2d_batch_set_eps_window"]
EPS0 = cpu.EPS0
R0, C0, NR, NC = cpu.DESIGN


class SessionOracle(OracleBatch):
    """OracleBatch plus probe_spectra, field_absmax and set_eps_window with the arithmetic fdtd2d_batch_design.h
    fixes."""

    def probe_spectra(self, omegas, first=0, count=None, peak=False):
        w = np.asarray(omegas, dtype=np.float64)
        w = np.broadcast_to(w, (self.count, w.shape[-1]))
        tr, step0 = self.probes["trace"], self.probes["step0"]
        recorded = min(tr.shape[2], self.step - step0)
        count = recorded - first if count is None else count
        assert 0 <= first and 0 <= count and first + count <= recorded
        re = np.zeros((self.count, tr.shape[1], w.shape[1]))
        im = np.zeros_like(re)
        for n in range(first, first + count):
            t = float(step0 + n + 1) * self.dt
            re = re + tr[:, :, n, None] * np.cos(w * t)[:, None, :]
            im = im + tr[:, :, n, None] * (-np.sin(w * t))[:, None, :]
        out = re + 1j * im
        if not peak:
            return out
        return out, np.abs(tr[:, :, first:first + count]).reshape(self.count, -1).max(axis=1, initial=0.0)

    def field_absmax(self, field="Ez"):
        f = {"Ez": self.Ez, "Hx": self.Hx, "Hy": self.Hy}[field]
        return np.abs(f.astype(np.float64)).reshape(self.count, -1).max(axis=1)

    def set_eps_window(self, window, eps):
        r0, c0, nr, nc = (int(v) for v in window)
        e = np.asarray(eps)
        assert e.shape == (self.count, nr, nc) and (r0, c0) != (0, 0)
        self.eps = self.eps.copy()          # set_materials may have kept a read-only view of the caller's array
        self.eps[:, r0:r0 + nr, c0:c0 + nc] = e.astype(self.dtype)
        return self


class NoBulkReads(SessionOracle):
    """A stand-in whose bulk read-backs are forbidden."""

    def _refuse(self, *a, **k):
        raise AssertionError("a bulk read-back was called")

    read_probes = download = read_dft_window = _refuse

    def hold_dft_window(self):
        self.held = (self.win["re"] + 1j * self.win["im"]).copy()
        return self

    def dft_window_product(self, coef):
        from oracle_batch import window_product
        k = np.asarray(coef, dtype=np.complex128)
        k = np.broadcast_to(k, (self.count, k.shape[-1]))
        cur = self.win["re"] + 1j * self.win["im"]
        return np.stack([window_product(k[b], self.held[b], cur[b]) for b in range(self.count)])


def session(fd, boundary, dtype=np.float64, eps=None, engine=SessionOracle, nsteps=cpu.NSTEPS, **kw):
    eps = cpu.design_eps(count=2) if eps is None else eps
    B = eps.shape[0]
    args = dict(nsteps=nsteps, sources=np.tile(cpu.SOURCE, (B, 1)), probes=cpu.PROBES, omegas=cpu.OMEGAS,
                design=cpu.DESIGN, fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, dtype=dtype, boundary=boundary,
                pml_cells=cpu.LAYER, engine=engine)
    args.update(kw)
    return fd.AdjointSession(eps, **args)


def agree(got, want, members):
    """The session's (J, grad, spectra, info) against the helper's, with the bounds of the module docstring."""
    J, g, s, info = got
    Jw, gw, sw, infow = want
    assert g.shape == gw.shape and g.dtype == np.float64 and s.shape == sw.shape and s.dtype == np.complex128
    for m in range(members):
        gmax = np.abs(gw[m]).max()
        assert gmax > 0 and np.abs(g[m] - gw[m]).max() <= 1e-9 * gmax, m
        assert np.abs(s[m] - sw[m]).max() <= 1e-12 * np.abs(sw[m]).max(), m
    assert np.allclose(J, Jw, rtol=1e-12, atol=0)
    assert sorted(info) == sorted(infow) == ["channels_shared", "condition", "residual_adjoint", "residual_forward"]
    assert info["condition"] == infow["condition"] and info["channels_shared"] == infow["channels_shared"]
    # the forward runs are the same run; the adjoint runs differ by the rounding of their weights (see the docstring)
    assert np.array_equal(info["residual_forward"], infow["residual_forward"])
    for k in ("residual_forward", "residual_adjoint"):
        print(f"{k}: worst relative difference {np.abs(info[k] / infow[k] - 1).max():.2e}")
        assert np.allclose(info[k], infow[k], rtol=1e-12), k


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


# ---- 1. the surface -------------------------------------------------------------------------------------------------

def test_batch_design_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == NAMES
    assert sorted(_abi.BATCH_DESIGN_SIGNATURES) == names
    for path in (os.path.join(_abi.HERE, "libfdtd2d.so"), os.path.join(_abi.HERE, "libfdtd2d_fused.so")):
        lib = ctypes.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared but not exported by {os.path.basename(path)}"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_DESIGN_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_DESIGN_SIGNATURES[n][0]
    # the prototypes, argument for argument
    proto = {n: re.search(rf"\bint\s+{n}\s*\(([^)]*)\)", txt).group(1) for n in names}
    kinds = {"fdtd2d_batch_t *": ctypes.c_void_p, "int": ctypes.c_int, "long long": ctypes.c_longlong,
             "const double *": ctypes.POINTER(ctypes.c_double), "double *": ctypes.POINTER(ctypes.c_double),
             "const void *": ctypes.c_void_p}
    for n, args in proto.items():
        got = []
        for a in args.split(","):
            a = " ".join(a.split())
            kind = re.match(r"(.*?[ *])\w+$", a).group(1).strip()
            got.append(kinds[kind])
        assert got == _abi.BATCH_DESIGN_SIGNATURES[n][1], n


def test_batch_design_constants_collide_with_none():
    pat = r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)"
    mine = dict(re.findall(pat, open(HEADER).read()))
    taken = {}
    for h in ("fdtd2d.h", "fdtd2d_batch_pml.h", "fdtd2d_batch_monitor.h", "fdtd2d_batch_adjoint.h"):
        taken.update(re.findall(pat, open(os.path.join(ROOT, "include", h)).read()))
    assert max(int(v) for k, v in taken.items() if k.startswith("BATCH_INFO")) == 13
    assert max(int(v) for k, v in taken.items() if k.startswith("BATCH_OPT")) == 2
    for k, v in mine.items():
        assert k not in taken and int(v) >= (14 if k.startswith("BATCH_INFO") else 3), k
    assert len({(k[:10], v) for k, v in mine.items()}) == len(mine)


def test_batch_session_python_surface():
    import fdtd2d_amd as fd
    E = fd.BatchEngine
    p = inspect.signature(E.probe_spectra).parameters
    assert list(p) == ["self", "omegas", "first", "count", "peak"]
    assert (p["first"].default, p["count"].default, p["peak"].default) == (0, None, False)
    p = inspect.signature(E.field_absmax).parameters
    assert list(p) == ["self", "field"] and p["field"].default == "Ez"
    assert list(inspect.signature(E.set_eps_window).parameters) == ["self", "window", "eps"]
    p = inspect.signature(fd.AdjointSession.__init__).parameters
    assert list(p) == ["self", "eps", "mu", "nsteps", "sources", "probes", "omegas", "design", "fc", "waveform", "dt",
                       "dx", "dtype", "boundary", "pml_cells", "device", "engine"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k not in ("self", "eps", "mu"))
    want = dict(mu=None, fc=30e9, waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml",
                pml_cells=40, device=0, engine=None)
    assert {k: p[k].default for k in want} == want
    assert list(inspect.signature(fd.AdjointSession.value_and_grad).parameters) == ["self", "objective"]
    assert list(inspect.signature(fd.AdjointSession.set_design_eps).parameters) == ["self", "eps_window"]
    assert "AdjointSession" in fd.__all__ and fd.AdjointSession is fd.adjoint.AdjointSession
    for name in ("probe_spectra", "field_absmax", "set_eps_window"):
        assert callable(getattr(E, name)) and callable(getattr(SessionOracle, name)), name
        assert name not in vars(OracleBatch)
    # batch_eps_gradient is as it was
    p = inspect.signature(fd.batch_eps_gradient).parameters
    assert list(p) == ["eps", "mu", "nsteps", "sources", "probes", "omegas", "design", "objective", "fc", "waveform",
                       "dt", "dx", "dtype", "boundary", "pml_cells", "device", "engine"]


def test_the_package_still_does_not_import_the_oracle():
    for name in ("adjoint.py", "batch.py"):
        src = open(os.path.join(ROOT, "fdtd-2d_amd", name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), name


def test_session_without_a_device_has_no_fallback(fd):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 4, 40, 40, 5e-14, 1e-4, _abi.F32, _abi.BOUNDARY_MUR5, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    with pytest.raises(fd.Fdtd2dError) as ei:
        session(fd, "pml", np.float32, engine=None, nsteps=400)
    assert ei.value.code == _abi.E_NODEVICE


def test_batch_design_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.fdtd2d_batch_probe_spectra(None, 1, dp, 0, 1, dp, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_field_absmax(None, _abi.FIELD_EZ, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_eps_window(None, 1, 1, 2, 2, d.ctypes.data, _abi.F64) == _abi.E_ARG


# ---- 2. the session is the helper -----------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_session_agrees_with_the_helper_before_and_after_a_design_update(fd, boundary):
    eps = cpu.design_eps(count=2)
    want = cpu.gradient(fd, boundary, np.float64, eps=eps)
    with session(fd, boundary, eps=eps) as s:
        assert isinstance(s.engine, SessionOracle)
        got = s.value_and_grad(cpu.objective)
        agree(got, want, 2)
        print(f"{boundary}: spectra {np.abs(got[2] - want[2]).max() / np.abs(want[2]).max():.2e} of their maximum, "
              f"gradient {max(np.abs(got[1][m] - want[1][m]).max() / np.abs(want[1][m]).max() for m in range(2)):.2e}")
        assert np.array_equal(s.eps, eps) and not s.eps.flags.writeable
        new = EPS0 * (1 + 2 * np.random.default_rng(7).random((2, NR, NC)))
        assert s.set_design_eps(new) is s
        eps2 = eps.copy()
        eps2[:, R0:R0 + NR, C0:C0 + NC] = new
        assert np.array_equal(s.eps, eps2) and np.array_equal(eps, cpu.design_eps(count=2))   # its own copy
        want2 = cpu.gradient(fd, boundary, np.float64, eps=eps2)
        assert not np.allclose(want2[1], want[1], rtol=1e-3)
        agree(s.value_and_grad(cpu.objective), want2, 2)
    assert s.engine is None


def test_session_survives_an_exception_from_the_objective(fd):
    eps = cpu.design_eps(count=2)
    with session(fd, "mur", eps=eps, nsteps=600) as s:
        first = s.value_and_grad(cpu.objective)

        def broken(spectra):
            raise KeyError("the user's objective failed")
        with pytest.raises(KeyError):
            s.value_and_grad(broken)
        with pytest.raises(ValueError, match="objective must return"):
            s.value_and_grad(lambda sp: (np.zeros(3), sp))
        again = s.value_and_grad(cpu.objective)
        for a, b in zip(first[:3], again[:3]):
            assert np.array_equal(a, b)


# ---- 3. no bulk read-back ---------------------------------------------------------------------------------------------

def test_session_never_reads_traces_fields_or_windows_back(fd):
    with session(fd, "pml", engine=NoBulkReads, nsteps=600) as s:
        with pytest.raises(AssertionError, match="bulk read-back"):
            s.engine.read_probes()
        a = s.value_and_grad(cpu.objective)
        s.set_design_eps(np.full((2, NR, NC), 2 * EPS0))
        b = s.value_and_grad(cpu.objective)
        assert np.all(np.isfinite(a[1])) and np.all(np.isfinite(b[1])) and not np.array_equal(a[1], b[1])


# ---- 4. a loop climbs ------------------------------------------------------------------------------------------------

def climb(s, iterations=5):
    """J (iterations + 1, B) along eps_window += 0.05 eps0 grad / max|grad|, clipped to [1, 3] eps0."""
    Js = []
    for it in range(iterations + 1):
        J, grad, _, _ = s.value_and_grad(cpu.objective)
        Js.append(J)
        if it < iterations:
            w = s.eps[:, R0:R0 + NR, C0:C0 + NC] + 0.05 * EPS0 * grad / np.abs(grad).max(axis=(1, 2), keepdims=True)
            s.set_design_eps(np.clip(w, EPS0, 3 * EPS0))
    return np.array(Js)


def test_a_gradient_ascent_loop_climbs_at_every_iteration(fd):
    with session(fd, "pml", eps=cpu.design_eps(0, 2), nsteps=2500) as s:
        Js = climb(s)
    print("J per iteration:", np.array2string(Js.T, precision=3))
    assert Js.shape == (6, 2) and np.all(np.diff(Js, axis=0) > 0)
    # the figures of the reference procedure (batch_eps_gradient and the plain stand-in, a fresh engine per iteration)
    assert np.allclose(Js[:, 0], [1.220, 1.312, 1.410, 1.508, 1.602, 1.691], atol=2e-3)
    assert np.allclose(Js[:, 1], [0.904, 0.998, 1.086, 1.175, 1.271, 1.358], atol=2e-3)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs,match", [
    (dict(sources=np.array([[24, 12], [24, 19]])), "member 1: .*forward source"),
    (dict(design=(5, 18, 16, 12), boundary="mur"), "6 cells from every edge"),
    (dict(design=(16, 18, 27, 12), boundary="mur"), "6 cells from every edge"),
    (dict(design=(7, 18, 16, 12)), "8 cells from every edge.*PML"),
    (dict(design=(16, 18, 0, 12)), "empty"),
    (dict(design=(16, 18, 16)), "4 integers"),
    (dict(boundary="none"), "rings down"),
    (dict(omegas=2 * np.pi * np.array([40e9, 40e9 * (1 + 1e-13)])), "member 0: .*condition number"),
    (dict(omegas=np.ones(17)), "1..16"),
    (dict(probes=np.zeros((65, 2), int)), "1..64"),
    (dict(probes=[[20, 38], [20, 38]]), "member 0: .*twice"),
    (dict(probes=[[48, 3]]), "in the 48x48 grid"),
    (dict(pml_cells=23), "does not fit"),
    (dict(nsteps=0), "nsteps"),
    (dict(mu=np.ones((2, 3, 3))), "mu must be a scalar"),
    (dict(dt=4e-12), "Courant"),
    (dict(sources=np.zeros((3, 2), int)), "sources must have shape"),
])
def test_session_refuses_bad_arguments_with_the_helpers_messages(fd, kwargs, match):
    def boom(*a, **k):
        raise AssertionError("an engine was created")
    args = dict(nsteps=400, sources=np.array([[24, 12], [24, 12]]), probes=cpu.PROBES, omegas=cpu.OMEGAS,
                design=cpu.DESIGN, fc=cpu.FC, dt=cpu.DT, dx=cpu.DX, boundary="pml", pml_cells=cpu.LAYER, engine=boom)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match) as helper:
        fd.batch_eps_gradient(cpu.design_eps(count=2), objective=cpu.objective, **args)
    with pytest.raises(ValueError, match=match) as sess:
        fd.AdjointSession(cpu.design_eps(count=2), **args)
    assert str(sess.value) == str(helper.value)


def test_set_design_eps_refuses_and_leaves_the_state(fd):
    eps = cpu.design_eps(count=2)
    with session(fd, "mur", eps=eps, nsteps=600) as s:
        before = s.value_and_grad(cpu.objective)
        good = np.full((2, NR, NC), 2 * EPS0)
        with pytest.raises(ValueError, match=r"shape \(2, 16, 12\)"):
            s.set_design_eps(good[:, :-1])
        with pytest.raises(ValueError, match=r"shape \(2, 16, 12\)"):
            s.set_design_eps(good[:1])
        for bad in (0.0, -EPS0, np.nan, np.inf):
            w = good.copy()
            w[1, 3, 4] = bad
            with pytest.raises(ValueError, match=r"positive and finite: members \[1\]"):
                s.set_design_eps(w)
        w = good.copy()
        w[0, 2, 2] = 0.1 * EPS0              # Courant number (1 / sqrt(0.1 eps0 mu0) dt) / dx = 1.52
        with pytest.raises(ValueError, match=r"Courant stability condition not met: members \[0\]"):
            s.set_design_eps(w)
        assert np.array_equal(s.eps, eps) and np.array_equal(s.engine.eps, eps)
        after = s.value_and_grad(cpu.objective)
        for a, b in zip(before[:3], after[:3]):
            assert np.array_equal(a, b)
    with pytest.raises(RuntimeError, match="closed"):
        s.value_and_grad(cpu.objective)
