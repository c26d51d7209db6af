"""GPU: line sources on the flux lines of Bloch batches and the adjoint gradients of flux
(fdtd2d_batch_bloch_flux_adjoint.h, kernels_batch_bloch_flux_adjoint.hpp, adjoint.py) against the stand-in of
tests/oracle_batch_bloch_flux_adjoint.py.

Shapes, members, lines and placements are those of tests/test_gpu_batch_bloch_flux.py: three members with phi = 0.4, 1.3,
-2.2, 320 steps from rest, 40x17 float32 / float64 (192 threads, 4 cells per thread), 90x33 float32 (768 threads, sums
that do not fit in LDS) and 40x17 float32 with the pole; resident with the sums in LDS, resident with them in global
memory, streamed, and 7 steps per launch on 40x17f32.  The lines: a whole-period row, a row in the layer, a column at
column 0 over all rows (the seam term; rows 0 and R-1, whose Hy[R-1] takes nothing), a column at C-2 (whose own H value
is the one the seam term of column 0 lands on), the first row line crossing both column lines.  The sources: K = 6
channels of unit normal noise per member, complex we of order 0.3 and wh of order 1e-3, beside the complex rectangle
source; every run is made with conjugate False and True.  A window DFT and probes run beside them.

Tolerances.  Fields and image column are bit-identical to the stand-in (exact build).  The raw sums differ only by the
device's sin and cos: 1e-12 max|stand-in|; P: 8e-12 dx sum (|Er| + |Ei|) (|Hr| + |Hi|), the bound of
test_gpu_batch_bloch_flux.py.  The device weights against the host path: 1e-12 max|weight| (the same float64 products,
summed in another order).  The gradients against the stand-in: 1e-9 max|gradient|, by the reasoning of
test_gpu_batch_flux_adjoint.py (two windows at 1e-12 each and a channel system whose condition number is below 10 leave
three orders of margin).  Measured on an MI355X: 1.9e-16 for a raw array, 2.2e-16 of the scale for P, 2.3e-16 for the
weights, 2.3e-15 for the gradients; every test prints them again."""
import ctypes

import numpy as np
import pytest

from oracle_batch_bloch_flux_adjoint import BlochLineSourceOracle
from test_gpu_batch_bloch_flux import B, CASES, DT, DX, EVERY, LAYER, NSTEPS, PHI, SPL_CASE, _cfg, _setup

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
K = 6
MODES = ("lds", "global", "streamed")
PARTS = ("Er", "Hr", "Ei", "Hi")
INFO_LINE_SOURCES = 23


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the stand-in restates the exact build's arithmetic")


def _sources(cfg, real=False):
    """(we, wh, channels): (B, cells, K) complex weights of order 0.3 and 1e-3, (B, K, NSTEPS) channels."""
    cells = sum(l[3] for l in cfg["lines"])
    rng = np.random.default_rng(23)
    cx = (lambda: rng.standard_normal((B, cells, K))) if real else \
        (lambda: rng.standard_normal((B, cells, K)) + 1j * rng.standard_normal((B, cells, K)))
    return 0.3 * cx(), 1e-3 * cx(), rng.standard_normal((B, K, NSTEPS))


def _read(b):
    (er, hr), (ei, hi) = b.read_bloch_flux_parts()
    return dict(Er=er, Hr=hr, Ei=ei, Hi=hi, P=b.flux())


def _drive(b, cfg, conj):
    """The same calls on a BatchEngine and on the stand-in."""
    _setup(b, cfg)
    b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2).set_probes(cfg["probes"], NSTEPS)
    b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
    we, wh, chan = _sources(cfg)
    b.set_bloch_flux_line_sources(we, wh)
    before = getattr(b, "launches", 0)
    b.run_bloch_channels(NSTEPS, cfg["amps"], chan, conjugate=conj)
    out = dict(fields=tuple(b.download()) + (b.download_ezx(),), dft=b.read_dft_window(), probes=b.read_probes(),
               launches=getattr(b, "launches", 0) - before)
    out.update(_read(b))
    return out


_refs, _runs = {}, {}


def _stand_in(case, conj):
    if (case, conj) not in _refs:
        cfg = _cfg(case)
        ref = BlochLineSourceOracle(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic")
        _refs[case, conj] = _drive(ref, cfg, conj)
        _refs[case, conj]["scale"] = ref.flux_scale()
    return _refs[case, conj]


def _device(fd, case, mode, conj):
    if (case, mode, conj) not in _runs:
        cfg = _cfg(case)
        with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic") as b:
            b.set_option(resident=0 if mode == "streamed" else None, steps_per_launch=7 if mode == "spl7" else None)
            b.set_flux_lds(mode != "global")
            out = _drive(b, cfg, conj)
            out["in_lds"] = b.flux_lines_in_lds
            assert b.resident == (mode != "streamed") and b.info(INFO_LINE_SOURCES) == K
            assert b.dispersive == (cfg["pole"] is not None)
            # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert out["launches"] == (2 * NSTEPS if mode == "streamed" else -(-NSTEPS // 7) if mode == "spl7" else 1)
        _runs[case, mode, conj] = out
    return _runs[case, mode, conj]


def _modes(case):
    return MODES + (("spl7",) if case == SPL_CASE else ())


ALL = [(c, m, j) for c in CASES for m in _modes(c) for j in (False, True)]


# ---- 1. against the stand-in, on every path, with either rotation --------------------------------------------------------

@pytest.mark.parametrize("case,mode,conj", ALL, ids=[f"{c}-{m}-{'conj' if j else 'plain'}" for c, m, j in ALL])
def test_fields_sums_and_flux_match_the_stand_in(fd, case, mode, conj):
    _exact_only(fd)
    got, want = _device(fd, case, mode, conj), _stand_in(case, conj)
    for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx"), got["fields"], want["fields"]):
        assert a.dtype == w.dtype and np.abs(w.imag).max() > 0 and np.array_equal(a, w), name     # the image column too
    assert np.array_equal(got["probes"], want["probes"])
    assert np.abs(got["dft"] - want["dft"]).max() <= 1e-12 * np.abs(want["dft"]).max()
    for name in PARTS:
        for part, pick in (("re", np.real), ("im", np.imag)):       # the eight raw arrays
            err, top = np.abs(pick(got[name]) - pick(want[name])).max(), np.abs(pick(want[name])).max()
            print(f"{case} {mode} conj={conj} {name} {part}: max error {err:.3e}, max |stand-in| {top:.3e}, "
                  f"ratio {err / top:.2e}")
            assert top > 0 and err <= 1e-12 * top, (name, part)
    err = np.abs(got["P"] - want["P"])
    print(f"{case} {mode} conj={conj} P: worst error over its scale {np.max(err / want['scale']):.2e}")
    assert np.all(want["scale"] > 0) and np.all(err <= 8e-12 * want["scale"])


def test_the_two_rotations_give_different_runs(fd):
    a, b = _device(fd, "40x17f32", "lds", False), _device(fd, "40x17f32", "lds", True)
    assert not np.array_equal(a["fields"][0], b["fields"][0]) and not np.array_equal(a["Hr"], b["Hr"])


# ---- 2. whatever the path, the placement and the launch split ----------------------------------------------------------

@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_results_do_not_depend_on_path_placement_or_split(fd, case, conj):
    first = _device(fd, case, "lds", conj)
    assert first["in_lds"] == (case != "90x33f32")
    for mode in _modes(case)[1:]:
        other = _device(fd, case, mode, conj)
        assert not other["in_lds"] or mode == "spl7"
        for k in PARTS + ("P", "dft", "probes"):
            assert np.array_equal(first[k], other[k]), (mode, k)
        for a, b in zip(first["fields"], other["fields"]):
            assert np.array_equal(a, b), mode


# ---- 3. phi = 0 with real weights is the real line source ---------------------------------------------------------------

@pytest.mark.parametrize("mode", ["lds", "streamed"])
@pytest.mark.parametrize("case", ["40x17f32", "40x17f64"])
def test_zero_phase_and_real_weights_are_the_periodic_engine(fd, case, mode):
    cfg = _cfg(case)
    we, wh, chan = _sources(cfg, real=True)
    amps, om = np.ascontiguousarray(cfg["amps"].real), np.abs(cfg["omegas"])
    out = []
    for bloch in (True, False):
        with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic") as b:
            b.set_option(resident=0 if mode == "streamed" else None)
            b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
            c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
            b.set_pml(LAYER, courant00=np.array(c00))
            if bloch:
                b.set_bloch_phase(0.0)
                b.set_bloch_flux_lines(cfg["lines"], om, every=EVERY).set_bloch_flux_line_sources(we, wh)
                b.run_bloch_channels(NSTEPS, amps, chan)
            else:
                b.set_flux_lines(cfg["lines"], om, every=EVERY).set_flux_line_sources(we, wh)
                b.run(NSTEPS, amps, chan)
            out.append(tuple(b.download()) + b.read_flux_lines(raw=True) + (b.flux(),))
    for name, z, r in zip(("Ez", "Hx", "Hy", "E sums", "H sums", "P"), *out):
        if name in ("Ez", "Hx", "Hy"):
            assert np.iscomplexobj(z) and not np.any(z.imag) and np.array_equal(z.real, r) and np.abs(r).max() > 0, name
        elif name == "P":
            assert np.abs(z - r).max() <= 1e-12 * np.abs(r).max()
        else:
            assert np.array_equal(z, r), name     # the real part's sums; the imaginary part's are zero


# ---- 4. state --------------------------------------------------------------------------------------------------------------

def _engine(fd, case="40x17f32"):
    cfg = _cfg(case)
    b = fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic")
    return _setup(b, cfg), cfg


def _state(b):
    return tuple(b.download()) + tuple(_read(b)[k] for k in PARTS)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_sources_are_silent_under_run_kept_and_dropped_as_documented(fd):
    b, cfg = _engine(fd)
    pole = _cfg("40x17pole")["pole"]
    we, wh, chan = _sources(cfg)
    n = 40
    with b:
        b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(n, cfg["amps"][:, :n])
        never = _state(b)                                     # a run that never had sources
        b.reset()
        b.set_bloch_flux_line_sources(we, wh)
        assert b.info(INFO_LINE_SOURCES) == K
        b.run(n, cfg["amps"][:, :n])
        assert _same(never, _state(b))                        # silent under run
        b.reset()
        assert b.info(INFO_LINE_SOURCES) == K                 # kept across reset
        b.run_bloch_channels(n, cfg["amps"][:, :n], chan[:, :, :n])
        driven = _state(b)
        assert not np.array_equal(driven[0], never[0])
        b.set_bloch_phase(PHI[::-1].copy())                   # kept across a new phase
        b.set_bloch_dispersion(*pole)                         # and across the pole, both ways
        assert b.info(INFO_LINE_SOURCES) == K and b.dispersive
        b.reset()
        b.run_bloch_channels(n, cfg["amps"][:, :n], chan[:, :, :n])           # with the pole the sources still drive
        assert not np.array_equal(_state(b)[0], driven[0])
        b.set_bloch_dispersion(None)
        b.set_bloch_phase(PHI)
        assert b.info(INFO_LINE_SOURCES) == K
        got = b.read_bloch_flux_line_sources()
        assert np.array_equal(got[0], we) and np.array_equal(got[1], wh)
        b.reset()
        b.run_bloch_channels(n, cfg["amps"][:, :n], chan[:, :, :n])
        assert _same(driven, _state(b))                       # the same sources, the same run
        b.set_bloch_flux_line_sources(None, None)             # removal: the plain flux kernels again
        assert b.info(INFO_LINE_SOURCES) == 0 and b.info(21) == len(cfg["lines"])
        b.reset()
        b.run(n, cfg["amps"][:, :n])
        assert _same(never, _state(b))
        b.set_bloch_flux_line_sources(we.real, None)          # a real array: the imaginary part is absent
        got = b.read_bloch_flux_line_sources()
        assert np.array_equal(got[0], we.real) and not np.any(got[1])
        b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)      # new lines drop the sources
        assert b.info(INFO_LINE_SOURCES) == 0
        b.set_bloch_flux_line_sources(we, wh)
        b.set_bloch_flux_lines(None, None)                    # and so does their removal
        assert b.info(INFO_LINE_SOURCES) == 0 and b.info(21) == 0


def test_return_codes_and_the_refusals_that_stay(fd):
    from fdtd2d_amd.api import EPS0, MU0
    b, cfg = _engine(fd)
    we, wh, chan = _sources(cfg)
    lib, dp = fd._abi.load(), ctypes.POINTER(ctypes.c_double)
    cells = we.shape[1]
    ptr = lambda a: a.ctypes.data_as(dp)
    wr = np.ascontiguousarray(we.real)
    ch4 = np.zeros((K, 4))
    with b:
        b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2)
        assert lib.fdtd2d_batch_set_bloch_flux_line_sources(b._h, K, ptr(wr), None, None, None) == E_STATE    # no lines
        b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        # without line sources the lines keep refusing the channels and the held window
        assert lib.fdtd2d_batch_run_bloch_channels(b._h, 4, None, None, ptr(ch4), 0, 0) == E_STATE
        assert lib.fdtd2d_batch_hold_bloch_window(b._h) == E_STATE
        assert lib.fdtd2d_batch_read_bloch_flux_line_sources(b._h, *(ptr(np.empty(B * cells * K)),) * 4) == E_STATE
        b.set_bloch_flux_line_sources(np.zeros((cells, K)), None)             # all-zero weights count
        b.run_bloch_channels(4, None, ch4)
        b.run_bloch_channels(4, None, ch4, conjugate=True)
        b.hold_bloch_window()
        assert b.bloch_window_product(np.ones(len(cfg["win_omegas"]))).shape == (B, cfg["window"][2], cfg["window"][3])
        # bad arguments leave the previous sources in place
        assert lib.fdtd2d_batch_set_bloch_flux_line_sources(b._h, 33, ptr(wr), None, None, None) == E_ARG
        assert lib.fdtd2d_batch_set_bloch_flux_line_sources(b._h, -1, ptr(wr), None, None, None) == E_ARG
        bad = wr.copy()
        bad[1, 3, 2] = np.inf
        for slot in range(4):
            args = [None] * 4
            args[slot] = ptr(bad)
            assert lib.fdtd2d_batch_set_bloch_flux_line_sources(b._h, K, *args) == E_ARG
        assert b.info(INFO_LINE_SOURCES) == K and not np.any(b.read_bloch_flux_line_sources()[0])
        assert lib.fdtd2d_batch_bloch_flux_line_weights(b._h, None, ptr(wr), 0, None, None) == E_ARG
        # what stays refused: Bloch point sources beside the lines, new lines beside a held window, the real entries
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.set_bloch_point_sources(np.array([[20, 3]]), np.ones((1, K)))
        assert ei.value.code == E_STATE
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"])
        assert ei.value.code == E_STATE
        assert lib.fdtd2d_batch_set_flux_line_sources(b._h, K, ptr(wr), None) == E_STATE
        assert lib.fdtd2d_batch_read_flux_line_sources(b._h, ptr(np.empty(B * cells * K)), ptr(np.empty(B * cells * K))) \
            == E_STATE
        assert lib.fdtd2d_batch_flux_line_weights(b._h, ptr(wr), ptr(wr), 0, None, None) == E_STATE
        # hold_bloch_window keeps refusing the pole; the sources go on driving with it
        b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2)          # drops the held window
        b.set_bloch_dispersion(*_cfg("40x17pole")["pole"])
        assert lib.fdtd2d_batch_hold_bloch_window(b._h) == E_STATE
        b.run_bloch_channels(4, None, ch4)
        b.set_bloch_dispersion(None)
        b.set_bloch_flux_line_sources(we, wh)                                 # the engine is still usable
        b.reset()
        b.run_bloch_channels(20, cfg["amps"][:, :20], chan[:, :, :20])
        assert np.abs(b.flux()).max() > 0
    # batches that carry no Bloch lines
    for boundary in ("mur", "lattice", "periodic"):
        with fd.BatchEngine(2, 40, 17, DT, DX, boundary=boundary) as e:
            e.set_materials(np.full((2, 40, 17), EPS0), np.full((2, 40, 17), MU0))
            w = np.zeros(2 * 8 * 2)
            assert lib.fdtd2d_batch_set_bloch_flux_line_sources(e._h, 2, ptr(w), None, None, None) == E_STATE, boundary
            assert lib.fdtd2d_batch_bloch_flux_line_weights(e._h, ptr(w), ptr(w), 0, None, None) == E_STATE, boundary
            assert e.info(INFO_LINE_SOURCES) == 0
            with pytest.raises(fd.Fdtd2dError) as ei:
                e.set_bloch_flux_line_sources(np.zeros((8, 2)), None)
            assert ei.value.code == E_STATE


# ---- 5. the weights kernel ---------------------------------------------------------------------------------------------------

def test_device_weights_equal_the_host_path(fd):
    from fdtd2d_amd.adjoint import bloch_flux_adjoint_weights
    b, cfg = _engine(fd, "40x17f64")
    rng = np.random.default_rng(5)
    F, N = cfg["omegas"].shape[1], len(cfg["lines"])
    with b:
        b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(120, cfg["amps"][:, :120])
        E, H = b.read_flux_lines(raw=True)
        cells = E.shape[2]
        dJdP, solve = rng.standard_normal((B, N, F)), rng.standard_normal((B, 2 * F, 2 * F))
        se, sh = 1 + rng.random((B, cells)), -(1 + rng.random((B, cells)))
        for scales in ((se, sh), (None, None)):
            for s in (solve, solve[0]):
                before = b.launches
                b.bloch_flux_adjoint_sources(dJdP, s, *scales)
                assert b.launches == before + 1 and b.info(INFO_LINE_SOURCES) == 2 * F
                got = b.read_bloch_flux_line_sources()
                want = bloch_flux_adjoint_weights(E, H, dJdP, cfg["lines"], cfg["omegas"], DT, DX, s, *scales)
                for g, w in zip(got, want):
                    err = np.abs(g.real - w).max() / np.abs(w).max()
                    print(f"device weights vs host path, per-member solve {s.ndim == 3}: {err:.2e} of max|weight|")
                    assert g.shape == w.shape == (B, cells, 2 * F) and not np.any(g.imag) and err <= 1e-12


# ---- 6. the gradients ----------------------------------------------------------------------------------------------------------

G_R, G_C, G_L, G_N, G_DT = 48, 17, 6, 800, 2e-13      # 160 ps: the three frequencies make a well-conditioned system
G_LINES = [("row", 38, 0, 16), ("row", 9, 0, 16), ("col", 0, 30, 6)]
G_OMEGAS = 2 * np.pi * np.array([45e9, 60e9, 80e9])
G_DESIGN = (18, 2, 10, 12)
G_SOURCE = (13, 0, 1, 16)
G_PHI = np.array([0.9, -2.2])
M1 = 15                               # the order m = -1 in np.fft.fftfreq order


def _g_materials():
    from fdtd2d_amd.api import EPS0
    rng = np.random.default_rng(8)
    r0, c0, nr, nc = G_DESIGN
    eps = np.full((2, G_R, G_C), EPS0)
    eps[:, r0:r0 + nr, c0:c0 + nc] = EPS0 * (1 + 2 * rng.random((2, nr, nc)))
    sigma = np.zeros((2, G_R, G_C))
    sigma[:, r0:r0 + nr, c0:c0 + nc] = 0.2 + 0.5 * rng.random((2, nr, nc))
    return eps, sigma


def _g_args(engine):
    return dict(bloch_phase=G_PHI, source_weights="ramp", nsteps=G_N, sources=np.tile(G_SOURCE, (2, 1)),
                flux_lines=G_LINES, omegas=G_OMEGAS, design=G_DESIGN, fc=60e9, dt=G_DT, dx=DX, dtype=np.float64,
                pml_cells=G_L, engine=engine)


def _o_quadratic(P):
    w = np.array([1.0, -2.0, 0.5])[None, None, :] * np.array([1.0, 0.5, -1.5])[None, :, None]
    return (w * P * P).sum(axis=(1, 2)), 2 * w * P


def _o_orders(P, Pm):
    g = np.zeros_like(Pm)
    g[:, :, M1] = 1.0
    return Pm[:, :, M1].sum(axis=1) + 0.5 * P[:, 1, :].sum(axis=1), 0.5 * (np.arange(3) == 1)[None, :, None] * np.ones_like(P), g


@pytest.mark.parametrize("name", ["quadratic", "orders"])
def test_gradient_helper_and_session_agree_with_the_stand_in(fd, name):
    _exact_only(fd)
    eps, sigma = _g_materials()
    objective, kw = (_o_quadratic, {}) if name == "quadratic" else (_o_orders, dict(orders_line=0))
    want = fd.batch_bloch_flux_gradient(eps, sigma, objective=objective, **_g_args(BlochLineSourceOracle), **kw)
    got = fd.batch_bloch_flux_gradient(eps, sigma, objective=objective, **_g_args(None), **kw)
    with fd.BlochFluxAdjointSession(eps, sigma, **{k: v for k, v in _g_args(None).items()}, **kw) as s:
        before = s.engine.launches
        J, grad, P, info = s.value_and_grad(objective)
        launches = s.engine.launches - before
        gs = s.sigma_gradient()
    assert want[4]["condition"] < 10 and np.abs(want[1]).max() > 0 and np.abs(want[2]).max() > 0
    for label, g_eps, g_sigma, JJ in (("helper", got[1], got[2], got[0]), ("session", grad, gs, J)):
        for what, a, w in (("eps", g_eps, want[1]), ("sigma", g_sigma, want[2])):
            err = np.abs(a - w).max() / np.abs(w).max()
            print(f"{name} {label} d/d{what}: device vs stand-in, worst / max|gradient| = {err:.2e}")
            assert err <= 1e-9
        assert np.allclose(JJ, want[0], rtol=1e-9, atol=0)
    assert np.abs(P - want[3]).max() <= 1e-9 * np.abs(want[3]).max()
    print(f"{name}: {launches} launches per session iteration")
    assert launches > 0
