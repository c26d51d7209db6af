"""GPU: flux lines on PML and periodic batches (fdtd2d_batch_flux.h, kernels_batch_flux.hpp) against the stand-in of
tests/oracle_batch_flux.py.

Three members that differ in eps, sources and frequencies, 320 steps from rest, on the smallest shapes at which each code
path can still go wrong: float32 periodic 40x17 (4 cells per thread) and 150x33 (8 per thread), float64 periodic 40x17,
"pml" 40x40 with a 6-cell layer, lossless (the batch then runs the lossy kernels with ca = 1) and with a conductivity
patch, and both boundaries with a pole.  Every shape runs resident with the sums in LDS, resident with them in global
memory (FDTD2D_BATCH_OPT_FLUX_LDS 0) and streamed; one also with 7 steps per launch, so that the sums cross launches.
The lines are set after 50 steps and sample every third step: a whole-period (or whole-width) row line, a row line inside
the layer, a column line at column 0 of the periodic members (the cyclic neighbour; column 1 and the whole height in the
box), a column line at C-2, and the first row line crosses both column lines (one cell on two lines).

Tolerances.  The fields are bit-identical to the stand-in's (exact build), so the sums differ only by the device's sin
and cos against NumPy's: 1e-12 max|stand-in| per array, as for the window DFT.  The flux is a sum of products of two such
factors: 4e-12 dx sum|E||H| per line (two factors at 1e-12 each, a margin of 2)."""
import ctypes

import numpy as np
import pytest

from oracle_batch_flux import flux_oracle_for

pytestmark = pytest.mark.gpu

DT, DX, LDS_LIMIT = 5e-14, 1e-4, 163840
E_ARG, E_STATE = -1, -4
B, NSTEPS, STEP0, EVERY, LAYER = 3, 320, 50, 3, 6
# case: (boundary, rows, cols, dtype, conductivity, pole)
CASES = {"per40x17f32": ("periodic", 40, 17, np.float32, False, False),
         "per150x33f32": ("periodic", 150, 33, np.float32, False, False),
         "per40x17f64": ("periodic", 40, 17, np.float64, False, False),
         "pml40x40": ("pml", 40, 40, np.float32, False, False),
         "pml40x40sigma": ("pml", 40, 40, np.float32, True, False),
         "pml40x40pole": ("pml", 40, 40, np.float32, False, True),
         "per40x17pole": ("periodic", 40, 17, np.float32, False, True)}
MODES = ("lds", "global", "streamed")
SPL_CASE = "per40x17f32"


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the stand-in restates the exact build's arithmetic")


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _mid(R):
    """The row of the first line; the sources lie within 5 rows of it, so that 320 steps reach the layer line."""
    return min(R // 2, 20)


def _lines(boundary, R, C):
    mid = _mid(R)
    if boundary == "periodic":
        return [("row", mid, 0, C - 1), ("row", 3, 2, 5), ("col", 0, 4, R - 10), ("col", C - 2, mid - 6, 12)]
    return [("row", mid, 0, C), ("row", 3, 8, 20), ("col", 1, 0, R), ("col", C - 2, mid - 6, 12)]


def _cfg(case):
    from fdtd2d_amd.api import EPS0, MU0, ricker_amplitude
    boundary, R, C, dtype, sigma, pole = CASES[case]
    rng = np.random.default_rng(11)
    mid, box = _mid(R), boundary == "pml"        # a box's sources keep out of its column layer
    cfg = dict(case=case, boundary=boundary, R=R, C=C, dtype=dtype,
               eps=(EPS0 * (1 + 2 * rng.random((B, R, C)))).astype(dtype),
               mu=(MU0 * (1 + 0.5 * rng.random((B, R, C)))).astype(dtype),
               rects=np.array([[mid - 5 + m, ((8, 12, C - 12) if box else (0, 2, C - 4))[m], 1,
                                ((C - 20, 3, 2) if box else (C - 1, 3, 2))[m]] for m in range(B)]),
               amps=np.stack([[ricker_amplitude(k * DT, 60e9 * (1 + 0.1 * m)) for k in range(NSTEPS)]
                              for m in range(B)]),
               omegas=2 * np.pi * np.array([[40e9, 60e9, 85e9], [35e9, 55e9, 75e9], [45e9, 65e9, 90e9]]),
               win_omegas=2 * np.pi * np.array([50e9, 70e9]), window=(mid - 2, 1, 5, 6),
               probes=np.array([[mid, 0], [mid + 3, C - 2], [4, 5]]), lines=_lines(boundary, R, C),
               sigma=None, pole=None)
    if sigma:
        s = np.zeros((B, R, C))
        s[:, 24:28, 12:25] = 5.0 * (1 + rng.random((B, 4, 13)))
        cfg["sigma"] = s
    if pole:
        wp2 = np.zeros((B, R, C))
        wp2[:, 25:30, (slice(0, C) if boundary == "periodic" else slice(10, 30))] = (2 * np.pi * 70e9) ** 2
        cfg["pole"] = (wp2, np.array([1e11, 0.0, 5e10]), 2 * np.pi * np.array([0.0, 50e9, 60e9]))
    return cfg


def _drive(b, cfg, lines=True, splits=None):
    """The same calls on a BatchEngine and on the stand-in: 50 steps, then the lines, then the rest."""
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
    b.set_pml(LAYER, courant00=np.array(c00))
    if cfg["sigma"] is not None:
        b.set_conductivity(cfg["sigma"])
    if cfg["pole"] is not None:
        b.set_dispersion(*cfg["pole"])
    b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2).set_probes(cfg["probes"], NSTEPS)
    done, launches = 0, 0
    for k in splits or (STEP0, NSTEPS - STEP0):
        if done == STEP0 and lines:
            b.set_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        before = getattr(b, "launches", 0)
        b.run(k, cfg["amps"][:, done:done + k])
        launches += getattr(b, "launches", 0) - before
        done += k
    assert done == NSTEPS
    out = dict(fields=tuple(b.download()), dft=b.read_dft_window(), probes=b.read_probes(), launches=launches)
    if lines:
        out["E"], out["H"] = b.read_flux_lines(raw=True)
        out["P"] = b.flux()
    return out


_refs, _runs = {}, {}


def _stand_in(case):
    if case not in _refs:
        cfg = _cfg(case)
        ref = flux_oracle_for(cfg["boundary"], cfg["pole"] is not None)(B, cfg["R"], cfg["C"], DT, DX,
                                                                       dtype=cfg["dtype"], boundary=cfg["boundary"])
        _refs[case] = _drive(ref, cfg)
        _refs[case]["scale"] = ref.flux_scale()
    return _refs[case]


def _expect_capacity(b, cfg, lines, lds_allowed, never):
    """The capacity rule, restated: seven arrays (ten with a pole; without lines a lossless box has six), the 4R + 4C
    factors, the window's phasor table and the lines' behind it, then the window's accumulators and the lines' sums when
    they fit."""
    esz, R, C = b.dtype.itemsize, b.rows, b.cols
    lossless_box = cfg["boundary"] == "pml" and cfg["sigma"] is None and cfg["pole"] is None
    arrays = 10 if cfg["pole"] is not None else 6 if lossless_box and not lines else 7
    seg = _seg(R * C, esz)
    fields = arrays * seg + _seg(4 * R, esz) + _seg(4 * C, esz)
    nf, nff = len(cfg["win_omegas"]), cfg["omegas"].shape[1] if lines else 0
    cells = sum(l[3] for l in cfg["lines"]) if lines else 0
    table, wacc, facc = 16 * nf + 16 * nff, 16 * nf * cfg["window"][2] * cfg["window"][3], 32 * nff * cells
    assert fields + table + wacc + facc <= LDS_LIMIT          # every case fits: the placement is the option's alone
    in_lds = lines and lds_allowed
    assert b.lds_bytes == fields + table + wacc + (facc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - (fields - arrays * seg) - table) // arrays // 16 * 16 // esz
    assert b.resident == (not never)
    assert b.flux_lines_in_lds == bool(in_lds and not never)
    assert b.info(21) == (len(cfg["lines"]) if lines else 0)
    assert not b.lossy or cfg["sigma"] is not None            # the conductivity the lines bring is not the user's


def _device(fd, case, mode):
    """mode: "lds", "global", "streamed", "spl7" (resident, 7 steps per launch) or "nolines" (resident)."""
    if (case, mode) not in _runs:
        cfg = _cfg(case)
        lines = mode != "nolines"
        with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"]) as b:
            b.set_option(resident=0 if mode == "streamed" else None, steps_per_launch=7 if mode == "spl7" else None)
            b.set_flux_lds(mode != "global")
            out = _drive(b, cfg, lines=lines)
            _expect_capacity(b, cfg, lines, mode != "global", mode == "streamed")
            # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            spl = 7 if mode == "spl7" else NSTEPS
            want = 2 * NSTEPS if mode == "streamed" else -(-STEP0 // spl) + -(-(NSTEPS - STEP0) // spl)
            assert out["launches"] == want
        _runs[case, mode] = out
    return _runs[case, mode]


def _modes(case):
    return MODES + (("spl7",) if case == SPL_CASE else ())


ALL = [(c, m) for c in CASES for m in _modes(c)]


# ---- 1. against the stand-in, on every path ------------------------------------------------------------------------

@pytest.mark.parametrize("case,mode", ALL, ids=[f"{c}-{m}" for c, m in ALL])
def test_sums_and_flux_match_the_stand_in(fd, case, mode):
    _exact_only(fd)
    got, want = _device(fd, case, mode), _stand_in(case)
    for name, a, w in zip(("Ez", "Hx", "Hy"), got["fields"], want["fields"]):
        assert a.dtype == w.dtype and np.array_equal(a, w), name
    for name in ("E", "H"):
        err, top = np.abs(got[name] - want[name]).max(), np.abs(want[name]).max()
        print(f"{case} {mode} {name}: max error {err:.3e}, max |stand-in| {top:.3e}, ratio {err / top:.2e}")
        assert top > 0 and err <= 1e-12 * top, name
    err = np.abs(got["P"] - want["P"])
    print(f"{case} {mode} P: worst error over its scale {np.max(err / want['scale']):.2e}")
    assert np.all(want["scale"] > 0) and np.all(err <= 4e-12 * want["scale"])
    # the crossing cell: one Ez on two lines
    n0, at = want["E"].shape[2], _cfg(case)["lines"]
    col, row = at[2][1], at[0][1]
    assert n0 == sum(l[3] for l in at)
    assert np.array_equal(got["E"][:, :, col - at[0][2]], got["E"][:, :, at[0][3] + at[1][3] + row - at[2][2]])


# ---- 2. whatever the path, the placement and the launch split ----------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_results_do_not_depend_on_path_placement_or_split(fd, case):
    first = _device(fd, case, "lds")
    for mode in _modes(case)[1:]:
        other = _device(fd, case, mode)
        for k in ("E", "H", "P", "dft", "probes"):
            assert np.array_equal(first[k], other[k]), (mode, k)
        for a, b in zip(first["fields"], other["fields"]):
            assert np.array_equal(a, b), mode


# ---- 3. the lines never change anything ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_lines_change_no_field_and_no_other_monitor(fd, case):
    """For the lossless box this compares the lossy kernels at ca = 1 (with lines) with the lossless ones (without)."""
    with_lines, without = _device(fd, case, "lds"), _device(fd, case, "nolines")
    for a, b in zip(with_lines["fields"], without["fields"]):
        assert np.array_equal(a, b)
    assert np.array_equal(with_lines["dft"], without["dft"]) and np.array_equal(with_lines["probes"], without["probes"])


# ---- 4. state ------------------------------------------------------------------------------------------------------------

def _engine(fd, case="per40x17f32"):
    cfg = _cfg(case)
    b = fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"])
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    b.set_pml(LAYER, courant00=0.1)
    return b, cfg


def test_reset_zeroes_the_sums_and_restarts_the_count(fd):
    b, cfg = _engine(fd)
    with b:
        b.set_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(40, cfg["amps"][:, :40])
        E, H = b.read_flux_lines()
        assert np.abs(E).max() > 0 and np.abs(H).max() > 0 and np.abs(b.flux()).max() > 0
        b.reset()
        E, H = b.read_flux_lines()
        assert not np.any(E) and not np.any(H) and not np.any(b.flux())
        b.run(40, cfg["amps"][:, :40])
        again = b.read_flux_lines()
    fresh, _ = _engine(fd)
    with fresh:
        fresh.set_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        fresh.run(40, cfg["amps"][:, :40])
        for a, c in zip(again, fresh.read_flux_lines()):
            assert np.array_equal(a, c)


def test_a_refused_call_keeps_the_old_lines(fd):
    b, cfg = _engine(fd)
    with b:
        b.set_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(40, cfg["amps"][:, :40])
        before = b.read_flux_lines(raw=True)
        lib, ip, dp = fd._abi.load(), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        om = np.ascontiguousarray(np.broadcast_to(cfg["omegas"][:, :1], (B, 17)))
        R, C = cfg["R"], cfg["C"]

        def call(lines, nfreq=1, every=1, omega=om):
            ln = np.array(lines, np.int32)
            return lib.fdtd2d_batch_set_flux_lines(b._h, len(lines), ln.ctypes.data_as(ip), nfreq,
                                                   None if omega is None else omega.ctypes.data_as(dp), every)
        assert call([[0, 5 + k, 0, 4] for k in range(5)]) == E_ARG               # 5 lines
        assert call([[0, 5, 0, 4]], nfreq=17) == E_ARG and call([[0, 5, 0, 4]], nfreq=0) == E_ARG
        assert call([[0, 0, 0, 4]]) == E_ARG and call([[0, R - 1, 0, 4]]) == E_ARG
        assert call([[1, C - 1, 0, 4]]) == E_ARG                                  # the image column
        assert call([[0, 5, 0, C]]) == E_ARG and call([[1, 5, R - 3, 4]]) == E_ARG
        assert call([[0, 5, 0, 0]]) == E_ARG and call([[2, 5, 0, 4]]) == E_ARG
        assert call([[0, 5, 0, 4]], every=0) == E_ARG and call([[0, 5, 0, 4]], omega=None) == E_ARG
        assert "line 0" in lib.fdtd2d_batch_last_error(b._h).decode() or "NULL" in lib.fdtd2d_batch_last_error(b._h).decode()
        assert b.info(21) == len(cfg["lines"])
        for a, c in zip(before, b.read_flux_lines(raw=True)):
            assert np.array_equal(a, c)
        b.run(20, cfg["amps"][:, 40:60])                                          # and they go on accumulating
        assert not np.array_equal(before[0], b.read_flux_lines(raw=True)[0])
        # what the lines exclude while they are set
        for refused in (lambda: b.set_bloch_phase(0.3),
                        lambda: fd._abi.check_batch(b._h, lib.fdtd2d_batch_set_periodic(b._h, 0))):
            with pytest.raises(fd.Fdtd2dError) as ei:
                refused()
            assert ei.value.code == E_STATE
        b.set_flux_lines(None, None)
        assert b.info(21) == 0 and not b.flux_lines_in_lds
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.flux()
        assert ei.value.code == E_STATE


def test_lines_come_and_go_on_a_lossless_box(fd):
    """The conductivity the lines bring goes with them: six arrays again, and the layer stays while they are set."""
    b, cfg = _engine(fd, "pml40x40")
    with b:
        six = b.lds_bytes
        b.set_flux_lines(cfg["lines"], cfg["omegas"])
        assert b.lds_bytes > six + _seg(40 * 40, 4) and not b.lossy
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.clear_pml()
        assert ei.value.code == E_STATE
        b.set_flux_lines(None, None)
        assert b.lds_bytes == six and not b.lossy


@pytest.mark.parametrize("kind", ["mur", "none", "bloch", "lattice"])
def test_batches_without_flux_kernels_refuse_with_the_state_error(fd, kind):
    from fdtd2d_amd.api import EPS0, MU0
    boundary = {"mur": "mur", "none": "none", "bloch": "periodic", "lattice": "lattice"}[kind]
    with fd.BatchEngine(2, 40, 17, DT, DX, boundary=boundary) as b:
        b.set_materials(np.full((2, 40, 17), EPS0), np.full((2, 40, 17), MU0))
        if kind == "bloch":
            b.set_bloch_phase(0.4)
        lib = fd._abi.load()
        ln, om = np.array([0, 20, 0, 8], np.int32), np.array([3e11, 3e11])
        rc = lib.fdtd2d_batch_set_flux_lines(b._h, 1, ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1,
                                             om.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1)
        assert rc == E_STATE and b.info(21) == 0
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.read_flux_lines()
        assert ei.value.code == E_STATE


# ---- 5. the one-call interface and point sources ------------------------------------------------------------------------

def test_run_fdtd_batch_returns_the_engines_flux(fd):
    cfg = _cfg("per40x17f32")
    n, lines, om = 120, cfg["lines"], cfg["omegas"]
    out = fd.run_fdtd_batch(cfg["eps"], cfg["mu"], nsteps=n, sources=cfg["rects"], fc=60e9, dt=DT, dx=DX,
                            dtype=np.float32, boundary="periodic", pml_cells=LAYER, dft_every=2, flux_lines=lines,
                            flux_omegas=om)
    assert len(out) == 4 and out[3].shape == (B, len(lines), om.shape[1]) and out[3].dtype == np.float64
    plain = fd.run_fdtd_batch(cfg["eps"], cfg["mu"], nsteps=n, sources=cfg["rects"], fc=60e9, dt=DT, dx=DX,
                              dtype=np.float32, boundary="periodic", pml_cells=LAYER, dft_every=2)
    assert len(plain) == 3 and all(np.array_equal(a, b) for a, b in zip(plain, out))
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=np.float32, boundary="periodic") as b:
        b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
        b.set_pml(LAYER, courant00=np.array(c00)).set_flux_lines(lines, om, every=2)
        b.run(n, fd.batch._waveform_amps("ricker", np.full(B, 60e9), n, DT))
        assert np.array_equal(b.flux(), out[3]) and np.abs(out[3]).max() > 0


@pytest.mark.parametrize("boundary", ["periodic", "pml"])
def test_a_point_source_run_accumulates_like_any_other(fd, boundary):
    _exact_only(fd)
    cfg = _cfg("per40x17f32" if boundary == "periodic" else "pml40x40")
    n = 90
    t = np.arange(n) * DT
    chan = np.stack([np.sin(2 * np.pi * 50e9 * (1 + c) * t + c) for c in range(2)])
    points = np.array([[cfg["R"] // 2 - 3, 0 if boundary == "periodic" else 2], [cfg["R"] // 2 + 4, 7]])
    weights = np.random.default_rng(2).standard_normal((B, 2, 2))

    def drive(b):
        b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
        b.set_pml(LAYER, courant00=0.1)
        b.set_point_sources(points, weights).set_flux_lines(cfg["lines"], cfg["omegas"], every=2)
        b.run(n, cfg["amps"][:, :n], chan)
        return b.read_flux_lines(raw=True) + (b.flux(),)
    ref = flux_oracle_for(boundary)(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=boundary)
    want, scale = drive(ref), ref.flux_scale()
    got = []
    for resident in (None, 0):
        with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=boundary) as b:
            b.set_option(resident=resident)
            got.append(drive(b))
            assert b.resident == (resident is None)
    for a, c in zip(*got):
        assert np.array_equal(a, c)
    for a, w in zip(got[0][:2], want[:2]):
        assert np.abs(a - w).max() <= 1e-12 * np.abs(w).max()
    assert np.all(np.abs(got[0][2] - want[2]) <= 4e-12 * scale)
