"""GPU: flux lines in the Hz polarisation (fdtd2d_batch_hz_flux.h, kernels_batch_hz_flux.hpp) against the stand-in of
tests/oracle_batch_hz_flux.py.

Three members that differ in eps, mu, sources and frequencies, 320 steps from rest, on the smallest shapes at which each
code path can still go wrong: float32 periodic 40x17 (4 cells per thread) and 130x33 (4290 cells, 5 per thread: the MAXC = 8
kernel, with arrays, tables and sums all in LDS), float64 periodic 40x17, "pml" 40x40 with a 6-cell layer plain, with a
conductivity patch and with a pole, and periodic 40x17 with a pole.  Every shape runs resident with the sums in LDS,
resident with them in global memory (FDTD2D_BATCH_OPT_FLUX_LDS 0) and streamed; one also with 7 steps per launch, so that
the sums cross launches.  The lines are set after 50 steps and sample every third step: a whole-period (or whole-width)
row line, a row line inside the layer, a column line at column 0 of the periodic members (the cyclic neighbour; column 1
and the whole height in the box), a column line at C-2, and the first row line crosses both column lines (one cell on two
lines).  A window DFT and three probes run alongside.

Tolerances, those of tests/test_gpu_batch_flux.py for its reasons.  The fields are bit-identical to the stand-in's (exact
build), so the sums differ only by the device's sin and cos against NumPy's: 1e-12 max|stand-in| per array, as for the
window DFT.  The flux is a sum of products of two such factors: 4e-12 dx sum|H||E| per line (two factors at 1e-12 each, a
margin of 2)."""
import ctypes

import numpy as np
import pytest

from oracle_batch_hz_flux import hz_flux_oracle_for

pytestmark = pytest.mark.gpu

DT, DX, LDS_LIMIT = 5e-14, 1e-4, 163840
E_ARG, E_STATE = -1, -4
B, NSTEPS, STEP0, EVERY, LAYER = 3, 320, 50, 3, 6
# case: (boundary, rows, cols, dtype, conductivity, pole)
CASES = {"per40x17f32": ("periodic", 40, 17, np.float32, False, False),
         "per130x33f32": ("periodic", 130, 33, np.float32, False, False),
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
    if sigma:                                    # rows and columns 6 .. n-8 may conduct (fdtd2d_batch_hz.h)
        s = np.zeros((B, R, C))
        s[:, 24:28, 12:25] = 5.0 * (1 + rng.random((B, 4, 13)))
        cfg["sigma"] = s
    if pole:
        wp2 = np.zeros((B, R, C))
        wp2[:, 25:30, (slice(0, C) if boundary == "periodic" else slice(10, 30))] = (2 * np.pi * 70e9) ** 2
        cfg["pole"] = (wp2, np.array([1e11, 0.0, 5e10]), 2 * np.pi * np.array([0.0, 50e9, 60e9]))
    return cfg


def _c00(cfg):
    return np.array([(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])])


def _drive(b, cfg, lines=True, splits=None):
    """The same calls on a BatchEngine in the Hz polarisation and on the stand-in: 50 steps, the lines, then the rest."""
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    b.set_pml(LAYER, courant00=_c00(cfg))
    if cfg["sigma"] is not None:
        b.set_conductivity(cfg["sigma"])
    if cfg["pole"] is not None:
        b.set_dispersion(*cfg["pole"])
    b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2).set_probes(cfg["probes"], NSTEPS)
    done, launches = 0, 0
    for k in splits or (STEP0, NSTEPS - STEP0):
        if done == STEP0 and lines:
            b.set_hz_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        before = getattr(b, "launches", 0)
        b.run(k, cfg["amps"][:, done:done + k])
        launches += getattr(b, "launches", 0) - before
        done += k
    assert done == NSTEPS
    out = dict(fields=tuple(b.download()), dft=b.read_dft_window(), probes=b.read_probes(), launches=launches)
    if lines:
        out["E"], out["H"] = b.read_flux_lines(raw=True)      # (Et_hat, Hz_hat)
        out["P"] = b.flux()
    return out


_refs, _runs = {}, {}


def _stand_in(case):
    if case not in _refs:
        cfg = _cfg(case)
        ref = hz_flux_oracle_for(cfg["boundary"])(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"],
                                                  boundary=cfg["boundary"])
        _refs[case] = _drive(ref, cfg)
        _refs[case]["scale"] = ref.flux_scale()
    return _refs[case]


def _hz_engine(fd, cfg):
    b = fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"])
    return b.set_polarization("hz")


def _expect_capacity(b, cfg, lines, lds_allowed, never):
    """The capacity rule, restated: seven arrays (twelve with a pole), the 4R + 4C factors, the window's phasor table and
    the lines' behind it, then the window's accumulators and the lines' sums when they fit."""
    esz, R, C = b.dtype.itemsize, b.rows, b.cols
    arrays = 12 if cfg["pole"] is not None else 7
    seg = _seg(R * C, esz)
    fields = arrays * seg + _seg(4 * R, esz) + _seg(4 * C, esz)
    nf, nff = len(cfg["win_omegas"]), cfg["omegas"].shape[1] if lines else 0
    cells = sum(l[3] for l in cfg["lines"]) if lines else 0
    table, wacc, facc = 16 * nf + 16 * nff, 16 * nf * cfg["window"][2] * cfg["window"][3], 32 * nff * cells
    assert fields + table + wacc + facc <= LDS_LIMIT          # every case fits: the placement is the option's alone
    in_lds = lines and lds_allowed
    assert b.polarization == "hz" and b.dispersive == (cfg["pole"] is not None)
    assert b.lds_bytes == fields + table + wacc + (facc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - (fields - arrays * seg) - table) // arrays // 16 * 16 // esz
    assert b.resident == (not never)
    assert b.flux_lines_in_lds == bool(in_lds and not never)
    assert b.info(21) == (len(cfg["lines"]) if lines else 0)
    return fields + table + wacc + facc


def test_the_large_periodic_case_takes_eight_cells_per_thread_with_everything_in_lds():
    """4290 cells on 1024 threads are 5 per thread (the MAXC = 8 kernel), and its arrays, tables and sums fit 160 KiB."""
    _, R, C, dtype, _, _ = CASES["per130x33f32"]
    assert 4096 < R * C <= 8192 and dtype is np.float32
    cells = sum(l[3] for l in _lines("periodic", R, C))
    total = 7 * _seg(R * C, 4) + _seg(4 * R, 4) + _seg(4 * C, 4) + 16 * 2 + 16 * 3 + 16 * 2 * 5 * 6 + 32 * 3 * cells
    assert total <= LDS_LIMIT


def _device(fd, case, mode):
    """mode: "lds", "global", "streamed", "spl7" (resident, 7 steps per launch) or "nolines" (resident)."""
    if (case, mode) not in _runs:
        cfg = _cfg(case)
        lines = mode != "nolines"
        with _hz_engine(fd, cfg) as b:
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
def test_hz_sums_and_flux_match_the_stand_in(fd, case, mode):
    _exact_only(fd)
    got, want = _device(fd, case, mode), _stand_in(case)
    for name, a, w in zip(("Hz", "Ex", "Ey"), got["fields"], want["fields"]):
        assert a.dtype == w.dtype and np.array_equal(a, w), name
    for name in ("E", "H"):
        err, top = np.abs(got[name] - want[name]).max(), np.abs(want[name]).max()
        print(f"{case} {mode} {name}: max error {err:.3e}, max |stand-in| {top:.3e}, ratio {err / top:.2e}")
        assert top > 0 and err <= 1e-12 * top, name
    err = np.abs(got["P"] - want["P"])
    print(f"{case} {mode} P: worst error over its scale {np.max(err / want['scale']):.2e}")
    assert np.all(want["scale"] > 0) and np.all(err <= 4e-12 * want["scale"])
    # the crossing cell: one Hz on two lines, two tangential E
    n0, at = want["H"].shape[2], _cfg(case)["lines"]
    col, row = at[2][1], at[0][1]
    assert n0 == sum(l[3] for l in at)
    on_row, on_col = col - at[0][2], at[0][3] + at[1][3] + row - at[2][2]
    assert np.array_equal(got["H"][:, :, on_row], got["H"][:, :, on_col])
    assert not np.array_equal(got["E"][:, :, on_row], got["E"][:, :, on_col])


# ---- 2. whatever the path, the placement and the launch split ----------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_hz_results_do_not_depend_on_path_placement_or_split(fd, case):
    first = _device(fd, case, "lds")
    for mode in _modes(case)[1:]:
        other = _device(fd, case, mode)
        for k in ("E", "H", "P", "dft", "probes"):
            assert np.array_equal(first[k], other[k]), (mode, k)
        for a, b in zip(first["fields"], other["fields"]):
            assert np.array_equal(a, b), mode


# ---- 3. the lines never change anything ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_hz_lines_change_no_field_and_no_other_monitor(fd, case):
    with_lines, without = _device(fd, case, "lds"), _device(fd, case, "nolines")
    for a, b in zip(with_lines["fields"], without["fields"]):
        assert np.array_equal(a, b)
    assert np.array_equal(with_lines["dft"], without["dft"]) and np.array_equal(with_lines["probes"], without["probes"])
    assert np.abs(with_lines["P"]).max() > 0


# ---- 4. duality on the device ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["lds", "streamed"])
@pytest.mark.parametrize("case", ["pml40x40", "per40x17f32"])
def test_hz_lines_are_the_ez_flux_kernels_lines_with_exchanged_materials(fd, case, mode):
    """Nothing set: Hz_hat == Ez_hat, Et_hat == -Ht_hat and P equal, bit for bit, device against device."""
    _exact_only(fd)
    cfg = _cfg(case)
    hz = _device(fd, case, mode)
    with fd.BatchEngine(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=cfg["boundary"]) as b:
        b.set_option(resident=0 if mode == "streamed" else None)
        b.set_materials(cfg["mu"], cfg["eps"]).set_sources(cfg["rects"])
        b.set_pml(LAYER, courant00=_c00(cfg))
        b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2).set_probes(cfg["probes"], NSTEPS)
        b.run(STEP0, cfg["amps"][:, :STEP0])
        b.set_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(NSTEPS - STEP0, cfg["amps"][:, STEP0:])
        assert b.resident == (mode != "streamed") and b.polarization == "ez"
        (e, hx, hy), (ez_hat, ht_hat), P = b.download(), b.read_flux_lines(raw=True), b.flux()
        dft, probes = b.read_dft_window(), b.read_probes()
    assert np.array_equal(hz["fields"][0], e) and np.array_equal(hz["fields"][1], -hx) and np.array_equal(hz["fields"][2], -hy)
    assert np.array_equal(hz["H"], ez_hat) and np.abs(ez_hat).max() > 0
    assert np.array_equal(hz["E"], -ht_hat) and np.abs(ht_hat).max() > 0
    assert np.array_equal(hz["P"], P) and np.all(P != 0)
    assert np.array_equal(hz["dft"], dft) and np.array_equal(hz["probes"], probes)


# ---- 5. state ------------------------------------------------------------------------------------------------------------

def _engine(fd, case="per40x17f32"):
    cfg = _cfg(case)
    b = _hz_engine(fd, cfg)
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    b.set_pml(LAYER, courant00=0.1)
    return b, cfg


def test_reset_zeroes_the_hz_sums_and_restarts_the_count(fd):
    b, cfg = _engine(fd)
    with b:
        b.set_hz_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
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
        fresh.set_hz_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        fresh.run(40, cfg["amps"][:, :40])
        for a, c in zip(again, fresh.read_flux_lines()):
            assert np.array_equal(a, c)


def test_what_leaves_the_hz_sums_alone(fd):
    """upload, set_materials, set_sources, set_pml, set_conductivity and set_dispersion keep the sums and their count."""
    b, cfg = _engine(fd)
    with b:
        b.set_hz_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(40, cfg["amps"][:, :40])
        before = b.read_flux_lines(raw=True)
        fields = b.download()
        b.upload(*fields)
        b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"]).set_pml(LAYER, courant00=0.1)
        s = np.zeros((B, cfg["R"], cfg["C"]))
        s[:, 20:24, :] = 1.0
        b.set_conductivity(s).set_dispersion(s * 1e22, 1e11, 0.0)
        assert b.info(21) == len(cfg["lines"]) and b.dispersive
        for a, c in zip(before, b.read_flux_lines(raw=True)):
            assert np.array_equal(a, c)
        b.set_dispersion(None).set_conductivity(None)
        for a, c in zip(before, b.read_flux_lines(raw=True)):
            assert np.array_equal(a, c)


def test_a_refused_call_keeps_the_old_hz_lines(fd):
    b, cfg = _engine(fd)
    with b:
        b.set_hz_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(40, cfg["amps"][:, :40])
        before = b.read_flux_lines(raw=True)
        lib, ip, dp = fd._abi.load(), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        om = np.ascontiguousarray(np.broadcast_to(cfg["omegas"][:, :1], (B, 17)))
        R, C = cfg["R"], cfg["C"]

        def call(lines, nfreq=1, every=1, omega=om, fn=lib.fdtd2d_batch_set_hz_flux_lines):
            ln = np.array(lines, np.int32)
            return fn(b._h, len(lines), ln.ctypes.data_as(ip), nfreq, None if omega is None else omega.ctypes.data_as(dp),
                      every)
        assert call([[0, 5 + k, 0, 4] for k in range(5)]) == E_ARG               # 5 lines
        assert call([[0, 5, 0, 4]], nfreq=17) == E_ARG and call([[0, 5, 0, 4]], nfreq=0) == E_ARG
        assert call([[0, 0, 0, 4]]) == E_ARG and call([[0, R - 1, 0, 4]]) == E_ARG
        assert call([[1, C - 1, 0, 4]]) == E_ARG                                  # the image column
        assert call([[0, 5, 0, C]]) == E_ARG and call([[1, 5, R - 3, 4]]) == E_ARG
        assert call([[0, 5, 0, 0]]) == E_ARG and call([[2, 5, 0, 4]]) == E_ARG
        assert call([[0, 5, 0, 4]], every=0) == E_ARG and call([[0, 5, 0, 4]], omega=None) == E_ARG
        assert "line 0" in lib.fdtd2d_batch_last_error(b._h).decode() or "NULL" in lib.fdtd2d_batch_last_error(b._h).decode()
        # the Ez entry points still refuse an Hz batch, and do not serve these lines
        assert call([[0, 5, 0, 4]], fn=lib.fdtd2d_batch_set_flux_lines) == E_STATE
        assert call([[0, 5, 0, 4]], fn=lib.fdtd2d_batch_set_bloch_flux_lines) == E_STATE
        assert lib.fdtd2d_batch_set_flux_line_sources(b._h, 2, om.ctypes.data_as(dp), om.ctypes.data_as(dp)) == E_STATE
        d4 = [np.empty(before[0].shape) for _ in range(4)]
        assert lib.fdtd2d_batch_read_flux_lines(b._h, *(a.ctypes.data_as(dp) for a in d4)) == E_STATE
        assert lib.fdtd2d_batch_flux(b._h, d4[0].ctypes.data_as(dp)) == E_STATE
        assert call([], fn=lib.fdtd2d_batch_set_flux_lines) == 0                  # nothing of its own to remove
        for refused in (lambda: b.set_flux_lines(cfg["lines"], cfg["omegas"]),
                        lambda: b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"]),
                        lambda: b.set_flux_line_sources(np.ones((1, 2)), None)):
            with pytest.raises(fd.Fdtd2dError, match="Hz polarisation") as ei:
                refused()
            assert ei.value.code == E_STATE
        b.set_flux_lines(None, None)                                              # leaves the Hz lines where they are
        assert b.info(21) == len(cfg["lines"])
        for a, c in zip(before, b.read_flux_lines(raw=True)):
            assert np.array_equal(a, c)
        b.run(20, cfg["amps"][:, 40:60])                                          # and they go on accumulating
        assert not np.array_equal(before[1], b.read_flux_lines(raw=True)[1])
        # what the lines exclude while they are set
        for refused in (lambda: b.set_polarization("ez"),
                        lambda: fd._abi.check_batch(b._h, lib.fdtd2d_batch_set_periodic(b._h, 0))):
            with pytest.raises(fd.Fdtd2dError) as ei:
                refused()
            assert ei.value.code == E_STATE
        assert b.polarization == "hz" and b.info(21) == len(cfg["lines"])
        b.set_hz_flux_lines(None, None)
        assert b.info(21) == 0 and not b.flux_lines_in_lds
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.flux()
        assert ei.value.code == E_STATE
        b.set_polarization("ez")
        assert b.polarization == "ez"


def test_hz_lines_come_and_go_and_the_layer_stays_while_they_are_set(fd):
    b, cfg = _engine(fd, "pml40x40")
    with b:
        seven = b.lds_bytes
        assert seven == 7 * _seg(40 * 40, 4) + 2 * _seg(4 * 40, 4)
        b.set_hz_flux_lines(cfg["lines"], cfg["omegas"])
        cells = sum(l[3] for l in cfg["lines"])
        assert b.lds_bytes == seven + 16 * 3 + 32 * 3 * cells and b.flux_lines_in_lds
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.clear_pml()
        assert ei.value.code == E_STATE
        b.set_hz_flux_lines(None, None)
        assert b.lds_bytes == seven
        b.clear_pml()


@pytest.mark.parametrize("kind", ["ez", "no-layer", "no-materials"])
def test_batches_that_cannot_carry_hz_lines_refuse_with_the_state_error(fd, kind):
    from fdtd2d_amd.api import EPS0, MU0
    with fd.BatchEngine(2, 40, 40, DT, DX, boundary="pml") as b:
        if kind != "ez":
            b.set_polarization("hz")
        if kind != "no-materials":
            b.set_materials(np.full((2, 40, 40), EPS0), np.full((2, 40, 40), MU0))
        if kind != "no-layer":
            b.set_pml(LAYER, courant00=0.1)
        lib, dp = fd._abi.load(), ctypes.POINTER(ctypes.c_double)
        ln, om = np.array([0, 20, 0, 8], np.int32), np.array([3e11, 3e11])
        rc = lib.fdtd2d_batch_set_hz_flux_lines(b._h, 1, ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1,
                                                om.ctypes.data_as(dp), 1)
        assert rc == E_STATE and b.info(21) == 0
        d = np.empty(64)
        assert lib.fdtd2d_batch_read_hz_flux_lines(b._h, *([d.ctypes.data_as(dp)] * 4)) == E_STATE
        assert lib.fdtd2d_batch_hz_flux(b._h, d.ctypes.data_as(dp)) == E_STATE
        if kind == "ez":
            with pytest.raises(fd.Fdtd2dError, match="needs the Hz polarisation") as ei:
                b.set_hz_flux_lines([("row", 20, 0, 8)], [3e11])
            assert ei.value.code == E_STATE


# ---- 6. the one-call interface and point sources ------------------------------------------------------------------------

def test_run_fdtd_batch_returns_the_hz_engines_flux(fd):
    cfg = _cfg("per40x17f32")
    n, lines, om = 120, cfg["lines"], cfg["omegas"]
    kw = dict(nsteps=n, sources=cfg["rects"], fc=60e9, dt=DT, dx=DX, dtype=np.float32, boundary="periodic",
              pml_cells=LAYER, dft_every=2, polarization="hz")
    out = fd.run_fdtd_batch(cfg["eps"], cfg["mu"], hz_flux_lines=lines, hz_flux_omegas=om, **kw)
    assert len(out) == 4 and out[3].shape == (B, len(lines), om.shape[1]) and out[3].dtype == np.float64
    plain = fd.run_fdtd_batch(cfg["eps"], cfg["mu"], **kw)
    assert len(plain) == 3 and all(np.array_equal(a, b) for a, b in zip(plain, out))
    with _hz_engine(fd, cfg) as b:
        b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
        b.set_pml(LAYER, courant00=_c00(cfg)).set_hz_flux_lines(lines, om, every=2)
        b.run(n, fd.batch._waveform_amps("ricker", np.full(B, 60e9), n, DT))
        assert np.array_equal(b.flux(), out[3]) and np.abs(out[3]).max() > 0


@pytest.mark.parametrize("boundary", ["periodic", "pml"])
def test_a_point_source_run_accumulates_on_hz_lines_like_any_other(fd, boundary):
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
        b.set_point_sources(points, weights).set_hz_flux_lines(cfg["lines"], cfg["omegas"], every=2)
        b.run(n, cfg["amps"][:, :n], chan)
        return b.read_flux_lines(raw=True) + (b.flux(),)
    ref = hz_flux_oracle_for(boundary)(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary=boundary)
    want, scale = drive(ref), ref.flux_scale()
    got = []
    for resident in (None, 0):
        with _hz_engine(fd, cfg) as b:
            b.set_option(resident=resident)
            got.append(drive(b))
            assert b.resident == (resident is None)
    for a, c in zip(*got):
        assert np.array_equal(a, c)
    for a, w in zip(got[0][:2], want[:2]):
        assert np.abs(a - w).max() <= 1e-12 * np.abs(w).max()
    assert np.all(np.abs(got[0][2] - want[2]) <= 4e-12 * scale)
