"""GPU: flux lines on Hz Bloch batches (fdtd2d_batch_hz_bloch_flux.h, kernels_batch_hz_bloch_flux.hpp) against the
stand-in of tests/oracle_batch_hz_bloch_flux.py.

Three members that differ in eps, mu, sources, phases (0.4, 1.3, -2.2), "ramp" weights and frequencies (one of them
negative), complex amplitudes, 320 steps from rest, on the shapes of tests/test_gpu_batch_bloch_flux.py (whose family
also has 11 arrays) plus the pole's: float32 and float64 40x17 (192 threads, 192 % 17 != 0, 4 cells per thread),
float32 90x33 (768 threads, and lines whose sums do not fit in LDS beside the member), float32 and float64 40x17 with
the pole and a conductivity on rows 25..29 of every column (clear of the 6-cell layer, touching the seam), and float32
60x29 with the pole (448 threads, 448 % 29 != 0, 4 cells per thread, 20 arrays beside which the sums of 123 line cells
do not fit).  The rule, restated in _expect_capacity and checked without a device in
tests/test_batch_hz_bloch_flux_cpu.py, says which case lands where.  Every case runs resident with the sums in LDS (where
the rule admits them), resident with them in global memory (FDTD2D_BATCH_OPT_FLUX_LDS 0) and streamed; one also with 7
steps per launch, so that the sums cross launches.  The lines are set after 50 steps and sample every third step: a
whole-period row line, a row line inside the layer, a column line at column 0 over all rows (the neighbour across the
seam; rows 0 and R-1), a column line at C-2, and the first row line crosses both column lines (one cell on two lines).
A window DFT and probes run beside them.

Tolerances.  The fields are bit-identical to the stand-in's (exact build), so the sums differ only by the device's sin
and cos against NumPy's: 1e-12 max|stand-in| for each of the eight raw arrays, the bound of the Ez Bloch lines.  The flux
is a sum of products of two factors, each a sum of two parts at 1e-12: 8e-12 dx sum (|Hr| + |Hi|) (|Er| + |Ei|) per line,
a margin of 2.  Measured on an MI355X: 1.9e-16 max|stand-in| at worst for a raw array and 6.4e-16 of the scale for P; the
test prints them again."""
import ctypes

import numpy as np
import pytest

from oracle_batch_hz_bloch_flux import HzBlochFluxOracle

pytestmark = pytest.mark.gpu

DT, DX, LDS_LIMIT = 5e-14, 1e-4, 163840
E_ARG, E_STATE = -1, -4
B, NSTEPS, STEP0, EVERY, LAYER = 3, 320, 50, 3, 6
PHI = np.array([0.4, 1.3, -2.2])
# case: (rows, cols, dtype, pole and conductivity, the sums fit in LDS)
CASES = {"40x17f32": (40, 17, np.float32, False, True),
         "40x17f64": (40, 17, np.float64, False, True),
         "90x33f32": (90, 33, np.float32, False, False),
         "40x17f32pole": (40, 17, np.float32, True, True),
         "40x17f64pole": (40, 17, np.float64, True, True),
         "60x29f32pole": (60, 29, np.float32, True, False)}
MODES = ("lds", "global", "streamed")
SPL_CASE = "40x17f32pole"
PARTS = ("Hr", "Er", "Hi", "Ei")


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the stand-in restates the exact build's arithmetic")


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _threads(cells):
    return min(1024, -(-(-(-cells // 4)) // 64) * 64)


def _lines(R, C):
    tall = {40: 12, 90: 40, 60: 30}[R]     # 90x33 and 60x29: enough cells that the sums do not fit in LDS
    return [("row", 20, 0, C - 1), ("row", 3, 2, 5), ("col", 0, 0, R), ("col", C - 2, 14, tall)]


def _cfg(case):
    from fdtd2d_amd.api import EPS0, MU0, ricker_amplitude
    R, C, dtype, pole, fits = CASES[case]
    rng = np.random.default_rng(11)
    ric = np.stack([[ricker_amplitude(k * DT, 60e9 * (1 + 0.1 * m)) for k in range(NSTEPS)] for m in range(B)])
    cfg = dict(case=case, R=R, C=C, dtype=dtype, fits=fits,
               eps=(EPS0 * (1 + 2 * rng.random((B, R, C)))).astype(dtype),
               mu=(MU0 * (1 + 0.5 * rng.random((B, R, C)))).astype(dtype),
               rects=np.array([[15 + m, (0, 2, C - 4)[m], 1, (C - 1, 3, 2)[m]] for m in range(B)]),
               amps=ric * np.exp(1j * np.array([0.0, 0.7, -1.1]))[:, None] + 0.2j * np.roll(ric, 9, axis=1),
               omegas=2 * np.pi * np.array([[40e9, 60e9, 85e9], [35e9, -55e9, 75e9], [45e9, 65e9, 90e9]]),
               win_omegas=2 * np.pi * np.array([50e9, 70e9]), window=(18, 1, 5, 6),
               probes=np.array([[20, 0], [23, C - 2], [4, 5]]), lines=_lines(R, C), pole=None, sigma=None)
    if pole:
        wp2, sigma = np.zeros((B, R, C)), np.zeros((B, R, C))
        wp2[:, 25:30, :] = (2 * np.pi * 70e9) ** 2 * (0.5 + rng.random((B, 5, C)))
        sigma[:, 25:30, :] = 4.0 * rng.random((B, 5, C))
        cfg["pole"] = (wp2, np.array([1e11, 0.0, 5e10]), 2 * np.pi * np.array([0.0, 50e9, 60e9]))
        cfg["sigma"] = sigma
    return cfg


def _new(fd, cfg, count=B, polarization="hz"):
    b = fd.BatchEngine(count, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic")
    return b.set_polarization(polarization) if polarization == "hz" else b


def _setup(b, cfg, phase=True):
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
    b.set_pml(LAYER, courant00=np.array(c00))
    if cfg["sigma"] is not None:
        b.set_conductivity(cfg["sigma"])
    if cfg["pole"] is not None:
        b.set_dispersion(*cfg["pole"])
    if phase:
        b.set_hz_bloch_phase(PHI).set_hz_bloch_source("ramp")
    return b


def _read(b):
    (hr, er), (hi, ei) = b.read_hz_bloch_flux_parts()
    return dict(Hr=hr, Er=er, Hi=hi, Ei=ei, P=b.flux())


def _drive(b, cfg, lines=True, splits=None):
    """The same calls on a BatchEngine and on the stand-in: 50 steps, then the lines, then the rest."""
    _setup(b, cfg)
    b.set_dft_window(cfg["window"], cfg["win_omegas"], every=2).set_probes(cfg["probes"], NSTEPS)
    done, launches = 0, 0
    for k in splits or (STEP0, NSTEPS - STEP0):
        if done == STEP0 and lines:
            b.set_hz_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        before = getattr(b, "launches", 0)
        b.run(k, cfg["amps"][:, done:done + k])
        launches += getattr(b, "launches", 0) - before
        done += k
    assert done == NSTEPS
    state = tuple(b.download_dispersion()) if cfg["pole"] is not None else ()
    out = dict(fields=tuple(b.download()) + (b.download_ezx(),) + state, dft=b.read_dft_window(),
               probes=b.read_probes(), launches=launches)
    if lines:
        out.update(_read(b))
    return out


_refs, _runs = {}, {}


def _stand_in(case):
    if case not in _refs:
        cfg = _cfg(case)
        ref = HzBlochFluxOracle(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic")
        _refs[case] = _drive(ref, cfg)
        _refs[case]["scale"] = ref.flux_scale()
    return _refs[case]


def capacity(R, C, esz, pole, nf, window, nff, cells):
    """The capacity rule of fdtd2d_batch_hz_bloch_flux.h, restated: 11 arrays (20 with the pole), the row factors, 16 (C - 1)
    bytes of source weights, the window's phasor table and the lines' behind it; then both window accumulators and, when
    they fit too, the 64 nff cells bytes of the lines' sums.  (bytes that always count, window accumulators, line sums)"""
    arrays = 20 if pole else 11
    fields = arrays * _seg(R * C, esz) + _seg(4 * R, esz)
    table = 16 * nf + 16 * nff + 16 * (C - 1)
    return fields + table, 2 * 16 * nf * window[2] * window[3], 64 * nff * cells


def _expect_capacity(b, cfg, lines, lds_allowed, never):
    """Returns whether the sums live in LDS on the path the run takes."""
    esz, R, C = b.dtype.itemsize, b.rows, b.cols
    pole = cfg["pole"] is not None
    arrays = 20 if pole else 11
    nf, nff = len(cfg["win_omegas"]), cfg["omegas"].shape[1] if lines else 0
    cells = sum(l[3] for l in cfg["lines"]) if lines else 0
    base, wacc, facc = capacity(R, C, esz, pole, nf, cfg["window"], nff, cells)
    assert base + wacc <= LDS_LIMIT                           # the window's accumulators fit in every case
    fits = base + wacc + facc <= LDS_LIMIT
    assert fits == cfg["fits"] or not lines
    in_lds = bool(lines and lds_allowed and fits)
    assert b.lds_bytes == base + wacc + (facc if in_lds else 0)
    table = base - arrays * _seg(R * C, esz) - _seg(4 * R, esz)
    assert b.resident_max_cells == (LDS_LIMIT - _seg(4 * R, esz) - table) // arrays // 16 * 16 // esz
    assert b.resident == (not never) and b.hz_bloch and not b.bloch and b.dispersive == pole
    assert b.flux_lines_in_lds == bool(in_lds and not never)
    assert b.info(21) == (len(cfg["lines"]) if lines else 0) and b.info(22) == int(in_lds and not never)
    return bool(in_lds and not never)


def _device(fd, case, mode):
    """mode: "lds", "global", "streamed", "spl7" (resident, 7 steps per launch) or "nolines" (resident)."""
    if (case, mode) not in _runs:
        cfg = _cfg(case)
        lines = mode != "nolines"
        with _new(fd, cfg) as b:
            b.set_option(resident=0 if mode == "streamed" else None, steps_per_launch=7 if mode == "spl7" else None)
            b.set_flux_lds(mode != "global")
            out = _drive(b, cfg, lines=lines)
            out["in_lds"] = _expect_capacity(b, cfg, lines, mode != "global", mode == "streamed")
            # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            spl = 7 if mode == "spl7" else NSTEPS
            want = 2 * NSTEPS if mode == "streamed" else -(-STEP0 // spl) + -(-(NSTEPS - STEP0) // spl)
            assert out["launches"] == want
        _runs[case, mode] = out
    return _runs[case, mode]


def _modes(case):
    return MODES + (("spl7",) if case == SPL_CASE else ())


ALL = [(c, m) for c in CASES for m in _modes(c)]


def test_the_shapes_walk_more_than_one_cell_per_thread_and_carry():
    for case, (R, C, _, _, _) in CASES.items():
        threads = _threads(R * C)
        assert threads % C != 0 and 1 < -(-R * C // threads) <= 4, case
    assert _threads(90 * 33) == 768 and _threads(40 * 17) == 192 and _threads(60 * 29) == 448


# ---- 1. against the stand-in, on every path ------------------------------------------------------------------------

@pytest.mark.parametrize("case,mode", ALL, ids=[f"{c}-{m}" for c, m in ALL])
def test_hz_bloch_sums_and_flux_match_the_stand_in(fd, case, mode):
    _exact_only(fd)
    got, want = _device(fd, case, mode), _stand_in(case)
    assert len(got["fields"]) == len(want["fields"]) == (8 if CASES[case][3] else 4)
    for k, (a, w) in enumerate(zip(got["fields"], want["fields"])):      # Hz, Ex, Ey, Hzx and the pole state
        assert np.iscomplexobj(a) and a.dtype == w.dtype and np.array_equal(a, w), k
    assert np.array_equal(got["probes"], want["probes"])
    assert np.abs(got["dft"] - want["dft"]).max() <= 1e-12 * np.abs(want["dft"]).max()
    for name in PARTS:
        for part, pick in (("re", np.real), ("im", np.imag)):       # the eight raw arrays
            err, top = np.abs(pick(got[name]) - pick(want[name])).max(), np.abs(pick(want[name])).max()
            print(f"{case} {mode} {name} {part}: max error {err:.3e}, max |stand-in| {top:.3e}, ratio {err / top:.2e}")
            assert top > 0 and err <= 1e-12 * top, (name, part)
    err = np.abs(got["P"] - want["P"])
    print(f"{case} {mode} P: worst error over its scale {np.max(err / want['scale']):.2e}")
    assert np.all(want["scale"] > 0) and np.all(err <= 8e-12 * want["scale"])
    # the crossing cells: one Hz on two lines (row 20 with column 0, and with column C-2), two different Et
    at = _cfg(case)["lines"]
    n01 = at[0][3] + at[1][3]
    for name in ("Hr", "Hi"):
        assert np.array_equal(got[name][:, :, 0], got[name][:, :, n01 + 20])
        assert np.array_equal(got[name][:, :, at[3][1]], got[name][:, :, n01 + at[2][3] + 20 - at[3][2]])
    assert not np.array_equal(got["Er"][:, :, 0], got["Er"][:, :, n01 + 20])


# ---- 2. whatever the path, the placement and the launch split ----------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_hz_bloch_results_do_not_depend_on_path_placement_or_split(fd, case):
    first = _device(fd, case, "lds")
    assert first["in_lds"] == CASES[case][4]
    assert all(np.abs(first[k]).max() > 0 for k in PARTS + ("P",))
    for mode in _modes(case)[1:]:
        other = _device(fd, case, mode)
        assert not other["in_lds"] or mode == "spl7"
        for k in PARTS + ("P", "dft", "probes"):
            assert np.array_equal(first[k], other[k]), (mode, k)
        for a, b in zip(first["fields"], other["fields"]):
            assert np.array_equal(a, b), mode


# ---- 3. the lines never change anything ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_hz_bloch_lines_change_no_field_and_no_other_monitor(fd, case):
    """The run without lines takes the kernels of batch_hz_bloch.hip."""
    with_lines, without = _device(fd, case, "lds"), _device(fd, case, "nolines")
    for a, b in zip(with_lines["fields"], without["fields"]):
        assert np.iscomplexobj(a) and np.abs(a.imag).max() > 0 and np.array_equal(a, b)
    assert np.array_equal(with_lines["dft"], without["dft"]) and np.array_equal(with_lines["probes"], without["probes"])


# ---- 4. device against device --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("case", ["40x17f32", "40x17f64"])
def test_lossless_lines_are_the_ez_bloch_lines_with_eps_and_mu_exchanged(fd, case, where):
    """Identity (b): H_k = its E_k, E_k = -its H_k, P equal, bit for bit."""
    _exact_only(fd)
    cfg = _cfg(case)
    out = []
    for pol in ("hz", "ez"):
        with _new(fd, cfg, polarization=pol) as b:
            b.set_option(resident=0 if where == "streamed" else None)
            if pol == "hz":
                _setup(b, cfg).set_hz_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
            else:
                b.set_materials(cfg["mu"], cfg["eps"]).set_sources(cfg["rects"])      # symmetric in eps and mu
                c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
                b.set_pml(LAYER, courant00=np.array(c00))
                b.set_bloch_phase(PHI).set_bloch_source("ramp")
                b.set_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
            b.run(120, cfg["amps"][:, :120])
            assert b.resident == (where == "resident")
            parts = b.read_hz_bloch_flux_parts() if pol == "hz" else b.read_bloch_flux_parts()
            out.append((parts, b.flux(), b.download()))
    ((hr, er), (hi, ei)), P, (hz, ex, ey) = out[0]
    ((zr, tr), (zi, ti)), Pz, (ez, hx, hy) = out[1]
    assert np.array_equal(hz, ez) and np.array_equal(ex, -hx) and np.array_equal(ey, -hy)
    assert all(np.abs(a).max() > 0 for a in (hr, er, hi, ei, P))
    assert np.array_equal(hr, zr) and np.array_equal(hi, zi)
    assert np.array_equal(er, -tr) and np.array_equal(ei, -ti)
    assert np.array_equal(P, Pz)


@pytest.mark.parametrize("case", ["40x17f32", "40x17f64pole"])
def test_phase_zero_is_the_real_hz_lines(fd, case):
    """Identity (a): c = 1, s = 0, real amplitudes, unit weights."""
    _exact_only(fd)
    cfg = _cfg(case)
    amps = np.ascontiguousarray(cfg["amps"].real[:, :120])
    with _new(fd, cfg) as b:
        _setup(b, cfg, phase=False).set_hz_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(120, amps)
        et, hz = b.read_flux_lines(raw=True)
        P = b.flux()
    with _new(fd, cfg) as b:
        _setup(b, cfg, phase=False).set_hz_bloch_phase(0.0)
        b.set_hz_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(120, amps + 0j)
        (hr, er), (hi, ei) = b.read_hz_bloch_flux_parts()
        assert np.abs(hz).max() > 0 and np.abs(et).max() > 0
        assert np.array_equal(hr, hz) and np.array_equal(er, et)
        assert not np.any(hi) and not np.any(ei)
        assert np.array_equal(b.flux(), P)


# ---- 5. state ------------------------------------------------------------------------------------------------------------

def _engine(fd, case="40x17f32"):
    cfg = _cfg(case)
    return _setup(_new(fd, cfg), cfg), cfg


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in PARTS + ("P",))


def test_hz_bloch_reset_zeroes_the_sums_and_restarts_the_count(fd):
    b, cfg = _engine(fd)
    with b:
        b.set_hz_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(40, cfg["amps"][:, :40])
        first = _read(b)
        assert all(np.abs(first[k]).max() > 0 for k in PARTS + ("P",))
        b.reset()
        assert not any(np.any(v) for v in _read(b).values())
        b.run(40, cfg["amps"][:, :40])
        assert _same(first, _read(b))


def test_a_new_phase_a_conductivity_and_the_pole_keep_the_lines_and_their_sums(fd):
    b, cfg = _engine(fd)
    pcfg = _cfg("40x17f32pole")
    with b:
        b.set_hz_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(40, cfg["amps"][:, :40])
        before = _read(b)
        b.set_hz_bloch_phase(PHI[::-1].copy())
        assert b.info(21) == 4 and _same(before, _read(b))
        b.set_conductivity(pcfg["sigma"])
        assert b.info(21) == 4 and _same(before, _read(b))
        b.set_dispersion(*pcfg["pole"])                      # the batch switches to the other kernel instance
        assert b.dispersive and b.info(21) == 4 and _same(before, _read(b))
        b.run(20, cfg["amps"][:, 40:60])
        with_pole = _read(b)
        assert not np.array_equal(before["Hr"], with_pole["Hr"])
        assert b.launches and b.hz_bloch
    # the same calls on the stand-in
    if fd.ARITHMETIC == "exact":
        ref = _setup(HzBlochFluxOracle(B, cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"], boundary="periodic"), cfg)
        ref.set_hz_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        ref.run(40, cfg["amps"][:, :40])
        ref.set_hz_bloch_phase(PHI[::-1].copy())
        ref.set_conductivity(pcfg["sigma"])
        ref.set_dispersion(*pcfg["pole"])
        ref.run(20, cfg["amps"][:, 40:60])
        want = _read(ref)
        for k in PARTS:
            assert np.abs(with_pole[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k


def test_every_hz_bloch_refusal_keeps_the_old_lines(fd):
    b, cfg = _engine(fd)
    with b:
        b.set_hz_bloch_flux_lines(cfg["lines"], cfg["omegas"], every=EVERY)
        b.run(40, cfg["amps"][:, :40])
        before = _read(b)
        lib, ip, dp = fd._abi.load(), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        om = np.ascontiguousarray(np.broadcast_to(cfg["omegas"][:, :1], (B, 17)))
        R, C = cfg["R"], cfg["C"]

        def call(lines, nfreq=1, every=1, omega=om, fn=lib.fdtd2d_batch_set_hz_bloch_flux_lines):
            ln = np.array(lines, np.int32)
            return fn(b._h, len(lines), ln.ctypes.data_as(ip), nfreq, None if omega is None else omega.ctypes.data_as(dp),
                      every)
        assert call([[0, 5 + k, 0, 4] for k in range(5)]) == E_ARG               # 5 lines
        assert call([[0, 5, 0, 4]], nfreq=17) == E_ARG and call([[0, 5, 0, 4]], nfreq=0) == E_ARG
        assert call([[0, 0, 0, 4]]) == E_ARG and call([[0, R - 1, 0, 4]]) == E_ARG
        assert call([[1, C - 1, 0, 4]]) == E_ARG and call([[1, -1, 0, 4]]) == E_ARG   # the image column
        assert call([[0, 5, 0, C]]) == E_ARG and call([[1, 5, R - 3, 4]]) == E_ARG
        assert call([[0, 5, 0, 0]]) == E_ARG and call([[2, 5, 0, 4]]) == E_ARG
        assert call([[0, 5, 0, 4]], every=0) == E_ARG and call([[0, 5, 0, 4]], omega=None) == E_ARG
        assert b.info(21) == len(cfg["lines"]) and _same(before, _read(b))
        # the other kinds of lines stay refused on this batch, each naming what it objects to
        for fn, what in ((lib.fdtd2d_batch_set_hz_flux_lines, "Bloch phase"), (lib.fdtd2d_batch_set_flux_lines, "Hz polarisation"),
                         (lib.fdtd2d_batch_set_bloch_flux_lines, "Hz polarisation")):
            assert call([[0, 5, 0, 4]], fn=fn) == E_STATE
            assert what in lib.fdtd2d_batch_last_error(b._h).decode()
        # and removing lines through them leaves these alone
        for fn in (lib.fdtd2d_batch_set_hz_flux_lines, lib.fdtd2d_batch_set_flux_lines, lib.fdtd2d_batch_set_bloch_flux_lines):
            assert fn(b._h, 0, None, 0, None, 1) == 0
        assert b.info(21) == len(cfg["lines"]) and _same(before, _read(b))
        # the readers of the other kinds refuse these lines, naming the right call
        buf = np.empty(B * 3 * 73)
        p4 = (buf.ctypes.data_as(dp),) * 4
        for rc, name in ((lib.fdtd2d_batch_read_flux_lines(b._h, *p4), "fdtd2d_batch_read_hz_bloch_flux_lines"),
                         (lib.fdtd2d_batch_read_hz_flux_lines(b._h, *p4), "fdtd2d_batch_read_hz_bloch_flux_lines"),
                         (lib.fdtd2d_batch_read_bloch_flux_lines(b._h, 0, *p4), "fdtd2d_batch_read_hz_bloch_flux_lines")):
            assert rc == E_STATE and name in lib.fdtd2d_batch_last_error(b._h).decode()
        for fn in (lib.fdtd2d_batch_flux, lib.fdtd2d_batch_hz_flux, lib.fdtd2d_batch_bloch_flux):
            assert fn(b._h, buf.ctypes.data_as(dp)) == E_STATE
            assert "fdtd2d_batch_hz_bloch_flux" in lib.fdtd2d_batch_last_error(b._h).decode()
        assert lib.fdtd2d_batch_read_hz_bloch_flux_lines(b._h, 2, *p4) == E_ARG
        # what the lines exclude while they are set
        assert lib.fdtd2d_batch_set_hz_bloch(b._h, None, None) == E_STATE
        assert "flux lines" in lib.fdtd2d_batch_last_error(b._h).decode()
        refused = [lambda: b.set_hz_bloch_phase(None),
                   lambda: fd._abi.check_batch(b._h, lib.fdtd2d_batch_set_periodic(b._h, 0)),
                   lambda: b.set_polarization("ez")]
        for k, f in enumerate(refused):
            with pytest.raises(fd.Fdtd2dError) as ei:
                f()
            assert ei.value.code == E_STATE, k
            assert b.info(21) == len(cfg["lines"]) and b.hz_bloch and _same(before, _read(b)), k
        b.run(20, cfg["amps"][:, 40:60])                                          # and they go on accumulating
        assert not np.array_equal(before["Hr"], _read(b)["Hr"])
        b.set_hz_bloch_flux_lines(None, None)
        assert b.info(21) == 0 and not b.flux_lines_in_lds
        for f in (b.flux, b.read_hz_bloch_flux_parts):
            with pytest.raises(fd.Fdtd2dError) as ei:
                f()
            assert ei.value.code == E_STATE
        b.set_hz_bloch_phase(None)                                                # nothing holds the phase any more
        assert not b.hz_bloch


def test_batches_that_cannot_carry_hz_bloch_lines_refuse_with_the_state_error(fd):
    from fdtd2d_amd.api import EPS0, MU0
    lib, ip, dp = fd._abi.load(), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    ln, om = np.array([0, 20, 0, 8], np.int32), np.array([3e11, 3e11])

    def call(b):
        return lib.fdtd2d_batch_set_hz_bloch_flux_lines(b._h, 1, ln.ctypes.data_as(ip), 1, om.ctypes.data_as(dp), 1)
    for kind in ("hz", "ezbloch", "pml", "hzpml"):
        boundary = "pml" if kind in ("pml", "hzpml") else "periodic"
        with fd.BatchEngine(2, 40, 17, DT, DX, boundary=boundary) as b:
            if kind in ("hz", "hzpml"):
                b.set_polarization("hz")
            b.set_materials(np.full((2, 40, 17), EPS0), np.full((2, 40, 17), MU0))
            if kind == "ezbloch":
                b.set_bloch_phase(0.4)
            assert call(b) == E_STATE and b.info(21) == 0, kind
            with pytest.raises(fd.Fdtd2dError) as ei:
                b.set_hz_bloch_flux_lines([("row", 20, 0, 8)], [3e11])
            assert ei.value.code == E_STATE, kind


# ---- 6. the one-call interface and the orders ---------------------------------------------------------------------------

def test_run_fdtd_batch_returns_the_engines_hz_bloch_flux(fd):
    cfg = _cfg("40x17f32pole")
    n, lines, om = 120, cfg["lines"], cfg["omegas"]
    kw = dict(nsteps=n, sources=cfg["rects"], fc=60e9, dt=DT, dx=DX, dtype=np.float32, boundary="periodic",
              pml_cells=LAYER, dft_every=2, polarization="hz", hz_bloch_phase=PHI, source_weights="ramp",
              conductivity=cfg["sigma"], dispersion=cfg["pole"])
    out = fd.run_fdtd_batch(cfg["eps"], cfg["mu"], hz_bloch_flux_lines=lines, hz_bloch_flux_omegas=om, **kw)
    assert len(out) == 4 and out[3].shape == (B, len(lines), om.shape[1]) and out[3].dtype == np.float64
    plain = fd.run_fdtd_batch(cfg["eps"], cfg["mu"], **kw)
    assert len(plain) == 3 and all(np.array_equal(a, b) for a, b in zip(plain, out))
    with _new(fd, cfg) as b:
        _setup(b, cfg).set_hz_bloch_flux_lines(lines, om, every=2)
        b.run(n, fd.batch._waveform_amps("ricker", np.full(B, 60e9), n, DT))
        assert np.array_equal(b.flux(), out[3]) and np.abs(out[3]).max() > 0
        # the orders of the whole-period line sum to its flux (Parseval)
        Pm = b.flux_orders(0)
        E, H = b.read_flux_lines()
        scale = DX * (np.abs(E[:, :, :16]) * np.abs(H[:, :, :16])).sum(axis=2)
        assert Pm.shape == (B, 3, 16) and np.all(np.abs(Pm.sum(axis=2) - out[3][:, 0, :]) <= 1e-10 * scale)
        with pytest.raises(ValueError):
            b.flux_orders(1)
