"""GPU: the lattice mode of the Hz polarisation (fdtd2d_batch_hz_lattice.h, kernels_batch_hz_lattice.hpp).

The seven complex fields (Hz, Ex, Ey, Jx, Qx, Jy, Qy) and the probe traces equal the stand-in of
tests/oracle_batch_hz_lattice.py bit for bit (exact build), window DFTs to 1e-12: both dtypes, with and without the pole,
with and without a conductivity, resident, 7 steps per launch, a run cut in three, streamed, and resident continued
streamed, on 11x13, 23x19 and 37x31 (the cell walk carries, no size is a multiple of the workgroup).  Five members with
distinct eps, mu, sigma, wp2, gamma and omega0 (a Drude one, a lossless one and one with wp2 = 0) and phases that mix 0, pi
and generic values of both signs on both seams; wp2 and sigma on every cell of the period, rows 0 and R-2 and columns 0 and
C-2 included; sources at both seams with complex amplitudes and ramp weights; a window next to both seams, probes in row
0, column 0, row R-2 and column C-2 and a random uploaded complex state that includes the pole's.  Every case asserts the
path it took and its launch count.

Device against device: identities (b), (d) and (e) of the header and the supercells with exact rotations, resident and
streamed, through the ``check_*`` functions of tests/test_batch_hz_lattice_cpu.py.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact stand-in: see FUSED_MEASURED."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_batch_hz_lattice_cpu as cpu
from oracle_batch_hz_lattice import HzLatticeOracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, LDS_LIMIT = 5e-14, 1e-4, 163840
E_ARG, E_STATE = -1, -4
B, NSTEPS = 5, 21
PHI_R = np.array([0.0, np.pi, 0.7, -2.1, 3.0])
PHI_C = np.array([np.pi, 0.0, -1.3, 2.4, 0.0])
GAMMA = np.array([1e11, 0.0, 5e10, 8e10, 2e10])
OMEGA0 = 2 * np.pi * np.array([0.0, 50e9, 60e9, 40e9, 0.0])      # member 0 Drude, 1 lossless, 4 has wp2 = 0
WP2_TOP = (2 * np.pi * 300e9) ** 2
CASES = {"11x13": (11, 13), "23x19": (23, 19), "37x31": (37, 31)}
# The fused build evaluates the rotations, the pole and the updates of Ex, Ey and Hz as the fma that
# fdtd2d_batch_hz_lattice.h and its parent headers write out, so its results differ from the exact stand-in's by rounding.
# Measured on an MI355X (the child process of test_fused_build_within_its_bounds): both parts of Hz after 300 steps of the
# members of FUSED_CASES from rest, worst member's max|fused - stand-in| / max|stand-in|.  The bound is ten times the
# measured value.
NSTEPS_FUSED = 300
FUSED_CASES = ("11x13", "23x19")
FUSED_MEASURED = {"f32": 3.6e-7, "f64": 6.4e-16}
FUSED_BOUND = {k: 10 * v for k, v in FUSED_MEASURED.items()}
NAMES = ("Hz", "Ex", "Ey", "Jx", "Qx", "Jy", "Qy")


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact stand-in in test_fused_build_within_its_bounds")


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _cfg(case, dtype, n=NSTEPS, seed=11, state=True, count=B):
    """The members of a case: materials, conductivity, strengths, phases, sources, monitors and (state) a random complex
    state.  `case`: a key of CASES or a shape."""
    from fdtd2d_amd.api import EPS0, MU0, ricker_amplitude
    R, C = CASES[case] if isinstance(case, str) else case
    rng = np.random.default_rng(seed)
    k = np.arange(count) % B
    per = (count, R - 1, C - 1)                                    # every cell of the period
    wp2, sigma = np.zeros((count, R, C)), np.zeros((count, R, C))
    wp2[:, :-1, :-1] = WP2_TOP * (0.05 + rng.random(per))          # the metal touches both seams
    wp2[k == 4] = 0.0
    sigma[:, :-1, :-1] = np.where(rng.random(per) < 0.3, 0.0, 5.0 * rng.random(per))
    real = np.stack([[ricker_amplitude(s * DT, 40e9 * (1 + 0.1 * m)) for s in range(n)] for m in range(B)])[k]
    rects = np.array([[(0, R - 3, R // 2, 2, R - 2)[m], (0, 2, C - 4, 1, 3)[m], (2, 2, 1, 3, 1)[m], (C - 1, 3, 3, 1, 4)[m]]
                      for m in range(B)])[k]
    cfg = dict(case=case, R=R, C=C, dtype=dtype, n=n, wp2=wp2, sigma=sigma, phi_r=PHI_R[k], phi_c=PHI_C[k],
               eps=(EPS0 * (1 + 3 * rng.random((count, R, C)))).astype(dtype),
               mu=(MU0 * (1 + 0.5 * rng.random((count, R, C)))).astype(dtype), rects=rects,
               amps=real * np.exp(1j * (0.4 * np.arange(count) - 0.3))[:, None], weights="ramp",
               omegas=2 * np.pi * np.array([45e9, 65e9]), window=(R - 6, C - 6, 5, 5),
               probes=np.array([[0, 0], [R - 2, C - 2], [0, C - 2], [R - 2, 0], [3, 4]]), gamma=GAMMA[k], omega0=OMEGA0[k])
    if state:                                                      # Hz, Ex, Ey, Jx, Qx, Jy, Qy
        shapes = ((count, R, C), (count, R, C - 1), (count, R - 1, C)) + ((count, R, C),) * 4
        st = [rng.standard_normal(s) + 1j * rng.standard_normal(s) for s in shapes]
        st[1][:, -1, :] = 0                                        # row R-1 of Ex and column C-1 of Ey are never written
        st[2][:, :, -1] = 0
        for a in st[3:]:                                           # the pole state lives on the period alone
            a[:, -1, :] = 0
            a[:, :, -1] = 0
        cfg["state"] = st
    return cfg


def _engine(fd, count, R, C, dtype, polarization="hz"):
    b = fd.BatchEngine(count, R, C, DT, DX, dtype=dtype, boundary="periodic")
    return b.set_polarization(polarization)


def _drive(b, cfg, pole=True, sigma=True):
    """The same calls on a BatchEngine and on the stand-in."""
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    b.set_hz_lattice_phase(cfg["phi_r"], cfg["phi_c"]).set_hz_bloch_source(cfg["weights"])
    if sigma:
        b.set_conductivity(cfg["sigma"])
    if pole:
        b.set_dispersion(cfg["wp2"], cfg["gamma"], cfg["omega0"])
    b.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
    if "state" in cfg:
        s = cfg["state"]
        b.upload(s[0], s[1], s[2])
        if pole:
            b.upload_hz_dispersion(*s[3:7])
    return b


def _results(b, pole=True):
    return dict(fields=tuple(b.download()) + (tuple(b.download_dispersion()) if pole else ()),
                dft=b.read_dft_window(), probes=b.read_probes())


_refs = {}


def _stand_in(case, dtype, pole=True, sigma=True, **kw):
    """The stand-in's results of a case, computed once."""
    key = (case, np.dtype(dtype).name, pole, sigma) + tuple(sorted(kw.items()))
    if key not in _refs:
        _refs[key] = _oracle_run(_cfg(case, dtype, **kw), pole, sigma)
    return _refs[key]


def _oracle_run(cfg, pole=True, sigma=True):
    ref = _drive(HzLatticeOracle(len(cfg["eps"]), cfg["R"], cfg["C"], DT, DX, dtype=cfg["dtype"]), cfg, pole, sigma)
    ref.run(cfg["n"], cfg["amps"])
    return _results(ref, pole)


def _expect_path(b, cfg, never=False, pole=True, window_lds=True):
    """The capacity rule, restated: eighteen arrays with the pole, nine without, no factors, the 2 (C-1) float64 source
    weights with the phasor table, and the accumulators of both parts when they fit."""
    esz, R, C = b.dtype.itemsize, b.rows, b.cols
    arrays = 18 if pole else 9
    fields = arrays * _seg(R * C, esz)
    nf = len(cfg["omegas"])
    table, acc = 16 * nf + 16 * (C - 1), 2 * 16 * nf * cfg["window"][2] * cfg["window"][3]
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = fields + table + acc <= LDS_LIMIT and window_lds
    assert b.polarization == "hz" and b.dispersive == pole
    assert b.hz_lattice and not b.hz_bloch and not b.bloch and not b.lattice
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - table) // arrays // 16 * 16 // esz
    assert b.resident == resident and b.window_in_lds == (resident and in_lds)
    return resident


def _device_run(fd, cfg, splits=None, resident=None, spl=None, pole=True, sigma=True, then_streamed=False,
                window_lds=True):
    """then_streamed: every run after the first is streamed."""
    with _engine(fd, len(cfg["eps"]), cfg["R"], cfg["C"], cfg["dtype"]) as b:
        _drive(b, cfg, pole, sigma)
        b.set_option(resident=resident, steps_per_launch=spl)
        if not window_lds:
            b.set_window_lds(False)
        path = _expect_path(b, cfg, never=resident == 0, pole=pole, window_lds=window_lds)
        done = 0
        for k in splits or (cfg["n"],):
            if then_streamed and done:
                b.set_option(resident=0)
                path = False
            launches = b.launches
            b.run(k, cfg["amps"][:, done:done + k])
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
    for name, a, w in zip(NAMES, got["fields"], want["fields"]):
        assert np.iscomplexobj(a) and a.dtype == w.dtype and np.array_equal(a, w), name
    assert len(got["fields"]) == len(want["fields"])
    assert np.iscomplexobj(got["probes"]) and np.array_equal(got["probes"], want["probes"])
    assert np.abs(got["dft"] - want["dft"]).max() <= 1e-12 * np.abs(want["dft"]).max()


def _fits(cfg, pole):
    esz = np.dtype(cfg["dtype"]).itemsize
    return (18 if pole else 9) * _seg(cfg["R"] * cfg["C"], esz) + 16 * len(cfg["omegas"]) + 16 * (cfg["C"] - 1) <= LDS_LIMIT


# ---- 1. against the stand-in, whatever the path ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_hz_lattice_runs_match_the_stand_in_on_every_path(fd, case, dtype):
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    want = _stand_in(case, dtype)
    assert all(np.any(a.real) and np.any(a.imag) for a in want["fields"])
    fits = _fits(cfg, True)                                        # 37x31 float64 with the pole: 18 arrays do not fit
    assert fits == (case != "37x31" or dtype == np.float32)
    runs = {"resident": _device_run(fd, cfg),
            "split7": _device_run(fd, cfg, spl=7),
            "cut_in_three": _device_run(fd, cfg, splits=(8, 6, 7)),
            "global_window": _device_run(fd, cfg, window_lds=False),
            "then_streamed": _device_run(fd, cfg, splits=(8, 13), then_streamed=True),
            "streamed": _device_run(fd, cfg, resident=0)}
    for name, got in runs.items():
        assert got["path"] == (fits and name not in ("then_streamed", "streamed")), name
        _matches(got, want)
    for name, got in runs.items():
        assert _same(got, runs["resident"]), name


@pytest.mark.parametrize("pole,sigma", [(False, True), (True, False), (False, False)], ids=["sigma", "pole", "plain"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_hz_lattice_runs_with_fewer_materials_match_the_stand_in(fd, case, dtype, pole, sigma):
    _exact_only(fd)
    cfg = _cfg(case, dtype)
    want = _stand_in(case, dtype, pole=pole, sigma=sigma)
    for kw in (dict(), dict(spl=7), dict(resident=0)):
        got = _device_run(fd, cfg, pole=pole, sigma=sigma, **kw)
        assert got["path"] == (_fits(cfg, pole) and kw.get("resident") != 0)
        _matches(got, want)


# ---- 2. the largest resident member of each variant, and the first that streams ------------------------------------------------

@pytest.mark.parametrize("pole", [False, True], ids=["plain", "pole"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_largest_member_is_resident_and_one_row_more_is_streamed(fd, dtype, pole):
    """The row count comes from resident_max_cells: 31 columns, so no multiple of the workgroup.  float32 without a pole
    has more than 4096 cells, five per thread; the others at most four."""
    _exact_only(fd)
    C, n = 31, 20
    probe = _cfg((40, C), dtype, n=n)
    with _engine(fd, B, 40, C, dtype) as b:
        _drive(b, probe, pole=pole)
        most = b.resident_max_cells
    rows = most // C
    cells = rows * C
    assert (cells > 4096) == (dtype == np.float32 and not pole)
    threads = min(1024, -(-(-(-cells // 4)) // 64) * 64)           # a wave multiple, at least a quarter of the cells
    assert -(-cells // threads) == (5 if cells > 4096 else 4)
    cfg = _cfg((rows, C), dtype, n=n, seed=3)
    got = _device_run(fd, cfg, pole=pole)
    assert got["path"] is True and cells <= most < cells + C
    _matches(got, _oracle_run(cfg, pole))
    big = _cfg((rows + 1, C), dtype, n=n, seed=5)
    got = _device_run(fd, big, pole=pole)
    assert got["path"] is False
    _matches(got, _oracle_run(big, pole))


def test_more_members_than_one_round_of_workgroups_reuse_lds(fd):
    """29x27 float64 with the pole: 18 arrays of 6264 B leave room for one workgroup per CU, so 300 members on 256 CUs
    send some workgroups round their member loop twice."""
    _exact_only(fd)
    count = 300
    cfg = _cfg((29, 27), np.float64, n=6, seed=9, count=count)
    with _engine(fd, count, 29, 27, np.float64) as b:
        _drive(b, cfg)
        assert 2 * b.lds_bytes > LDS_LIMIT and b.resident
    got = _device_run(fd, cfg)
    assert got["path"] is True
    _matches(got, _oracle_run(cfg))


# ---- 3. device against device ---------------------------------------------------------------------------------------------

def _new(fd, never):
    def new(count, R, C, dtype):
        b = _engine(fd, count, R, C, dtype)
        return b
    return new


def _prepare(where):
    def prepare(e):
        e.set_option(resident=0 if where == "streamed" else None)
        assert e.resident == (where == "resident")
    return prepare


@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_lossless_run_is_the_ez_lattice_run_with_exchanged_materials(fd, dtype, where):
    """(b): against k_batch_resident_lattice and its streamed pair, without the stand-in."""
    _exact_only(fd)
    new_ez = lambda count, R, C, dt: fd.BatchEngine(count, R, C, DT, DX, dtype=dt, boundary="lattice")
    cpu.check_duality(_new(fd, where), new_ez, dtype, 23, 19, prepare=_prepare(where))


@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_transpose_and_conjugate_hold_on_the_device(fd, dtype, where):
    """(d) and (e), and (a) and (c) with them."""
    _exact_only(fd)
    new, prepare = _new(fd, where), _prepare(where)
    cpu.check_transpose(new, dtype, 23, 19, prepare=prepare)
    cpu.check_conjugate(new, dtype, 23, 19, prepare=prepare)
    cpu.check_unit_rotations(new, dtype, 11, 13, prepare=prepare)
    cpu.check_empty_pole(new, dtype, 11, 13, prepare=prepare)


@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("rot_r,rot_c", cpu.SUPER_CASES)
def test_exact_rotations_match_their_supercell_on_the_device(fd, rot_r, rot_c, where):
    _exact_only(fd)
    for dtype in (np.float32, np.float64):
        cpu.check_supercell_exact(_new(fd, where), dtype, 12, 14, rot_r, rot_c, prepare=_prepare(where))


# ---- 4. transfers, new phases, turning the mode off -----------------------------------------------------------------------------

def _rot(c, s, z, dtype):
    """rho * z as the library forms it: two products and one sum per part, each rounded to the batch dtype."""
    T = np.dtype(dtype).type
    c, s, re, im = (np.asarray(v).astype(T) for v in (c, s, z.real, z.imag))
    return (c * re - s * im) + 1j * (s * re + c * im)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_round_trips_overwrite_the_images_and_return_them_rotated(fd, dtype):
    _exact_only(fd)
    cfg = _cfg("11x13", dtype)
    s = [a.copy() for a in cfg["state"]]
    with _engine(fd, B, 11, 13, dtype) as b:
        _drive(b, cfg)
        got = _results(b)["fields"]
    T = cpu.cdtype(dtype)
    hz = s[0].astype(T)
    cr, sr = (f(PHI_R).astype(dtype)[:, None] for f in (np.cos, np.sin))
    cc, sc = (f(PHI_C).astype(dtype)[:, None] for f in (np.cos, np.sin))
    want = hz.copy()
    want[:, :, -1] = _rot(cc, sc, hz[:, :, 0], dtype)              # what was uploaded in the images is gone
    want[:, -1, :] = _rot(cr, sr, want[:, 0, :], dtype)            # the corner: rho_r * (rho_c * Hz[0, 0])
    assert np.array_equal(got[0], want) and not np.array_equal(got[0], hz)
    for name, a, w in zip(NAMES[1:], got[1:], s[1:]):
        assert np.array_equal(a, w.astype(T)), name                # no images: as uploaded


def test_new_phases_keep_everything_and_turning_the_mode_off_keeps_the_real_parts(fd):
    cfg = _cfg("23x19", np.float32)
    R, C = cfg["R"], cfg["C"]
    with _engine(fd, B, R, C, np.float32) as b:
        _drive(b, cfg)
        b.run(5, cfg["amps"])
        before = _results(b)
        b.set_hz_lattice_phase(PHI_C[::-1].copy(), PHI_R[::-1].copy())
        assert b.hz_lattice and b.step_count == 5
        after = _results(b)
        for name, a, w in zip(NAMES, after["fields"], before["fields"]):
            if name == "Hz":                                       # the images are delivered rotated by the new phases
                a, w = a[:, :-1, :-1], w[:, :-1, :-1]
            assert np.array_equal(a, w), name
        assert np.array_equal(after["dft"], before["dft"]) and np.array_equal(after["probes"], before["probes"])
        # off: refused while sigma or wp2 sits in the rows a periodic batch forbids, the batch as it was
        _raises(fd, E_ARG, "non-zero within 6 rows", lambda: b.set_hz_lattice_phase(None, None))
        assert b.hz_lattice and _same(_results(b), after)
        inner = np.zeros((B, R, C))
        inner[:, 6:R - 7, :-1] = 1.0
        b.set_conductivity(cfg["sigma"] * inner)
        _raises(fd, E_ARG, "wp2 is non-zero within 6 rows", lambda: b.set_hz_lattice_phase(None, None))
        b.set_dispersion(cfg["wp2"] * inner, cfg["gamma"], cfg["omega0"])
        b.set_hz_lattice_phase(None, None)
        assert not b.hz_lattice and not b.hz_bloch and not b.bloch and not b.lattice
        assert b.dispersive and b.polarization == "hz" and b.periodic
        hz, ex, ey = b.download()
        off = (hz, ex, ey) + tuple(b.download_dispersion())
        for name, a, w in zip(NAMES, off, after["fields"]):
            assert not np.iscomplexobj(a), name
            if name == "Hz":
                assert np.array_equal(a[:, :, -1], a[:, :, 0])     # a plain periodic batch: the image is column 0
                a, w = a[:, :-1, :-1], w[:, :-1, :-1]
            assert np.array_equal(a, w.real), name
        b.run(3, cfg["amps"].real)                                 # and it runs on the real Hz kernels again
        b.set_hz_lattice_phase(0.5, -0.5)                          # the mode set again starts with zero imaginary parts
        hz, ex, ey = b.download()
        parts = (hz[:, :-1, :-1], ex, ey) + b.download_dispersion()
        assert b.hz_lattice and np.any(hz.real) and not any(np.any(a.imag) for a in parts)


def test_materials_set_before_the_mode_are_kept(fd):
    """sigma and the pole under the periodic rule first, then the mode: the same run as the other order."""
    _exact_only(fd)
    cfg = _cfg("23x19", np.float64)
    R, C = cfg["R"], cfg["C"]
    inner = np.zeros((B, R, C))
    inner[:, 6:R - 7, :-1] = 1.0
    cfg["sigma"], cfg["wp2"] = cfg["sigma"] * inner, cfg["wp2"] * inner
    want = _oracle_run(cfg)
    with _engine(fd, B, R, C, np.float64) as b:
        b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
        b.set_conductivity(cfg["sigma"]).set_dispersion(cfg["wp2"], cfg["gamma"], cfg["omega0"])
        b.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
        b.set_hz_lattice_phase(cfg["phi_r"], cfg["phi_c"]).set_hz_bloch_source("ramp")
        assert not any(np.any(a) for a in b.download_dispersion())
        s = cfg["state"]
        b.upload(s[0], s[1], s[2]).upload_hz_dispersion(*s[3:7])
        _expect_path(b, cfg)
        b.run(cfg["n"], cfg["amps"])
        _matches(_results(b), want)
        b.reset()
        got = _results(b)
        assert not any(np.any(a) for a in got["fields"]) and not np.any(got["dft"]) and b.step_count == 0


# ---- 5. refusals leave the batch as it was ------------------------------------------------------------------------------------

def _raises(fd, code, match, call):
    with pytest.raises(fd.Fdtd2dError, match=match) as ei:
        call()
    assert ei.value.code == code


def test_refusals_leave_an_hz_lattice_batch_as_it_was(fd):
    _exact_only(fd)
    cfg = _cfg("23x19", np.float32)
    R, C = cfg["R"], cfg["C"]
    want = _stand_in("23x19", np.float32)
    with _engine(fd, B, R, C, np.float32) as b:
        _drive(b, cfg)
        lds = b.lds_bytes
        L = b._lib
        one = np.ones(B * R * C)
        dp = one.ctypes.data_as(L.fdtd2d_batch_set_bloch.argtypes[1])
        ipt = L.fdtd2d_batch_set_point_sources.argtypes[2]
        ip = np.array([8, 1], np.int32).ctypes.data_as(ipt)
        line = np.array([0, 10, 0, C - 1], np.int32).ctypes.data_as(L.fdtd2d_batch_set_hz_flux_lines.argtypes[2])
        colf = np.ones(B * 4 * C, np.float32)
        rowf = np.ones(B * 4 * R, np.float32)
        for rc in (L.fdtd2d_batch_set_pml(b._h, rowf.ctypes.data, colf.ctypes.data, 0, 3),
                   L.fdtd2d_batch_transfer_ezx(b._h, one.ctypes.data, 1, 0),
                   L.fdtd2d_batch_set_hz_bloch(b._h, dp, dp), L.fdtd2d_batch_set_hz_bloch(b._h, None, None),
                   L.fdtd2d_batch_set_hz_flux_lines(b._h, 1, line, 1, dp, 1),
                   L.fdtd2d_batch_set_hz_bloch_flux_lines(b._h, 1, line, 1, dp, 1),
                   L.fdtd2d_batch_set_dft(b._h, dp, 1), L.fdtd2d_batch_set_point_sources(b._h, 1, ip, 1, dp),
                   L.fdtd2d_batch_run_channels(b._h, 2, None, dp, 0),
                   L.fdtd2d_batch_set_polarization(b._h, 0), L.fdtd2d_batch_set_periodic(b._h, 0),
                   L.fdtd2d_batch_transfer_hz_bloch(b._h, None, None, None, one.ctypes.data, 1, 0),
                   # the Ez Bloch and lattice entry points keep refusing an Hz batch
                   L.fdtd2d_batch_set_lattice(b._h, dp, dp, dp, dp), L.fdtd2d_batch_set_lattice(b._h, None, None, None, None),
                   L.fdtd2d_batch_set_bloch(b._h, dp, dp), L.fdtd2d_batch_set_bloch(b._h, None, None),
                   L.fdtd2d_batch_set_bloch_source(b._h, None, None), L.fdtd2d_batch_run_bloch(b._h, 1, None, None),
                   L.fdtd2d_batch_transfer_bloch(b._h, one.ctypes.data, None, None, None, 1, 0),
                   L.fdtd2d_batch_read_dft_window_bloch(b._h, dp, dp), L.fdtd2d_batch_read_probes_bloch(b._h, dp, 0, 1),
                   L.fdtd2d_batch_set_bloch_dispersion(b._h, one.ctypes.data, 1, dp, dp),
                   L.fdtd2d_batch_hold_dft_window(b._h), L.fdtd2d_batch_hold_bloch_window(b._h)):
            assert rc == E_STATE
        assert L.fdtd2d_batch_is_lattice(b._h) == 0 and L.fdtd2d_batch_is_hz_lattice(b._h) == 1
        assert L.fdtd2d_batch_set_polarization(b._h, 1) == 0          # the polarisation it has: nothing to do
        nan = np.full(B, np.nan)
        assert L.fdtd2d_batch_set_hz_lattice(b._h, dp, dp, nan.ctypes.data_as(type(dp)), dp) == E_ARG
        assert "member 0" in L.fdtd2d_batch_last_error(b._h).decode()
        assert L.fdtd2d_batch_set_hz_lattice(b._h, dp, dp, dp, None) == E_ARG
        _raises(fd, E_ARG, "touches row 22 or column 18", lambda: b.set_dft_window((R - 5, 3, 5, 5), cfg["omegas"]))
        _raises(fd, E_ARG, "touches row 22 or column 18", lambda: b.set_dft_window((3, C - 5, 5, 5), cfg["omegas"]))
        _raises(fd, E_ARG, "touches row 22 or column 18", lambda: b.set_probes([(8, 0), (R - 1, 3)], 10))
        _raises(fd, E_ARG, "touches row 22 or column 18", lambda: b.set_probes([(8, C - 1)], 10))
        win = np.array([R - 5, 3, 5, 5], np.int32)
        assert L.fdtd2d_batch_set_dft_window(b._h, *(int(v) for v in win), 1, dp, 1) == E_ARG
        cell = np.tile(np.array([(R - 1) * C + 3], np.int32), B)
        assert L.fdtd2d_batch_set_probes(b._h, 1, cell.ctypes.data_as(ipt), 10) == E_ARG
        for bad in ([R - 2, 3, 2, 2], [3, C - 2, 2, 2]):
            rects = cfg["rects"].copy()
            rects[2] = bad
            _raises(fd, E_ARG, "member 2: source", lambda: b.set_sources(rects))
        for call, match in ((lambda: b.set_pml(3), "lattice mode"), (b.download_ezx, "lattice mode"),
                            (lambda: b.set_hz_bloch_phase(0.3), "lattice mode"),
                            (lambda: b.set_hz_flux_lines([("row", 10, 0, C - 1)], [3e11]), "lattice mode"),
                            (lambda: b.set_hz_bloch_flux_lines([("row", 10, 0, C - 1)], [3e11]), "lattice mode"),
                            (lambda: b.set_dft(3e11), "lattice mode"),
                            (lambda: b.set_point_sources(np.array([[8, 1]]), np.ones((1, 1))), "lattice mode"),
                            (lambda: b.run(2, None, np.zeros((1, 2))), "lattice mode"),
                            (lambda: b.set_polarization("ez"), "lattice mode"),
                            (lambda: b.set_lattice_phase(0.1, 0.2), 'boundary="lattice"'),
                            (lambda: b.set_bloch_phase(0.5), "lattice mode")):
            _raises(fd, E_STATE, match, call)
        assert b.dispersive and b.polarization == "hz" and b.lds_bytes == lds and b.hz_lattice
        b.run(cfg["n"], cfg["amps"])
        _matches(_results(b), want)


def test_the_mode_is_refused_where_it_cannot_be_entered(fd):
    R, C = 23, 19
    c = np.ones(B)
    with _engine(fd, B, R, C, np.float32) as b:
        L = b._lib
        cp = c.ctypes.data_as(L.fdtd2d_batch_set_hz_lattice.argtypes[1])
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE       # no materials yet
        cfg = _cfg("23x19", np.float32)
        b.set_materials(cfg["eps"], cfg["mu"])
        assert L.fdtd2d_batch_set_hz_lattice(b._h, None, None, None, None) == 0 and not b.hz_lattice
        b.set_pml(4)                                              # a layer
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE
        _raises(fd, E_STATE, "has no layer", lambda: b.set_hz_lattice_phase(0.1, 0.2))
        b.clear_pml()
        b.set_hz_bloch_phase(0.3)                                  # the phase of fdtd2d_batch_hz_bloch.h
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE
        _raises(fd, E_STATE, "Bloch phase", lambda: b.set_hz_lattice_phase(0.1, 0.2))
        b.set_hz_bloch_flux_lines([("row", 10, 0, C - 1)], [3e11])
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE
        b.set_hz_bloch_flux_lines(None, None).set_hz_bloch_phase(None)
        b.set_hz_flux_lines([("row", 10, 0, C - 1)], [3e11])       # flux lines of fdtd2d_batch_hz_flux.h
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE
        _raises(fd, E_STATE, "flux lines", lambda: b.set_hz_lattice_phase(0.1, 0.2))
        b.set_hz_flux_lines(None, None)
        b.set_dft(3e11)                                            # the whole-grid transform
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE
        b.set_dft(None)
        b.set_point_sources(np.array([[8, 1]]), np.ones((1, 1)))  # point sources
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE
        _raises(fd, E_STATE, "point source", lambda: b.set_hz_lattice_phase(0.1, 0.2))
        b.set_point_sources(None)
        b.set_dft_window((R - 5, 3, 5, 5), [3e11])                 # a window in the image row
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_ARG
        b.set_dft_window((3, 3, 5, 5), [3e11]).set_probes([(R - 1, 2)], 4)
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_ARG
        b.set_probes([(R - 2, 2)], 4).set_sources(np.array([[R - 2, 2, 2, 2]] * B))
        assert L.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_ARG
        assert "member 0" in L.fdtd2d_batch_last_error(b._h).decode()
        assert not b.hz_lattice and not b.hz_bloch and b.info(25) == 0
        b.set_sources(np.array([[R - 3, 2, 2, 2]] * B))
        b.set_hz_lattice_phase(0.1, 0.2)
        assert b.hz_lattice and b.info(25) == 1 and not b.hz_bloch and not b.lattice and not b.bloch
    with fd.BatchEngine(B, R, C, DT, DX, boundary="periodic") as b:          # the Ez polarisation
        b.set_materials(cfg["eps"], cfg["mu"])
        assert b._lib.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE and not b.hz_lattice
        _raises(fd, E_STATE, "needs the Hz polarisation", lambda: b.set_hz_lattice_phase(0.3, 0.1))
    with fd.BatchEngine(B, R, C, DT, DX, boundary="pml") as b:               # no periodic columns
        b.set_polarization("hz").set_materials(cfg["eps"], cfg["mu"])
        assert b._lib.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE and not b.hz_lattice
    with fd.BatchEngine(B, R, C, DT, DX, boundary="lattice") as b:           # the Ez lattice mode stays closed to Hz
        _raises(fd, E_STATE, "lattice", lambda: b.set_polarization("hz"))
        assert b.lattice and not b.hz_lattice
        assert b._lib.fdtd2d_batch_set_hz_lattice(b._h, cp, cp, cp, cp) == E_STATE


def test_run_fdtd_batch_takes_the_hz_lattice_phase(fd):
    _exact_only(fd)
    from fdtd2d_amd.api import MU0
    cfg = _cfg("23x19", np.float64, n=30, state=False)
    eps = cfg["eps"].astype(np.float64)
    out = fd.run_fdtd_batch(eps, nsteps=30, sources=cfg["rects"], fc=35e9, dtype=np.float64, boundary="periodic", pml_cells=0,
                            polarization="hz", hz_lattice_phase=(PHI_R, PHI_C), source_weights="ramp",
                            dispersion=(cfg["wp2"], GAMMA, OMEGA0), conductivity=cfg["sigma"], probes=cfg["probes"],
                            dft_window=cfg["window"], window_omegas=cfg["omegas"])
    ref = HzLatticeOracle(B, cfg["R"], cfg["C"], DT, DX, dtype=np.float64)
    ref.set_materials(eps, MU0).set_sources(cfg["rects"]).set_hz_lattice_phase(PHI_R, PHI_C).set_hz_bloch_source("ramp")
    ref.set_conductivity(cfg["sigma"]).set_dispersion(cfg["wp2"], GAMMA, OMEGA0)
    ref.set_dft_window(cfg["window"], cfg["omegas"]).set_probes(cfg["probes"], 30)
    ref.run(30, np.tile([fd.ricker_amplitude(i * DT, 35e9) for i in range(30)], (B, 1)))
    assert len(out) == 5
    for a, w in zip(out[:3] + out[4:], ref.download() + (ref.read_probes(),)):
        assert np.iscomplexobj(a) and np.array_equal(a, w)
    assert np.abs(out[3] - ref.read_dft_window()).max() <= 1e-12 * np.abs(ref.read_dft_window()).max()
    assert np.any(ref.Jx_i) and np.any(ref.Jy_i)


# ---- 6. the fused build -----------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_hz_lattice as t
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
print("HZ_LATTICE_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's complex Hz after 300 steps against the exact stand-in's; in that build too the resident and the
    streamed path agree bit for bit.  The device runs in a process of its own, which selects the fused library."""
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(tmp_path)!r}\n" + CHILD],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC="fused"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("HZ_LATTICE_RESULT ")][-1][18:])
    assert r["arithmetic"] == "fused" and r["paths"] is True, r
    worst = {}
    for k, dtype in (("f32", np.float32), ("f64", np.float64)):
        f = np.load(tmp_path / f"hz_{k}.npy").astype(np.complex128)
        e = np.concatenate([_stand_in(case, dtype, n=NSTEPS_FUSED, state=False)["fields"][0].reshape(B, -1)
                            for case in FUSED_CASES], axis=1).astype(np.complex128)
        n1 = CASES[FUSED_CASES[0]][0] * CASES[FUSED_CASES[0]][1]   # the two cases' cells lie side by side in a row
        worst[k] = max(np.abs(f[m, s] - e[m, s]).max() / np.abs(e[m, s]).max()
                       for m in range(B) for s in (slice(0, n1), slice(n1, None)))
        print(f"fused vs the exact stand-in, Hz {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
