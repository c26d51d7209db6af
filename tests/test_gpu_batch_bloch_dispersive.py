"""GPU: the Drude-Lorentz pole of Bloch and lattice batches (fdtd2d_batch_bloch_dispersive.h,
kernels_batch_bloch_dispersive.hpp).

Complex Ez, Hx, Hy, Ezx (Bloch), Jh, Q and the probe traces equal the stand-in of tests/oracle_batch_bloch_dispersive.py
bit for bit (exact build), window DFTs and bloch_probe_spectra to 1e-12 (the device's float64 cos and sin are not
NumPy's, the project's bound for every window DFT): both dtypes; resident in two runs, 7 steps per launch, global
accumulators, and streamed; 5 members with distinct (gamma, omega0, phases), one of them a Drude pole, one lossless and
one with wp2 = 0; random wp2 wherever it may be, the seams and the images included; a conductivity, complex amplitudes,
ramp weights, a window, three probes and a random uploaded complex state with Jh and Q.  The shapes: Bloch 23 x 11 and
29 x 13, each with a 4-cell layer and with PEC rows; lattice 11 x 13, 23 x 19 (128 threads, 128 % 19 = 14: the cell walk
carries) and 37 x 31 (4 cells per thread).  The largest member the capacity rule admits (read from the library) runs
resident in one launch, one row more streams.  The exact properties of tests/test_batch_bloch_dispersive_cpu.py hold on the
device; a Bloch member needs 13 rows to have a row that takes the plain update, so its properties run on 13 x 11 alone.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_BOUND."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_batch_bloch_dispersive_cpu as cpu

pytestmark = pytest.mark.gpu

ROOT = cpu.ROOT
DT, DX, LDS_LIMIT = cpu.DT, cpu.DX, 163840
E_ARG, E_STATE = -1, -4
EPS0, MU0 = cpu.EPS0, cpu.MU0
# kind, rows, columns, layer
CASES = {"bloch_23x11_pml": ("bloch", 23, 11, 4), "bloch_23x11_pec": ("bloch", 23, 11, 0),
         "bloch_29x13_pml": ("bloch", 29, 13, 4), "bloch_29x13_pec": ("bloch", 29, 13, 0),
         "lattice_11x13": ("lattice", 11, 13, 0), "lattice_23x19": ("lattice", 23, 19, 0),
         "lattice_37x31": ("lattice", 37, 31, 0)}
# The fused build evaluates the multiply-add pairs of the step, of the pole (batch_disp_j, batch_lossy_e) and of the seams'
# rotations as one fma each, so its results differ from the exact build's by rounding.  The quantity is: complex Ez after
# 300 steps from rest, the 5 members of cpu.members on 29 x 13 with a 4-cell layer (Bloch) and on 37 x 31 (lattice), worst
# member, max|fused - exact| / max|exact|.  FUSED_MEASURED is what test_fused_build_within_its_bounds printed on its first
# MI355X run; the bounds are ten times that, the project's margin (tests/test_gpu_batch_lattice.py).
NSTEPS_FIELD = 300
FUSED_CASES = {"bloch": "bloch_29x13_pml", "lattice": "lattice_37x31"}
FUSED_MEASURED = {"bloch_f32": 3.144e-07, "bloch_f64": 7.250e-16, "lattice_f32": 4.914e-07, "lattice_f64": 7.169e-16}
FUSED_BOUND = {k: 10 * v for k, v in FUSED_MEASURED.items()}      # 3.1e-6, 7.3e-15, 4.9e-6, 7.2e-15


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _threads(cells):
    return min(1024, -(-(-(-cells // 4)) // 64) * 64)


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_within_its_bounds")


def _rule(kind, esz, R, Cc, nf=0, window_cells=0, pole=True):
    """The capacity rule, restated: 16 arrays (Bloch: its 11, Jh and Q twice, cj) or 14 (lattice: its 9 and those five),
    the row factors of a Bloch batch, 16 (C-1) bytes of source weights beside the phasor table, twice the accumulators.
    Returns (arrays, bytes beside the arrays, accumulator bytes)."""
    arrays = (16 if pole else 11) if kind == "bloch" else (14 if pole else 9)
    beside = (_seg(4 * R, esz) if kind == "bloch" else 0) + 16 * nf + 16 * (Cc - 1)
    return arrays, beside, 2 * 16 * nf * window_cells


def _expect_path(b, kind, nf, window_cells, never=False, lds_allowed=True, pole=True):
    esz, R, Cc = b.dtype.itemsize, b.rows, b.cols
    arrays, beside, acc = _rule(kind, esz, R, Cc, nf, window_cells, pole)
    fields = arrays * _seg(R * Cc, esz)
    resident = fields + beside <= LDS_LIMIT and not never
    in_lds = bool(nf) and lds_allowed and fields + beside + acc <= LDS_LIMIT
    assert b.dispersive == pole and b.periodic and b.lattice == (kind == "lattice") and b.bloch == (kind == "bloch")
    assert b.lds_bytes == fields + beside + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - beside) // arrays // 16 * 16 // esz
    assert b.resident == resident
    assert b.window_in_lds == (in_lds and resident)
    return resident


def _device_run(fd, case, dtype, splits, resident=None, spl=None, lds=True, monitors=True, **mk):
    """cpu.members on the device, run in `splits`; asserts the path the rule gives and its launch count."""
    kind, R, Cc, layer = case if isinstance(case, tuple) else CASES[case]
    n = sum(splits)
    b, amps = cpu.members(fd.BatchEngine, kind, dtype, R, Cc, n, layer, monitors=monitors, **mk)
    with b:
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        pole = mk.get("pole", True)
        path = _expect_path(b, kind, 2 if monitors else 0, 12, never=resident == 0, lds_allowed=lds, pole=pole)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, amps[:, done:done + k])
            done += k
        if path:      # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * sum(splits)
        out = cpu.outputs(b, kind, pole=pole, monitors=monitors)
        if monitors:
            out["spectra"] = b.bloch_probe_spectra(2 * np.pi * np.array([30e9, 55e9]))
        out["path"], out["in_lds"] = path, b.window_in_lds
        return out


def _stand_in(case, dtype, n, monitors=True, **mk):
    kind, R, Cc, layer = case if isinstance(case, tuple) else CASES[case]
    ref, amps = cpu.members(cpu.oracle_for(kind), kind, dtype, R, Cc, n, layer, monitors=monitors, **mk)
    ref.run(n, amps)
    out = cpu.outputs(ref, kind, pole=mk.get("pole", True), monitors=monitors)
    if monitors:
        out["spectra"] = ref.bloch_probe_spectra(2 * np.pi * np.array([30e9, 55e9]))
    return out


EXACT_KEYS = ("Ez", "Hx", "Hy", "Ezx", "Jh", "Q", "probes")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in EXACT_KEYS + ("dft",) if k in a)


def _agrees(got, ref):
    """Fields, the pole's state and the probes bit for bit, the window DFT and the spectra to 1e-12; both parts moved."""
    for k in EXACT_KEYS:
        if k in ref:
            assert np.iscomplexobj(got[k]) and np.array_equal(got[k], ref[k]), k
    for k in ("Ez", "Jh", "Q"):
        assert np.abs(got[k].real).max() > 0 and np.abs(got[k].imag).max() > 0, k
    for k in ("dft", "spectra"):
        if k in ref:
            assert np.abs(got[k] - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), k


# ---- 1. against the stand-in ------------------------------------------------------------------------------------------------

N_STEPS = 50


@functools.lru_cache(maxsize=None)
def _reference(dtype, case):
    return _stand_in(case, dtype, N_STEPS)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_runs_match_the_stand_in_on_every_path(fd, dtype, case):
    _exact_only(fd)
    kind, R, Cc, _ = CASES[case]
    cells, threads = R * Cc, _threads(R * Cc)
    if case == "lattice_23x19":
        assert threads % Cc != 0                                      # the walk carries
    if case == "lattice_37x31":
        assert -(-cells // threads) == 4                              # 4 cells per thread
    ref = _reference(dtype, case)
    variants = dict(resident=dict(), spl7=dict(spl=7), global_acc=dict(lds=False), streamed=dict(resident=0))
    for name, kw in variants.items():
        got = _device_run(fd, case, dtype, (27, 23), **kw)
        assert got["path"] == (name != "streamed"), name
        assert got["in_lds"] == (name in ("resident", "spl7")), name
        _agrees(got, ref)


@pytest.mark.parametrize("case", ["bloch_23x11_pml", "lattice_23x19"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_runs_are_bit_identical_on_every_path(fd, dtype, case):
    """In either build: streamed, split runs, steps per launch and the accumulators' place change no bit."""
    base = _device_run(fd, case, dtype, (60,))
    assert base["path"] and base["in_lds"]
    variants = dict(streamed=dict(resident=0), spl=dict(spl=7), split=dict(splits=(1, 32, 27)), global_acc=dict(lds=False))
    for name, kw in variants.items():
        splits = kw.pop("splits", (60,))
        got = _device_run(fd, case, dtype, splits, **kw)
        assert got["path"] == (name != "streamed"), name
        assert _same(base, got), name


# ---- 2. the images of Jh and Q ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bloch", "lattice"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_images_of_the_state_are_rotated_on_download_and_rewritten_on_upload(fd, dtype, kind):
    B, R, Cc, n = 3, 23, 19, 12
    lattice = kind == "lattice"
    rng = np.random.default_rng(3)
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(cpu.cdtype(dtype))
    Jh, Q = cplx(B, R, Cc), cplx(B, R, Cc)          # their image slots hold garbage: an upload overwrites them
    rot_r = (np.array([0.0, -1.0, 0.6]), np.array([1.0, 0.0, 0.8]))          # i, -1 and a general rotation
    rot_c = (np.array([-1.0, 0.0, 0.28]), np.array([0.0, 1.0, 0.96]))        # -1, i and a general rotation
    g = 0 if lattice else 6
    wp2 = np.zeros((B, R, Cc))
    wp2[:, g:R - g] = 2e25 * rng.random((B, R - 2 * g, Cc))
    amps = rng.standard_normal((B, n)) + 0j

    def drive(e):
        e.set_materials(np.full((B, R, Cc), EPS0), MU0)
        if lattice:
            e.set_lattice_phase(0, 0, rotation=(rot_r, rot_c))
        else:
            e.set_bloch_phase(None, rotation=rot_c)
        e.set_sources(np.array([(g + 1, 2, 1, 3)] * B))
        e.set_bloch_dispersion(wp2, 1e11, 2e11)
        return e

    with drive(fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="lattice" if lattice else "periodic")) as b:
        assert not any(np.any(a) for a in b.download_bloch_dispersion())
        b.upload_bloch_dispersion(Jh, Q)
        ref = drive(cpu.oracle_for(kind)(B, R, Cc, DT, DX, dtype=dtype)).upload_bloch_dispersion(Jh, Q)
        for step in range(2):
            got, want = b.download_bloch_dispersion(), ref.download_bloch_dispersion()
            for name, a, w, given in zip(("Jh", "Q"), got, want, (Jh, Q)):
                assert np.array_equal(a[:2], w[:2]), name               # exact rotations
                if fd.ARITHMETIC == "exact":
                    assert np.array_equal(a[2], w[2]), name
                else:
                    assert np.abs(a[2] - w[2]).max() <= 4 * np.finfo(dtype).eps * np.abs(w[2]).max(), name
                rows = slice(0, R - 1) if lattice else slice(0, R)
                # member 0: rho_c = -1 (and rho_r = i), member 1: rho_c = i (and rho_r = -1): the images, exactly
                assert np.array_equal(a[0, rows, -1], -a[0, rows, 0]) and np.array_equal(a[1, rows, -1], 1j * a[1, rows, 0])
                if lattice:
                    assert np.array_equal(a[0, -1, :-1], 1j * a[0, 0, :-1]) and np.array_equal(a[1, -1, :-1], -a[1, 0, :-1])
                    assert a[0, -1, -1] == -1j * a[0, 0, 0] and a[1, -1, -1] == -1j * a[1, 0, 0]
                if step == 0:                                           # the upload kept the period and dropped the garbage
                    assert np.array_equal(a[:, rows, :-1], given[:, rows, :-1]) and not np.array_equal(a, given)
            b.run(n, amps)                                              # and again after a run
            ref.run(n, amps)
            assert step == 1 or np.any(b.download_bloch_dispersion()[0] != got[0])
        cur = b.download_bloch_dispersion()[0]
        b.upload_bloch_dispersion(Q=Q.real)                             # a real upload has a zero imaginary part; Jh stays
        jh2, q2 = b.download_bloch_dispersion()
        assert not q2[:, :R - 1, :Cc - 1].imag.any() and np.array_equal(jh2, cur)
        b.reset()
        assert not any(np.any(a) for a in b.download_bloch_dispersion()) and b.dispersive


# ---- 3. the paths ---------------------------------------------------------------------------------------------------------------

def test_a_member_resident_without_the_pole_streams_with_it(fd):
    dtype, case, n = np.float32, ("lattice", 61, 61, 0), 4             # 3721 cells: 9 arrays fit, 14 do not
    a = _device_run(fd, case, dtype, (n,), monitors=False, pole=False)
    b = _device_run(fd, case, dtype, (n,), monitors=False)
    assert a["path"] and not b["path"]
    if fd.ARITHMETIC == "exact":
        _agrees(b, _stand_in(case, dtype, n, monitors=False))


def _largest_rows(fd, kind, dtype, Cc):
    """The most rows of a Cc-column member that the rule admits with the pole and no monitors: restated here, then
    checked against the library's own figure, read at run time."""
    esz = np.dtype(dtype).itemsize

    def fits(R):
        arrays, beside, _ = _rule(kind, esz, R, Cc)
        return R * Cc <= (LDS_LIMIT - beside) // arrays // 16 * 16 // esz
    R = max(r for r in range(13, 400) if fits(r))
    for rows, want in ((R, True), (R + 1, False)):
        b, _ = cpu.members(fd.BatchEngine, kind, dtype, rows, Cc, 1, 4 if kind == "bloch" else 0, monitors=False, state=False)
        with b:
            assert (rows * Cc <= b.resident_max_cells) == want and b.resident == want
    return R


@pytest.mark.parametrize("kind", ["bloch", "lattice"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_largest_member_is_resident_and_one_row_more_streams(fd, dtype, kind):
    _exact_only(fd)
    Cc, n = 41, 6
    R = _largest_rows(fd, kind, dtype, Cc)
    # about 2560 float32 / 1280 float64 cells (Bloch), 2924 / 1462 (lattice), before the factors and tables come off
    lo, hi = {("bloch", 4): (2400, 2560), ("bloch", 8): (1200, 1280), ("lattice", 4): (2800, 2926),
              ("lattice", 8): (1400, 1463)}[kind, np.dtype(dtype).itemsize]
    assert lo < R * Cc <= hi and -(-R * Cc // _threads(R * Cc)) <= 4      # 4 cells per thread is the only instance
    for rows, resident in ((R, True), (R + 1, False)):
        case = (kind, rows, Cc, 4 if kind == "bloch" else 0)
        got = _device_run(fd, case, dtype, (n,), monitors=False)          # one launch, or two per step: asserted there
        assert got["path"] == resident, rows
        _agrees(got, _stand_in(case, dtype, n, monitors=False))


def test_more_members_than_one_round_of_workgroups(fd):
    dtype, case, B, n = np.float32, CASES["bloch_23x11_pml"], 300, 6
    a = _device_run(fd, case, dtype, (n,), monitors=False, B=B)
    b = _device_run(fd, case, dtype, (n,), monitors=False, B=B, resident=0)
    assert a["path"] and not b["path"] and _same(a, b)
    assert len({a["Ez"][m].tobytes() for m in range(B)}) == B
    if fd.ARITHMETIC == "exact":
        _agrees(a, _stand_in(case, dtype, n, monitors=False, B=B))


# ---- 4. equivalences ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["bloch_23x11_pml", "lattice_23x19"])
@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
def test_zero_strength_and_removal_equal_the_engine_without_the_pole(fd, case, resident):
    """In either build: with wp2 = 0 and zero state jn is exactly zero, and a removed pole leaves no trace."""
    dtype, n = np.float32, 40
    kind, R, Cc, layer = CASES[case]
    plain = _device_run(fd, case, dtype, (n,), resident=resident, pole=False, state="fields")
    zero = _device_run(fd, case, dtype, (n,), resident=resident, wp2_zero=True, state="fields")
    for k in plain:
        if k in EXACT_KEYS + ("dft", "spectra"):
            assert np.array_equal(plain[k], zero[k]), k
    assert not np.any(zero["Jh"]) and not np.any(zero["Q"]) and np.abs(zero["Ez"].imag).max() > 0
    b, amps = cpu.members(fd.BatchEngine, kind, dtype, R, Cc, n, layer, state="fields")
    with b:
        b.set_option(resident=resident)
        arrays = b.lds_bytes
        b.set_bloch_dispersion(None)
        assert not b.dispersive and b.lds_bytes < arrays
        with pytest.raises(fd.Fdtd2dError, match="no pole is set"):
            b.download_bloch_dispersion()
        _expect_path(b, kind, 2, 12, never=resident == 0, pole=False)
        b.run(n, amps)
        removed = cpu.outputs(b, kind, pole=False)
        for k in removed:
            assert np.array_equal(removed[k], plain[k]), k
        b.set_bloch_dispersion(0.0)                                     # and set again: the state starts from zero
        assert b.dispersive and not any(np.any(a) for a in b.download_bloch_dispersion())


@pytest.mark.parametrize("kind", ["bloch", "lattice"])
def test_new_rotations_keep_the_pole_and_its_state(fd, kind):
    _exact_only(fd)
    dtype, n = np.float64, 30
    case = CASES["bloch_23x11_pml" if kind == "bloch" else "lattice_23x19"]
    _, R, Cc, layer = case
    new = 0.2 + 0.5 * np.arange(5)
    res = []
    for engine in (fd.BatchEngine, cpu.oracle_for(kind)):
        e, amps = cpu.members(engine, kind, dtype, R, Cc, 2 * n, layer)
        with e:
            e.run(n, amps[:, :n])
            if kind == "bloch":
                e.set_bloch_phase(new)
            else:
                e.set_lattice_phase(-new, new + 0.3)
            e.set_bloch_source("ramp")
            assert e.dispersive
            mid = e.download_bloch_dispersion()
            e.run(n, amps[:, n:])
            res.append((cpu.outputs(e, kind), mid))
    (got, mid_g), (ref, mid_r) = res
    for a, w in zip(mid_g, mid_r):
        assert np.array_equal(a, w)
    _agrees(got, ref)


def _engine(fd, resident):
    def make(*a, **k):
        return fd.BatchEngine(*a, **k).set_option(resident=resident)
    return make


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_negated_phases_give_the_conjugate_on_the_device(fd, dtype, resident):
    cpu.check_conjugate(_engine(fd, resident), "lattice", dtype, 11, 13)
    cpu.check_conjugate(_engine(fd, resident), "lattice", dtype, 13, 11)
    cpu.check_conjugate(_engine(fd, resident), "bloch", dtype, 13, 11)            # row 6 alone takes the plain update
    cpu.check_conjugate(_engine(fd, resident), "bloch", dtype, 13, 11, layer=4)


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_exact_rotations_match_their_supercell_on_the_device(fd, dtype, resident):
    cpu.check_supercell_exact(_engine(fd, resident), "lattice", dtype, 11, 13)    # against 21 x 37
    cpu.check_supercell_exact(_engine(fd, resident), "lattice", dtype, 13, 11)    # against 25 x 31
    cpu.check_supercell_exact(_engine(fd, resident), "bloch", dtype, 13, 11)      # period 10 against period 20


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))


def _state(b, kind):
    out = cpu.outputs(b, kind)
    return [out[k] for k in sorted(out)] + [b.lds_bytes, b.resident_max_cells, b.dispersive, b.step_count]


@pytest.mark.parametrize("kind", ["bloch", "lattice"])
def test_the_library_refuses_what_the_pole_excludes(fd, kind):
    _exact_only(fd)
    from fdtd2d_amd import _abi
    dtype, n = np.float32, 12
    case = CASES["bloch_23x11_pml" if kind == "bloch" else "lattice_23x19"]
    _, R, Cc, layer = case
    B = 5
    one, zero, w11 = np.ones(B), np.zeros(B), np.full(B, 1e11)
    b, amps = cpu.members(fd.BatchEngine, kind, dtype, R, Cc, n, layer)
    ref, _ = cpu.members(cpu.oracle_for(kind), kind, dtype, R, Cc, n, layer)
    with b:
        lib, h = b._lib, b._h
        err = lambda: lib.fdtd2d_batch_last_error(h).decode()
        b.run(5, amps[:, :5])
        ref.run(5, amps[:, :5])
        assert b.info(_abi.BATCH_INFO_DISPERSIVE) == 1
        state = _state(b, kind)
        cells, wts, chan = np.array([[8, 3]] * B, dtype=np.int32), np.ones((B, 1)), np.zeros((1, 4))
        out, f32 = np.zeros(4 * B * R * Cc), np.zeros((B, R, Cc), np.float32)
        win = np.array([8, 0, 2, 2], np.int32)
        refused = [                                                     # E_STATE, named as a dispersive pole excludes them
            (lambda: lib.fdtd2d_batch_set_periodic(h, 0), "dispersive pole"),
            (lambda: lib.fdtd2d_batch_set_dispersion(h, f32.ctypes.data, 0, dp(w11), dp(zero)), "fdtd2d_batch_set_bloch_dispersion"),
            (lambda: lib.fdtd2d_batch_set_dispersion(h, None, 0, None, None), "fdtd2d_batch_set_bloch_dispersion"),
            (lambda: lib.fdtd2d_batch_set_dispersion_window(h, ip(win), f32.ctypes.data, 0),
             "fdtd2d_batch_set_bloch_dispersion_window"),
            (lambda: lib.fdtd2d_batch_transfer_dispersion(h, f32.ctypes.data, None, 0, 0),
             "fdtd2d_batch_transfer_bloch_dispersion"),
        ]
        pole_or_mode = "dispersive pole" if kind == "bloch" else "lattice mode"       # the lattice mode refuses these first
        refused += [
            (lambda: lib.fdtd2d_batch_set_bloch_point_sources(h, 1, ip(cells), 1, dp(wts)), pole_or_mode),
            (lambda: lib.fdtd2d_batch_run_bloch_channels(h, 4, None, None, dp(chan), 0, 0), pole_or_mode),
            (lambda: lib.fdtd2d_batch_hold_bloch_window(h), pole_or_mode),
            (lambda: lib.fdtd2d_batch_bloch_window_product(h, dp(one), dp(zero), dp(out)), pole_or_mode),
        ]
        if kind == "bloch":
            refused.append((lambda: lib.fdtd2d_batch_set_bloch(h, None, None), "dispersive pole"))
        else:
            refused.append((lambda: lib.fdtd2d_batch_set_lattice(h, None, None, None, None), "dispersive pole"))
        for k, (call, what) in enumerate(refused):
            assert call() == E_STATE and what in err(), (k, err())
        # through the Python wrappers (the adjoint helpers go through them) the same refusals arrive as Fdtd2dError
        for call in (lambda: b.set_bloch_point_sources([(8, 3)], np.ones((1, 1))), lambda: b.hold_bloch_window(),
                     lambda: b.run_bloch_channels(4, None, np.zeros((0, 4))), lambda: b.bloch_window_product(np.ones(2))):
            with pytest.raises(fd.Fdtd2dError) as ei:
                call()
            assert ei.value.code == E_STATE
        # E_ARG, naming the member
        ok = ref.wp2.copy()
        g = 0 if kind == "lattice" else 6
        bad = [(-1.0, (1, 8, 3), "member 1: wp2 must be >= 0"), (np.nan, (3, 8, 3), "member 3: wp2 must be >= 0"),
               (20.0 / DT ** 2, (4, 8, 3), "member 4: the pole at cell (8,3) is unstable")]
        if kind == "bloch":
            bad += [(1e22, (1, 5, 3), "member 1: wp2 is non-zero at cell (5,3)"),
                    (1e22, (2, R - 6, 0), f"member 2: wp2 is non-zero at cell ({R - 6},0)")]
        gam, om0 = np.resize(cpu.GAMMA, B), np.resize(cpu.OMEGA0, B)
        for v, at, msg in bad:
            w = ok.copy()
            w[at] = v
            assert lib.fdtd2d_batch_set_bloch_dispersion(h, w.ctypes.data, 1, dp(gam), dp(om0)) == E_ARG and msg in err(), err()
            assert lib.fdtd2d_batch_set_bloch_dispersion_window(
                h, ip(np.array([at[1], at[2], 1, 1], np.int32)), np.full(B, v).ctypes.data, 1) == E_ARG, msg
        for gv, ov, msg in ((-1.0, 0.0, "member 2: gamma"), (np.inf, 0.0, "member 2: gamma"), (0.0, -1.0, "member 2: omega0"),
                            (0.0, np.nan, "member 2: omega0"), (0.0, 2.0 / DT, "is unstable")):
            g2, o2 = gam.copy(), om0.copy()
            g2[2], o2[2] = gv, ov
            if msg == "is unstable":
                o2[:] = ov
            assert lib.fdtd2d_batch_set_bloch_dispersion(h, ok.ctypes.data, 1, dp(g2), dp(o2)) == E_ARG and msg in err(), err()
        assert lib.fdtd2d_batch_set_bloch_dispersion(h, ok.ctypes.data, 1, dp(gam), None) == E_ARG and "all be given" in err()
        assert lib.fdtd2d_batch_set_bloch_dispersion_window(h, ip(np.array([R - 1, 0, 2, 2], np.int32)), f32.ctypes.data,
                                                            0) == E_ARG and "outside" in err()
        # materials that break the pole's stability: refused, the batch as it was
        thin = np.full((B, R, Cc), EPS0 * 1e-3, np.float32)
        assert lib.fdtd2d_batch_set_materials(h, thin.ctypes.data, np.full((B, R, Cc), MU0, np.float32).ctypes.data, 0) == E_ARG
        assert "is unstable" in err()
        assert lib.fdtd2d_batch_set_eps_window(h, 8, 1, 1, 1, np.full(B, EPS0 * 1e-3, np.float32).ctypes.data, 0) == E_ARG
        assert "is unstable" in err()
        now = _state(b, kind)
        assert all(np.array_equal(x, y) for x, y in zip(state, now))
        # what keeps working, against the stand-in: new strengths in a window, a conductivity window, the layer of a Bloch
        # batch cleared and set again, the source weights, a new window and new probes, the spectra and the maxima
        for e in (b, ref):
            e.set_bloch_dispersion_window((8, 0, 2, 3), np.full((B, 2, 3), 1e24))
            e.set_conductivity_window((8, 1, 2, 2), np.full((B, 2, 2), 2.0))
            if kind == "bloch":
                e.clear_pml()
                e.set_pml(3, courant00=cpu.COURANT0)
            e.set_bloch_source(None)
            e.set_dft_window((9, 1, 2, 3), 2 * np.pi * np.array([40e9]))
            e.set_probes(np.array([(8, 0), (10, Cc - 2)]), n - 5)
        b.set_option(steps_per_launch=4)
        b.run(n - 5, amps[:, 5:])
        ref.run(n - 5, amps[:, 5:])
        got, want = cpu.outputs(b, kind), cpu.outputs(ref, kind)
        om = 2 * np.pi * np.array([40e9])
        got["spectra"], want["spectra"] = b.bloch_probe_spectra(om), ref.bloch_probe_spectra(om)
        _agrees(got, want)
        assert np.array_equal(b.bloch_field_absmax("Ez"), ref.bloch_field_absmax("Ez"))
    # a batch with real fields: pointed to fdtd2d_batch_set_dispersion; with what the pole excludes already there
    with fd.BatchEngine(2, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as p:
        lib, h = p._lib, p._h
        err = lambda: lib.fdtd2d_batch_last_error(h).decode()
        p.set_materials(None, None)
        z2, w2 = np.zeros(2), np.zeros((2, R, Cc))
        assert lib.fdtd2d_batch_set_bloch_dispersion(h, w2.ctypes.data, 1, dp(z2), dp(z2)) == E_STATE
        assert "fdtd2d_batch_set_dispersion" in err() and not p.dispersive
        assert lib.fdtd2d_batch_set_bloch_dispersion(h, None, 1, None, None) == E_STATE
        assert lib.fdtd2d_batch_transfer_bloch_dispersion(h, w2.ctypes.data, None, None, None, 1, 0) == E_STATE
        p.set_bloch_phase(0.4)
        assert lib.fdtd2d_batch_set_bloch_dispersion_window(h, ip(np.array([8, 0, 1, 1], np.int32)), z2.ctypes.data, 1) == E_STATE
        assert "no pole is set" in err()
        assert lib.fdtd2d_batch_transfer_bloch_dispersion(h, w2.ctypes.data, None, None, None, 1, 0) == E_STATE
        assert lib.fdtd2d_batch_set_dispersion(h, w2.ctypes.data, 1, dp(z2), dp(z2)) == E_STATE       # as before this pole
        assert "Bloch phase" in err()
        p.set_bloch_point_sources([(8, 3)], np.ones((1, 1)))
        assert lib.fdtd2d_batch_set_bloch_dispersion(h, w2.ctypes.data, 1, dp(z2), dp(z2)) == E_STATE and "point sources" in err()
        p.set_bloch_point_sources(None).set_dft_window((8, 0, 2, 2), [1e11]).hold_bloch_window()
        assert lib.fdtd2d_batch_set_bloch_dispersion(h, w2.ctypes.data, 1, dp(z2), dp(z2)) == E_STATE and "held window" in err()
        assert not p.dispersive and p.bloch
        p.set_dft_window((8, 0, 2, 2), [1e11])                          # the held window goes with the window
        assert lib.fdtd2d_batch_set_bloch_dispersion(h, w2.ctypes.data, 1, dp(z2), dp(z2)) == 0 and p.dispersive
        assert lib.fdtd2d_batch_set_bloch_dispersion(h, None, 1, None, None) == 0 and not p.dispersive
        assert lib.fdtd2d_batch_set_bloch(h, None, None) == 0 and not p.bloch         # without the pole the phase goes off


def test_the_bloch_adjoint_helpers_refuse_an_engine_with_this_pole(fd):
    """An engine factory whose engines carry a phase and this pole: refused through the helpers' check of `dispersive`,
    before any run."""
    class Dispersive(fd.BatchEngine):
        ran = False

        def __init__(self, *a, **k):
            fd.BatchEngine.__init__(self, *a, **k)
            self.set_materials(None, None).set_bloch_phase(0.1).set_bloch_dispersion(0.0)

        def run(self, *a, **k):
            Dispersive.ran = True
            return fd.BatchEngine.run(self, *a, **k)

        run_bloch_channels = run

    eps = np.full((2, 23, 11), EPS0)
    args = dict(bloch_phase=0.3, nsteps=20, sources=np.array([[8, 0, 1, 10]] * 2), probes=np.array([(9, 3)]),
                omegas=2 * np.pi * np.array([40e9]), design=(10, 1, 3, 3), dt=DT, dx=DX, dtype=np.float64, pml_cells=4,
                engine=Dispersive)
    objective = lambda S: (np.abs(S).sum(axis=(1, 2)) ** 2, np.conj(S))
    for call in (lambda: fd.batch_bloch_gradient(eps, objective=objective, **args),
                 lambda: fd.BlochAdjointSession(eps, **args)):
        with pytest.raises(fd.Fdtd2dError, match="dispersive pole") as ei:
            call()
        assert ei.value.code == E_STATE
    assert not Dispersive.ran


# ---- 6. the run helper ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["periodic", "lattice"])
def test_run_fdtd_batch_takes_a_bloch_dispersion(fd, boundary):
    _exact_only(fd)
    dtype, (R, Cc), B, n = np.float64, (23, 19), 3, 40
    eps = np.full((B, R, Cc), EPS0)
    wp2 = np.zeros((B, R, Cc))
    wp2[:, 8:14, 5:11] = (2 * np.pi * 200e9) ** 2                     # a metal rod in the unit cell
    phase = np.array([0.0, 1.0, np.pi]) if boundary == "periodic" else (np.array([0.0, np.pi, np.pi]), np.array([0.0, 0.0, np.pi]))
    pole = (wp2, 1e11, 0.0)
    kw = dict(nsteps=n, sources=np.array([(7, 0, 1, Cc - 1)] * B), fc=60e9, dt=DT, dx=DX, dtype=dtype, boundary=boundary,
              pml_cells=4, dft_window=(15, 0, 2, 5), window_omegas=[2 * np.pi * 60e9], probes=[(6, 0), (15, 5)])
    Ez, Hx, Hy, W, tr = fd.run_fdtd_batch(eps, bloch_phase=phase, source_weights="ramp", bloch_dispersion=pole, **kw)
    plain = fd.run_fdtd_batch(eps, bloch_phase=phase, source_weights="ramp", **kw)
    assert not np.array_equal(plain[0], Ez)                             # the rod is seen
    amps = np.tile([fd.ricker_amplitude(i * DT, 60e9) for i in range(n)], (B, 1))
    res = []
    for engine in (fd.BatchEngine, cpu.oracle_for("lattice" if boundary == "lattice" else "bloch")):
        with engine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:      # driven by hand
            b.set_materials(eps, MU0)
            if boundary == "periodic":
                b.set_pml(4, courant00=cpu.COURANT0)
            b.set_sources(kw["sources"])
            if boundary == "lattice":
                b.set_lattice_phase(*phase)
            else:
                b.set_bloch_phase(phase)
            b.set_bloch_source("ramp").set_bloch_dispersion(*pole)
            b.set_dft_window(kw["dft_window"], 2 * np.pi * np.array([60e9])).set_probes(np.array(kw["probes"]), n)
            b.run(n, amps)
            res.append(b.download() + (b.read_dft_window(), b.read_probes()))
    for a, w in zip((Ez, Hx, Hy, W, tr), res[0]):
        assert np.iscomplexobj(a) and np.array_equal(a, w)
    for a, w in zip((Ez, Hx, Hy, tr), res[1][:3] + res[1][4:]):
        assert np.array_equal(a, w)
    assert np.abs(W - res[1][3]).max() <= 1e-12 * np.abs(W).max()
    assert np.abs(Ez[1:].imag).max() > 0 and not Ez[0].imag.any()      # a zero phase (Gamma) stays real


# ---- 7. the fused build ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_bloch_dispersive as t
out = {"arithmetic": fd.ARITHMETIC, "paths": True}
for kind, case in t.FUSED_CASES.items():
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        got = t._device_run(fd, case, dtype, (t.NSTEPS_FIELD,), state=False)
        np.save(f"{OUT}/field_{kind}_{name}.npy", got["Ez"])
        b = t._device_run(fd, case, dtype, (t.NSTEPS_FIELD,), state=False, resident=0)      # against streamed, in this build
        out["paths"] = out["paths"] and got["path"] and not b["path"] and t._same(got, b)
print("BLOCH_DISPERSIVE_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's complex Ez against the exact build's (which the stand-in pins), both on the device, each in a
    process of its own; in both builds the resident and the streamed path agree bit for bit."""
    res = {}
    tag = "BLOCH_DISPERSIVE_RESULT "
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith(tag)][-1][len(tag):])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"field_{k}.npy").astype(np.complex128) for k in FUSED_BOUND}
    worst = {}
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m] - e[m]).max() / np.abs(e[m]).max() for m in range(e.shape[0]))
        print(f"fused vs exact, complex Ez {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
