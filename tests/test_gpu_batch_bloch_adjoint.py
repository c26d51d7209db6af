"""GPU: point sources, the conjugate rotation, the held window and its product, probe spectra and field maxima of Bloch
batches (fdtd2d_batch_bloch_adjoint.h, kernels_batch_bloch_adjoint.hpp), and the gradients built on them.

Complex fields, Ezx and probe traces equal the stand-in of tests/oracle_batch_bloch_adjoint.py bit for bit (exact build),
window DFTs to 1e-12: both dtypes, resident, 7 steps per launch and streamed, 23 x 11 and 29 x 13 members (64 and 128
threads, neither a multiple of C), a 4-cell layer and PEC rows, 5 members with distinct phases, the rotation as given and
conjugated, complex rectangle amplitudes with ramp weights in the same run, 1, 6 and 32 channels (shared and per member),
and point cells in column 0 (the duplicated image entry), in column C-2, next to the layer, inside it and at a thread's
last slot.  The members are those of tests/test_gpu_batch_bloch.py.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's: see FUSED_BOUND."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_bloch_adjoint import BlochAdjointOracle
import test_batch_bloch_adjoint_cpu as acpu
import test_gpu_batch_bloch as gb
from test_batch_periodic_cpu import g_objective

pytestmark = pytest.mark.gpu

ROOT = gb.ROOT
DT, DX, LAYER, LDS_LIMIT, SHAPES = gb.DT, gb.DX, gb.LAYER, gb.LDS_LIMIT, gb.SHAPES
E_ARG, E_STATE = -1, -4
# The fused build evaluates the step's multiply-add pairs, the seam's rotations and the window product's terms as one fma
# each.  The quantities: complex Ez after 300 steps with point sources (5 members of 29 x 13, conjugate rotation, float32
# and float64), and both gradients of the 2-member float64 case below; each max|fused - exact| / max|exact|, worst
# member.  FUSED_MEASURED is what test_fused_build_within_its_bounds printed on its first MI355X run; the bounds are ten
# times that, the project's convention (a margin for box-to-box rounding in the order of the host-side sums).
NSTEPS_FIELD = 300
FUSED_MEASURED = {"field_f32": 9.630e-07, "field_f64": 2.368e-15, "grad_eps": 3.403e-15, "grad_sigma": 7.718e-16}
FUSED_BOUND = {k: 10 * v for k, v in FUSED_MEASURED.items()}


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def point_cells(R, Cc, layer=LAYER):
    """Column 0 (listed again at its image), column C-2, next to the layer, inside it in column 0, a thread's last slot."""
    nthr = min(1024, -(-(-(-R * Cc // 4)) // 64) * 64)
    last = ((R * Cc - 1) // nthr) * nthr + 5                 # a cell of the last slot of the cell walk
    last += 2 * (last % Cc == Cc - 1)                        # ... that is not in the image column
    cells = [(R // 2, 0), (R // 2 + 2, Cc - 2), (max(layer, 1), 3), (1, 0), (last // Cc, last % Cc)]
    assert all(c < Cc - 1 for _, c in cells) and len(set(cells)) == len(cells) and last // nthr == (R * Cc - 1) // nthr
    return np.array(cells)


def _cfg(fd, seed, B, R, Cc, dtype, n, nchan=6, per_member=False, cells=None):
    cfg = gb._cfg(fd, seed, B, R, Cc, dtype, n)
    rng = np.random.default_rng(seed + 1000)
    cfg["cells"] = point_cells(R, Cc) if cells is None else cells
    P = cfg["cells"].shape[-2]
    cfg["w"] = rng.standard_normal((B, P, nchan)) * 1e-3
    t = np.arange(n) * DT
    chan = np.stack([np.sin(2 * np.pi * 30e9 * (1 + 0.2 * k) * t + k) for k in range(nchan)])
    cfg["chan"] = np.stack([chan * (1 + 0.1 * m) for m in range(B)]) if per_member else chan
    return cfg


def _drive(b, cfg, layer, monitors=True, points=True):
    gb._drive(b, cfg, layer, monitors)
    if points:
        b.set_bloch_point_sources(cfg["cells"], cfg["w"])
    return b


def _expect_path(b, nf, window_cells, npts, never=False, lds_allowed=True):
    """gb._expect_path's rule with the 8 bytes per table entry of the point sources."""
    esz, R, Cc = b.dtype.itemsize, b.rows, b.cols
    fields = 11 * gb._seg(R * Cc, esz) + gb._seg(4 * R, esz)
    table, acc = 16 * nf + 8 * npts + 16 * (Cc - 1), 2 * 16 * nf * window_cells
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = bool(nf) and lds_allowed and fields + table + acc <= LDS_LIMIT
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - gb._seg(4 * R, esz) - table) // 11 // 16 * 16 // esz
    assert b.resident == resident and b.window_in_lds == (in_lds and resident)
    return resident


def _table_entries(cfg):
    """Entries per member: the cells and the images of those in column 0, the most any member has."""
    c = np.broadcast_to(cfg["cells"], (cfg["eps"].shape[0],) + cfg["cells"].shape[-2:])
    return c.shape[1] + int((c[..., 1] == 0).sum(axis=1).max())


def _device_run(fd, dtype, R, Cc, cfg, splits, layer=LAYER, monitors=True, resident=None, spl=None, lds=True,
                conjugate=False):
    B = cfg["eps"].shape[0]
    from fdtd2d_amd import _abi
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        _drive(b, cfg, layer, monitors)
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        assert b.info(_abi.BATCH_INFO_BLOCH_POINT_SOURCES) == cfg["cells"].shape[-2]
        assert b.info(_abi.BATCH_INFO_POINT_SOURCES) == 0
        w = cfg["window"]
        path = _expect_path(b, cfg["omegas"].shape[1] if monitors else 0, w[2] * w[3], _table_entries(cfg),
                            never=resident == 0, lds_allowed=lds)
        done, launches = 0, b.launches
        for k in splits:
            b.run_bloch_channels(k, cfg["amps"][:, done:done + k], cfg["chan"][..., done:done + k], conjugate=conjugate)
            done += k
        if path:      # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * sum(splits)
        out = dict(fields=b.download() + (b.download_ezx(),), path=path, in_lds=b.window_in_lds)
        if monitors:
            out.update(dft=b.read_dft_window(), probes=b.read_probes())
        return out


def _stand_in(dtype, R, Cc, cfg, layer=LAYER, monitors=True, conjugate=False):
    B = cfg["eps"].shape[0]
    ref = _drive(BlochAdjointOracle(B, R, Cc, DT, DX, dtype=dtype), cfg, layer, monitors)
    ref.run_bloch_channels(cfg["n"], cfg["amps"], cfg["chan"], conjugate=conjugate)
    out = dict(fields=ref.download() + (ref.download_ezx(),))
    if monitors:
        out.update(dft=ref.read_dft_window(), probes=ref.read_probes())
    return out


def _agrees(got, ref, cfg, conjugate=False):
    """Fields, Ezx and probes bit for bit, the window DFT to 1e-12; both parts and the seam saw the field, and the image
    column is the rotation the run used times column 0."""
    for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx"), got["fields"], ref["fields"]):
        assert np.iscomplexobj(a) and np.array_equal(a, w), name
    Ez = got["fields"][0]
    assert np.abs(Ez.real).max() > 0 and np.abs(Ez.imag).max() > 0 and np.abs(Ez[:, :, 0]).max() > 0
    rho = np.exp((-1j if conjugate else 1j) * cfg["phis"])[:, None]
    assert np.abs(Ez[:, :, -1] - rho * Ez[:, :, 0]).max() <= 1e-6 * np.abs(Ez).max()
    if "dft" in ref:
        assert np.array_equal(got["probes"], ref["probes"]) and np.abs(got["probes"][:, 0].imag).max() > 0
        assert np.abs(got["dft"] - ref["dft"]).max() <= 1e-12 * np.abs(ref["dft"]).max()


# ---- 1. against the stand-in ------------------------------------------------------------------------------------------------

N_STEPS = 50
CHANNELS = {("23x11", LAYER): (6, False), ("23x11", 0): (1, True), ("29x13", LAYER): (32, True), ("29x13", 0): (6, False)}


@functools.lru_cache(maxsize=None)
def _reference(fd, dtype, shape, layer, conjugate):
    R, Cc = SHAPES[shape]
    nchan, per_member = CHANNELS[shape, layer]
    cfg = _cfg(fd, R + layer, 5, R, Cc, dtype, N_STEPS, nchan, per_member)
    return cfg, _stand_in(dtype, R, Cc, cfg, layer, conjugate=conjugate)


@pytest.mark.parametrize("conjugate", [False, True], ids=["rho", "conj"])
@pytest.mark.parametrize("layer", [LAYER, 0], ids=["layer4", "pec"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("where", ["resident", "resident_spl7", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bloch_point_source_runs_match_the_stand_in(fd, dtype, where, shape, layer, conjugate):
    gb._exact_only(fd)
    R, Cc = SHAPES[shape]
    cfg, ref = _reference(fd, dtype, shape, layer, conjugate)
    got = _device_run(fd, dtype, R, Cc, cfg, (27, 23), layer, resident=0 if where == "streamed" else None,
                      spl=7 if where == "resident_spl7" else 0, conjugate=conjugate)
    assert got["path"] == (where != "streamed")
    _agrees(got, ref, cfg, conjugate)


@pytest.mark.parametrize("which", ["64", "60+4"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_sixty_four_table_entries(fd, dtype, which):
    """64 point cells, none in column 0; and 60 of which member 1 alone has 4 in column 0, so that its table holds 64
    entries and the other members' tables end in silent ones."""
    gb._exact_only(fd)
    (R, Cc), B, n = SHAPES["29x13"], 3, 20
    rng = np.random.default_rng(64)
    flat = rng.permutation(np.arange(R * Cc)[np.arange(R * Cc) % Cc < Cc - 1])
    inner = flat[flat % Cc != 0][:64]
    if which == "64":
        cells = np.stack([inner // Cc, inner % Cc], axis=1)
    else:
        cells = np.tile(np.stack([inner[:60] // Cc, inner[:60] % Cc], axis=1), (B, 1, 1))
        cells[1, :4] = [(3, 0), (11, 0), (17, 0), (R - 2, 0)]
    cfg = _cfg(fd, 64, B, R, Cc, dtype, n, nchan=3, cells=cells)
    assert _table_entries(cfg) == 64
    ref = _stand_in(dtype, R, Cc, cfg)
    for resident in (None, 0):
        got = _device_run(fd, dtype, R, Cc, cfg, (n,), resident=resident)
        assert got["path"] == (resident is None)
        _agrees(got, ref, cfg)


# ---- 2. silent points, and the conjugate rotation is the member at -phi --------------------------------------------------------

@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_zero_weights_leave_the_bloch_run_unchanged(fd, dtype, resident):
    """Zero weights and conjugate False against run() on a Bloch batch without point sources: bit for bit, in both
    builds."""
    (R, Cc), n = SHAPES["29x13"], 40
    cfg = _cfg(fd, 31, 5, R, Cc, dtype, n)
    cfg["w"] = np.zeros_like(cfg["w"])
    got = _device_run(fd, dtype, R, Cc, cfg, (n,), resident=resident)
    plain = gb._device_run(fd, dtype, R, Cc, cfg, (n,), resident=resident)
    assert gb._same(got, plain) and np.abs(got["fields"][0]).max() > 0


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_conjugate_is_a_second_engine_at_minus_phi(fd, dtype, resident):
    """conjugate True against an engine given (c, -s) through set_bloch_phase(rotation=) and conjugate False: bit for
    bit, in both builds (the source weights are the same arrays)."""
    (R, Cc), B, n = SHAPES["29x13"], 5, 40
    cfg = _cfg(fd, 32, B, R, Cc, dtype, n)
    got = _device_run(fd, dtype, R, Cc, cfg, (n,), resident=resident, conjugate=True)
    ramp = np.exp(1j * cfg["phis"][:, None] * np.arange(Cc - 1)[None, :] / (Cc - 1))
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        _drive(b, cfg, LAYER)
        b.set_bloch_phase(None, rotation=(np.cos(cfg["phis"]), -np.sin(cfg["phis"]))).set_bloch_source(ramp)
        b.set_option(resident=resident)
        b.run_bloch_channels(n, cfg["amps"], cfg["chan"])
        other = dict(fields=b.download() + (b.download_ezx(),), dft=b.read_dft_window(), probes=b.read_probes())
    assert gb._same(got, other) and np.abs(got["fields"][0].imag).max() > 0


# ---- 3. bit-identical whatever the path, in both builds -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bloch_point_source_runs_are_bit_identical_on_every_path(fd, dtype):
    R, Cc = SHAPES["29x13"]
    cfg = _cfg(fd, 5, 6, R, Cc, dtype, 60, nchan=6, per_member=True)
    base = _device_run(fd, dtype, R, Cc, cfg, (60,), conjugate=True)
    assert base["path"] and base["in_lds"]
    variants = dict(streamed=dict(resident=0), spl=dict(spl=7), split=dict(splits=(1, 32, 27)),
                    global_acc=dict(lds=False), split_spl=dict(splits=(33, 27), spl=10, lds=False))
    for name, kw in variants.items():
        splits = kw.pop("splits", (60,))
        got = _device_run(fd, dtype, R, Cc, cfg, splits, conjugate=True, **kw)
        assert got["path"] == (name != "streamed"), name
        assert got["in_lds"] == (name in ("spl", "split")), name
        assert gb._same(base, got), name


# ---- 4. the capacity rule, many members -------------------------------------------------------------------------------------------

def _cells64(R, Cc):
    flat = np.random.default_rng(R).permutation(np.arange(R * Cc)[(np.arange(R * Cc) % Cc < Cc - 1) &
                                                                   (np.arange(R * Cc) % Cc > 0)])[:64]
    return np.stack([flat // Cc, flat % Cc], axis=1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_largest_member_with_64_point_cells_is_resident_and_one_row_more_streams(fd, dtype):
    gb._exact_only(fd)
    Cc, B, n = 41, 3, 12
    # the largest member without point sources, then with them: the library's own figure, read at run time
    R = gb._largest_rows(fd, dtype, Cc)
    while True:
        with fd.BatchEngine(1, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
            b.set_materials(None, None).set_bloch_phase(0.5)
            before = b.resident_max_cells
            b.set_bloch_point_sources(_cells64(R, Cc), np.ones((64, 2)))
            assert b.resident_max_cells == (LDS_LIMIT - gb._seg(4 * R, b.dtype.itemsize) - 8 * 64 - 16 * (Cc - 1)) \
                // 11 // 16 * 16 // b.dtype.itemsize <= before
            if R * Cc <= b.resident_max_cells:
                assert b.resident
                break
            assert not b.resident
        R -= 1
    with fd.BatchEngine(1, R + 1, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        b.set_materials(None, None).set_bloch_phase(0.5).set_bloch_point_sources(_cells64(R + 1, Cc), np.ones((64, 2)))
        assert (R + 1) * Cc > b.resident_max_cells and not b.resident
    assert -(-R * Cc // min(1024, -(-(-(-R * Cc // 4)) // 64) * 64)) <= 4     # at most 4 cells per thread
    for rows, resident in ((R, True), (R + 1, False)):
        cfg = _cfg(fd, rows, B, rows, Cc, dtype, n, nchan=2, cells=_cells64(rows, Cc))
        got = _device_run(fd, dtype, rows, Cc, cfg, (n,), monitors=False, conjugate=True)
        assert got["path"] == resident, rows
        _agrees(got, _stand_in(dtype, rows, Cc, cfg, monitors=False, conjugate=True), cfg, conjugate=True)


def test_more_members_than_one_round_of_workgroups(fd):
    dtype, (R, Cc), B, n = np.float32, SHAPES["29x13"], 300, 10
    cfg = _cfg(fd, 9, B, R, Cc, dtype, n, nchan=2, per_member=True)
    a = _device_run(fd, dtype, R, Cc, cfg, (n,), monitors=False)
    b = _device_run(fd, dtype, R, Cc, cfg, (n,), monitors=False, resident=0)
    assert a["path"] and not b["path"] and gb._same(a, b)
    Ez = a["fields"][0]
    assert len({Ez[m].tobytes() for m in range(B)}) == B
    if fd.ARITHMETIC == "exact":                                      # three of them against the stand-in
        pick = [0, 151, 299]
        sub = {k: (v[pick] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in cfg.items()}
        ref = _stand_in(dtype, R, Cc, sub, monitors=False)
        for x, y in zip(a["fields"], ref["fields"]):
            assert np.array_equal(x[pick], y)


# ---- 5. the product, the spectra, the maxima ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_product_spectra_and_maxima_on_the_device(fd, dtype, resident):
    from fdtd2d_amd import _abi
    (R, Cc), B, n = SHAPES["29x13"], 4, 60
    cfg = _cfg(fd, 41, B, R, Cc, dtype, n)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        _drive(b, cfg, LAYER).set_option(resident=resident)
        b.run(n, cfg["amps"])
        assert b.info(_abi.BATCH_INFO_HELD_BLOCH_WINDOW) == 0
        b.hold_bloch_window()
        assert b.info(_abi.BATCH_INFO_HELD_BLOCH_WINDOW) == 1 and b.info(_abi.BATCH_INFO_HELD_WINDOW) == 0
        held = b.read_dft_window()
        b.reset()
        b.run_bloch_channels(40, None, cfg["chan"][..., :40], conjugate=True)      # the held window survives both
        cur = b.read_dft_window()
        assert np.abs(held).max() > 0 and np.abs(cur.imag).max() > 0 and not np.array_equal(held, cur)
        coef = np.exp(1j * np.arange(B * 3).reshape(B, 3)) * (1 + np.arange(3))
        want = (coef[:, :, None, None] * held * cur).real.sum(axis=1)
        launches = b.launches
        got = b.bloch_window_product(coef)
        assert b.launches - launches == 1
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        # the stand-in's order on the same windows: exact in the exact build
        from oracle_batch import window_product
        order = np.stack([window_product(coef[m], held[m], cur[m]) for m in range(B)])
        if fd.ARITHMETIC == "exact":
            assert np.array_equal(got, order)
        # spectra against the host transform of the traces, also for a sub-range; the peak is the larger part's
        tr = b.read_probes(0, 40)
        steps = np.arange(40) + 1
        X = np.stack([tr[m] @ np.exp(-1j * np.outer(steps * DT, cfg["omegas"][m])) for m in range(B)])
        S, peak = b.bloch_probe_spectra(cfg["omegas"], peak=True)
        assert np.abs(S - X).max() <= 1e-12 * np.abs(X).max() and np.abs(X).max() > 0
        assert np.array_equal(peak, np.maximum(np.abs(tr.real).max(axis=(1, 2)), np.abs(tr.imag).max(axis=(1, 2))))
        sub = b.bloch_probe_spectra(cfg["omegas"], 7, 21)
        Xs = np.stack([tr[m][:, 7:28] @ np.exp(-1j * np.outer(steps[7:28] * DT, cfg["omegas"][m])) for m in range(B)])
        assert np.abs(sub - Xs).max() <= 1e-12 * np.abs(X).max()
        only_peak = b.bloch_probe_spectra(np.empty((B, 0)), 0, 40, peak=True)[1]
        assert np.array_equal(only_peak, peak)
        # maxima against download, exactly
        fields = b.download()
        top = lambda f: np.maximum(np.abs(f.real).max(axis=(1, 2)), np.abs(f.imag).max(axis=(1, 2))).astype(np.float64)
        assert np.array_equal(b.bloch_field_absmax("Ez"), top(fields[0][:, :, :-1]))
        assert np.array_equal(b.bloch_field_absmax("Hx"), top(fields[1]))
        assert np.array_equal(b.bloch_field_absmax("Hy"), top(fields[2]))
        # a new window drops the held one
        b.set_dft_window(cfg["window"], cfg["omegas"])
        assert b.info(_abi.BATCH_INFO_HELD_BLOCH_WINDOW) == 0
        with pytest.raises(fd.Fdtd2dError, match="no held window") as ei:
            b.bloch_window_product(coef)
        assert ei.value.code == E_STATE


# ---- 6. the gradients -------------------------------------------------------------------------------------------------------------

G_R, G_C, G_L, G_NSTEPS = 40, 13, 8, 1500
G_DESIGN, G_SOURCE = (14, 0, 10, 12), (10, 0, 1, 12)
G_PROBES = np.array([(29, c) for c in (0, 4, 8, 11)])


def g_case(B, seed=17):
    rng = np.random.default_rng(seed)
    r0, c0, nr, nc = G_DESIGN
    eps, sigma = np.full((B, G_R, G_C), acpu.EPS0), np.zeros((B, G_R, G_C))
    sigma[:, G_L:G_R - G_L, :] = 0.1
    eps[:, r0:r0 + nr, c0:c0 + nc] = acpu.EPS0 * (1 + 2 * rng.random((B, nr, nc)))
    sigma[:, r0:r0 + nr, c0:c0 + nc] = 0.2 + 0.5 * rng.random((B, nr, nc))
    sigma[:, 29, :] = 0
    eps[:, :, -1], sigma[:, :, -1] = eps[:, :, 0], sigma[:, :, 0]
    phi = 2.2 + 0.9 * np.arange(B) / max(B - 1, 1)
    return eps, sigma, phi


def g_kw(B, engine, dtype=np.float64):
    return dict(bloch_phase=g_case(B)[2], source_weights="ramp", nsteps=G_NSTEPS, sources=np.tile(G_SOURCE, (B, 1)),
                probes=G_PROBES, omegas=acpu.A_OMEGAS, design=G_DESIGN, fc=acpu.A_FC, dt=acpu.A_DT, dx=acpu.A_DX,
                dtype=dtype, pml_cells=G_L, engine=engine)


@functools.lru_cache(maxsize=None)
def g_reference(fd, B):
    eps, sigma, _ = g_case(B)
    return fd.batch_bloch_gradient(eps, sigma, objective=g_objective, **g_kw(B, BlochAdjointOracle))


def counting(fd, log):
    class Counting(fd.BatchEngine):
        def run(self, *a, **k):
            before = self.launches
            fd.BatchEngine.run(self, *a, **k)
            log.append((self.resident, self.launches - before))
            return self

        def run_bloch_channels(self, *a, **k):
            before = self.launches
            fd.BatchEngine.run_bloch_channels(self, *a, **k)
            log.append((self.resident, self.launches - before))
            return self
    return Counting


def _close(got, want, bound, B):
    for name, g, w in (("grad_eps", got[0], want[0]), ("grad_sigma", got[1], want[1])):
        for m in range(B):
            d = np.abs(g[m] - w[m]).max() / np.abs(w[m]).max()
            assert d <= bound, (name, m, d)


@pytest.mark.parametrize("B", [2, 8])
def test_bloch_gradients_match_the_stand_in(fd, B):
    """batch_bloch_gradient and BlochAdjointSession, float64, against the stand-in: 1e-9 of max|gradient|; every run of
    both is one launch."""
    gb._exact_only(fd)
    eps, sigma, phi = g_case(B)
    J, ge, gs, sp, info = g_reference(fd, B)
    log = []
    got = fd.batch_bloch_gradient(eps, sigma, objective=g_objective, **g_kw(B, counting(fd, log)))
    assert log == [(True, 1), (True, 1)]
    _close(got[1:3], (ge, gs), 1e-9, B)
    assert np.allclose(got[0], J, rtol=1e-11, atol=0) and np.abs(got[3] - sp).max() <= 1e-11 * np.abs(sp).max()
    for k in ("residual_forward", "residual_adjoint"):
        assert np.allclose(got[4][k], info[k], rtol=1e-6), k
    del log[:]
    with fd.BlochAdjointSession(eps, **g_kw(B, counting(fd, log))) as s:
        s.set_conductivity(sigma)
        Js, g, sps, infos = s.value_and_grad(g_objective)
        _close((g, s.sigma_gradient()), (ge, gs), 1e-9, B)
        assert log == [(True, 1), (True, 1)]
        assert np.allclose(Js, J, rtol=1e-11, atol=0) and np.abs(sps - sp).max() <= 1e-11 * np.abs(sp).max()
        for k in ("residual_forward", "residual_adjoint"):
            assert np.allclose(infos[k], info[k], rtol=1e-6), k
        # the phase changes between iterations: the helper at the new phases
        s.set_bloch_phase(phi[::-1].copy())
        _, g2, _, _ = s.value_and_grad(g_objective)
        gs2 = s.sigma_gradient()
    kw = g_kw(B, None)
    kw["bloch_phase"] = phi[::-1].copy()
    want2 = fd.batch_bloch_gradient(eps, sigma, objective=g_objective, **kw)
    _close((g2, gs2), want2[1:3], 1e-9, B)
    assert not np.allclose(g2, g, rtol=1e-3)


def test_float32_gradients_are_close_to_float64(fd):
    """float32 against float64 on the device: bound 1e-5 of max|gradient|, as for the real adjoint."""
    B = 2
    eps, sigma, _ = g_case(B)
    g64 = fd.batch_bloch_gradient(eps, sigma, objective=g_objective, **g_kw(B, None))
    g32 = fd.batch_bloch_gradient(eps, sigma, objective=g_objective, **g_kw(B, None, np.float32))
    for m in range(B):
        for k in (1, 2):
            d = np.abs(g32[k][m] - g64[k][m]).max() / np.abs(g64[k][m]).max()
            print(f"member {m}, {'eps' if k == 1 else 'sigma'}: float32 vs float64 {d:.3e}")
            assert d <= 1e-5


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def test_the_library_refuses_bad_bloch_adjoint_calls(fd):
    from fdtd2d_amd import _abi
    B, (R, Cc) = 2, SHAPES["29x13"]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    cells, wts, chan = np.array([[6, 6]] * B, dtype=np.int32), np.ones((B, 1)), np.zeros((1, 4))
    one, out, w = np.ones(B), np.zeros(4 * B * R * Cc), np.full(B, 1e11)
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="periodic") as b:
        lib, h = b._lib, b._h
        err = lambda: lib.fdtd2d_batch_last_error(h).decode()
        b.set_materials(None, None).set_dft_window((3, 2, 2, 3), [1e11]).set_probes([(4, 2)], 8)
        # without a phase: E_STATE, each
        assert lib.fdtd2d_batch_set_bloch_point_sources(h, 1, ip(cells), 1, dp(wts)) == E_STATE and "no Bloch phase" in err()
        assert lib.fdtd2d_batch_run_bloch_channels(h, 4, None, None, dp(chan), 0, 0) == E_STATE
        assert lib.fdtd2d_batch_hold_bloch_window(h) == E_STATE
        assert lib.fdtd2d_batch_bloch_window_product(h, dp(one), dp(one), dp(out)) == E_STATE
        assert lib.fdtd2d_batch_bloch_probe_spectra(h, 1, dp(w), 0, 0, dp(out), dp(out), None) == E_STATE
        assert lib.fdtd2d_batch_bloch_field_absmax(h, 0, dp(out)) == E_STATE
        b.set_bloch_phase([0.4, 1.1])
        # with one: the arguments
        assert lib.fdtd2d_batch_run_bloch_channels(h, 4, None, None, dp(chan), 0, 0) == E_STATE and "no point sources" in err()
        bad = np.array([[6, 6], [7, Cc - 1]], dtype=np.int32)
        assert lib.fdtd2d_batch_set_bloch_point_sources(h, 1, ip(bad), 1, dp(wts)) == E_ARG
        assert "member 1 point source 0" in err() and "column 12" in err()
        assert lib.fdtd2d_batch_set_bloch_point_sources(h, 65, ip(cells), 1, dp(wts)) == E_ARG
        assert lib.fdtd2d_batch_set_bloch_point_sources(h, 1, ip(cells), 33, dp(wts)) == E_ARG
        twice = np.array([[6, 6], [6, 6]] * B, dtype=np.int32)
        assert lib.fdtd2d_batch_set_bloch_point_sources(h, 2, ip(twice), 1, dp(np.ones((B, 2, 1)))) == E_ARG
        assert "listed twice" in err()
        assert b.info(_abi.BATCH_INFO_BLOCH_POINT_SOURCES) == 0
        b.set_bloch_point_sources([(6, 6)], np.ones((1, 1)))
        assert b.info(_abi.BATCH_INFO_BLOCH_POINT_SOURCES) == 1 and b.info(_abi.BATCH_INFO_POINT_SOURCES) == 0
        assert lib.fdtd2d_batch_run_bloch_channels(h, -1, None, None, dp(chan), 0, 0) == E_ARG
        assert lib.fdtd2d_batch_run_bloch_channels(h, 4, None, None, None, 0, 0) == E_ARG
        assert lib.fdtd2d_batch_run_bloch_channels(h, 4, None, dp(out), dp(chan), 0, 0) == E_ARG
        assert lib.fdtd2d_batch_bloch_window_product(h, dp(one), dp(one), dp(out)) == E_STATE and "no held window" in err()
        assert lib.fdtd2d_batch_bloch_window_product(h, None, dp(one), dp(out)) == E_ARG
        assert lib.fdtd2d_batch_bloch_probe_spectra(h, 17, dp(w), 0, 0, dp(out), dp(out), None) == E_ARG
        assert lib.fdtd2d_batch_bloch_probe_spectra(h, 1, dp(w), 0, 1, dp(out), dp(out), None) == E_ARG   # nothing recorded
        assert lib.fdtd2d_batch_bloch_probe_spectra(h, 0, None, 0, 0, None, None, None) == E_ARG
        assert lib.fdtd2d_batch_bloch_field_absmax(h, 3, dp(out)) == E_ARG
        assert lib.fdtd2d_batch_bloch_field_absmax(h, 0, None) == E_ARG
        # the plain calls keep refusing; new rotations keep the point sources; the phase off drops them
        assert lib.fdtd2d_batch_set_point_sources(h, 1, ip(cells), 1, dp(wts)) == E_STATE
        assert lib.fdtd2d_batch_run_channels(h, 4, None, dp(chan), 0) == E_STATE
        assert lib.fdtd2d_batch_hold_dft_window(h) == E_STATE
        b.set_bloch_phase([0.5, 1.2])
        assert b.info(_abi.BATCH_INFO_BLOCH_POINT_SOURCES) == 1
        b.hold_bloch_window()
        assert b.info(_abi.BATCH_INFO_HELD_BLOCH_WINDOW) == 1
        b.run_bloch_channels(4, None, chan, conjugate=True)
        assert b.step_count == 4
        b.set_bloch_phase(None)
        assert not b.bloch and b.info(_abi.BATCH_INFO_BLOCH_POINT_SOURCES) == 0 and b.info(_abi.BATCH_INFO_POINT_SOURCES) == 0
        assert b.info(_abi.BATCH_INFO_HELD_BLOCH_WINDOW) == 0 and b.info(_abi.BATCH_INFO_HELD_WINDOW) == 0
        assert lib.fdtd2d_batch_run_channels(h, 4, None, dp(chan), 0) == E_STATE and "no point sources" in err()
        b.set_point_sources([(6, 6)], np.ones((1, 1))).run(4, None, chan)          # a plain periodic batch again
        assert b.step_count == 8


# ---- 8. the fused build -------------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_bloch as gb
import test_gpu_batch_bloch_adjoint as t
out = {"arithmetic": fd.ARITHMETIC, "paths": True}
R, Cc = t.SHAPES["29x13"]
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    cfg = t._cfg(fd, 23, 5, R, Cc, dtype, t.NSTEPS_FIELD)
    got = t._device_run(fd, dtype, R, Cc, cfg, (t.NSTEPS_FIELD,), conjugate=True)
    np.save(f"{OUT}/field_{name}.npy", got["fields"][0])
    b = t._device_run(fd, dtype, R, Cc, cfg, (t.NSTEPS_FIELD,), resident=0, conjugate=True)
    out["paths"] = out["paths"] and gb._same(got, b)
eps, sigma, _ = t.g_case(2)
g = fd.batch_bloch_gradient(eps, sigma, objective=t.g_objective, **t.g_kw(2, None))
np.save(f"{OUT}/grad_eps.npy", g[1])
np.save(f"{OUT}/grad_sigma.npy", g[2])
print("BLOCH_ADJOINT_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build against the exact build, both on the device, each in a process of its own: complex Ez after 300
    steps with point sources, and the gradients of the 2-member case; in both builds the resident and the streamed path
    agree bit for bit."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("BLOCH_ADJOINT_RESULT ")][-1][21:])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"{k}.npy").astype(np.complex128) for k in FUSED_BOUND}
    worst = {}
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m] - e[m]).max() / np.abs(e[m]).max() for m in range(e.shape[0]))
        print(f"fused vs exact, {k}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
