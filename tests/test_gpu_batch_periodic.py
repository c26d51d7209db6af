"""GPU: periodic columns in the batched engine (fdtd2d_batch_periodic.h, kernels_batch_periodic.hpp).

Fields, Ezx and probe traces equal the stand-in of tests/oracle_batch_periodic.py bit for bit (exact build), window DFTs
to 1e-12: both dtypes, resident and streamed, with and without conductivity, monitors and point sources, with the layer
on the rows and with PEC there, with source, point and probe cells in columns 0 and C-2 (and probes and windows on the
image column).  Everything is bit-identical whatever the path, the launch split and the accumulators' placement, also
with 264 members; every case asserts the path it took and its launch count.  The three exact properties of
tests/test_batch_periodic_cpu.py hold on the device.  The gradients of that file's configuration equal the stand-in's to
1e-9 of max|gradient| through the helper and the session.

The fused build (FDTD2D_ARITHMETIC=fused) is checked against the exact build's on the same members: see FUSED_BOUND."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch_periodic import PeriodicOracle
import test_batch_periodic_cpu as pcpu

pytestmark = pytest.mark.gpu

ROOT = pcpu.ROOT
DT, DX, LAYER, LDS_LIMIT = 5e-14, 1e-4, 10, 163840
E_ARG, E_STATE = -1, -4
# The fused build evaluates the multiply-add pairs of the step as one fma each (batch_periodic_split, _plain and
# batch_lossy_e), so its results differ from the exact build's by rounding.  Measured on an MI355X (the child processes
# of test_fused_build_within_its_bounds), worst member:
#   Ez after 300 steps with conductivity, monitors and point sources, 6 members of 60x61 (48x41 in float64),
#   max|fused - exact| / max|exact|:   float32 1.9e-7,   float64 1.8e-16
#   both gradients of batch_material_gradient (the 2-member configuration of test_batch_periodic_cpu, 1500 steps), of
#   max|gradient| over the design window:   float32 eps 3.0e-7 sigma 9.0e-8,   float64 eps 3.6e-15 sigma 9.8e-16
# The bounds are ten times the measured values.
NSTEPS_FIELD, NSTEPS_F = 300, 1500
FUSED_BOUND = {
    ("field", "f32"): 1.9e-6, ("field", "f64"): 1.8e-15,
    ("eps", "f32"): 3.0e-6, ("sigma", "f32"): 9.0e-7,
    ("eps", "f64"): 3.6e-14, ("sigma", "f64"): 9.8e-15,
}


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _threads(cells):
    return min(1024, -(-(-(-cells // 4)) // 64) * 64)


def _shape(dtype):
    return (48, 41) if dtype == np.float64 else (60, 61)


def _window(R, Cc, dtype):
    """Both hold cells of the image column."""
    return (R // 2 - 6, Cc - 8, 12, 8) if dtype == np.float32 else (R // 2 - 2, Cc - 6, 3, 6)


def _cfg(fd, rng, B, R, Cc, dtype, n, K=6, points=None, image_row=13):
    """Members with their own materials (the image column's are random too: they are never read), line sources that
    touch column 0, column C-2 or span the whole period, and point cells in columns 0 and C-2, two owned by one thread of
    the resident walk, a layer row, the last row, cell [0, 0] and a cell of the rectangle source.  The probes are the
    point cells and a cell of the image column.  points: other point cells, (B, P, 2); image_row: that probe's row."""
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(dtype)
    mu = (fd.MU0 * np.where(rng.random((B, R, Cc)) < 0.1, 1.5, 1.0)).astype(dtype)
    spans = [(0, Cc - 1), (0, 5), (Cc - 6, 5), (3, Cc - 7)]
    rects = np.array([[R // 2 + (m % 3) - 1, spans[m % 4][0], 1, spans[m % 4][1]] for m in range(B)])
    amps = np.stack([[fd.ricker_amplitude(k * DT, 30e9 * (1 + 0.1 * m)) for k in range(n)] for m in range(B)])
    omegas = (2 * np.pi * np.linspace(10e9, 100e9, 10))[None, :] * (1 + 0.01 * np.arange(B))[:, None]
    twin = divmod(12 * Cc + 10 + _threads(R * Cc), Cc)
    if points is None:
        points = np.stack([[[10 + m % 2, 0], [11, Cc - 2], [12, 10], list(twin), [2 + m % 2, Cc // 3], [R - 1, 5],
                            [0, 0], [int(r[0]), int(r[1]) + 1]] for m, r in enumerate(rects)])
    points = np.asarray(points)
    probes = np.concatenate([points, np.tile([[[image_row, Cc - 1]]], (B, 1, 1))], axis=1)
    weights = rng.standard_normal((B, points.shape[1], K))
    t = np.arange(n) * DT
    chan = np.stack([np.sin(2 * np.pi * 20e9 * (1 + c) * t + c) * np.exp(-((t - 20 * DT) / (15 * DT)) ** 2)
                     for c in range(K)])
    chan = np.stack([chan * (1 + 0.25 * m) for m in range(B)])
    return dict(eps=eps, mu=mu, rects=rects, amps=amps, omegas=omegas, points=points, probes=probes, weights=weights,
                chan=chan, n=n)


def _sigma(rng, B, R, Cc, layer, top=20.0):
    """Random conductivity up to `top` S/m on the rows that may conduct, every column (the image column's is never
    read), zero on 30 % of the cells."""
    g = max(6, layer)
    s = np.zeros((B, R, Cc))
    inner = top * rng.random((B, R - 2 * g, Cc))
    s[:, g:R - g, :] = np.where(rng.random(inner.shape) < 0.3, 0.0, inner)
    return s


def _drive(b, cfg, window, layer, sigma, monitors):
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    if layer:
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])]
        b.set_pml(layer, courant00=np.array(c00))
    else:
        b.clear_pml()
    if sigma is not None:
        b.set_conductivity(sigma)
    if monitors:
        b.set_dft_window(window, cfg["omegas"]).set_probes(cfg["probes"], cfg["n"])
        b.set_point_sources(cfg["points"], cfg["weights"])
    return b


def _expect_path(b, nf, window_cells, ntab, never=False, lds_allowed=True):
    """The capacity rule, restated: the lossy PML one (7 arrays and the 4R + 4C factors), whatever is set; ntab counts
    the point sources and the images of those in column 0."""
    esz, R, Cc = b.dtype.itemsize, b.rows, b.cols
    seg = _seg(R * Cc, esz)
    fields = 7 * seg + _seg(4 * R, esz) + _seg(4 * Cc, esz)
    table, acc = 16 * nf + 8 * ntab, 16 * nf * window_cells
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = bool(nf) and lds_allowed and fields + table + acc <= LDS_LIMIT
    assert b.periodic
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident_max_cells == (LDS_LIMIT - (fields - 7 * seg) - table) // 7 // 16 * 16 // esz
    assert b.resident == resident
    assert b.window_in_lds == (in_lds and resident)
    return resident


def _device_run(fd, dtype, R, Cc, cfg, window, splits, sigma=None, layer=LAYER, monitors=True, resident=None, spl=None,
                lds=True):
    B = cfg["eps"].shape[0]
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        _drive(b, cfg, window, layer, sigma, monitors)
        assert b.lossy == (sigma is not None) and b.pml == bool(layer)
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        npts = cfg["points"].shape[1]
        images = max(int((cfg["points"][m, :, 1] == 0).sum()) for m in range(B))
        assert b.info(12) == (npts if monitors else 0)            # FDTD2D_BATCH_INFO_POINT_SOURCES: as given
        path = _expect_path(b, cfg["omegas"].shape[1] if monitors else 0, window[2] * window[3],
                            npts + images if monitors else 0, never=resident == 0, lds_allowed=lds)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, cfg["amps"][:, done:done + k], cfg["chan"][..., done:done + k] if monitors else None)
            done += k
        if path:      # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * sum(splits)
        out = dict(fields=b.download() + (b.download_ezx(),), path=path, in_lds=b.window_in_lds)
        if monitors:
            out.update(dft=b.read_dft_window(), probes=b.read_probes())
        return out


def _stand_in(dtype, R, Cc, cfg, window, sigma=None, layer=LAYER, monitors=True):
    B = cfg["eps"].shape[0]
    ref = _drive(PeriodicOracle(B, R, Cc, DT, DX, dtype=dtype), cfg, window, layer, sigma, monitors)
    ref.run(cfg["n"], cfg["amps"], cfg["chan"] if monitors else None)
    out = dict(fields=ref.download() + (ref.download_ezx(),))
    if monitors:
        out.update(dft=ref.read_dft_window(), probes=ref.read_probes())
    return out


def _same(a, b):
    ok = all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"]))
    if "dft" in a:
        ok = ok and np.array_equal(a["dft"], b["dft"]) and np.array_equal(a["probes"], b["probes"])
    return ok


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_within_its_bounds")


# ---- 1. against the stand-in ------------------------------------------------------------------------------------------------

VARIANTS = {"full": dict(conduct=True, layer=LAYER, monitors=True),
            "lossless": dict(conduct=False, layer=LAYER, monitors=True),
            "bare": dict(conduct=False, layer=LAYER, monitors=False),
            "pec": dict(conduct=True, layer=0, monitors=True),
            "pec_bare": dict(conduct=False, layer=0, monitors=False)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_periodic_runs_match_the_stand_in(fd, dtype, where, variant):
    _exact_only(fd)
    v = VARIANTS[variant]
    R, Cc = _shape(dtype)
    B, n = 4, 40
    window = _window(R, Cc, dtype)
    rng = np.random.default_rng(R + len(variant))
    cfg = _cfg(fd, rng, B, R, Cc, dtype, n)
    sigma = _sigma(rng, B, R, Cc, v["layer"]) if v["conduct"] else None
    got = _device_run(fd, dtype, R, Cc, cfg, window, (23, 17), sigma, v["layer"], v["monitors"],
                      resident=None if where == "resident" else 0)
    assert got["path"] == (where == "resident")
    ref = _stand_in(dtype, R, Cc, cfg, window, sigma, v["layer"], v["monitors"])
    for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx"), got["fields"], ref["fields"]):
        assert np.array_equal(a, w), name
    Ez, Ezx = got["fields"][0], got["fields"][3]
    assert np.abs(Ez).max() > 0 and np.array_equal(Ez[:, :, -1], Ez[:, :, 0]) and np.array_equal(Ezx[:, :, -1], Ezx[:, :, 0])
    assert np.abs(Ez[:, :, 0]).max() > 0 and (not v["layer"] or np.abs(Ezx).max() > 0)
    if v["monitors"]:
        assert np.array_equal(got["probes"], ref["probes"])
        assert np.abs(got["dft"] - ref["dft"]).max() <= 1e-12 * np.abs(ref["dft"]).max()
        assert np.abs(got["probes"][:, -1]).max() > 0                 # the probe on the image column saw the field


def test_a_member_too_large_for_lds_streams_and_matches_the_stand_in(fd):
    _exact_only(fd)
    dtype, R, Cc, B, n = np.float32, 100, 121, 3, 30
    window = (40, 0, 6, Cc)                 # the whole period and the image column
    rng = np.random.default_rng(17)
    cfg = _cfg(fd, rng, B, R, Cc, dtype, n)
    sigma = _sigma(rng, B, R, Cc, LAYER)
    got = _device_run(fd, dtype, R, Cc, cfg, window, (n,), sigma)
    assert not got["path"]
    ref = _stand_in(dtype, R, Cc, cfg, window, sigma)
    for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx"), got["fields"], ref["fields"]):
        assert np.array_equal(a, w), name
    assert np.array_equal(got["probes"], ref["probes"])
    assert np.abs(got["dft"] - ref["dft"]).max() <= 1e-12 * np.abs(ref["dft"]).max()


# ---- 2. bit-identical whatever the path -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_periodic_runs_are_bit_identical_on_every_path(fd, dtype):
    R, Cc = _shape(dtype)
    window = _window(R, Cc, dtype)
    rng = np.random.default_rng(5)
    cfg = _cfg(fd, rng, 6, R, Cc, dtype, 60)
    sigma = _sigma(rng, 6, R, Cc, LAYER)
    base = _device_run(fd, dtype, R, Cc, cfg, window, (60,), sigma)
    assert base["path"]
    variants = dict(streamed=dict(resident=0), spl=dict(spl=7), split=dict(splits=(1, 32, 27)),
                    global_acc=dict(lds=False), split_spl=dict(splits=(33, 27), spl=10, lds=False))
    seen_lds = {base["in_lds"]}
    for name, kw in variants.items():
        splits = kw.pop("splits", (60,))
        got = _device_run(fd, dtype, R, Cc, cfg, window, splits, sigma, **kw)
        assert got["path"] == (name != "streamed"), name
        assert _same(base, got), name
        seen_lds.add(got["in_lds"])
    assert seen_lds == {True, False}


def test_more_members_than_one_round_of_workgroups(fd):
    dtype, B, n = np.float32, 264, 30
    R, Cc = _shape(dtype)
    window = (R // 2 - 2, Cc - 6, 3, 6)
    rng = np.random.default_rng(9)
    cfg = _cfg(fd, rng, B, R, Cc, dtype, n)
    sigma = _sigma(rng, B, R, Cc, LAYER)
    a = _device_run(fd, dtype, R, Cc, cfg, window, (n,), sigma)
    b = _device_run(fd, dtype, R, Cc, cfg, window, (n,), sigma, resident=0)
    assert a["path"] and not b["path"] and _same(a, b)
    assert all(np.abs(a["fields"][0][m]).max() > 0 for m in range(B))
    assert len({a["fields"][0][m].tobytes() for m in range(B)}) == B


# ---- 3. the three exact properties on the device ---------------------------------------------------------------------------

def _engine(fd, resident):
    def make(*a, **k):
        return fd.BatchEngine(*a, **k).set_option(resident=resident)
    return make


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_period_equals_both_halves_of_a_double_period_on_the_device(fd, dtype, resident):
    """Two engines of different shape (64 x 21 and 64 x 41)."""
    pcpu.check_supercell(_engine(fd, resident), dtype)


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_cyclic_shift_shifts_the_fields_on_the_device(fd, dtype, resident):
    pcpu.check_cyclic_shift(_engine(fd, resident), dtype)


@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_column_uniform_members_stay_column_uniform_on_the_device(fd, dtype, resident):
    pcpu.check_column_invariance(_engine(fd, resident), dtype)


# ---- 4. state, options and refusals ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_upload_overwrites_the_image_column_as_the_stand_in_does(fd, dtype):
    _exact_only(fd)
    R, Cc = _shape(dtype)
    B, n = 3, 25
    rng = np.random.default_rng(3)
    cfg = _cfg(fd, rng, B, R, Cc, dtype, n)
    Ez, Ezx = rng.standard_normal((B, R, Cc)), rng.standard_normal((B, R, Cc))      # the image column is wrong
    Hx, Hy = rng.standard_normal((B, R, Cc - 1)), rng.standard_normal((B, R - 1, Cc))
    Ez[:, 0], Ez[:, -1], Ezx[:, 0], Ezx[:, -1] = 0, 0, 0, 0
    Hy[:, :, -1] = 0
    window = _window(R, Cc, dtype)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
        _drive(b, cfg, window, LAYER, None, False)
        ref = _drive(PeriodicOracle(B, R, Cc, DT, DX, dtype=dtype), cfg, window, LAYER, None, False)
        for e in (b, ref):
            e.upload(Ez, Hx, Hy).upload_ezx(Ezx)
        got = b.download()
        assert np.array_equal(got[0][:, :, -1], Ez.astype(dtype)[:, :, 0]) and np.array_equal(got[0], ref.download()[0])
        assert np.array_equal(b.download_ezx(), ref.download_ezx())
        for e in (b, ref):
            e.run(n, cfg["amps"])
        for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx"), b.download() + (b.download_ezx(),),
                              ref.download() + (ref.download_ezx(),)):
            assert np.array_equal(a, w), name


def test_switching_periodicity_off_returns_the_batch_to_the_pml_kernels(fd):
    """set_periodic(0) followed by a PML run equals a fresh boundary="pml" engine with the same factors."""
    dtype, B, n = np.float32, 3, 40
    R, Cc = _shape(dtype)
    rng = np.random.default_rng(4)
    cfg = _cfg(fd, rng, B, R, Cc, dtype, n)
    rects = np.array([[R // 2, 20, 1, 5]] * B)
    rowf, _ = fd.batch.batch_pml_profiles(B, R, 2 * LAYER + 3, (1 / np.sqrt(fd.EPS0 * fd.MU0) * DT) / DX, LAYER, dtype=dtype)
    prof = {k: rowf[:, i * R:(i + 1) * R] for i, k in enumerate(("ahr", "bhr", "aer", "ber"))}
    prof.update({k: np.ones(Cc, dtype) for k in ("ahc", "bhc", "aec", "bec")})
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b, \
            fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="pml") as fresh:
        b.set_materials(cfg["eps"], cfg["mu"]).set_sources(rects).set_pml(LAYER, profiles=prof)
        assert b.periodic and b.lds_bytes == 7 * _seg(R * Cc, 4) + _seg(4 * R, 4) + _seg(4 * Cc, 4)
        b._ck(b._lib.fdtd2d_batch_set_periodic(b._h, 0))
        fresh.set_materials(cfg["eps"], cfg["mu"]).set_sources(rects).set_pml(LAYER, profiles=prof)
        assert not b.periodic and not b.lossy and b.lds_bytes == fresh.lds_bytes
        before = b.launches, fresh.launches
        for e in (b, fresh):
            e.run(n, cfg["amps"])
        assert b.launches - before[0] == fresh.launches - before[1] == 1
        for a, w in zip(b.download() + (b.download_ezx(),), fresh.download() + (fresh.download_ezx(),)):
            assert np.abs(w).max() > 0 and np.array_equal(a, w)
        # and on again: the image column is column 0's
        b._ck(b._lib.fdtd2d_batch_set_periodic(b._h, 1))
        assert b.periodic and np.array_equal(b.download()[0][:, :, -1], b.download()[0][:, :, 0])
        b.run(5, cfg["amps"])


def test_the_library_refuses_what_the_image_column_excludes(fd):
    R, Cc, B = 60, 61, 3

    def refused(b, call, code, match):
        with pytest.raises(fd.Fdtd2dError, match=match) as ei:
            call()
        assert ei.value.code == code

    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="mur") as b:
        assert b._lib.fdtd2d_batch_set_periodic(b._h, 1) == E_STATE and not b.periodic
        assert "Mur" in b._lib.fdtd2d_batch_last_error(b._h).decode()
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="periodic") as b:
        b.set_materials()
        ok = np.array([[30, 0, 1, Cc - 1]] * B)
        b.set_sources(ok)
        bad = ok.copy()
        bad[1] = (30, 50, 1, 11)
        refused(b, lambda: b.set_sources(bad), E_ARG, r"member 1: source \(30,50\)\+1x11 reaches column 60")
        cells = np.array([[[10, 0], [11, 59]]] * B)
        b.set_point_sources(cells, np.ones((2, 1)))
        assert b.info(12) == 2
        cells[2, 1] = (11, 60)
        refused(b, lambda: b.set_point_sources(cells, np.ones((2, 1))), E_ARG, r"member 2 point source 1: cell \(11,60\)")
        many = np.array([[[r, 0] for r in range(33)]] * B)
        refused(b, lambda: b.set_point_sources(many, np.ones((33, 1))), E_ARG, "member 0: 33 point sources and the 33 images")
        refused(b, lambda: b.set_pml(29), E_ARG, "a 29-cell layer does not fit")
        b.set_pml(28)                                   # 2 L + 3 <= rows alone: a square member stops at 28 as well
        one = {k: np.ones(R if k.endswith("r") else Cc, np.float32) for k in ("ahr", "bhr", "aer", "ber", "ahc", "bhc",
                                                                             "aec", "bec")}
        one["bec"] = one["bec"].copy()
        one["bec"][7] = 0.5
        refused(b, lambda: b.set_pml(10, profiles=one), E_ARG, "member 0: column factor 190 is not exactly 1")
        b.set_pml(10)
        s = np.zeros((B, R, Cc))
        s[:, 10:50, :] = 1.0                            # every column, the image included
        b.set_conductivity(s)
        assert b.lossy
        s[1, 9, 0] = 1.0
        refused(b, lambda: b.set_conductivity(s), E_ARG, r"member 1: sigma is non-zero at cell \(9,0\), within 10 cells")
        s[1, 9, 0], s[1, 9, 60] = 0.0, 1.0              # the image column is never read
        b.set_conductivity(s)
        refused(b, lambda: b.set_pml(12), E_ARG, "member 0: sigma is non-zero within 12 cells")
        b.set_conductivity(None)
        assert not b.lossy and b.periodic and b.resident
    with fd.BatchEngine(B, 30, 101, DT, DX, boundary="periodic") as b:       # a layer that no square rule would fit
        b.set_materials().set_pml(13)
        refused(b, lambda: b.set_pml(14), E_ARG, "a 14-cell layer does not fit a 30x101 member")
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="pml") as b:               # a layer with graded columns stays a PML batch
        b.set_materials().set_sources(np.array([[30, 50, 1, 11]] * B)).set_pml(10)
        assert b._lib.fdtd2d_batch_set_periodic(b._h, 1) == E_ARG and not b.periodic
        assert "reaches column 60" in b._lib.fdtd2d_batch_last_error(b._h).decode()
        b.set_sources(np.array([[30, 40, 1, 11]] * B))
        assert b._lib.fdtd2d_batch_set_periodic(b._h, 1) == E_ARG and not b.periodic
        assert "not exactly 1" in b._lib.fdtd2d_batch_last_error(b._h).decode()


def test_uniform_materials_get_coefficient_arrays(fd):
    """A uniform-material periodic batch equals the same batch with material arrays (there is no uniform kernel)."""
    dtype, B, n = np.float32, 2, 40
    R, Cc = _shape(dtype)
    cfg = _cfg(fd, np.random.default_rng(8), B, R, Cc, dtype, n)
    out = []
    for arrays in (False, True):
        with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="periodic") as b:
            if arrays:
                b.set_materials(np.full((B, R, Cc), 2 * fd.EPS0), np.full((B, R, Cc), fd.MU0))
            else:
                b.set_materials(2 * fd.EPS0, fd.MU0)
            b.set_sources(cfg["rects"]).set_pml(LAYER)
            assert b.resident and not b.lossy
            b.run(n, cfg["amps"])
            out.append(b.download())
    assert np.abs(out[0][0]).max() > 0 and all(np.array_equal(a, w) for a, w in zip(*out))


# ---- 5. the gradients ----------------------------------------------------------------------------------------------------------

_reference = {}


def _gradient_reference(fd, count, dtype, nsteps):
    key = (count, np.dtype(dtype).name, nsteps)
    if key not in _reference:
        eps, sigma = pcpu.g_materials(count)
        _reference[key] = pcpu.g_gradient(fd, eps=eps, sigma=sigma, dtype=dtype, nsteps=nsteps)
    return _reference[key]


@pytest.mark.parametrize("count", [2, 8])
def test_periodic_gradients_match_the_stand_in(fd, count):
    _exact_only(fd)
    dtype, nsteps = np.float64, pcpu.G_NSTEPS
    Jr, ger, gsr, sr, ir = _gradient_reference(fd, count, dtype, nsteps)
    eps, sigma = pcpu.g_materials(count)
    J, ge, gs, s, info = pcpu.g_gradient(fd, eps=eps, sigma=sigma, dtype=dtype, nsteps=nsteps, engine=None)
    assert ge.shape == gs.shape == (count, 12, 16) and s.shape == (count, 16, 3)
    assert np.array_equal(s, sr) and np.array_equal(J, Jr)          # the probe traces are the stand-in's bit for bit
    for m in range(count):
        for g, w in ((ge, ger), (gs, gsr)):
            gmax = np.abs(w[m]).max()
            assert gmax > 0 and np.abs(g[m] - w[m]).max() <= 1e-9 * gmax, m
    assert np.allclose(info["residual_forward"], ir["residual_forward"], rtol=1e-12)
    assert len({gsr[m].tobytes() for m in range(count)}) == count


@pytest.mark.parametrize("count", [2, 8])
def test_periodic_session_matches_the_stand_in(fd, count):
    _exact_only(fd)
    dtype, nsteps = np.float64, pcpu.G_NSTEPS
    want = _gradient_reference(fd, count, dtype, nsteps)
    eps, sigma = pcpu.g_materials(count)
    with fd.AdjointSession(eps, **pcpu.g_args(count, engine=None, nsteps=nsteps, dtype=dtype)) as s:
        s.set_conductivity(sigma)
        assert s.engine.periodic and s.engine.lossy and s.engine.resident
        launches = s.engine.launches
        J, ge, sp, info = s.value_and_grad(pcpu.g_objective)
        gs = s.sigma_gradient()
        assert s.engine.launches - launches == 2 + 2 + 2 + 1 + 1      # runs, spectra, maxima, two products
    for m in range(count):
        for g, w in ((ge, want[1]), (gs, want[2])):
            assert np.abs(g[m] - w[m]).max() <= 1e-9 * np.abs(w[m]).max(), m
        assert np.abs(sp[m] - want[3][m]).max() <= 1e-12 * np.abs(want[3][m]).max(), m
    assert np.allclose(J, want[0], rtol=1e-12, atol=0)


# ---- 6. the fused build ---------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_gpu_batch_periodic as t
out = {"arithmetic": fd.ARITHMETIC, "paths": True}
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    R, Cc = t._shape(dtype)
    rng = np.random.default_rng(23)
    cfg = t._cfg(fd, rng, 6, R, Cc, dtype, t.NSTEPS_FIELD)
    sigma = t._sigma(rng, 6, R, Cc, t.LAYER)
    got = t._device_run(fd, dtype, R, Cc, cfg, t._window(R, Cc, dtype), (t.NSTEPS_FIELD,), sigma)
    np.save(f"{OUT}/field_{name}.npy", got["fields"][0])
    # resident against streamed, in this build
    b = t._device_run(fd, dtype, R, Cc, cfg, t._window(R, Cc, dtype), (t.NSTEPS_FIELD,), sigma, resident=0)
    out["paths"] = out["paths"] and t._same(got, b)
    out["differs"] = out.get("differs", []) + [f"{name} {k}" for k, x, y in zip(("Ez", "Hx", "Hy", "Ezx", "dft", "probes"),
        got["fields"] + (got["dft"], got["probes"]), b["fields"] + (b["dft"], b["probes"])) if not np.array_equal(x, y)]
    eps, sig = t.pcpu.g_materials(2)
    g = t.pcpu.g_gradient(fd, eps=eps, sigma=sig, dtype=dtype, nsteps=t.NSTEPS_F, engine=None)
    np.save(f"{OUT}/eps_{name}.npy", g[1])
    np.save(f"{OUT}/sigma_{name}.npy", g[2])
print("PERIODIC_RESULT " + json.dumps(out))
"""


def test_fused_build_within_its_bounds(fd, tmp_path):
    """The fused build's periodic fields and gradients against the exact build's, both on the device, each in a process
    of its own; in both builds the resident and the streamed path agree bit for bit."""
    res = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=900, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("PERIODIC_RESULT ")][-1][16:])
        assert r["arithmetic"] == arith and r["paths"] is True, r
        res[arith] = {k: np.load(out / f"{k[0]}_{k[1]}.npy").astype(np.float64) for k in FUSED_BOUND}
    worst = {}
    for k in FUSED_BOUND:
        e, f = res["exact"][k], res["fused"][k]
        worst[k] = max(np.abs(f[m] - e[m]).max() / np.abs(e[m]).max() for m in range(e.shape[0]))
        print(f"fused vs exact, {k[0]} {k[1]}: worst member {worst[k]:.3e} (bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
