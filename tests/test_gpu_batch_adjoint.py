"""GPU: point sources with channels, the held window and its product, and batch_eps_gradient
(fdtd2d_batch_adjoint.h, adjoint.py).  Fields and probe traces equal the oracle-backed stand-in of
tests/oracle_batch.py bit for bit, window DFTs to 1e-12, and everything is bit-identical whatever the path (resident or
streamed), the launch split and the accumulators' placement; every case asserts the path it took.

The fused build's gradient (FDTD2D_ARITHMETIC=fused) is checked against the exact build's: see FUSED_BOUND below."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_batch import OracleBatch, window_product
import test_batch_adjoint_cpu as cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX = 5e-14, 1e-4
LDS_LIMIT = 163840
OMEGAS = 2 * np.pi * np.linspace(10e9, 100e9, 10)
LAYER = 10
# The fused build contracts a*b+c into FMA, so its fields differ from the exact build's by rounding.  Measured on an
# MI355X with the configuration of test_batch_eps_gradient_matches_the_stand_in (8 members, 5000 steps), worst member,
# max|fused - exact| / max|exact| over the design window: float64 pml 3.0e-15, mur 5.1e-15; float32 pml 1.1e-6,
# mur 8.5e-7.  The bounds are ten times the measured values.
FUSED_BOUND = {("pml", "f64"): 3.0e-14, ("mur", "f64"): 5.1e-14, ("pml", "f32"): 1.1e-5, ("mur", "f32"): 8.5e-6}


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _threads(cells):
    return min(1024, -(-(-(-cells // 4)) // 64) * 64)


def _expect_path(b, nf, window_cells, ncell, never=False, lds_allowed=True, uniform=False):
    """The capacity rule with monitors and point sources, restated; returns whether the run is resident.  uniform: the
    batch holds no coefficient arrays (two arrays fewer)."""
    esz, R, Cc = b.dtype.itemsize, b.rows, b.cols
    arrays = (6 if b.pml else 5) - 2 * uniform
    fields = arrays * _seg(R * Cc, esz) + (_seg(4 * R, esz) + _seg(4 * Cc, esz) if b.pml else 0)
    table, acc = 16 * nf + 8 * ncell, 16 * nf * window_cells
    resident = fields + table <= LDS_LIMIT and not never
    in_lds = bool(nf) and lds_allowed and fields + table + acc <= LDS_LIMIT
    assert b.lds_bytes == fields + table + (acc if in_lds else 0)
    assert b.resident == resident
    assert b.window_in_lds == (in_lds and resident)
    return resident


def _shape(boundary, dtype, where):
    if where == "streamed":
        return (72, 72) if dtype == np.float64 else (100, 120)
    return (48, 48) if (boundary, dtype) == ("pml", np.float64) else (60, 60)


def _setup(fd, rng, B, R, Cc, dtype, K, n, cells=None, uniform=False):
    """Members with their own materials, line sources and amplitudes; point cells: two interior cells owned by one
    thread of the resident walk, a frame / layer cell, an edge cell, the corner and a cell of the rectangle source.
    cells: other point cells, (B, P, 2).  uniform: one permittivity for every cell of every member (what a batch with
    uniform materials holds), for _drive(uniform=True)."""
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(dtype)
    if uniform:
        eps = np.full((B, R, Cc), fd.EPS0 * (1 + 3 * rng.random())).astype(dtype)
    mu = np.full((B, R, Cc), fd.MU0).astype(dtype)
    rects = np.array([[R // 2 + (m % 3) - 1, 3, 1, Cc - 6] for m in range(B)])
    amps = np.stack([[fd.ricker_amplitude(k * DT, 30e9 * (1 + 0.1 * m)) for k in range(n)] for m in range(B)])
    omegas = OMEGAS[None, :] * (1 + 0.01 * np.arange(B))[:, None]
    twin = divmod(10 * Cc + 10 + _threads(R * Cc), Cc)
    if cells is None:
        cells = np.stack([[[10, 10], list(twin), [2 + m % 2, Cc // 3], [R - 1, 5], [0, 0], [int(r[0]), Cc // 2]]
                          for m, r in enumerate(rects)])
    cells = np.asarray(cells)
    weights = rng.standard_normal((B, cells.shape[1], K))
    t = np.arange(n) * DT
    chan = np.stack([np.sin(2 * np.pi * 20e9 * (1 + c) * t + c) * np.exp(-((t - 20 * DT) / (15 * DT)) ** 2)
                     for c in range(K)])
    if K == 6:      # per member
        chan = np.stack([chan * (1 + 0.25 * m) for m in range(B)])
    return eps, mu, rects, amps, omegas, cells, weights, chan


def _drive(b, boundary, cfg, window, splits, uniform=False, layer=LAYER):
    eps, mu, rects, amps, omegas, cells, weights, chan = cfg
    if uniform:      # scalars: the batch keeps no coefficient arrays
        assert np.all(eps == eps[0, 0, 0]) and np.all(mu == mu[0, 0, 0])
        b.set_materials(float(eps[0, 0, 0]), float(mu[0, 0, 0]))
    else:
        b.set_materials(eps, mu)
    b.set_sources(rects)
    if boundary == "pml":
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(eps[:, 0, 0], mu[:, 0, 0])]
        b.set_pml(layer, courant00=np.array(c00))
    n = sum(splits)
    b.set_dft_window(window, omegas).set_probes(cells, n).set_point_sources(cells, weights)
    return n


def _device_run(fd, boundary, dtype, R, Cc, cfg, window, splits, resident=None, spl=None, lds=True, uniform=False,
                layer=LAYER):
    B = cfg[0].shape[0]
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        n = _drive(b, boundary, cfg, window, splits, uniform, layer)
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        path = _expect_path(b, cfg[4].shape[1], window[2] * window[3], cfg[5].shape[1], never=resident == 0,
                            lds_allowed=lds, uniform=uniform)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, cfg[3][:, done:done + k], cfg[7][..., done:done + k])
            done += k
        if path:
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * n
        fields = b.download() + ((b.download_ezx(),) if boundary == "pml" else ())
        return dict(fields=fields, dft=b.read_dft_window(), probes=b.read_probes(), path=path, in_lds=b.window_in_lds)


def _same(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"])) and
            np.array_equal(a["dft"], b["dft"]) and np.array_equal(a["probes"], b["probes"]))


# ---- 4. point sources against the stand-in's restatement --------------------------------------------------------

@pytest.mark.parametrize("K", [1, 6, 32])
@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_point_sources_match_the_stand_in(fd, boundary, dtype, where, K):
    R, Cc = _shape(boundary, dtype, where)
    B, n = 4, 40
    window = (R // 2 - 6, 8, 12, 20)
    cfg = _setup(fd, np.random.default_rng(R + K), B, R, Cc, dtype, K, n)
    got = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (23, 17))
    assert got["path"] == (where == "resident")
    ref = OracleBatch(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary)
    _drive(ref, boundary, cfg, window, (n,))
    ref.run(n, cfg[3], cfg[7])
    for name, a, w in zip(("Ez", "Hx", "Hy"), got["fields"], ref.download()):
        assert np.array_equal(a, w), name
    assert np.array_equal(got["probes"], ref.read_probes())
    assert np.abs(ref.read_probes()[:, 4]).max() > 0       # the corner cell's source shows in its own probe
    want = ref.read_dft_window()
    assert np.abs(got["dft"] - want).max() <= 1e-12 * np.abs(want).max()
    # the point sources changed the fields: a run without channels differs
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        _drive(b, boundary, cfg, window, (n,))
        b.run(n, cfg[3])
        assert not np.array_equal(b.download()[0], got["fields"][0])


# ---- 5. bit-identical whatever the path ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_point_sources_are_bit_identical_on_every_path(fd, boundary, dtype):
    R, Cc = _shape(boundary, dtype, "resident")
    window = (R // 2 - 6, 8, 12, 20) if dtype == np.float32 else (R // 2 - 2, 8, 3, 6)
    cfg = _setup(fd, np.random.default_rng(5), 6, R, Cc, dtype, 6, 60)
    base = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (60,))
    assert base["path"]
    variants = dict(streamed=dict(resident=0), spl=dict(spl=7), split=dict(splits=(1, 32, 27)),
                    global_acc=dict(lds=False), split_spl=dict(splits=(33, 27), spl=10, lds=False))
    seen_lds = {base["in_lds"]}
    for name, kw in variants.items():
        splits = kw.pop("splits", (60,))
        got = _device_run(fd, boundary, dtype, R, Cc, cfg, window, splits, **kw)
        assert got["path"] == (name != "streamed"), name
        seen_lds.add(got["in_lds"])
        assert _same(base, got), name
    assert seen_lds == {True, False}


# ---- 6. one cell, one channel, weight 1.0 is the 1x1 rectangle source ------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_unit_point_source_equals_the_one_cell_rectangle(fd, boundary, where):
    dtype = np.float32
    R, Cc = _shape(boundary, dtype, where)
    B, n = 5, 50
    eps, mu, _, amps, _, _, _, _ = _setup(fd, np.random.default_rng(9), B, R, Cc, dtype, 1, n)
    spots = np.array([[R // 2 + m, Cc // 2 - m] for m in range(B)])
    out = []
    for point in (False, True):
        with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
            b.set_materials(eps, mu)
            if boundary == "pml":
                b.set_pml(LAYER)
            assert b.resident == (where == "resident")
            if point:
                b.set_point_sources(spots[:, None, :], np.ones((B, 1, 1)))
                b.run(n, None, amps[:, None, :])
            else:
                b.set_sources(spots)
                b.run(n, amps)
            out.append(b.download())
    assert np.abs(out[0][0]).max() > 0
    for a, w in zip(out[1], out[0]):
        assert np.array_equal(a, w)


# ---- 7. the held window and the product ------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
def test_window_product_matches_numpy_and_the_held_copy_survives(fd, where):
    boundary, dtype = "pml", np.float32
    R, Cc = _shape(boundary, dtype, where)
    B, n = 5, 40
    window = (R // 2 - 6, 8, 12, 20)
    cfg = _setup(fd, np.random.default_rng(3), B, R, Cc, dtype, 6, n)
    rng = np.random.default_rng(4)
    coef = rng.standard_normal((B, 10)) + 1j * rng.standard_normal((B, 10))
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary) as b:
        _drive(b, boundary, cfg, window, (n,))
        assert b.info(fd._abi.BATCH_INFO_POINT_SOURCES) == 6 and b.info(fd._abi.BATCH_INFO_HELD_WINDOW) == 0
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.dft_window_product(coef)
        assert ei.value.code == fd._abi.E_STATE
        b.run(n, cfg[3])
        first = b.read_dft_window()
        b.hold_dft_window()
        assert b.info(fd._abi.BATCH_INFO_HELD_WINDOW) == 1
        b.reset()
        assert not b.read_dft_window().any()
        inside = np.array([[R // 2 - 3, 10], [R // 2, 15], [R // 2 + 2, 20]])      # three cells of the window
        b.set_sources(np.zeros((B, 4), int)).set_point_sources(inside, cfg[6][:, :3])
        b.run(n, None, cfg[7])
        second = b.read_dft_window()
        assert np.abs(second).max() > 0 and not np.array_equal(first, second)
        launches = b.launches
        got = b.dft_window_product(coef)
        assert b.launches - launches == 1
        want = np.stack([window_product(coef[m], first[m], second[m]) for m in range(B)])
        assert got.shape == (B, 12, 20) and np.array_equal(got, want)
        assert np.array_equal(b.dft_window_product(coef[0]), np.stack([window_product(coef[0], first[m], second[m])
                                                                       for m in range(B)]))
        # setting the window again drops the held copy; removing it leaves nothing to multiply
        b.set_dft_window(window, cfg[4])
        assert b.info(fd._abi.BATCH_INFO_HELD_WINDOW) == 0
        for call in (lambda: b.dft_window_product(coef), ):
            with pytest.raises(fd.Fdtd2dError) as ei:
                call()
            assert ei.value.code == fd._abi.E_STATE
        b.set_dft_window(None, None)
        for call in (b.hold_dft_window, lambda: b.dft_window_product(coef)):
            with pytest.raises(fd.Fdtd2dError) as ei:
                call()
            assert ei.value.code == fd._abi.E_STATE


def test_point_source_arguments_are_checked(fd):
    E_ARG, E_STATE = fd._abi.E_ARG, fd._abi.E_STATE
    with fd.BatchEngine(3, 40, 40, DT, DX) as b:
        b.set_materials()
        ok_cells, ok_w = np.array([[5, 5], [6, 6]]), np.ones((2, 4))
        bad = [(np.zeros((65, 2), int), np.ones((65, 1))), (ok_cells, np.ones((2, 33))), (ok_cells, np.ones((2, 0))),
               (np.array([[5, 5], [40, 6]]), ok_w), (np.array([[5, 5], [6, -1]]), ok_w),
               (np.array([[5, 5], [5, 5]]), ok_w), (ok_cells, np.array([[1.0, 2, 3, np.inf]] * 2)),
               (ok_cells, np.array([[1.0, np.nan, 3, 4]] * 2))]
        for cells, w in bad:
            with pytest.raises(fd.Fdtd2dError) as ei:
                b.set_point_sources(cells, w)
            assert ei.value.code == E_ARG, (cells.shape, w.shape)
        assert b.info(fd._abi.BATCH_INFO_POINT_SOURCES) == 0
        rc = b._lib.fdtd2d_batch_run_channels(b._h, 4, None, np.zeros(16).ctypes.data_as(
            __import__("ctypes").POINTER(__import__("ctypes").c_double)), 0)
        assert rc == E_STATE
        b.set_point_sources(ok_cells, ok_w)
        assert b.info(fd._abi.BATCH_INFO_POINT_SOURCES) == 2
        assert b._lib.fdtd2d_batch_run_channels(b._h, 4, None, None, 0) == E_ARG
        with pytest.raises(ValueError, match="channels"):
            b.run(4, None, np.zeros((3, 4)))
        # fdtd2d_batch_run keeps ignoring point sources
        b.run(4)
        assert not b.download()[0].any()
        b.set_point_sources(None)
        assert b.info(fd._abi.BATCH_INFO_POINT_SOURCES) == 0


# ---- 9. members are independent -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
def test_point_source_members_are_independent(fd, where):
    boundary, dtype = "mur", np.float32
    R, Cc = _shape(boundary, dtype, where)
    window = (R // 2 - 6, 8, 12, 20)
    cfg = list(_setup(fd, np.random.default_rng(11), 6, R, Cc, dtype, 6, 40))
    a = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (40,))
    cfg[6] = cfg[6].copy()
    cfg[6][2] *= -1.5
    b = _device_run(fd, boundary, dtype, R, Cc, cfg, window, (40,))
    for m in range(6):
        same = (all(np.array_equal(x[m], y[m]) for x, y in zip(a["fields"], b["fields"])) and
                np.array_equal(a["dft"][m], b["dft"][m]) and np.array_equal(a["probes"][m], b["probes"][m]))
        assert same == (m != 2), m


# ---- 8. batch_eps_gradient on the device against the stand-in ----------------------------------------------------------------

_stand_in = {}


def _reference(fd, boundary, dtype):
    key = (boundary, np.dtype(dtype).name)
    if key not in _stand_in:
        _stand_in[key] = cpu.gradient(fd, boundary, dtype, eps=cpu.design_eps(count=8))
    return _stand_in[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["pml", "mur"])
def test_batch_eps_gradient_matches_the_stand_in(fd, boundary, dtype):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_gradient")
    Jr, gr, sr, ir = _reference(fd, boundary, dtype)
    J, g, s, info = cpu.gradient(fd, boundary, dtype, eps=cpu.design_eps(count=8), engine=None)
    assert g.shape == (8, 16, 12) and g.dtype == np.float64 and s.shape == (8, 8, 3)
    assert np.array_equal(s, sr) and np.array_equal(J, Jr)          # the probe traces are the oracle's bit for bit
    for m in range(8):
        gmax = np.abs(gr[m]).max()
        assert gmax > 0 and np.abs(g[m] - gr[m]).max() <= 1e-9 * gmax, m
    assert np.allclose(info["residual_forward"], ir["residual_forward"], rtol=1e-12)
    assert len({gr[m].tobytes() for m in range(8)}) == 8            # eight different members


def test_batch_eps_gradient_beyond_one_round_of_workgroups(fd):
    """More members than resident workgroups fit on the device at once: every workgroup takes several members."""
    if fd.ARITHMETIC != "exact":
        pytest.skip("the fused build is checked against the exact one in test_fused_build_gradient")
    cus = 256                                         # compute units of an MI355X
    dtype, boundary = np.float64, "pml"
    with fd.BatchEngine(4, cpu.R, cpu.C, cpu.DT, cpu.DX, dtype=dtype, boundary=boundary) as b:
        b.set_materials().set_pml(cpu.LAYER)
        per_cu = LDS_LIMIT // b.lds_bytes
        assert b.resident and per_cu >= 1
    B = per_cu * cus + 8
    gr = _reference(fd, boundary, dtype)[1]
    eps = np.concatenate([cpu.design_eps(count=8)] * -(-B // 8))[:B]
    g = cpu.gradient(fd, boundary, dtype, eps=eps, engine=None)[1]
    for m in range(B):
        assert np.abs(g[m] - gr[m % 8]).max() <= 1e-9 * np.abs(gr[m % 8]).max(), m


CHILD = r"""
import json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import numpy as np
import fdtd2d_amd as fd
import test_batch_adjoint_cpu as cpu
out = {"arithmetic": fd.ARITHMETIC}
for boundary in ("pml", "mur"):
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        g = cpu.gradient(fd, boundary, dtype, eps=cpu.design_eps(count=8), engine=None)[1]
        np.save(f"{OUT}/{boundary}_{name}.npy", g)
print("ADJ_RESULT " + json.dumps(out))
"""


def test_fused_build_gradient_within_its_bound(fd, tmp_path):
    """The fused build's gradients against the exact build's, both on the device, each in a process of its own."""
    worst = {}
    grads = {}
    for arith in ("exact", "fused"):
        out = tmp_path / arith
        out.mkdir()
        p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nOUT = {str(out)!r}\n" + CHILD],
                           capture_output=True, text=True, timeout=900, env=dict(os.environ, FDTD2D_ARITHMETIC=arith))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        res = json.loads([l for l in p.stdout.splitlines() if l.startswith("ADJ_RESULT ")][-1][11:])
        assert res["arithmetic"] == arith
        grads[arith] = {k: np.load(out / f"{k[0]}_{k[1]}.npy") for k in FUSED_BOUND}
    for k in FUSED_BOUND:
        e, f = grads["exact"][k], grads["fused"][k]
        worst[k] = max(np.abs(f[m] - e[m]).max() / np.abs(e[m]).max() for m in range(8))
        print(f"fused vs exact gradient, {k[0]} {k[1]}: worst member {worst[k]:.3e} of max|gradient| "
              f"(bound {FUSED_BOUND[k]:.1e})")
    for k in FUSED_BOUND:
        assert worst[k] <= FUSED_BOUND[k], k
