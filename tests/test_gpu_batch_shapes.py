"""GPU: the batched resident kernels at every cells-per-thread variant (MAXC = 4, 8, 16) the capacity rule can reach.

The rows are those of tests/test_batch_shapes_cpu.py (CASES), which also chooses their point cells and window and checks
on the CPU that each row is resident at the stated cells per thread with nthr % C != 0.  Exercised here, as
(family, MAXC): monitors + point sources with Mur and with the PML at 4, 8 and 16 in float32 and at 4 and 8 in float64
(8: uniform materials); monitors alone (no point sources) with Mur and with the PML at 8 and 16 in float32 and at 8 in
float64, the float32 Mur rows also against Engine; lossy with Mur and with the PML at 4 and 8 in float32 and at 4 in
float64; periodic (layer and PEC rows) at 4 and 8 in float32 and at 4 in float64.
Unreachable, whatever the shape: MAXC = 16 for lossy, periodic and every float64 family, MAXC = 8 for float64 with
material arrays (5, 6 or 7 arrays in LDS).

Every row runs 3 members for 40 steps as run(23), run(17), with a line source and point cells that are probes too: one
thread's slots {0, 5, 7} (8 cells per thread), {0, 5, 7, 9, last} (MAXC = 16) or the like where the walk is shorter
(wanted_slots), another thread's last slot alone (slot 4 or higher at MAXC = 8, 8 or higher at 16), the grid's last
cell, a cell of the last row, cell (0, 0) and a cell of the line source; periodic rows add columns 0 and C - 2 at slot 4
or higher and a probe on the image column.  The 3 x 6 window lies around that lone cell (in a periodic row around the
cell of column C - 2, with the image column): a wave travels six cells in 40 steps, so only a point source of its own
fills a window past 4 nthr (8 nthr) of the cell walk.  A batch with uniform materials holds one eps and mu for all its
members, so those rows' members differ by their sources, frequencies and weights alone.

Exact build: fields (and Ezx) and probe traces equal the stand-in's bit for bit, the window DFT to 1e-12 of its maximum.
Both builds: the streamed path (resident=0) and the accumulators in global memory give the same bits, as do
steps_per_launch=7 and the split (1, 22, 17) at one MAXC = 8 and one MAXC = 16 row per family; every case asserts the
path it took, its launch count and where the accumulators were.  The float32 Mur rows with one member and no point
sources equal a plain Engine bit for bit.

Forcing the slot that fdtd2d_batch_set_point_sources writes to min(cell / nthr, 3) fails every MAXC = 8 and 16 row of
the first test here, and reading the slot mask as pts >> (q & 3) in the lossy Mur resident kernel fails that family's
MAXC = 8 row, while the sibling modules' tests still pass with either."""
import numpy as np
import pytest

from oracle_batch import OracleBatch
from oracle_batch_lossy import LossyOracle
import test_batch_shapes_cpu as tab
import test_gpu_batch_adjoint as adj
import test_gpu_batch_lossy as los
import test_gpu_batch_periodic as per

pytestmark = pytest.mark.gpu

DT, DX = adj.DT, adj.DX
B, N, SPLITS, K = 3, 40, (23, 17), 6
DTYPES = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _sigma(rng, c, top=20.0):
    """Random conductivity up to `top` S/m on the cells that may conduct (none of an 11-row member), zero on 30 %."""
    g = max(6, c.layer)
    s = np.zeros((B, c.R, c.C))
    inner = s[:, g:c.R - g, :] if c.family == "periodic" else s[:, g:c.R - g, g:c.C - g]
    if inner.size:
        inner[...] = np.where(rng.random(inner.shape) < 0.3, 0.0, top * rng.random(inner.shape))
    return s


_configs = {}


def _config(fd, c):
    """(cfg of the family's driver, sigma or None), seeded with R + C."""
    if c not in _configs:
        rng = np.random.default_rng(c.R + c.C)
        dtype = DTYPES[c.dtype]
        cells = np.array(tab.point_cells(c, B))
        if c.family == "periodic":
            cfg = per._cfg(fd, rng, B, c.R, c.C, dtype, N, K, points=cells, image_row=tab.image_probe(c)[0])
            rects = cfg["rects"]
        else:
            cfg = list(adj._setup(fd, rng, B, c.R, c.C, dtype, K, N, cells=cells, uniform=c.materials == "uniform"))
            if c.materials == "arrays":
                cfg[1] = (fd.MU0 * np.where(rng.random((B, c.R, c.C)) < 0.1, 1.5, 1.0)).astype(dtype)
            rects = cfg[2]
        for m, (r0, c0, nr, nc) in enumerate(rects):      # the last point cell lies in the member's line source
            r, j = cells[m, -1]
            assert r0 <= r < r0 + nr and c0 <= j < c0 + nc and nr == 1 and nc > 1
        _configs[c] = (cfg, None if c.family == "points" else _sigma(rng, c))
    return _configs[c]


def _ntab(c, cfg):
    """Entries of the point-source table: a periodic batch lists the cells of column 0 at their images too."""
    if c.family != "periodic":
        return cfg[5].shape[1]
    return cfg["points"].shape[1] + max(int((cfg["points"][m, :, 1] == 0).sum()) for m in range(B))


def _run(fd, c, splits=SPLITS, **kw):
    """The family's own driver: it asserts the capacity rule, the path and the launch count."""
    cfg, sigma = _config(fd, c)
    dtype, window = DTYPES[c.dtype], tab.window(c)
    if c.family == "points":
        return adj._device_run(fd, c.boundary, dtype, c.R, c.C, cfg, window, splits, uniform=c.materials == "uniform",
                               layer=c.layer, **kw)
    if c.family == "lossy":
        return los._device_run(fd, c.boundary, dtype, c.R, c.C, cfg, window, splits, sigma, layer=c.layer, **kw)
    return per._device_run(fd, dtype, c.R, c.C, cfg, window, splits, sigma, layer=c.layer, **kw)


def _stand_in(fd, c):
    cfg, sigma = _config(fd, c)
    dtype, window = DTYPES[c.dtype], tab.window(c)
    if c.family == "periodic":
        return per._stand_in(dtype, c.R, c.C, cfg, window, sigma, c.layer)
    if c.family == "points":
        ref = OracleBatch(B, c.R, c.C, DT, DX, dtype=dtype, boundary=c.boundary)
        adj._drive(ref, c.boundary, cfg, window, (N,), c.materials == "uniform", c.layer)
    else:
        ref = LossyOracle(B, c.R, c.C, DT, DX, dtype=dtype, boundary=c.boundary)
        los._drive(ref, c.boundary, cfg, window, N, True, c.layer)
        ref.set_conductivity(sigma)
    ref.run(N, cfg[3], cfg[7])
    fields = ref.download() + ((ref.Ezx.copy(),) if c.boundary == "pml" else ())
    return dict(fields=fields, dft=ref.read_dft_window(), probes=ref.read_probes())


def _silent(fd, c):
    """Ez of the same members run without channels: the point sources stay silent."""
    cfg, sigma = _config(fd, c)
    dtype, window = DTYPES[c.dtype], tab.window(c)
    boundary = "periodic" if c.family == "periodic" else c.boundary
    with fd.BatchEngine(B, c.R, c.C, DT, DX, dtype=dtype, boundary=boundary) as b:
        if c.family == "periodic":
            per._drive(b, cfg, window, c.layer, sigma, True)
            amps = cfg["amps"]
        elif c.family == "lossy":
            los._drive(b, c.boundary, cfg, window, N, True, c.layer)
            b.set_conductivity(sigma)
            amps = cfg[3]
        else:
            adj._drive(b, c.boundary, cfg, window, (N,), c.materials == "uniform", c.layer)
            amps = cfg[3]
        assert b.resident
        b.run(N, amps)
        return b.download()[0]


def _same(a, b):
    return (len(a["fields"]) == len(b["fields"]) and all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"]))
            and np.array_equal(a["dft"], b["dft"]) and np.array_equal(a["probes"], b["probes"]))


# ---- 1. every row against the stand-in, the streamed path and the other placement of the accumulators ---------------------

@pytest.mark.parametrize("c", tab.CASES, ids=tab.case_id)
def test_the_row_matches_the_stand_in_and_the_streamed_path(fd, c):
    cfg, _ = _config(fd, c)
    npoint = len(tab.fixed_cells(c)) + 1
    got = _run(fd, c)
    assert got["path"] and got["in_lds"] == tab.window_in_lds(c, _ntab(c, cfg), 18)
    # both builds: the streamed path and the accumulators in global memory give the same bits
    streamed = _run(fd, c, resident=0)
    assert not streamed["path"] and _same(got, streamed)
    in_global = _run(fd, c, lds=False)
    assert in_global["path"] and not in_global["in_lds"] and _same(got, in_global)
    # every point cell's source acted: its own probe saw it, and the fields differ from a run without channels
    assert got["probes"].shape == (B, npoint + (c.family == "periodic"), N)
    assert np.all(np.abs(got["probes"][:, :npoint]).max(axis=2) > 0)
    assert np.abs(got["dft"]).max() > 0
    assert not np.array_equal(_silent(fd, c), got["fields"][0])
    if c.family == "periodic":
        Ez, Ezx = got["fields"][0], got["fields"][3]
        assert np.array_equal(Ez[:, :, -1], Ez[:, :, 0]) and np.array_equal(Ezx[:, :, -1], Ezx[:, :, 0])
        assert np.abs(got["probes"][:, -1]).max() > 0             # the probe on the image column saw the field
    if fd.ARITHMETIC != "exact":      # the fused build's fields differ from the stand-in's by rounding
        return
    ref = _stand_in(fd, c)
    names = ("Ez", "Hx", "Hy", "Ezx")
    assert len(got["fields"]) == len(ref["fields"]) == (3 if c.boundary == "mur" else 4)
    for name, a, w in zip(names, got["fields"], ref["fields"]):
        assert np.array_equal(a, w), name
    assert np.array_equal(got["probes"], ref["probes"])
    assert np.abs(got["dft"] - ref["dft"]).max() <= 1e-12 * np.abs(ref["dft"]).max()


# ---- 2. steps_per_launch and the launch split at one MAXC = 8 and one MAXC = 16 row per family ------------------------------------

def _first(family, maxc, boundary):
    return next(c for c in tab.CASES if (c.family, c.maxc, c.boundary) == (family, maxc, boundary))


SPLIT_CASES = [_first("points", 8, "mur"), _first("points", 8, "pml"), _first("points", 16, "mur"),
               _first("points", 16, "pml"), _first("lossy", 8, "mur"), _first("lossy", 8, "pml"),
               _first("periodic", 8, "layer")]


@pytest.mark.parametrize("c", SPLIT_CASES, ids=tab.case_id)
def test_launch_splits_are_bit_identical_at_the_wide_variants(fd, c):
    base = _run(fd, c, splits=(N,))
    assert base["path"] and np.abs(base["fields"][0]).max() > 0
    chunked = _run(fd, c, splits=(N,), spl=7)
    assert chunked["path"] and _same(base, chunked)
    split = _run(fd, c, splits=(1, 22, 17))
    assert split["path"] and _same(base, split)


# ---- 3. monitors alone: the monitored kernels without point sources, against the stand-in and against Engine ---------------

WIDE_POINTS = [c for c in tab.CASES if c.family == "points" and c.maxc > 4]


def _monitors_alone(fd, c, make, resident=None):
    """The row's members with window and probes but no point sources, run as (23, 17) without channels.  The line
    sources move down to the rows of the lone cell and the window lies across them, past 4 nthr (8 nthr)."""
    cfg = list(_config(fd, c)[0])
    dtype, uniform = DTYPES[c.dtype], c.materials == "uniform"
    row = min(tab.fixed_cells(c)["lone"][0], c.R - 3)
    cfg[2] = cfg[2] + [row - c.R // 2, 0, 0, 0]
    window = (row - 1, c.C // 2 - 3, 3, 6)
    assert window[0] * c.C + window[1] >= c.maxc // 2 * tab.resident_threads(c.R * c.C)
    with make(B, c.R, c.C, DT, DX, dtype=dtype, boundary=c.boundary) as b:
        adj._drive(b, c.boundary, cfg, window, (N,), uniform, c.layer)
        b.set_point_sources(None)
        if make is not OracleBatch:
            b.set_option(resident=resident)
            assert b.info(fd._abi.BATCH_INFO_POINT_SOURCES) == 0
            path = adj._expect_path(b, cfg[4].shape[1], 18, 0, never=resident == 0, uniform=uniform)
            assert path == (resident is None)
            launches = b.launches
        done = 0
        for k in SPLITS:
            b.run(k, cfg[3][:, done:done + k])
            done += k
        if make is not OracleBatch:
            assert b.launches - launches == (len(SPLITS) if path else 2 * N)
        fields = b.download() + ((b.Ezx.copy() if make is OracleBatch else b.download_ezx(),) if c.boundary == "pml"
                                 else ())
        return dict(fields=fields, dft=b.read_dft_window(), probes=b.read_probes())


@pytest.mark.parametrize("c", WIDE_POINTS, ids=tab.case_id)
def test_monitors_alone_match_the_stand_in_and_the_streamed_path(fd, c):
    assert {(k.boundary, k.maxc) for k in WIDE_POINTS} == {("mur", 8), ("mur", 16), ("pml", 8), ("pml", 16)}
    got = _monitors_alone(fd, c, fd.BatchEngine)
    assert _same(got, _monitors_alone(fd, c, fd.BatchEngine, resident=0))
    assert np.abs(got["fields"][0]).max() > 0 and np.abs(got["dft"]).max() > 0 and np.abs(got["probes"]).max() > 0
    if fd.ARITHMETIC != "exact":
        return
    ref = _monitors_alone(fd, c, OracleBatch)
    for name, a, w in zip(("Ez", "Hx", "Hy", "Ezx"), got["fields"], ref["fields"]):
        assert np.array_equal(a, w), name
    assert np.array_equal(got["probes"], ref["probes"])
    assert np.abs(got["dft"] - ref["dft"]).max() <= 1e-12 * np.abs(ref["dft"]).max()


ENGINE_CASES = [c for c in tab.CASES if (c.family, c.boundary, c.dtype) == ("points", "mur", "f32") and c.maxc > 4]


@pytest.mark.parametrize("c", ENGINE_CASES, ids=tab.case_id)
def test_one_monitored_member_equals_engine(fd, c):
    """One member, window and probes but no point sources (the monitored kernels without them) against Engine.  The
    fields are the check: the line source's wave does not reach the row's window and probe cells in 40 steps."""
    assert {k.maxc for k in ENGINE_CASES} == {8, 16}
    cfg, _ = _config(fd, c)
    eps, mu, rects, amps, omegas = (a[:1] for a in cfg[:5])
    dtype, window, uniform = DTYPES[c.dtype], tab.window(c), c.materials == "uniform"
    fixed = tab.fixed_cells(c)
    cells = np.array([fixed["lone"], fixed[max((k for k in fixed if k.startswith("many")), key=lambda k: fixed[k])],
                      fixed["last"]])
    materials = (float(eps[0, 0, 0]), float(mu[0, 0, 0])) if uniform else None
    with fd.BatchEngine(1, c.R, c.C, DT, DX, dtype=dtype, boundary="mur") as b:
        b.set_materials(*(materials or (eps, mu))).set_sources(rects)
        b.set_dft_window(window, omegas).set_probes(cells, N)
        assert adj._expect_path(b, omegas.shape[1], 18, 0, uniform=uniform)
        launches = b.launches
        b.run(N, amps)
        assert b.launches - launches == 1
        got = dict(fields=b.download(), dft=b.read_dft_window()[0], probes=b.read_probes()[0])
    r, j, nr, nc = (int(v) for v in rects[0])
    for p, (pr, pc) in enumerate(cells):
        with fd.Engine(c.R, c.C, DT, DX, dtype=dtype) as e:
            e.set_materials(*(materials or (eps[0], mu[0])))
            e.set_source_extent(nr, nc)
            e.set_probe(int(pr), int(pc), N)
            e.set_dft(window, omegas[0], 1)
            e.run(N, r, j, amps[0, :N])
            assert np.array_equal(e.read_probe(0, N), got["probes"][p]), p
            if p == 0:
                want = e.read_dft()
                assert np.abs(got["dft"] - want).max() <= 1e-12 * np.abs(want).max()
                for name, a, w in zip(("Ez", "Hx", "Hy"), got["fields"], e.download()):
                    assert np.abs(w).max() > 0 and np.array_equal(a[0], w), name
