"""GPU: the batch monitors (BatchEngine.set_dft_window / set_probes, fdtd2d_batch_monitor.h).  Probe traces equal the
oracle's Ez step by step, window DFTs equal the float64 sum over the oracle's Ez to 1e-12, and both are bit-identical
whatever the path (resident or streamed), the accumulators' placement (LDS or global memory) and the launch split;
every case asserts the path it took."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX = 5e-14, 1e-4
LDS_LIMIT = 163840
OMEGAS = 2 * np.pi * np.linspace(10e9, 100e9, 10)
WINDOWS = ("30x1", "12x20")


def _window(name, R):
    """A 30 x 1 column and a 12 x 20 patch, both across the members' line sources (rows R // 2 - 1 .. R // 2 + 1)."""
    return (9, 30, 30, 1) if name == "30x1" else (R // 2 - 6, 8, 12, 20)


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def _rule(b, nf, window_cells, lds_allowed=True):
    """The capacity rule with monitors, restated: (resident, accumulators in LDS, LDS bytes)."""
    esz = b.dtype.itemsize
    R, Cc = b.rows, b.cols
    if b.pml:
        fields = 6 * _seg(R * Cc, esz) + _seg(4 * R, esz) + _seg(4 * Cc, esz)
    else:
        fields = 5 * _seg(R * Cc, esz)
    table, acc = 16 * nf, 16 * nf * window_cells
    resident = fields + table <= LDS_LIMIT
    in_lds = bool(nf) and lds_allowed and fields + table + acc <= LDS_LIMIT
    return resident, in_lds, fields + table + (acc if in_lds else 0)


def _expect_path(b, nf, window_cells, never=False, lds_allowed=True):
    resident, in_lds, lds = _rule(b, nf, window_cells, lds_allowed)
    assert b.lds_bytes == lds
    assert b.resident == (resident and not never)
    assert b.window_in_lds == (in_lds and b.resident)
    return b.resident


def _members(fd, rng, B, R, Cc, dtype):
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(dtype)
    mu = np.full((B, R, Cc), fd.MU0).astype(dtype)
    rects = np.array([[R // 2 + (m % 3) - 1, 3, 1, Cc - 6] for m in range(B)])        # Ricker line sources
    fcs = 30e9 * (1 + 0.1 * np.arange(B))
    amps = np.stack([[fd.ricker_amplitude(n * DT, f) for n in range(200)] for f in fcs])
    omegas = OMEGAS[None, :] * (1 + 0.01 * np.arange(B))[:, None]
    return eps, mu, rects, amps, omegas


def _probe_cells(R, Cc, rects):
    """An interior cell, a corner (Mur band) cell, a source cell and a cell in a 10-cell PML layer, per member."""
    return np.stack([[[R // 2 + 7, Cc // 2 + 3], [0, 0], [int(r[0]), Cc // 2], [3, Cc // 3]] for r in rects])


def _oracle(fd, boundary, eps, mu, rect, amps, n, L=10):
    """Ez (float64) after every step of one member, and its final fields."""
    from oracle import fdtd_numpy as onp
    from oracle import pml_numpy as pm
    R, Cc = eps.shape
    Ez, Hx, Hy = onp.grid_zeros(R, Cc, eps.dtype)
    r, c, nr, nc = (int(v) for v in rect)
    trace = []
    if boundary == "pml":
        Ezx = np.zeros_like(Ez)
        S = (1 / np.sqrt(float(eps[0, 0]) * float(mu[0, 0])) * DT) / DX
        P = pm.profiles(R, Cc, S, L=L, dtype=eps.dtype)
        for k in range(n):
            pm.step(Ez, Ezx, Hx, Hy, eps, mu, DT, DX, P)
            Ez[r:r + nr, c:c + nc] = (Ez[r:r + nr, c:c + nc].astype(np.float64) + amps[k]).astype(Ez.dtype)
            trace.append(Ez.astype(np.float64))
    else:
        onp.leapfrog(Ez, Hx, Hy, eps, mu, DT, DX, n, r, c, amps=amps[:n], extent=(nr, nc),
                     on_step=lambda i, E, *_: trace.append(E.astype(np.float64)))
    return np.array(trace), (Ez, Hx, Hy)


def _dft_of(trace, window, omegas, every, step0=0):
    """The float64 window DFT of a trace (trace[k] = Ez after step k + 1), summed step by step."""
    r0, c0, nr, nc = window
    re = np.zeros((len(omegas), nr, nc))
    im = np.zeros((len(omegas), nr, nc))
    for k in range(len(trace)):
        s = k + 1
        if (s - step0) % every:
            continue
        e = trace[k][r0:r0 + nr, c0:c0 + nc]
        for f, w in enumerate(omegas):
            t = s * DT
            re[f] += e * np.cos(w * t)
            im[f] += e * -np.sin(w * t)
    return re + 1j * im


def _make(fd, boundary, B, R, Cc, dtype, eps, mu, rects, L=10):
    b = fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary=boundary)
    b.set_materials(eps, mu).set_sources(rects)
    if boundary == "pml":
        c00 = [(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(eps[:, 0, 0], mu[:, 0, 0])]
        b.set_pml(L, courant00=np.array(c00))
    return b


def _monitored_run(fd, boundary, dtype, R, Cc, window, every, splits, B=8, seed=0, resident=None, spl=None,
                   lds=True, omegas=None, cells=None, whole=None):
    rng = np.random.default_rng(seed)
    eps, mu, rects, amps, om = _members(fd, rng, B, R, Cc, dtype)
    om = om if omegas is None else omegas
    cells = _probe_cells(R, Cc, rects) if cells is None else cells
    n = sum(splits)
    with _make(fd, boundary, B, R, Cc, dtype, eps, mu, rects) as b:
        b.set_option(resident=resident, steps_per_launch=spl).set_window_lds(lds)
        if whole is not None:
            b.set_dft(whole, every)
        b.set_dft_window(window, om, every).set_probes(cells, n + 5)
        path = _expect_path(b, om.shape[1], window[2] * window[3], never=resident == 0, lds_allowed=lds)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, amps[:, done:done + k])
            done += k
        if path:
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * done
        assert b.probe_samples == n
        out = dict(dft=b.read_dft_window(), probes=b.read_probes(), fields=b.download(), path=path,
                   in_lds=b.window_in_lds, whole=b.read_dft() if whole is not None else None)
    return out, (eps, mu, rects, amps, om, cells)


def _shape(boundary, dtype, where):
    if where == "streamed":
        return (72, 72) if dtype == np.float64 else (100, 120)
    return (48, 48) if (boundary, dtype) == ("pml", np.float64) else (60, 60)


# ---- 1. oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("wname", WINDOWS)
@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_monitors_match_the_oracle(fd, boundary, dtype, where, wname, every):
    R, Cc = _shape(boundary, dtype, where)
    window = _window(wname, R)
    got, (eps, mu, rects, amps, om, cells) = _monitored_run(fd, boundary, dtype, R, Cc, window, every, (23, 17),
                                                            seed=R + every + len(wname))
    assert got["path"] == (where == "resident")
    n = 40
    for m in range(8):
        trace, fields = _oracle(fd, boundary, eps[m], mu[m], rects[m], amps[m], n)
        for p, (r, c) in enumerate(cells[m]):
            assert np.array_equal(got["probes"][m, p], trace[:, r, c]), (m, p)
        want = _dft_of(trace, window, om[m], every)
        assert np.abs(want).max() > 0
        assert np.abs(got["dft"][m] - want).max() <= 1e-12 * np.abs(want).max(), m
        for a, w in zip(got["fields"], fields):
            assert np.array_equal(a[m], w), m


# ---- 2. invariance --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["mur", "pml"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_monitors_do_not_depend_on_path_placement_or_split(fd, boundary, dtype):
    R, Cc = _shape(boundary, dtype, "resident")
    window = _window("30x1", R)
    runs = {}
    for key, kw in {"lds": {}, "global": dict(lds=False), "spl7": dict(spl=7), "streamed": dict(resident=0)}.items():
        runs[key], _ = _monitored_run(fd, boundary, dtype, R, Cc, window, 3, (19, 20), seed=5, **kw)
    assert runs["lds"]["in_lds"] and not runs["global"]["in_lds"] and runs["lds"]["path"]
    assert not runs["streamed"]["path"]
    for key in ("global", "spl7", "streamed"):
        assert np.array_equal(runs[key]["dft"], runs["lds"]["dft"]), key
        assert np.array_equal(runs[key]["probes"], runs["lds"]["probes"]), key
        for a, w in zip(runs[key]["fields"], runs["lds"]["fields"]):
            assert np.array_equal(a, w), key


def test_window_accumulators_too_large_for_lds_stay_global(fd):
    """A window whose accumulators do not fit beside the arrays: resident, accumulators in global memory."""
    got, _ = _monitored_run(fd, "mur", np.float32, 60, 60, (0, 0, 60, 30), 1, (11,), B=4)
    assert np.abs(got["dft"]).max() > 0
    assert got["path"] and not got["in_lds"]


# ---- 3. against the whole-grid DFT -------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_window_equals_the_whole_grid_dft(fd, boundary, where):
    dtype = np.float32
    R, Cc = _shape(boundary, dtype, where)
    r0, c0, nr, nc = window = _window("12x20", R)
    base, _ = _monitored_run(fd, boundary, dtype, R, Cc, window, 3, (30,), seed=9)
    om = _members(fd, np.random.default_rng(9), 8, R, Cc, dtype)[4]
    for k in (0, 4, 9):     # both monitors in one run
        got, _ = _monitored_run(fd, boundary, dtype, R, Cc, window, 3, (30,), seed=9, whole=om[:, k])
        assert got["path"] == (where == "resident")
        assert np.array_equal(got["whole"][:, r0:r0 + nr, c0:c0 + nc], got["dft"][:, k]), k
        assert np.array_equal(got["dft"], base["dft"]) and np.array_equal(got["probes"], base["probes"])


# ---- 4. against Engine -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_monitors_match_engine(fd, dtype):
    R, Cc = 60, 60
    window, every, n = _window("30x1", R), 1, 40
    got, (eps, mu, rects, amps, om, cells) = _monitored_run(fd, "mur", dtype, R, Cc, window, every, (n,), seed=3)
    m = 5
    r, c, nr, nc = (int(v) for v in rects[m])
    for p, (pr, pc) in enumerate(cells[m]):
        e = fd.Engine(R, Cc, DT, DX, dtype=dtype)
        e.set_materials(eps[m], mu[m])
        e.set_source_extent(nr, nc)
        e.set_probe(int(pr), int(pc), n)
        if p == 0:
            e.set_dft(window, om[m], every)
        e.run(n, r, c, amps[m, :n])
        assert np.array_equal(e.read_probe(0, n), got["probes"][m, p]), p
        if p == 0:
            want = e.read_dft()
            assert np.abs(got["dft"][m] - want).max() <= 1e-12 * np.abs(want).max()
        e.close()


# ---- 5. no side effects ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
@pytest.mark.parametrize("boundary", ["mur", "pml"])
def test_monitors_leave_the_fields_alone(fd, boundary, where):
    dtype = np.float32
    R, Cc = _shape(boundary, dtype, where)
    got, (eps, mu, rects, amps, om, cells) = _monitored_run(fd, boundary, dtype, R, Cc, _window("30x1", R), 1, (25,),
                                                            seed=11)
    with _make(fd, boundary, 8, R, Cc, dtype, eps, mu, rects) as b:
        b.run(25, amps[:, :25])
        plain = b.download()
    for a, w in zip(got["fields"], plain):
        assert np.array_equal(a, w)


# ---- 6. member independence ------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["resident", "streamed"])
def test_members_are_independent(fd, where):
    dtype = np.float64
    R, Cc = _shape("mur", dtype, where)
    window = _window("12x20", R)
    base, (eps, mu, rects, amps, om, cells) = _monitored_run(fd, "mur", dtype, R, Cc, window, 1, (20,), seed=13)
    om2, cells2 = om.copy(), cells.copy()
    om2[2] *= 1.7
    cells2[2] = [[1, 1], [R - 2, Cc - 2], [5, 5], [10, 11]]
    got, _ = _monitored_run(fd, "mur", dtype, R, Cc, window, 1, (20,), seed=13, omegas=om2, cells=cells2)
    others = [m for m in range(8) if m != 2]
    assert np.array_equal(got["dft"][others], base["dft"][others])
    assert np.array_equal(got["probes"][others], base["probes"][others])
    assert not np.array_equal(got["dft"][2], base["dft"][2]) and not np.array_equal(got["probes"][2], base["probes"][2])


# ---- 7. lifecycle and refusals ---------------------------------------------------------------------------------

@pytest.mark.parametrize("resident", [None, 0])
def test_lifecycle(fd, resident):
    rng = np.random.default_rng(17)
    B, R, Cc, dtype = 4, 40, 40, np.float32
    eps, mu, rects, amps, om = _members(fd, rng, B, R, Cc, dtype)
    cells = _probe_cells(R, Cc, rects)
    window = (10, 10, 6, 7)
    with _make(fd, "mur", B, R, Cc, dtype, eps, mu, rects) as b:
        b.set_option(resident=resident)
        b.run(5, amps[:, :5])                               # monitors count from their own call
        b.set_dft_window(window, om[:, :3], 2).set_probes(cells, 12)
        b.run(9, amps[:, 5:14])
        assert b.probe_samples == 9 and b.read_probes().shape == (B, 4, 9)
        b.run(6, amps[:, 14:20])
        full = b.read_probes()
        assert full.shape == (B, 4, 12) and b.probe_samples == 12      # capacity cut-off
        assert np.array_equal(b.read_probes(3, 4), full[:, :, 3:7])
        assert b.read_probes(12, 0).shape == (B, 4, 0)
        dft1 = b.read_dft_window()
        assert dft1.shape == (B, 3, 6, 7) and np.abs(dft1).max() > 0
        # reset: zero fields and monitors, counts restart at step 0; the same run gives the same samples
        b.reset()
        assert b.probe_samples == 0 and np.abs(b.read_dft_window()).max() == 0
        b.run(20, amps[:, :20])
        again = b.read_probes()
        trace = [(_oracle(fd, "mur", eps[m], mu[m], rects[m], amps[m], 12)[0]) for m in range(B)]
        for m in range(B):
            for p, (r, c) in enumerate(cells[m]):
                assert np.array_equal(again[m, p], trace[m][:, r, c])
        # refusals: the library's codes, nothing changed
        E = fd.Fdtd2dError
        for args in [((0, 0, 0, 3), om[:, :3], 1), ((38, 0, 3, 3), om[:, :3], 1), ((0, -1, 3, 3), om[:, :3], 1),
                     ((0, 0, 3, 3), np.ones((B, 17)), 1), ((0, 0, 3, 3), om[:, :3], 0)]:
            with pytest.raises(E) as ei:
                b.set_dft_window(*args)
            assert ei.value.code == -1, args
        for cl, cap in [(np.zeros((B, 65, 2), int), 4), ([[40, 0]], 4), ([[0, -1]], 4), ([[1, 1]], 0)]:
            with pytest.raises(E) as ei:
                b.set_probes(cl, cap)
            assert ei.value.code == -1, (cl, cap)
        for first, count in [(-1, 2), (0, 13), (11, 2), (3, -1)]:
            with pytest.raises(E) as ei:
                b.read_probes(first, count)
            assert ei.value.code == -1, (first, count)
        assert np.array_equal(b.read_probes(), again) and b.read_dft_window().shape == (B, 3, 6, 7)
        b.run(2, amps[:, :2])                               # still usable
        # removal: reading a removed monitor is E_STATE
        b.set_dft_window(None, None).set_probes(None, 0)
        for read in (b.read_dft_window, b.read_probes):
            with pytest.raises(E) as ei:
                read()
            assert ei.value.code == -4
        launches = b.launches
        b.run(3, amps[:, :3])
        assert b.launches - launches == (1 if b.resident else 6)


# ---- 8. scale --------------------------------------------------------------------------------------------------

def test_many_resident_members(fd):
    """2048 members: every workgroup walks several members, so the LDS hand-over between them is exercised."""
    B, R, Cc, dtype = 2048, 60, 60, np.float32
    rng = np.random.default_rng(21)
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(dtype)
    mu = np.full((B, R, Cc), fd.MU0).astype(dtype)
    rects = np.array([[R // 2 + (m % 5) - 2, 3, 1, Cc - 6] for m in range(B)])
    amps = rng.standard_normal((B, 30))
    om = OMEGAS[None, :] * (1 + 0.001 * np.arange(B))[:, None]
    cells = _probe_cells(R, Cc, rects)
    window = _window("12x20", R)

    def run(idx):
        with _make(fd, "mur", len(idx), R, Cc, dtype, eps[idx], mu[idx], rects[idx]) as b:
            b.set_dft_window(window, om[idx], 1).set_probes(cells[idx], 30)
            assert _expect_path(b, 10, 240)
            b.run(30, amps[idx])
            return b.read_dft_window(), b.read_probes()

    dft, probes = run(np.arange(B))
    sample = np.array([0, 1, 511, 1024, 1500, 2047])
    d2, p2 = run(sample)
    assert np.array_equal(dft[sample], d2) and np.array_equal(probes[sample], p2)


# ---- 9. fused build --------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, ROOT)
import fdtd2d_amd as fd
assert fd.ARITHMETIC == "fused"
DT, DX = 5e-14, 1e-4
rng = np.random.default_rng(4)
out = {}
for where, (R, Cc) in (("resident", (60, 60)), ("streamed", (100, 120))):
    B, n = 4, 30
    eps = (fd.EPS0 * np.where(rng.random((B, R, Cc)) < 0.3, 4.0, 1.0)).astype(np.float32)
    mu = np.full((B, R, Cc), fd.MU0).astype(np.float32)
    rects = np.array([[R // 2, 3, 1, Cc - 6]] * B)
    amps = rng.standard_normal((B, n))
    om = 2 * np.pi * np.linspace(10e9, 100e9, 10)
    cells = np.array([[R // 2 + 7, Cc // 2], [0, 0], [R // 2, 9], [3, 4]])
    window = (9, 30, 30, 1)
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=np.float32) as b:
        b.set_materials(eps, mu).set_sources(rects)
        b.set_dft_window(window, om, 1).set_probes(cells, n)
        res = b.resident
        trace = []
        for k in range(n):
            b.run(1, amps[:, k:k + 1])
            trace.append(b.download()[0].astype(np.float64))
        trace = np.array(trace)
        probes, dft = b.read_probes(), b.read_dft_window()
    ok_p = all(np.array_equal(probes[:, p], trace[:, :, r, c].T) for p, (r, c) in enumerate(cells))
    want = np.zeros(dft.shape, complex)
    for k in range(n):
        t = (k + 1) * DT
        e = trace[k][:, 9:39, 30:31]
        for f, w in enumerate(om):
            want[:, f] += e * np.cos(w * t) + 1j * (e * -np.sin(w * t))
    err = float(np.abs(dft - want).max() / np.abs(want).max())
    out[where] = dict(resident=bool(res), probes=bool(ok_p), dft=err)
print("FUSED_MON " + json.dumps(out))
"""


def test_fused_build_monitors_are_self_consistent():
    env = dict(os.environ, FDTD2D_ARITHMETIC="fused")
    p = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("FUSED_MON ")][-1]
    out = json.loads(line.split(" ", 1)[1])
    assert out["resident"]["resident"] is True and out["streamed"]["resident"] is False, out
    for where in ("resident", "streamed"):
        assert out[where]["probes"] and out[where]["dft"] <= 1e-12, out
