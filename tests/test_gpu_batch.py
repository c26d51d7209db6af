"""GPU: the batched engine (BatchEngine / fdtd2d_batch_*).  Every member is value-identical to the oracle and to a
single Engine run on it, on both paths (one resident launch per run for members that fit in LDS, one launch per
half-step otherwise), in both dtypes; every case asserts the path it took."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX = 5e-14, 1e-4
DTYPES = [("f32", np.float32), ("f64", np.float64)]


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


@pytest.fixture(scope="module")
def onp():
    from oracle import fdtd_numpy
    return fdtd_numpy


def _max_cells(fd, dtype, arrays=True):
    """What the library reports as the largest resident member (materials as arrays or uniform)."""
    with fd.BatchEngine(1, 11, 11, DT, DX, dtype=dtype) as b:
        if arrays:
            b.set_materials(np.full((1, 11, 11), fd.EPS0), np.full((1, 11, 11), fd.MU0))
        else:
            b.set_materials()
        return b.resident_max_cells


def _shape_of(cells, at_least):
    """A rows x cols shape (both >= 11) with rows * cols == cells, or the next larger product if none exists."""
    n = cells
    while True:
        for r in range(int(np.sqrt(n)), 10, -1):
            if n % r == 0 and n // r >= 11:
                return r, n // r
        if not at_least:
            raise ValueError(cells)
        n += 1


def _expect_path(fd, b, never=False):
    """The capacity rule, restated: resident iff rows * cols <= the reported maximum (and not switched off)."""
    assert b.resident == (not never and b.rows * b.cols <= b.resident_max_cells)
    return b.resident


def _oracle(onp, state, eps, mu, nsteps, rect, amps, on_step=None):
    """One member through the NumPy oracle (in place on copies); rect = (row, col, nrows, ncols)."""
    Ez, Hx, Hy = (a.copy() for a in state)
    r, c, nr, nc = (int(v) for v in rect)
    if nr == 0:
        r, c, nr, nc, amps = 0, 0, 1, 1, np.zeros(nsteps)
    onp.leapfrog(Ez, Hx, Hy, eps, mu, DT, DX, nsteps, r, c, amps=amps, extent=(nr, nc), on_step=on_step)
    return Ez, Hx, Hy


def _assert_fields_equal(got, want, what=""):
    for a, b, k in zip(got, want, ("Ez", "Hx", "Hy")):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: {k} differs"


# ---- 1. goldens ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,dtype", DTYPES)
@pytest.mark.parametrize("name", ["g2_vacuum_64x64", "g3_disk_64x80", "g7_vacuum_96x96_2000", "g4_config1_256x256"])
def test_batch_goldens(fd, onp, golden_dir, name, tag, dtype):
    """Member 0 carries the golden's own source and amplitudes and equals the fixture at every stored snapshot; the
    other members (other eps, a corner source, other amplitudes) equal the oracle run on each of them."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    R, Cc = int(g["rows"]), int(g["cols"])
    sr, sc = (int(v) for v in g["src"])
    snaps = [int(s) for s in g["snaps"]]
    n = snaps[-1]
    B = 4
    rng = np.random.default_rng(R * 7 + Cc + len(tag))
    eps0 = g["eps"] if "eps" in g.files else np.full((R, Cc), float(g["eps_uniform"]))
    eps = np.stack([eps0] + [fd.EPS0 * rng.uniform(1, 6, (R, Cc)) for _ in range(B - 1)]).astype(dtype)
    mu = np.full((B, R, Cc), onp.MU0).astype(dtype)
    rects = np.array([[sr, sc, 1, 1], [0, 0, 1, 1], [R // 3, Cc // 4, 1, 1], [R - 7, Cc - 9, 1, 1]])
    amps = np.stack([g["amps"][:n]] + [rng.standard_normal(n) for _ in range(B - 1)])
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype) as b:
        b.set_materials(eps, mu).set_sources(rects)
        path = _expect_path(fd, b)
        done = 0
        for s in snaps:
            b.run(s - done, amps[:, done:s])
            done = s
            if f"Ez_{tag}_{s}" not in g.files:
                continue
            got = b.download()
            _assert_fields_equal([a[0] for a in got], [g[f"{k}_{tag}_{s}"] for k in ("Ez", "Hx", "Hy")],
                                 f"{name} member 0 step {s} ({'resident' if path else 'streamed'})")
        got = b.download()
        assert b.step_count == n
    for m in range(1, B):
        want = _oracle(onp, onp.grid_zeros(R, Cc, dtype), eps[m], mu[m], n, rects[m], amps[m])
        _assert_fields_equal([a[m] for a in got], want, f"{name} member {m}")


def test_batch_goldens_cover_both_paths(fd):
    """The golden shapes above take the resident path (g2 both dtypes, g3 float32) and the streamed one (g7, g4)."""
    for dtype, shapes in ((np.float32, [(64, 64), (64, 80)]), (np.float64, [(64, 64)])):
        assert all(r * c <= _max_cells(fd, dtype) for r, c in shapes)
    for dtype in (np.float32, np.float64):
        assert 96 * 96 > _max_cells(fd, dtype) and 256 * 256 > _max_cells(fd, dtype)


def test_resident_capacity_meets_the_minimum_sizes(fd):
    assert _max_cells(fd, np.float32, arrays=True) >= 80 * 80
    assert _max_cells(fd, np.float32, arrays=False) >= 96 * 96
    assert _max_cells(fd, np.float64, arrays=True) >= 60 * 60
    assert _max_cells(fd, np.float64, arrays=False) >= 64 * 64


# ---- 2. ragged random states -----------------------------------------------------------------------------------

def _random_members(fd, rng, B, R, Cc, dtype):
    state = (rng.standard_normal((B, R, Cc)).astype(dtype),
             (rng.standard_normal((B, R, Cc - 1)) * 1e-3).astype(dtype),
             (rng.standard_normal((B, R - 1, Cc)) * 1e-3).astype(dtype))
    eps = (fd.EPS0 * rng.uniform(1, 8, (B, R, Cc))).astype(dtype)
    mu = (fd.MU0 * rng.uniform(1, 2, (B, R, Cc))).astype(dtype)
    # a line, a patch, a one-cell source at a corner, and a member without a source
    rects = np.array([[R // 2, 1, 1, Cc - 2], [1, Cc - 4, 3, 2], [R - 1, Cc - 1, 1, 1], [0, 0, 0, 0]])[:B]
    return state, eps, mu, rects


def _run_batch(fd, B, R, Cc, dtype, state, eps, mu, rects, amps, splits, resident=None, spl=None):
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype) as b:
        b.set_materials(eps, mu).set_sources(rects).upload(*state)
        b.set_option(resident=resident, steps_per_launch=spl)
        path = _expect_path(fd, b, never=resident == 0)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, amps[:, done:done + k])
            done += k
        if path:       # one launch per run, or per steps_per_launch chunk of it
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * done
        assert b.step_count == done
        return b.download(), path


@pytest.mark.parametrize("tag,dtype", DTYPES)
@pytest.mark.parametrize("shape", ["11x11", "12x13", "13x70", "60x60", "61x97", "max", "max+1"])
def test_batch_ragged_random_states(fd, onp, tag, dtype, shape):
    if shape.startswith("max"):
        R, Cc = _shape_of(_max_cells(fd, dtype) + (1 if shape == "max+1" else 0), at_least=shape == "max+1")
    else:
        R, Cc = (int(v) for v in shape.split("x"))
    B, splits = 4, (1, 7, 37)
    n = sum(splits)
    rng = np.random.default_rng(R * 1000 + Cc + len(tag))
    state, eps, mu, rects = _random_members(fd, rng, B, R, Cc, dtype)
    amps = rng.standard_normal((B, n))
    got, path = _run_batch(fd, B, R, Cc, dtype, state, eps, mu, rects, amps, splits)
    if shape == "max":
        assert path
    if shape == "max+1":
        assert not path
    for m in range(B):
        want = _oracle(onp, [a[m] for a in state], eps[m], mu[m], n, rects[m], amps[m])
        _assert_fields_equal([a[m] for a in got], want, f"{shape} member {m} vs oracle")
        with fd.Engine(R, Cc, DT, DX, dtype=dtype) as eng:
            eng.set_materials(eps[m], mu[m]).upload(*(a[m] for a in state))
            r, c, nr, nc = (int(v) for v in rects[m])
            if nr:
                eng.set_source_extent(nr, nc)
            done = 0
            for k in splits:
                eng.run(k, r, c, amps[m, done:done + k] if nr else None)
                done += k
            _assert_fields_equal([a[m] for a in got], eng.download(), f"{shape} member {m} vs Engine")
    # the path and the launch length never change a bit
    for resident, spl in ((0, None), (None, 1), (None, 5)):
        other, _ = _run_batch(fd, B, R, Cc, dtype, state, eps, mu, rects, amps, splits, resident, spl)
        _assert_fields_equal(other, got, f"{shape} resident={resident} steps_per_launch={spl}")


# ---- 3. independence -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,Cc", [(60, 60), (100, 100)])
def test_batch_members_are_independent(fd, R, Cc):
    """Changing only member k's inputs leaves every other member's outputs bit-identical (member offsets, borders)."""
    B, k, n = 5, 2, 40
    rng = np.random.default_rng(R)
    state, eps, mu, _ = _random_members(fd, rng, B, R, Cc, np.float32)
    rects = np.array([[5 + m, 7 + 3 * m, 2, 3] for m in range(B)])
    amps = rng.standard_normal((B, n))

    def run(state, eps, rects, amps):
        with fd.BatchEngine(B, R, Cc, DT, DX, dtype=np.float32) as b:
            b.set_materials(eps, mu).set_sources(rects).upload(*state)
            _expect_path(fd, b)
            b.run(n, amps)
            return b.download(), b.resident

    base, path = run(state, eps, rects, amps)
    assert path == (R * Cc <= _max_cells(fd, np.float32))
    state2 = [a.copy() for a in state]
    for a in state2:
        a[k] = rng.standard_normal(a[k].shape).astype(np.float32) * a[k].std()
    eps2, rects2, amps2 = eps.copy(), rects.copy(), amps.copy()
    eps2[k] = (fd.EPS0 * rng.uniform(1, 3, (R, Cc))).astype(np.float32)
    rects2[k] = [0, 0, R, 1]
    amps2[k] = rng.standard_normal(n) * 100
    changed, _ = run(state2, eps2, rects2, amps2)
    for m in range(B):
        same = all(np.array_equal(a[m], b[m]) for a, b in zip(changed, base))
        assert same == (m != k), f"member {m}"


# ---- 4. Courant ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,Cc", [(60, 60), (100, 100)])
def test_batch_courant_refuses_to_run(fd, R, Cc):
    B = 3
    eps = np.full((B, R, Cc), fd.EPS0)
    eps[1] = fd.EPS0 / 100                       # Courant 1.5 at dt = 5e-14, dx = 1e-4
    rng = np.random.default_rng(1)
    Ez = rng.standard_normal((B, R, Cc)).astype(np.float32)
    with fd.BatchEngine(B, R, Cc, DT, DX) as b:
        b.set_materials(eps, fd.MU0).set_sources(np.full((B, 2), 5)).upload(Ez)
        c = b.courant()
        assert c.shape == (B,) and c[1] > 1 and c[0] <= 1 and c[2] <= 1
        assert c[1] == pytest.approx(fd.courant_number(eps[1].astype(np.float32), fd.MU0, DT, DX), rel=1e-6)
        before, launches = b.download(), b.launches
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.run(10, np.ones((B, 10)))
        assert ei.value.code == -5
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.run_waveform(10, "ricker", 30e9)
        assert ei.value.code == -5
        assert b.step_count == 0 and b.launches == launches
        _assert_fields_equal(b.download(), before, "after a refused run")
    with pytest.raises(AssertionError):
        fd.run_fdtd_batch(eps, nsteps=10, sources=np.full((B, 2), 5))


# ---- 5. waveforms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,dtype", DTYPES)
@pytest.mark.parametrize("kind", ["ricker", "sinusoidal"])
@pytest.mark.parametrize("R,Cc", [(40, 50), (100, 90)])
def test_batch_run_waveform(fd, tag, dtype, kind, R, Cc):
    """run_waveform(per-member fc, step0 != 0) equals run() fed the library's waveform (the one Engine.run_waveform
    uses) bit for bit, and run() fed ricker_amplitude / sinusoidal_amplitude to the last bit of the amplitudes (libm's
    exp / sin and NumPy's differ there)."""
    from fdtd2d_amd import _abi
    lib = _abi.load()
    B, n, step0 = 3, 60, 1234
    fc = np.array([20e9, 30e9, 45e9])
    rects = np.array([[R // 2, 3, 1, Cc - 6], [4, 4, 1, 1], [R - 6, Cc - 6, 2, 2]])
    code = {"ricker": _abi.SRC_RICKER, "sinusoidal": _abi.SRC_SINUSOIDAL}[kind]
    f = {"ricker": fd.ricker_amplitude, "sinusoidal": fd.sinusoidal_amplitude}[kind]
    lib_amps = np.array([[lib.fdtd2d_source_amplitude(code, (step0 + i) * DT, v) for i in range(n)] for v in fc])
    py_amps = np.array([[f((step0 + i) * DT, v) for i in range(n)] for v in fc])
    assert np.allclose(lib_amps, py_amps, rtol=1e-12, atol=1e-300)
    out = []
    for mode in ("waveform", "lib", "py"):
        with fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype) as b:
            b.set_materials(np.full((B, R, Cc), fd.EPS0), fd.MU0).set_sources(rects)
            _expect_path(fd, b)
            if mode == "waveform":
                b.run_waveform(n, kind, fc, step0)
            else:
                b.run(n, lib_amps if mode == "lib" else py_amps)
            out.append(b.download())
    _assert_fields_equal(out[0], out[1], "run_waveform vs run(library amplitudes)")
    for a, b in zip(out[0], out[2]):
        scale = np.abs(b).max()
        assert np.abs(a.astype(np.float64) - b).max() <= (1e-5 if dtype == np.float32 else 1e-12) * scale


# ---- 6. DFT, dataset-style -------------------------------------------------------------------------------------

@pytest.mark.parametrize("every", [1, 5, 16])
@pytest.mark.parametrize("resident", [None, 0])
def test_batch_dft_dataset_style(fd, onp, every, resident):
    """generate_data's mapping (random binary eps, line source, sinusoid at a per-member frequency) -> field at
    omega = 2 pi fc: fields value-identical to the oracle, the transform within 1e-12 of the float64 sum over the
    oracle's Ez sequence."""
    B, R, Cc, n = 8, 60, 60, 320
    rng = np.random.default_rng(every)
    eps = np.where(rng.random((B, R, Cc)) < 0.5, onp.EPS0, 5 * onp.EPS0).astype(np.float32)
    mu = np.full((B, R, Cc), onp.MU0, np.float32)
    fc = rng.uniform(20e9, 60e9, B)
    omega = 2 * np.pi * fc
    rows = rng.integers(8, 52, B)
    rects = np.stack([rows, np.full(B, 6), np.ones(B, int), np.full(B, 48)], axis=1)
    amps = np.array([[onp.sinusoidal_amplitude(i * DT, v) for i in range(n)] for v in fc])
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=np.float32) as b:
        b.set_materials(eps, mu).set_sources(rects).set_option(resident=resident)
        assert _expect_path(fd, b, never=resident == 0) == (resident is None)
        b.set_dft(omega, every)
        b.run(100, amps[:, :100])
        b.run(n - 100, amps[:, 100:])
        got = b.download()
        dft = b.read_dft()
        b.set_dft(None)
        with pytest.raises(fd.Fdtd2dError):
            b.read_dft()
    assert dft.shape == (B, R, Cc) and dft.dtype == np.complex128
    for m in range(B):
        want = np.zeros((R, Cc), np.complex128)

        def on_step(i, E, *_):
            k = i + 1
            if k % every == 0:
                e = E.astype(np.float64)
                want[...] += e * np.cos(omega[m] * (k * DT)) + 1j * (e * -np.sin(omega[m] * (k * DT)))
        ref = _oracle(onp, onp.grid_zeros(R, Cc, np.float32), eps[m], mu[m], n, rects[m], amps[m], on_step)
        _assert_fields_equal([a[m] for a in got], ref, f"member {m}")
        assert np.abs(want).max() > 0
        assert np.abs(dft[m] - want).max() <= 1e-12 * np.abs(want).max()


def test_run_fdtd_batch_returns_the_transform(fd, onp):
    B, R, Cc, n = 3, 40, 44, 150
    rng = np.random.default_rng(5)
    eps = np.where(rng.random((B, R, Cc)) < 0.5, onp.EPS0, 5 * onp.EPS0)
    fc = np.array([25e9, 35e9, 50e9])
    rects = np.array([[20, 4, 1, 36], [10, 10, 2, 2], [3, 3, 1, 1]])
    Ez, Hx, Hy, dft = fd.run_fdtd_batch(eps, nsteps=n, sources=rects, fc=fc, waveform="sinusoidal", dt=DT, dx=DX,
                                        omega=2 * np.pi * fc, dft_every=4)
    assert Ez.dtype == np.float64 and dft.shape == (B, R, Cc)
    for m in range(B):
        with fd.BatchEngine(1, R, Cc, DT, DX, dtype=np.float64) as b:
            b.set_materials(eps[m:m + 1], onp.MU0).set_sources(rects[m:m + 1]).set_dft(2 * np.pi * fc[m], 4)
            b.run(n, np.array([[fd.sinusoidal_amplitude(i * DT, fc[m]) for i in range(n)]]))
            one = b.download()
            _assert_fields_equal([a[m] for a in (Ez, Hx, Hy)], [a[0] for a in one], f"member {m}")
            assert np.array_equal(dft[m], b.read_dft()[0])
        with fd.Engine(R, Cc, DT, DX, dtype=np.float64) as eng:
            eng.set_materials(eps[m], np.full((R, Cc), onp.MU0)).set_source_extent(*rects[m][2:])
            eng.run(n, rects[m][0], rects[m][1], [fd.sinusoidal_amplitude(i * DT, fc[m]) for i in range(n)])
            _assert_fields_equal([a[m] for a in (Ez, Hx, Hy)], eng.download(), f"member {m} vs Engine")


# ---- 7. scale --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [2048, 1])
def test_batch_scale(fd, onp, B):
    """2048 members of 60 x 60 (more than one round of resident workgroups) and a batch of one."""
    from oracle import c_oracle
    R, Cc, n = 60, 60, 300
    rng = np.random.default_rng(B)
    eps = (fd.EPS0 * rng.uniform(1, 4, (B, R, Cc))).astype(np.float32)
    mu = np.full((B, R, Cc), fd.MU0, np.float32)
    rows, cols = rng.integers(0, R, B), rng.integers(0, Cc, B)
    amps = rng.standard_normal((B, n))
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=np.float32) as b:
        b.set_materials(eps, mu).set_sources(np.stack([rows, cols], axis=1))
        assert _expect_path(fd, b)
        b.run(n, amps)
        assert b.launches == 1
        got = b.download()
    for m in sorted({0, 1, 1023, 2047} & set(range(B))):
        want = c_oracle.run(*onp.grid_zeros(R, Cc, np.float32), eps[m], mu[m], DT, DX, n, int(rows[m]),
                            int(cols[m]), amps=amps[m])
        _assert_fields_equal([a[m] for a in got], want, f"member {m}")


# ---- 8. the fused build ----------------------------------------------------------------------------------------

CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, ROOT)
import fdtd2d_amd as fd
from fdtd2d_amd import _abi
assert fd.ARITHMETIC == "fused" and _abi.LIB_PATH.endswith("libfdtd2d_fused.so")
DT, DX = 5e-14, 1e-4
rel = lambda a, ref: float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())
G = os.path.join(ROOT, "tests", "golden")
out = {}
for name, n, uniform in (("g4_config1_256x256", 500, False), ("g7_vacuum_96x96_2000", 2000, True)):
    g = np.load(os.path.join(G, name + ".npz"))
    R, C = int(g["rows"]), int(g["cols"])
    B = 3
    with fd.BatchEngine(B, R, C, DT, DX, dtype=np.float32) as b:
        if uniform:
            b.set_materials()
        else:
            b.set_materials(np.full((B, R, C), float(g["eps_uniform"])), np.full((B, R, C), fd.MU0))
        b.set_sources(np.tile(g["src"], (B, 1)))
        out[name + "_resident"] = b.resident
        b.run(n, np.tile(g["amps"][:n], (B, 1)))
        got = b.download()
    out[name] = max(rel(a[m], g[f"{k}_f64_{n}"]) for a, k in zip(got, ("Ez", "Hx", "Hy")) for m in range(B))
print("FUSED_BATCH " + json.dumps(out))
'''


def test_fused_build_batch_within_the_stated_tolerances():
    env = dict(os.environ, FDTD2D_ARITHMETIC="fused")
    p = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("FUSED_BATCH ")][-1]
    out = json.loads(line.split(" ", 1)[1])
    assert out["g4_config1_256x256_resident"] is False and out["g7_vacuum_96x96_2000_resident"] is True, out
    assert out["g4_config1_256x256"] <= 5e-6, out
    assert out["g7_vacuum_96x96_2000"] <= 1e-4, out
