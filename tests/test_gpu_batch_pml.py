"""GPU: the split-field PML of the batched engine (BatchEngine(boundary="pml"), fdtd2d_batch_set_pml).  Every member is
value-identical to oracle/pml_numpy run with its own factor arrays and to an Engine(boundary="pml") given the same
factors, on both paths (one resident launch per run for members that fit in LDS, one launch per half-step
otherwise), in both dtypes; every case asserts the path it took."""
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
LDS_LIMIT = 163840


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


@pytest.fixture(scope="module")
def pm():
    from oracle import pml_numpy
    return pml_numpy


def _lds_rule(R, Cc, dtype, arrays):
    """The capacity rule, restated: arrays x seg(R*C) + seg(4R) + seg(4C) bytes, seg = rounded up to 16 bytes."""
    esz = np.dtype(dtype).itemsize
    seg = lambda n: -(-n * esz // 16) * 16
    return (6 if arrays else 4) * seg(R * Cc) + seg(4 * R) + seg(4 * Cc)


def _expect_path(b, arrays, never=False):
    need = _lds_rule(b.rows, b.cols, b.dtype, arrays)
    assert b.lds_bytes == need
    assert b.resident == (not never and need <= LDS_LIMIT)
    assert b.resident == (not never and b.rows * b.cols <= b.resident_max_cells)
    return b.resident


def _layer(R, Cc, L):
    i, j = np.mgrid[0:R, 0:Cc]
    return (i < L) | (i > R - 1 - L) | (j < L) | (j > Cc - 1 - L)


def _oracle(pm, state, eps, mu, nsteps, rect, amps, P, on_step=None):
    """One member through pml_numpy.step (in place on copies), then the rectangle source on the total field as
    (T)((double)Ez + amp); state = (Ez, Ezx, Hx, Hy)."""
    Ez, Ezx, Hx, Hy = (a.copy() for a in state)
    r, c, nr, nc = (int(v) for v in rect)
    for n in range(nsteps):
        pm.step(Ez, Ezx, Hx, Hy, eps, mu, DT, DX, P)
        if nr:
            Ez[r:r + nr, c:c + nc] = (Ez[r:r + nr, c:c + nc].astype(np.float64) + amps[n]).astype(Ez.dtype)
        if on_step is not None:
            on_step(n, Ez)
    return Ez, Ezx, Hx, Hy


def _assert_equal(got, want, what=""):
    for a, b, k in zip(got, want, ("Ez", "Ezx", "Hx", "Hy")):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: {k} differs"


def _random_members(fd, rng, B, R, Cc, L, dtype, arrays=True):
    Ez = rng.standard_normal((B, R, Cc)).astype(dtype)
    Ezx = (0.3 * rng.standard_normal((B, R, Cc)) * _layer(R, Cc, L)).astype(dtype)   # non-zero in the layer only
    Hx = (rng.standard_normal((B, R, Cc - 1)) * 1e-3).astype(dtype)
    Hy = (rng.standard_normal((B, R - 1, Cc)) * 1e-3).astype(dtype)
    if arrays:
        eps = (fd.EPS0 * rng.uniform(1, 8, (B, R, Cc))).astype(dtype)
        mu = (fd.MU0 * rng.uniform(1, 2, (B, R, Cc))).astype(dtype)
    else:
        eps = np.full((B, R, Cc), fd.EPS0).astype(dtype)
        mu = np.full((B, R, Cc), fd.MU0).astype(dtype)
    # a line, a patch, a one-cell source at a corner, and a member without a source
    rects = np.array([[R // 2, 1, 1, Cc - 2], [1, Cc - 4, 3, 2], [R - 1, Cc - 1, 1, 1], [0, 0, 0, 0]])[:B]
    courant00 = np.array([0.15, 0.48, 0.3, 0.07])[:B]
    return (Ez, Ezx, Hx, Hy), eps, mu, rects, courant00


def _make(fd, B, R, Cc, dtype, eps, mu, arrays, rects, L, courant00, state=None):
    b = fd.BatchEngine(B, R, Cc, DT, DX, dtype=dtype, boundary="pml")
    if arrays:
        b.set_materials(eps, mu)
    else:
        b.set_materials()
    b.set_sources(rects).set_pml(L, courant00=courant00)
    if state is not None:
        b.upload(state[0], state[2], state[3]).upload_ezx(state[1])
    return b


def _download(b):
    Ez, Hx, Hy = b.download()
    return Ez, b.download_ezx(), Hx, Hy


def _run(fd, B, R, Cc, dtype, state, eps, mu, arrays, rects, L, courant00, amps, splits, resident=None, spl=None):
    with _make(fd, B, R, Cc, dtype, eps, mu, arrays, rects, L, courant00, state) as b:
        b.set_option(resident=resident, steps_per_launch=spl)
        path = _expect_path(b, arrays, never=resident == 0)
        done, launches = 0, b.launches
        for k in splits:
            b.run(k, amps[:, done:done + k])
            done += k
        if path:
            assert b.launches - launches == sum(-(-k // spl) if spl else 1 for k in splits)
        else:
            assert b.launches - launches == 2 * done
        assert b.step_count == done
        return _download(b), path


# ---- 1. oracle parity from random states ---------------------------------------------------------------------

@pytest.mark.parametrize("tag,dtype", DTYPES)
@pytest.mark.parametrize("materials", ["arrays", "uniform"])
@pytest.mark.parametrize("L", [4, 10])
@pytest.mark.parametrize("shape", ["37x53", "60x60", "64x64", "80x80", "96x130"])
def test_batch_pml_random_states_match_the_oracle(fd, pm, tag, dtype, materials, L, shape):
    R, Cc = (int(v) for v in shape.split("x"))
    arrays = materials == "arrays"
    B, splits = 4, (1, 7, 23)
    n = sum(splits)
    rng = np.random.default_rng(R * 1000 + Cc + 10 * L + len(tag) + arrays)
    state, eps, mu, rects, c00 = _random_members(fd, rng, B, R, Cc, L, dtype, arrays)
    amps = rng.standard_normal((B, n))
    got, path = _run(fd, B, R, Cc, dtype, state, eps, mu, arrays, rects, L, c00, amps, splits)
    streamed, spath = _run(fd, B, R, Cc, dtype, state, eps, mu, arrays, rects, L, c00, amps, splits, resident=0)
    assert not spath
    for m in range(B):
        P = pm.profiles(R, Cc, c00[m], L=L, dtype=dtype)
        want = _oracle(pm, [a[m] for a in state], eps[m], mu[m], n, rects[m], amps[m], P)
        _assert_equal([a[m] for a in got], want, f"{shape} member {m} ({'resident' if path else 'streamed'})")
        _assert_equal([a[m] for a in streamed], want, f"{shape} member {m} (forced streamed)")


def test_batch_pml_capacity_rule(fd):
    """The shapes the rule admits (and the one it does not), as the library reports them."""
    cases = [(np.float32, True, 60, 60, True), (np.float32, True, 64, 64, True), (np.float32, True, 80, 80, True),
             (np.float64, True, 56, 56, True), (np.float64, False, 64, 64, True), (np.float64, True, 60, 60, False)]
    for dtype, arrays, R, Cc, resident in cases:
        with fd.BatchEngine(2, R, Cc, DT, DX, dtype=dtype, boundary="pml") as b:
            if arrays:
                b.set_materials(np.full((2, R, Cc), fd.EPS0), np.full((2, R, Cc), fd.MU0))
            else:
                b.set_materials()
            plain = (b.resident, b.lds_bytes)
            b.set_pml(10)
            assert _expect_path(b, arrays) == resident, (dtype, arrays, R, Cc)
            b.clear_pml()
            assert (b.resident, b.lds_bytes) == plain        # nothing changes without a layer
    with fd.BatchEngine(1, 60, 60, DT, DX, dtype=np.float32, boundary="pml") as b:
        b.set_materials(np.full((1, 60, 60), fd.EPS0), np.full((1, 60, 60), fd.MU0)).set_pml(10)
        assert b.lds_bytes == 88320


# ---- 2. the same result as Engine --------------------------------------------------------------------------

@pytest.mark.parametrize("tag,dtype", DTYPES)
@pytest.mark.parametrize("R,Cc,L", [(64, 64, 10), (96, 130, 20)])
def test_batch_pml_member_equals_engine(fd, pm, tag, dtype, R, Cc, L):
    B, n = 3, 45
    rng = np.random.default_rng(R + L + len(tag))
    state, eps, mu, rects, c00 = _random_members(fd, rng, B, R, Cc, L, dtype)
    amps = rng.standard_normal((B, n))
    got, path = _run(fd, B, R, Cc, dtype, state, eps, mu, True, rects, L, c00, amps, (n,))
    for m in range(B):
        P = pm.profiles(R, Cc, c00[m], L=L, dtype=dtype)
        with fd.Engine(R, Cc, DT, DX, dtype=dtype, boundary="pml") as eng:
            eng.set_materials(eps[m], mu[m]).set_pml(L, profiles=P)
            eng.upload(state[0][m], state[2][m], state[3][m]).upload_ezx(state[1][m])
            r, c, nr, nc = (int(v) for v in rects[m])
            if nr:
                eng.set_source_extent(nr, nc)
            eng.run(n, r, c, amps[m] if nr else None)
            Ez, Hx, Hy = eng.download()
            want = (Ez, eng.download_ezx(), Hx, Hy)
        _assert_equal([a[m] for a in got], want, f"member {m} vs Engine ({'resident' if path else 'streamed'})")


# ---- 3. path invariance ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,dtype", DTYPES)
def test_batch_pml_path_and_launch_length_never_change_a_bit(fd, tag, dtype):
    B, R, Cc, L, splits = 4, 56, 56, 10, (5, 30)
    n = sum(splits)
    rng = np.random.default_rng(7 + len(tag))
    state, eps, mu, rects, c00 = _random_members(fd, rng, B, R, Cc, L, dtype)
    amps = rng.standard_normal((B, n))
    base, path = _run(fd, B, R, Cc, dtype, state, eps, mu, True, rects, L, c00, amps, splits)
    assert path
    with _make(fd, B, R, Cc, dtype, eps, mu, True, rects, L, c00, state) as b:
        l0 = b.launches
        b.run(n, amps)
        assert b.launches - l0 == 1                       # a resident run(n) is one launch
        _assert_equal(_download(b), base, "one run")
    for resident, spl in ((0, None), (None, 1), (None, 7), (None, 0)):
        other, _ = _run(fd, B, R, Cc, dtype, state, eps, mu, True, rects, L, c00, amps, splits, resident, spl)
        _assert_equal(other, base, f"resident={resident} steps_per_launch={spl}")


# ---- 4. layer behaviour ------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,Cc", [(60, 60), (96, 130)])
def test_batch_pml_layer_behaviour(fd, R, Cc):
    B, L, n = 3, 10, 120
    rng = np.random.default_rng(R)
    eps = (fd.EPS0 * rng.uniform(1, 4, (B, R, Cc))).astype(np.float32)
    mu = np.full((B, R, Cc), fd.MU0, np.float32)
    rects = np.array([[R // 2, Cc // 2, 1, 1], [20, 15, 3, 4], [R // 2, 2, 1, Cc - 4]])
    amps = rng.standard_normal((B, n)) * 10
    layer = _layer(R, Cc, L)
    with _make(fd, B, R, Cc, np.float32, eps, mu, True, rects, L, 0.15) as b:
        _expect_path(b, True)
        assert not b.download_ezx().any()                 # Ezx starts at zero
        b.run(n, amps)
        Ez, Ezx, Hx, Hy = _download(b)
        assert np.abs(Ezx[:, layer]).max() > 0
        assert not Ezx[:, ~layer].any()                   # exactly 0 outside the layer
        assert not Ez[:, 0, :].any() and not Ez[:, -1, :].any() and not Ez[:, :, 0].any() and not Ez[:, :, -1].any()
        b.reset()
        assert b.step_count == 0 and not b.download_ezx().any() and not any(a.any() for a in b.download())
        # removing the layer gives a plain "none" batch, bit for bit
        state = [rng.standard_normal(s).astype(np.float32) for s in ((B, R, Cc), (B, R, Cc - 1), (B, R - 1, Cc))]
        b.clear_pml()
        assert not b.pml
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.download_ezx()
        assert ei.value.code == -4
        b.upload(*state).run(n, amps)
        got = b.download()
    with fd.BatchEngine(B, R, Cc, DT, DX, dtype=np.float32, boundary="none") as nb:
        nb.set_materials(eps, mu).set_sources(rects).upload(*state).run(n, amps)
        want = nb.download()
    for a, w in zip(got, want):
        assert np.array_equal(a, w)


# ---- 5. member independence --------------------------------------------------------------------------------

@pytest.mark.parametrize("R,Cc", [(64, 64), (96, 130)])
def test_batch_pml_members_are_independent(fd, R, Cc):
    B, L, n = 5, 10, 60
    rng = np.random.default_rng(R + 1)
    state, eps, mu, _, _ = _random_members(fd, rng, B, R, Cc, L, np.float32)
    rects = np.array([[5 + m, 7 + 3 * m, 2, 3] for m in range(B)])
    rects[3] = 0
    for a in state:
        a[3] = 0                                           # member 3: all zero, no source
    c00 = np.array([0.15, 0.4, 0.25, 0.15, 0.6])
    amps = rng.standard_normal((B, n))
    with _make(fd, B, R, Cc, np.float32, eps, mu, True, rects, L, c00, state) as b:
        path = _expect_path(b, True)
        b.run(n, amps)
        got = _download(b)
    assert not any(a[3].any() for a in got)
    for m in range(B):
        one = [a[m:m + 1] for a in state]
        with _make(fd, 1, R, Cc, np.float32, eps[m:m + 1], mu[m:m + 1], True, rects[m:m + 1], L, c00[m], one) as b1:
            assert b1.resident == path
            b1.run(n, amps[m:m + 1])
            _assert_equal([a[m] for a in got], [a[0] for a in _download(b1)], f"member {m}")


# ---- 6. dataset-style DFT with the PML ---------------------------------------------------------------------

@pytest.mark.parametrize("every", [1, 16])
@pytest.mark.parametrize("resident", [None, 0])
def test_batch_pml_dft_dataset_style(fd, pm, every, resident):
    """generate_data's mapping (random binary eps, line source, sinusoid at a per-member frequency) with a 10-cell
    layer: fields value-identical to the oracle, the transform within 1e-12 of the float64 sum over its Ez."""
    from oracle import fdtd_numpy as onp
    B, R, Cc, n, L = 8, 60, 60, 320, 10
    rng = np.random.default_rng(every)
    eps = np.where(rng.random((B, R, Cc)) < 0.5, onp.EPS0, 5 * onp.EPS0).astype(np.float32)
    mu = np.full((B, R, Cc), onp.MU0, np.float32)
    fc = rng.uniform(20e9, 60e9, B)
    omega = 2 * np.pi * fc
    rows = rng.integers(8, 52, B)
    rects = np.stack([rows, np.full(B, 6), np.ones(B, int), np.full(B, 48)], axis=1)
    amps = np.array([[onp.sinusoidal_amplitude(i * DT, v) for i in range(n)] for v in fc])
    c00 = np.array([(1 / np.sqrt(float(e) * onp.MU0) * DT) / DX for e in eps[:, 0, 0]])
    with _make(fd, B, R, Cc, np.float32, eps, mu, True, rects, L, c00) as b:
        b.set_option(resident=resident)
        assert _expect_path(b, True, never=resident == 0) == (resident is None)
        b.set_dft(omega, every)
        b.run(100, amps[:, :100])
        b.run(n - 100, amps[:, 100:])
        got = _download(b)
        dft = b.read_dft()
    for m in range(B):
        want = np.zeros((R, Cc), np.complex128)

        def on_step(i, E):
            k = i + 1
            if k % every == 0:
                e = E.astype(np.float64)
                want[...] += e * np.cos(omega[m] * (k * DT)) + 1j * (e * -np.sin(omega[m] * (k * DT)))
        P = pm.profiles(R, Cc, c00[m], L=L, dtype=np.float32)
        zero = [np.zeros((R, Cc), np.float32), np.zeros((R, Cc), np.float32), np.zeros((R, Cc - 1), np.float32),
                np.zeros((R - 1, Cc), np.float32)]
        ref = _oracle(pm, zero, eps[m], mu[m], n, rects[m], amps[m], P, on_step)
        _assert_equal([a[m] for a in got], ref, f"member {m}")
        assert np.abs(want).max() > 0
        assert np.abs(dft[m] - want).max() <= 1e-12 * np.abs(want).max()


def test_run_fdtd_batch_with_the_pml(fd, pm):
    """run_fdtd_batch(boundary="pml") grades each member's layer with its own eps[0,0], mu[0,0]."""
    B, R, Cc, n, L = 3, 40, 44, 150, 8
    rng = np.random.default_rng(5)
    eps = fd.EPS0 * rng.uniform(1, 4, (B, R, Cc))
    rects = np.array([[20, 4, 1, 36], [10, 10, 2, 2], [30, 30, 1, 1]])
    fc = np.array([25e9, 35e9, 50e9])
    Ez, Hx, Hy = fd.run_fdtd_batch(eps, nsteps=n, sources=rects, fc=fc, waveform="sinusoidal", dt=DT, dx=DX,
                                   boundary="pml", pml_cells=L)
    for m in range(B):
        c00 = (1 / np.sqrt(float(eps[m, 0, 0]) * float(fd.MU0)) * DT) / DX
        P = pm.profiles(R, Cc, c00, L=L)
        zero = [np.zeros((R, Cc)), np.zeros((R, Cc)), np.zeros((R, Cc - 1)), np.zeros((R - 1, Cc))]
        amps = np.array([fd.sinusoidal_amplitude(i * DT, fc[m]) for i in range(n)])
        want = _oracle(pm, zero, eps[m], np.full((R, Cc), fd.MU0), n, rects[m], amps, P)
        for a, w, k in zip((Ez[m], Hx[m], Hy[m]), (want[0], want[2], want[3]), ("Ez", "Hx", "Hy")):
            assert np.array_equal(a, w), f"member {m} {k}"


# ---- 7. physics pin ----------------------------------------------------------------------------------------

def test_batch_pml_reflection_against_an_open_domain(fd):
    """A Ricker pulse at 150 GHz (20 cells per wavelength, Courant 0.48) in 64x64 members with a 10-cell layer,
    against the same sources centred in 400x400 members (40-cell layer, nothing returns in 260 steps): the
    reflection max|E - E_open| / max|E_open| at a normal and a ~45 degree probe is <= 1e-3 and >= 100x below the
    Mur frame's at the same probes (the oracle gives 3.1e-5 / 4.8e-5 against 5.4e-2 / 8.3e-2)."""
    dt, dx, fc, n = 1.6e-13, 1e-4, 1.5e11, 260
    S = (1 / np.sqrt(fd.EPS0 * fd.MU0) * dt) / dx
    amps = np.array([[fd.ricker_amplitude(i * dt, fc) for i in range(n)]] * 2)
    probes = {"normal": (32, 52), "oblique": (50, 50)}

    def run(size, boundary, L=None):
        o = (size - 64) // 2
        series = {k: [] for k in probes}
        with fd.BatchEngine(2, size, size, dt, dx, dtype=np.float64, boundary=boundary) as b:
            b.set_materials().set_sources(np.array([[32 + o, 32 + o], [32 + o, 32 + o]]))
            if boundary == "pml":
                b.set_pml(L, courant00=S)
            for i in range(n):
                b.run(1, amps[:, i:i + 1])
                Ez = b.download()[0]
                assert np.array_equal(Ez[0], Ez[1])
                for k, (r, c) in probes.items():
                    series[k].append(Ez[0, r + o, c + o])
            resident = b.resident
        return {k: np.array(v) for k, v in series.items()}, resident

    (open_, r_open), (pml, r_pml), (mur, _) = run(400, "pml", 40), run(64, "pml", 10), run(64, "mur")
    assert not r_open and r_pml
    refl = {k: (np.abs(pml[k] - open_[k]).max() / np.abs(open_[k]).max(),
                np.abs(mur[k] - open_[k]).max() / np.abs(open_[k]).max()) for k in probes}
    assert np.abs(open_["normal"]).max() > 1e-2
    assert refl["normal"][0] <= 1e-3 and refl["oblique"][0] <= 1e-3, refl
    assert refl["normal"][0] * 100 <= refl["normal"][1] and refl["oblique"][0] * 100 <= refl["oblique"][1], refl


# ---- 8. refusals -------------------------------------------------------------------------------------------

def test_batch_pml_refusals_leave_the_fields_untouched(fd):
    import ctypes
    from fdtd2d_amd import _abi
    lib = _abi.load()
    B, R, Cc = 3, 60, 60
    rng = np.random.default_rng(3)
    state = [rng.standard_normal(s).astype(np.float32) for s in ((B, R, Cc), (B, R, Cc - 1), (B, R - 1, Cc))]
    rowf, colf = fd.batch_pml_profiles(B, R, Cc, 0.15, L=10, dtype=np.float32)
    rowd, cold = rowf.astype(np.float64), colf.astype(np.float64)

    def same(b, ezx=None):
        for a, w in zip(b.download(), state):
            assert np.array_equal(a, w)
        if ezx is not None:
            assert np.array_equal(b.download_ezx(), ezx)

    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="mur") as b:
        b.set_materials().upload(*state)
        rc = lib.fdtd2d_batch_set_pml(b._h, rowf.ctypes.data, colf.ctypes.data, _abi.F32, 10)
        assert rc == _abi.E_STATE and lib.fdtd2d_batch_last_error(b._h)
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.set_pml(10)
        assert ei.value.code == _abi.E_STATE
        same(b)
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="pml") as b:
        b.set_materials().set_sources(np.full((B, 2), 30)).upload(*state)
        with pytest.raises(fd.Fdtd2dError) as ei:          # no layer yet
            b.run(3, np.ones((B, 3)))
        assert ei.value.code == _abi.E_STATE
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.run_waveform(3, "ricker", 30e9)
        assert ei.value.code == _abi.E_STATE
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.download_ezx()
        assert ei.value.code == _abi.E_STATE
        for L in (29, 0):                                   # 2L + 3 > 60, L < 1
            with pytest.raises(fd.Fdtd2dError) as ei:
                b.set_pml(L)
            assert ei.value.code == _abi.E_ARG
        assert not b.pml and b.step_count == 0
        same(b)
        b.set_pml(10)
        ezx = (rng.standard_normal((B, R, Cc)) * _layer(R, Cc, 10)).astype(np.float32)
        b.upload_ezx(ezx)
        for args in ((rowd.ctypes.data, cold.ctypes.data, _abi.F64, 10),     # wrong dtype
                     (rowf.ctypes.data, None, _abi.F32, 10),                  # one NULL
                     (None, colf.ctypes.data, _abi.F32, 10),
                     (rowf.ctypes.data, colf.ctypes.data, _abi.F32, 29)):     # does not fit
            assert lib.fdtd2d_batch_set_pml(b._h, *args) == _abi.E_ARG, args
        same(b, ezx)
        assert lib.fdtd2d_batch_transfer_ezx(b._h, ctypes.c_void_p(0), _abi.F32, 0) == _abi.E_ARG
        same(b, ezx)
    # a Courant-unstable member is still refused, with the layer on
    eps = np.full((B, R, Cc), fd.EPS0)
    eps[1] = fd.EPS0 / 100
    with fd.BatchEngine(B, R, Cc, DT, DX, boundary="pml") as b:
        b.set_materials(eps, fd.MU0).set_sources(np.full((B, 2), 30)).set_pml(10).upload(*state)
        launches = b.launches
        with pytest.raises(fd.Fdtd2dError) as ei:
            b.run(10, np.ones((B, 10)))
        assert ei.value.code == _abi.E_COURANT and b.launches == launches and b.step_count == 0
        same(b, np.zeros((B, R, Cc), np.float32))


# ---- 9. the fused build ------------------------------------------------------------------------------------

CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, ROOT)
import fdtd2d_amd as fd
from fdtd2d_amd import _abi
from oracle import pml_numpy as pm
assert fd.ARITHMETIC == "fused" and _abi.LIB_PATH.endswith("libfdtd2d_fused.so")
DT, DX, n, L, B = 5e-14, 1e-4, 500, 10, 2
rel = lambda a, ref: float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())
amps = np.array([fd.ricker_amplitude(i * DT, 30e9) for i in range(n)])
S = (1 / np.sqrt(fd.EPS0 * fd.MU0) * DT) / DX
out = {}
for R, C in ((64, 64), (96, 130)):
    rng = np.random.default_rng(R)
    eps64 = fd.EPS0 * rng.uniform(1, 4, (B, R, C))
    src = np.array([[R // 2, C // 2], [R // 3, C // 4]])
    with fd.BatchEngine(B, R, C, DT, DX, dtype=np.float32, boundary="pml") as b:
        b.set_materials(eps64.astype(np.float32), np.full((B, R, C), fd.MU0, np.float32)).set_sources(src)
        b.set_pml(L, courant00=S)
        out[f"{R}x{C}_resident"] = b.resident
        b.run(n, np.tile(amps, (B, 1)))
        Ez, Hx, Hy = b.download()
        got = (Ez, b.download_ezx(), Hx, Hy)
    for tag, dt in (("f32", np.float32), ("f64", np.float64)):
        worst = 0.0
        for m in range(B):
            st = [np.zeros((R, C), dt), np.zeros((R, C), dt), np.zeros((R, C - 1), dt), np.zeros((R - 1, C), dt)]
            P = pm.profiles(R, C, S, L=L, dtype=dt)
            want = pm.leapfrog(*st, eps64[m].astype(dt), np.full((R, C), fd.MU0, dt), DT, DX, n, int(src[m, 0]),
                               int(src[m, 1]), amps, P)
            worst = max([worst] + [rel(a[m], w) for a, w in zip(got, want) if np.abs(w).max() > 0])
        out[f"{R}x{C}_{tag}"] = worst
print("FUSED_BATCH_PML " + json.dumps(out))
'''


def test_fused_build_batch_pml_within_the_stated_tolerances():
    env = dict(os.environ, FDTD2D_ARITHMETIC="fused")
    p = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("FUSED_BATCH_PML ")][-1]
    out = json.loads(line.split(" ", 1)[1])
    print(out)
    assert out["64x64_resident"] is True and out["96x130_resident"] is False, out
    for shape in ("64x64", "96x130"):
        assert out[f"{shape}_f32"] <= 1e-5, out
        assert out[f"{shape}_f64"] <= 5e-6, out
