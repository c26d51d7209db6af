"""CPU-only checks of the batched engine's split-field PML (fdtd2d_batch_set_pml): the two entry points are declared,
exported and bound, the Python surface keeps its shape, a layer that does not fit is refused before any device is
touched, the per-member factors equal pml_profiles member by member, there is no CPU fallback, and the oracle
figures the GPU physics pin relies on."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_pml_symbols_are_declared_exported_and_bound():
    """include/fdtd2d_batch_pml.h, the library's exports and _abi.BATCH_PML_SIGNATURES agree."""
    from fdtd2d_amd import _abi
    txt = open(os.path.join(ROOT, "include", "fdtd2d_batch_pml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["fdtd2d_batch_set_pml", "fdtd2d_batch_transfer_ezx"]
    assert sorted(_abi.BATCH_PML_SIGNATURES) == names
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared but not exported"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_PML_SIGNATURES[n][1]


def test_batch_pml_python_surface():
    import fdtd2d_amd as fd
    assert list(inspect.signature(fd.BatchEngine).parameters) == ["count", "rows", "cols", "dt", "dx", "dtype",
                                                                  "boundary", "device"]
    assert list(inspect.signature(fd.BatchEngine.set_pml).parameters) == ["self", "L", "m", "R0", "courant00",
                                                                          "profiles"]
    for name in ("clear_pml", "upload_ezx", "download_ezx"):
        assert callable(getattr(fd.BatchEngine, name))
    p = inspect.signature(fd.run_fdtd_batch).parameters["pml_cells"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 40
    assert fd.batch_pml_profiles is fd.batch.batch_pml_profiles and "batch_pml_profiles" in fd.__all__


@pytest.mark.parametrize("R,Cc,L,largest", [(60, 60, 40, 28), (60, 60, 29, 28), (37, 53, 18, 17), (64, 64, 0, 30)])
def test_run_fdtd_batch_refuses_a_layer_that_does_not_fit(monkeypatch, R, Cc, L, largest):
    import fdtd2d_amd as fd

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", no_device)
    eps = np.full((2, R, Cc), fd.EPS0)
    with pytest.raises(ValueError, match=rf"largest that does is {largest}\b"):
        fd.run_fdtd_batch(eps, nsteps=4, sources=np.full((2, 2), 5), boundary="pml", pml_cells=L)
    assert fd.batch.pml_fits(R, Cc, largest) and not fd.batch.pml_fits(R, Cc, largest + 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("courant00", ["scalar", "per-member"])
def test_batch_pml_profiles_equal_pml_profiles_member_by_member(dtype, courant00):
    import fdtd2d_amd as fd
    B, R, Cc, L = 5, 37, 53, 10
    c = 0.48 if courant00 == "scalar" else np.array([0.48, 0.2, 0.48, 0.31, 0.2])
    rowf, colf = fd.batch_pml_profiles(B, R, Cc, c, L=L, m=3, R0=1e-6, dtype=dtype)
    assert rowf.shape == (B, 4 * R) and colf.shape == (B, 4 * Cc)
    assert rowf.dtype == dtype and colf.dtype == dtype
    for b in range(B):
        P = fd.pml_profiles(R, Cc, float(np.broadcast_to(c, (B,))[b]), L, 3, 1e-6, dtype)
        assert np.array_equal(rowf[b], np.concatenate([P[k] for k in ("ahr", "bhr", "aer", "ber")]))
        assert np.array_equal(colf[b], np.concatenate([P[k] for k in ("ahc", "bhc", "aec", "bec")]))
    # the oracle's definition gives the same factors
    from oracle import pml_numpy as pm
    P = pm.profiles(R, Cc, float(np.broadcast_to(c, (B,))[1]), L=L, dtype=dtype)
    assert np.array_equal(rowf[1], np.concatenate([P[k] for k in ("ahr", "bhr", "aer", "ber")]))
    assert np.array_equal(colf[1], np.concatenate([P[k] for k in ("ahc", "bhc", "aec", "bec")]))


def test_batch_pml_without_a_device_has_no_fallback():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 4, 60, 60, 5e-14, 1e-4, _abi.F32, _abi.BOUNDARY_NONE, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    import fdtd2d_amd as fd
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.BatchEngine(4, 60, 60, boundary="pml")
    assert ei.value.code == _abi.E_NODEVICE and "no CPU path" in str(ei.value)
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, 40, 40), fd.EPS0), nsteps=4, sources=np.full((2, 2), 20), boundary="pml",
                          pml_cells=10)
    assert ei.value.code == _abi.E_NODEVICE


def test_batch_pml_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    buf = np.zeros(16, np.float32)
    assert lib.fdtd2d_batch_set_pml(None, buf.ctypes.data, buf.ctypes.data, _abi.F32, 4) == _abi.E_ARG
    assert lib.fdtd2d_batch_transfer_ezx(None, buf.ctypes.data, _abi.F32, 0) == _abi.E_ARG


def test_oracle_reflection_figures_of_the_batch_physics_pin():
    """The set-up of the GPU physics pin (test_gpu_batch_pml.py), through the NumPy oracle: a 64x64 grid with a
    10-cell layer reflects about 3e-5 (normal) / 5e-5 (~45 degrees) against an open domain, more than 1000x less
    than the Mur frame at the same probes."""
    from oracle import fdtd_numpy as onp
    from oracle import pml_numpy as pm
    dt, dx, fc, n = 1.6e-13, 1e-4, 1.5e11, 260
    S = (1 / np.sqrt(onp.EPS0 * onp.MU0) * dt) / dx
    amps = [onp.ricker_amplitude(i * dt, fc) for i in range(n)]
    probes = {"normal": (32, 52), "oblique": (50, 50)}

    def run(size, L):
        o = (size - 64) // 2
        eps, mu = onp.vacuum_materials(size, size)
        Ez, Hx, Hy = onp.grid_zeros(size, size)
        Ezx = np.zeros_like(Ez)
        P = pm.profiles(size, size, S, L=L) if L else None
        series = {k: [] for k in probes}
        for i in range(n):
            if L:
                pm.leapfrog(Ez, Ezx, Hx, Hy, eps, mu, dt, dx, 1, 32 + o, 32 + o, [amps[i]], P)
            else:
                onp.leapfrog(Ez, Hx, Hy, eps, mu, dt, dx, 1, 32 + o, 32 + o, amps=[amps[i]])
            for k, (r, c) in probes.items():
                series[k].append(Ez[r + o, c + o])
        return {k: np.array(v) for k, v in series.items()}

    open_, pml, mur = run(400, 40), run(64, 10), run(64, 0)
    refl = {k: (np.abs(pml[k] - open_[k]).max() / np.abs(open_[k]).max(),
                np.abs(mur[k] - open_[k]).max() / np.abs(open_[k]).max()) for k in probes}
    assert refl["normal"][0] <= 1e-4 and refl["oblique"][0] <= 1e-4, refl
    assert refl["normal"][0] * 1000 < refl["normal"][1] and refl["oblique"][0] * 1000 < refl["oblique"][1], refl
