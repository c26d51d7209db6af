"""CPU-only checks of the batch monitors (fdtd2d_batch_monitor.h): the entry points are declared, exported and bound,
the constants are named, the Python surface has its shape, run_fdtd_batch refuses bad monitor arguments before any
device is touched, and without a device a monitored batch fails instead of falling back to anything."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdtd2d_batch_monitor.h")


def test_batch_monitor_symbols_are_declared_exported_and_bound():
    from fdtd2d_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(fdtd2d_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["fdtd2d_batch_read_dft_window", "fdtd2d_batch_read_probes", "fdtd2d_batch_set_dft_window",
                     "fdtd2d_batch_set_probes"]
    assert sorted(_abi.BATCH_MONITOR_SIGNATURES) == names
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared but not exported"
    loaded = _abi.load()
    for n in names:
        assert getattr(loaded, n).argtypes == _abi.BATCH_MONITOR_SIGNATURES[n][1]
        assert getattr(loaded, n).restype == _abi.BATCH_MONITOR_SIGNATURES[n][0]


def test_batch_monitor_constants_are_named_and_bound():
    from fdtd2d_amd import _abi
    defs = dict(re.findall(r"#define\s+FDTD2D_(BATCH_\w+)\s+(-?\d+)", open(HEADER).read()))
    assert defs == {"BATCH_INFO_DFT_WINDOW_LDS": "10", "BATCH_INFO_PROBE_SAMPLES": "11",
                    "BATCH_OPT_DFT_WINDOW_LDS": "2", "BATCH_MAX_DFT_FREQS": "16", "BATCH_MAX_PROBES": "64"}
    for k, v in defs.items():
        assert getattr(_abi, k) == int(v), k
    # the next free numbers after fdtd2d.h's
    base = dict(re.findall(r"#define\s+FDTD2D_(BATCH_(?:INFO|OPT)_\w+)\s+(-?\d+)",
                           open(os.path.join(ROOT, "include", "fdtd2d.h")).read()))
    assert max(int(v) for k, v in base.items() if k.startswith("BATCH_INFO")) == 9
    assert max(int(v) for k, v in base.items() if k.startswith("BATCH_OPT")) == 1


def test_batch_monitor_python_surface():
    import fdtd2d_amd as fd
    E = fd.BatchEngine
    assert list(inspect.signature(E).parameters) == ["count", "rows", "cols", "dt", "dx", "dtype", "boundary",
                                                     "device"]
    assert list(inspect.signature(E.set_dft_window).parameters) == ["self", "window", "omegas", "every"]
    assert inspect.signature(E.set_dft_window).parameters["every"].default == 1
    assert list(inspect.signature(E.read_dft_window).parameters) == ["self"]
    assert list(inspect.signature(E.set_probes).parameters) == ["self", "cells", "capacity"]
    p = inspect.signature(E.read_probes).parameters
    assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None
    kw = inspect.signature(fd.run_fdtd_batch).parameters
    for name in ("dft_window", "window_omegas", "probes"):
        assert kw[name].kind is inspect.Parameter.KEYWORD_ONLY and kw[name].default is None, name


def _no_device(monkeypatch, fd):
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(fd.batch, "BatchEngine", boom)


W10 = np.linspace(10e9, 100e9, 10) * 2 * np.pi


@pytest.mark.parametrize("kwargs,match", [
    (dict(dft_window=(0, 0, 30, 1)), "together"),
    (dict(window_omegas=W10), "together"),
    (dict(dft_window=(0, 0, 0, 1), window_omegas=W10), "empty or leaves"),
    (dict(dft_window=(-1, 0, 3, 1), window_omegas=W10), "empty or leaves"),
    (dict(dft_window=(20, 39, 3, 2), window_omegas=W10), "empty or leaves"),
    (dict(dft_window=(20, 30, 21, 1), window_omegas=W10), "empty or leaves"),
    (dict(dft_window=(1.5, 0, 3, 1), window_omegas=W10), "4 integers"),
    (dict(dft_window=(0, 0, 3), window_omegas=W10), "4 integers"),
    (dict(dft_window=(0, 0, 3, 1), window_omegas=np.ones(17)), "1..16"),
    (dict(dft_window=(0, 0, 3, 1), window_omegas=np.ones((3, 2))), "shape"),
    (dict(dft_window=(0, 0, 3, 1), window_omegas=[np.nan]), "finite"),
    (dict(dft_window=(0, 0, 3, 1), window_omegas=W10, dft_every=0), "dft_every"),
    (dict(probes=np.zeros((65, 2), int)), "1..64"),
    (dict(probes=np.zeros((0, 2), int)), "1..64"),
    (dict(probes=[[40, 3]]), "in the 40x40 grid"),
    (dict(probes=[[3, -1]]), "in the 40x40 grid"),
    (dict(probes=np.zeros((2, 3, 2), int)), "shape"),
    (dict(probes=[[1.5, 2.0]]), "integers"),
])
def test_run_fdtd_batch_refuses_bad_monitors_on_the_host(monkeypatch, kwargs, match):
    import fdtd2d_amd as fd
    _no_device(monkeypatch, fd)
    eps = np.full((4, 40, 40), fd.EPS0)
    with pytest.raises(ValueError, match=match):
        fd.run_fdtd_batch(eps, nsteps=4, sources=np.full((4, 2), 5), **kwargs)


def test_batch_monitors_without_a_device_have_no_fallback():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), 4, 40, 40, 5e-14, 1e-4, _abi.F32, _abi.BOUNDARY_MUR5, 0)
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
        pytest.skip("a GPU is present")
    import fdtd2d_amd as fd
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.run_fdtd_batch(np.full((2, 40, 40), fd.EPS0), nsteps=4, sources=np.full((2, 2), 20),
                          dft_window=(10, 20, 5, 1), window_omegas=W10, probes=[[20, 20], [5, 5]])
    assert ei.value.code == _abi.E_NODEVICE


def test_batch_monitor_entry_points_check_the_handle():
    from fdtd2d_amd import _abi
    lib = _abi.load()
    d = np.zeros(16)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cells = np.zeros(2, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.fdtd2d_batch_set_dft_window(None, 0, 0, 1, 1, 1, dp, 1) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_dft_window(None, dp, dp) == _abi.E_ARG
    assert lib.fdtd2d_batch_set_probes(None, 1, cells, 4) == _abi.E_ARG
    assert lib.fdtd2d_batch_read_probes(None, dp, 0, 1) == _abi.E_ARG
