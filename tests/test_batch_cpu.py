"""CPU-only checks of the batched engine (fdtd2d_batch_*): the C ABI is exported and bound, the Python
surface is importable, arguments are checked before any device is touched, and without a GPU a valid
batch fails loudly instead of falling back to anything."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch_symbols():
    txt = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fdtd2d_batch_[a-z0-9_]+)\s*\(", txt)))


def test_batch_symbols_are_exported_and_bound():
    from fdtd2d_amd import _abi
    names = _batch_symbols()
    want = {"create", "destroy", "last_error", "info", "set_option", "set_stream", "set_materials",
            "set_materials_uniform", "courant", "upload", "download", "reset", "set_sources", "run",
            "run_waveform", "set_dft", "read_dft", "sync"}
    assert {n[len("fdtd2d_batch_"):] for n in names} == want
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in fdtd2d.h but not exported"
        assert n in _abi.SIGNATURES, f"{n} not bound in _abi.SIGNATURES"
    _abi.load()


def test_batch_constants_are_named_and_bound():
    from fdtd2d_amd import _abi
    txt = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    defs = dict(re.findall(r"#define\s+FDTD2D_(BATCH_\w+)\s+(-?\d+)", txt))
    assert {"BATCH_INFO_COUNT", "BATCH_INFO_ROWS", "BATCH_INFO_COLS", "BATCH_INFO_DTYPE", "BATCH_INFO_STEP",
            "BATCH_INFO_RESIDENT", "BATCH_INFO_LAUNCHES", "BATCH_INFO_RESIDENT_MAX_CELLS",
            "BATCH_OPT_RESIDENT", "BATCH_OPT_STEPS_PER_LAUNCH"} <= set(defs)
    for k, v in defs.items():
        assert getattr(_abi, k) == int(v), k


def test_batch_api_is_exported_from_the_package():
    import inspect
    import fdtd2d_amd as fd
    assert fd.BatchEngine is fd.batch.BatchEngine and fd.run_fdtd_batch is fd.batch.run_fdtd_batch
    assert "BatchEngine" in fd.__all__ and "run_fdtd_batch" in fd.__all__
    assert list(inspect.signature(fd.BatchEngine).parameters) == ["count", "rows", "cols", "dt", "dx", "dtype",
                                                                  "boundary", "device"]
    kw = inspect.signature(fd.run_fdtd_batch).parameters
    for name in ("nsteps", "sources", "fc", "waveform", "dt", "dx", "dtype", "boundary", "omega", "dft_every",
                 "device"):
        assert kw[name].kind is inspect.Parameter.KEYWORD_ONLY, name


def _create(count, rows, cols, dtype=0, boundary=1, device=0):
    from fdtd2d_amd import _abi
    lib = _abi.load()
    h = ctypes.c_void_p()
    rc = lib.fdtd2d_batch_create(ctypes.byref(h), count, rows, cols, 5e-14, 1e-4, dtype, boundary, device)
    msg = lib.fdtd2d_batch_last_error(None).decode()
    if rc == 0:
        lib.fdtd2d_batch_destroy(h)
    return rc, msg


@pytest.mark.parametrize("count,rows,cols,dtype,boundary", [
    (0, 64, 64, 0, 1),      # no members
    (-3, 64, 64, 0, 1),
    (4, 10, 11, 0, 1),      # below the 11 x 11 minimum of the 5-px Mur band
    (4, 11, 10, 1, 1),
    (4, 64, 64, 0, 2),      # PML: out of scope for batches
    (4, 64, 64, 0, 7),      # unknown boundary
    (4, 64, 64, 2, 1),      # bad dtype
])
def test_batch_create_checks_arguments_before_the_device(count, rows, cols, dtype, boundary):
    from fdtd2d_amd import _abi
    rc, msg = _create(count, rows, cols, dtype, boundary)
    assert rc == _abi.E_ARG and msg


def test_batch_without_a_device_has_no_fallback():
    """On a machine without a GPU a valid batch is E_NODEVICE with a message; there is no CPU path."""
    from fdtd2d_amd import _abi
    rc, msg = _create(16, 60, 60)
    if rc == 0:
        pytest.skip("a GPU is present")
    assert rc == _abi.E_NODEVICE and "no CPU path" in msg
    import fdtd2d_amd as fd
    with pytest.raises(fd.Fdtd2dError) as ei:
        fd.BatchEngine(16, 60, 60)
    assert ei.value.code == _abi.E_NODEVICE


def test_run_fdtd_batch_checks_inputs_before_the_device():
    import fdtd2d_amd as fd
    eps = np.full((3, 20, 20), fd.EPS0)
    with pytest.raises(ValueError):
        fd.run_fdtd_batch(eps[0], nsteps=4, sources=np.zeros((3, 2), int))              # not (B, R, C)
    with pytest.raises(ValueError):
        fd.run_fdtd_batch(eps, np.full((3, 20, 21), fd.MU0), nsteps=4, sources=np.zeros((3, 2), int))
    bad = eps.copy()
    bad[1] = fd.EPS0 / 100                   # Courant 1.5 at dt = 5e-14, dx = 1e-4
    with pytest.raises(AssertionError, match=r"members \[1\]"):
        fd.run_fdtd_batch(bad, nsteps=4, sources=np.zeros((3, 2), int))
