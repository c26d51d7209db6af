"""The fused build's single-grid Mur engine, bit for bit: every launch shape of tests/fused_cases.py against the C oracle
that states libfdtd2d_fused.so's arithmetic exactly (oracle/fdtd_oracle.c, the _fma symbols: four forms as one
correctly rounded fma each, everything else one rounding per operation; tests/test_fused_oracle_cpu.py checks that
oracle against rational arithmetic).

  1. the exact build, in this process, against the plain oracle: proves the table and the runner without the fused
     library;
  2. the fused build, in child processes (the library is chosen when the package is first imported), one per group of
     cases, one after another, against the fused oracle;
  3. the table reaches every variant it promises, by what the engines reported while the cases ran.

A fused case that differs while its exact twin passes means a kernel fuses another pair than the four stated ones, or
none: the fix is to write the form out in that kernel, as staged_level (csrc/kernels_split.hpp) does, not a tolerance."""
import json
import os
import subprocess
import sys

import pytest

import fused_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# seconds per child: all six together take 6 s on an MI355X box (the C oracle of the widest grids dominates); the limit
# only ends a hang
LIMITS = {"small": 120, "passes32": 120, "passes64": 120, "sources": 120, "window": 120, "wide": 180}

CHILD = r'''
import json, sys
sys.path[:0] = [ROOT, TESTS]
import fdtd2d_amd as fd
from fdtd2d_amd import _abi
import fused_cases as fc
assert fd.ARITHMETIC == "fused" and _abi.LIB_PATH.endswith("libfdtd2d_fused.so")
assert "fused" in _abi.load().fdtd2d_version().decode()
print("FUSED_PARITY " + json.dumps(fc.run_group(fd, GROUP, True)))
'''

_seen = {}          # case name -> variant tuple, from whichever of the runs below came first


def _failures(results):
    """One line per case that differs or did not launch what it names, with positions and the worst ulp distance."""
    out = []
    for name, res in results.items():
        if res["launch"]:
            out.append(f"{name}: launched something else: {res['launch']}")
        bad = {k: v for k, v in res["fields"].items() if not v["equal"]}
        if bad:
            out.append(f"{name}: " + "; ".join(f"{k} {v['ndiff']} cells differ, first {v['first']}, worst {v['max_ulp']:.0f} ulp"
                                               for k, v in bad.items()))
    return out


def _note(results):
    for name, res in results.items():
        if res["variant"] is not None:
            _seen.setdefault(name, tuple(res["variant"]))


@pytest.fixture(scope="module")
def fused_results():
    """Every group in a fresh child with FDTD2D_ARITHMETIC=fused.  Returns (results by case name, error text or None);
    after a child that died of a signal or ran into its limit no further child is started."""
    results = {}
    for group in fc.GROUPS:
        code = f"ROOT = {ROOT!r}\nTESTS = {os.path.join(ROOT, 'tests')!r}\nGROUP = {group!r}\n" + CHILD
        try:
            p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=LIMITS[group],
                               env=dict(os.environ, FDTD2D_ARITHMETIC="fused"))
        except subprocess.TimeoutExpired:
            return results, f"group {group}: no result after {LIMITS[group]} s; later groups not started"
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            return results, f"group {group}: child ended with {p.returncode}; later groups not started\n" + p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("FUSED_PARITY ")]
        if p.returncode != 0 or not lines:
            return results, f"group {group}: child failed ({p.returncode})\n" + p.stdout[-1000:] + p.stderr[-4000:]
        results.update(json.loads(lines[-1][len("FUSED_PARITY "):]))
    _note(results)
    return results, None


def test_exact_build_matches_the_plain_oracle_in_every_case():
    import fdtd2d_amd as fd
    if fd.ARITHMETIC != "exact":
        pytest.skip("this half runs in the exact build's process")
    results = {}
    for group in fc.GROUPS:
        results.update(fc.run_group(fd, group, False))
    _note(results)
    assert set(results) == {c["name"] for c in fc.CASES}
    bad = _failures(results)
    assert not bad, f"{len(bad)} of {len(results)} cases:\n" + "\n".join(bad)


def test_fused_build_matches_the_fused_oracle_in_every_case(fused_results):
    results, error = fused_results
    assert error is None, error
    assert set(results) == {c["name"] for c in fc.CASES}
    bad = _failures(results)
    assert not bad, f"{len(bad)} of {len(results)} cases:\n" + "\n".join(bad)


def test_the_table_reaches_every_variant_it_promises(fused_results):
    """(dtype, last pass steps, waves, side waves, xcd map, zone tiles fused, windowed) as the engines reported them."""
    results, error = fused_results
    assert error is None, error
    seen = set(_seen.values())
    assert len(_seen) >= 150
    for nt in (8, 16):
        assert any(v[0] == "float64" and v[1] == nt for v in seen), ("float64", nt)
    for nt in (8, 16, 20):
        assert any(v[0] == "float32" and v[1] == nt for v in seen), ("float32", nt)
    for waves in (1, 4, 8):
        assert any(v[2] == waves for v in seen), ("waves", waves)
    for side in (1, 2, 4):
        assert any(v[3] == side for v in seen), ("side waves", side)
        assert any(v[0] == "float64" and v[3] == side for v in seen), ("float64 side waves", side)
    for xcd in (0, 1):
        assert any(v[4] == xcd and v[3] > 1 for v in seen), ("xcd map", xcd)
    for fuse in (0, 1):
        assert any(v[0] == "float32" and v[1] == 20 and v[5] == fuse for v in seen), ("zone tiles fused", fuse)
    for dt in ("float32", "float64"):
        assert any(v[0] == dt and v[6] == 1 for v in seen), ("windowed", dt)
