"""CPU-only: the diagonal bounds of the active window (Oct, support_oct, dirty_oct, window_oct of csrc/active_window.hpp)
against boolean support maps.

tests/active_window_oct_check.cpp is a stand-alone program (its own main, host compiler, address and undefined-behaviour
sanitizers) in the manner of tests/active_window_check.cpp.  It propagates "may be non-zero" maps with the dependency
pattern of a step (H from E, stages A-D of mur_rules.hpp, the source) and checks after every transition that the maps lie
inside rectangle AND diagonal bounds, that a pass writing only the cells inside both would have written every cell that
changes or is stale, and that the bounds are gone before the first frame cell turns non-zero.  Fixed cases: point, patch
and line sources, two sources in turn, half-steps, add_point, a copy, an uncommitted launch, the four edges; then random
sequences.  With a third argument the program checks a copy of the bounds tightened by one cell: it must fail."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("awo") / "active_window_oct_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "active_window_oct_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_support_maps_stay_inside_the_octagon(check, seed):
    p = subprocess.run([check, str(seed), "200"], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert " 0 failures" in p.stdout


def test_a_bound_tightened_by_one_fails(check):
    """The net bites: the same program against bounds moved inward by one cell reports cells outside them -- in the
    fixed cases alone (no random sequences), where a point spreads without a source and the bounds are exact."""
    p = subprocess.run([check, "1", "0", "1"], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 1, (p.stdout[-3000:], p.stderr[-3000:])
    assert "outside" in p.stdout and " 0 failures" not in p.stdout


def test_the_device_test_is_the_header_test():
    """strip_of_block's test (task_meets_oct, kernels_stream.hpp) and Oct::meets are the same four comparisons."""
    hdr = open(os.path.join(ROOT, "fdtd-2d_amd", "csrc", "active_window.hpp")).read()
    dev = open(os.path.join(ROOT, "fdtd-2d_amd", "csrc", "kernels_stream.hpp")).read()
    assert "return rb - 1 + cb - 1 >= s0 && ra + ca <= s1 && rb - 1 - ca >= d0 && ra - (cb - 1) <= d1;" in hdr
    assert ("return rb - 1 + cb - 1 >= p.oct_s0 && ra + ca <= p.oct_s1 && rb - 1 - ca >= p.oct_d0 && ra - (cb - 1) <= p.oct_d1;"
            in dev)
    assert "const int ca = strip * ow, cb = (strip + 1) * ow < p.g.C ? (strip + 1) * ow : p.g.C;" in dev
