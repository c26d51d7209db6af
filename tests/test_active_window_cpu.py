"""CPU-only: the bookkeeping of the active window (csrc/active_window.hpp) against boolean support maps.

tests/active_window_check.cpp is a stand-alone program (its own main, host compiler, address and undefined-behaviour
sanitizers).  On small grids it drives random event sequences -- committed passes of 1, 2, 4, 8, 16 and 20 steps with random
source rectangles, half-steps, add_point, trial launches, copies, uploads, resets -- through the header and through
boolean maps that follow the exact dependency pattern of a step (H from E, stages A-D of mur_rules.hpp, the source), and
checks after every event that the maps lie inside the rectangles, that a pass restricted to the window would have written
every cell that changes, and that the rows and strips of the restricted launch cover the window."""
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
    exe = str(tmp_path_factory.mktemp("aw") / "active_window_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "active_window_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_support_maps_stay_inside_the_window(check, seed):
    p = subprocess.run([check, str(seed), "250"], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert " 0 failures" in p.stdout


def test_header_has_no_hip_in_it():
    txt = open(os.path.join(ROOT, "fdtd-2d_amd", "csrc", "active_window.hpp")).read()
    assert "#include <hip" not in txt and "__device__" not in txt and "__global__" not in txt
