"""GPU tests of the loading wave of the level-split pass in its GENERAL body (edge strips, source strips).

That body loads its rows unmasked and applies the masks -- zeros in the lanes outside the grid, the update masks of the
coefficient rows -- in the tick in which a row becomes the wave's input (mask_input, kernels_split.hpp).  What the move
could break shows only where fields are non-zero next to the grid's edges, so every case here uploads pseudo-random
fields in EVERY cell (tests/fused_cases.py, _state: Ez of order 1, H of order 1e-3, seeded) and compares Ez, Hx and Hy with
the C oracle bit for bit (np.array_equal; the fused build against the oracle's fused arithmetic).  This pins that every
instantiation computes what it did.  It does NOT see the masks applied one tick late (mutation study, DESIGN.md section
5.2: 36 of 36 pass): a row is then still masked before any level updates it, and its one unmasked use reaches only lanes
outside the grid, whose coefficients are zero -- with finite fields the loader's masks guard against non-finite garbage
alone.

200 rows; widths at which lanes of both edge strips fall outside the grid: one strip (200 columns: the strip holds 256),
two strips (230, 300, 449: the last strip is shifted left to end at the edge), five (1000); float64 strips hold 128
columns, so 100, 130 and 300.  16-step passes on 4 and 8 waves, 20-step and 8-step passes, float64, eps and mu arrays
(their m_e / m_h masks are the ones that moved), a source in an interior strip and on a strip seam (those strips run the
general body too)."""
import numpy as np
import pytest

import fused_cases as fc

pytestmark = pytest.mark.gpu

CASES = []


def _add(name, shape, dtype, nt, n, src, kind="uniform", nw=None, **kw):
    opts = dict(max_pass_steps=nt, band_rows=48)
    if nw:
        opts["split_waves"] = nw
    expect = dict(passes_min=1, last_nt=nt)
    if nw:
        expect["shape"] = {1: nw}
    CASES.append(dict(name=name, group="loader", driver="engine", shape=shape, dtype=dtype, kind=kind, eps_r=1.9, n=n, src=src,
                      seed=shape[0] * shape[1] + nt + (nw or 0), options=opts, expect=expect,
                      allow_uniform=kind == "uniform", **kw))


R = 200
for _c in (200, 230, 300, 449, 1000):
    for _nw in (4, 8):
        _add(f"f32_16_{_c}_nw{_nw}", (R, _c), fc.F32, 16, 35, (21, _c // 2), nw=_nw)
for _c in (230, 1000):
    _add(f"f32_20_{_c}", (R, _c), fc.F32, 20, 20, (24, _c // 2))
for _c in (200, 230, 449, 1000):
    _add(f"f32_8_{_c}", (R, _c), fc.F32, 8, 19, (30, _c // 3), nw=4)
_add("f32_8_449_nw8", (R, 449), fc.F32, 8, 19, (30, 150), nw=8)
for _c in (100, 130, 300):
    for _nw in (4, 8):
        _add(f"f64_16_{_c}_nw{_nw}", (R, _c), fc.F64, 16, 35, (21, _c // 2), nw=_nw)
_add("f64_8_130", (R, 130), fc.F64, 8, 19, (30, 40), nw=4)
# coefficient arrays: eps alone, mu alone, both
for _c, _kind, _nw in ((230, "eps+mu", 8), (449, "eps+mu", 4), (1000, "eps+mu", 8), (300, "eps", 8), (300, "mu", 4)):
    _add(f"f32_16_{_c}_{_kind}_nw{_nw}", (R, _c), fc.F32, 16, 35, (21, _c // 2), kind=_kind, nw=_nw)
_add("f32_20_449_eps+mu", (R, 449), fc.F32, 20, 20, (24, 200), kind="eps+mu")
_add("f32_8_449_eps+mu", (R, 449), fc.F32, 8, 19, (30, 150), kind="eps+mu", nw=4)
_add("f64_16_130_eps+mu", (R, 130), fc.F64, 16, 35, (21, 60), kind="eps+mu", nw=8)
# the source strips: a point in the interior strip 2 (columns [448, 672)), one on the seam 448 (strips 1 and 2), a patch
_add("f32_16_1000_src_strip2", (R, 1000), fc.F32, 16, 35, (100, 560), nw=8)
_add("f32_16_1000_src_seam", (R, 1000), fc.F32, 16, 35, (100, 448), nw=8)
_add("f32_16_1000_src_seam_nw4_eps", (R, 1000), fc.F32, 16, 35, (100, 447), kind="eps", nw=4)
_add("f32_16_1000_patch", (R, 1000), fc.F32, 16, 35, (90, 440), nw=8, extent=(20, 12))


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_general_loader_matches_oracle(fd, name):
    case = next(c for c in CASES if c["name"] == name)
    res = fc.run_case(fd, case, fused=fd._abi.ARITHMETIC == "fused")
    print(name, res)
    assert res["launch"] is None, res["launch"]
    for k in fc.NAMES:
        assert res["fields"][k]["equal"], (k, res["fields"][k])
