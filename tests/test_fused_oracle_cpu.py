"""CPU: the fused variant of the C oracle (oracle/fdtd_oracle.c, suffixes _f32_fma / _f64_fma; c_oracle.*(fused=True)) --
the statement of libfdtd2d_fused.so's arithmetic that tests/test_gpu_fused_parity.py holds the fused build to, bit for bit.

The variant is checked against exact arithmetic, not against itself: every output cell of one H and one E half-step is
recomputed in fractions.Fraction from the oracle's own inputs, stage by stage in the C code's order (curl, left / right
bands, top / bottom bands, corners), every stage reading the correctly ROUNDED values of the stage before.  The four
fused forms are one exact expression each --
    hx - ch * dr        hy + ch * dc        e + (dhy - dhx) * ce        inward_old + k * (inward_new - own_old)
-- with dr, dc, dhy - dhx and inward_new - own_old rounded differences; ch, ce and k are taken as the oracle forms them
(one rounding per operation).  A cell passes when it is a correctly rounded value of its exact expression: |exact - got|
is no larger than the distance from exact to either floating-point neighbour of got.  The unfused oracle rounds the
product first and must fail that check somewhere in every field.

And the fused oracle is within the project's stated tolerances of the float64 goldens (tests/test_fused_build.py)."""
import os
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle.fdtd_numpy import EPS0, MU0

DT, DX = 5e-14, 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = [np.float32, np.float64]


def _rnd(x, dtype):
    """Fraction -> nearest value of dtype, ties to even (no double rounding through float64)."""
    c = dtype(float(x))
    cands = [np.nextafter(c, dtype(-np.inf)), c, np.nextafter(c, dtype(np.inf))]
    itype = np.int32 if dtype == np.float32 else np.int64
    best = min(cands, key=lambda v: (abs(F(float(v)) - x), int(np.array(v).view(itype)) & 1))
    return dtype(best)


def _bad_cells(got, exact):
    """Cells of `got` that are not a correctly rounded value of `exact` (same-shape nested list of Fractions)."""
    dtype = got.dtype.type
    bad = []
    for i in range(got.shape[0]):
        for j in range(got.shape[1]):
            g, x = got[i, j], exact[i][j]
            err = abs(x - F(float(g)))
            lo, hi = np.nextafter(g, dtype(-np.inf)), np.nextafter(g, dtype(np.inf))
            if err > abs(x - F(float(lo))) or err > abs(x - F(float(hi))):
                bad.append((i, j))
    return bad


def _state(r, c, dtype):
    rng = np.random.default_rng(100 * r + c)
    Ez = rng.standard_normal((r, c)).astype(dtype)
    Hx = (rng.standard_normal((r, c - 1)) * 1e-3).astype(dtype)
    Hy = (rng.standard_normal((r - 1, c)) * 1e-3).astype(dtype)
    eps = (EPS0 * rng.uniform(1, 10, (r, c))).astype(dtype)
    mu = (MU0 * rng.uniform(1, 3, (r, c))).astype(dtype)
    return Ez, Hx, Hy, eps, mu


def _exact_h(Ez, Hx, Hy, mu):
    """Exact hx - ch * dr and hy + ch * dc per cell (rounded ch, dr, dc); cells the half-step leaves alone keep
    their value."""
    T = Ez.dtype.type
    r, c = Ez.shape
    ch = T(DT) / (mu * T(DX))                                   # one rounding per operation, as the oracle forms it
    fx = lambda a: F(float(a))
    ex = [[fx(Hx[i, j]) for j in range(c - 1)] for i in range(r)]
    ey = [[fx(Hy[i, j]) for j in range(c)] for i in range(r - 1)]
    for i in range(r - 1):
        for j in range(c - 1):
            dr = _rnd(fx(Ez[i + 1, j]) - fx(Ez[i, j]), T)
            dc = _rnd(fx(Ez[i, j + 1]) - fx(Ez[i, j]), T)
            ex[i][j] = fx(Hx[i, j]) - fx(ch[i, j]) * fx(dr)
            ey[i][j] = fx(Hy[i, j]) + fx(ch[i, j]) * fx(dc)
    return ex, ey


def _exact_e(P, Hx, Hy, mu, eps):
    """The E half-step in the C code's sequential order; cur holds the rounded value of every cell so far, ex the exact
    expression of its last assignment."""
    T = P.dtype.type
    r, c = P.shape
    fx = lambda a: F(float(a))
    ce = T(DT) / (eps * T(DX))
    mc = corc.lib().orc_mur_coef_f32 if T == np.float32 else corc.lib().orc_mur_coef_f64
    k = fx(T(mc(mu[0, 0], eps[0, 0], DT, DX)))
    cur = [[fx(P[i, j]) for j in range(c)] for i in range(r)]
    ex = [row[:] for row in cur]
    p = [row[:] for row in cur]
    rd = lambda x: fx(_rnd(x, T))

    def put(i, j, x):
        ex[i][j] = x
        cur[i][j] = rd(x)

    for i in range(1, r - 1):
        for j in range(1, c - 1):
            dhy = rd(fx(Hy[i, j]) - fx(Hy[i, j - 1]))
            dhx = rd(fx(Hx[i, j]) - fx(Hx[i - 1, j]))
            put(i, j, p[i][j] + rd(dhy - dhx) * fx(ce[i, j]))
    for b in range(5):
        for i in range(1, r - 1):
            put(i, b, p[i][b + 1] + k * rd(cur[i][b + 1] - p[i][b]))
    for b in range(5):
        for i in range(1, r - 1):
            j = c - 1 - b
            put(i, j, p[i][j - 1] + k * rd(cur[i][j - 1] - p[i][j]))
    for b in range(5):
        for j in range(1, c - 1):
            put(b, j, p[b + 1][j] + k * rd(cur[b + 1][j] - p[b][j]))
    for b in range(5):
        i = r - 1 - b
        for j in range(1, c - 1):
            put(i, j, p[i - 1][j] + k * rd(cur[i - 1][j] - p[i][j]))
    for a in range(5):
        for b in range(5):
            t, u, l, rr = a, r - 1 - a, b, c - 1 - b
            put(t, l, (cur[t][l + 1] + cur[t + 1][l]) / 2)
            put(t, rr, (cur[t][rr - 1] + cur[t + 1][rr]) / 2)
            put(u, l, (cur[u - 1][l] + cur[u][l + 1]) / 2)
            put(u, rr, (cur[u - 1][rr] + cur[u][rr - 1]) / 2)
    return ex


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(11, 11), (12, 13)])
def test_fused_oracle_is_correctly_rounded_and_the_unfused_one_is_not(shape, dtype):
    r, c = shape
    Ez, Hx, Hy, eps, mu = _state(r, c, dtype)
    ex_hx, ex_hy = _exact_h(Ez, Hx, Hy, mu)
    out = {}
    for fused in (True, False):
        hx, hy = Hx.copy(), Hy.copy()
        corc.update_h(Ez, hx, hy, mu, eps, DT, DX, fused=fused)
        out[fused] = (hx, hy)
    hx, hy = out[True]
    assert _bad_cells(hx, ex_hx) == [] and _bad_cells(hy, ex_hy) == []
    assert _bad_cells(out[False][0], ex_hx) and _bad_cells(out[False][1], ex_hy)        # the check has teeth
    # the E half-step from the fused oracle's own H fields
    ex_e = _exact_e(Ez, hx, hy, mu, eps)
    e_f, e_u = Ez.copy(), Ez.copy()
    corc.update_e(e_f, hx, hy, mu, eps, DT, DX, fused=True)
    corc.update_e(e_u, hx, hy, mu, eps, DT, DX, fused=False)
    assert _bad_cells(e_f, ex_e) == []
    bad = _bad_cells(e_u, ex_e)
    assert bad, "the unfused oracle passes the check of the fused arithmetic: the check proves nothing"


def test_run_is_the_half_steps_and_the_plain_symbols_are_untouched():
    """orc_run_*_fma = H, E, source of the fused half-steps; fused=False gives what it always gave (the goldens pin
    it in test_oracle_golden.py) and differs from fused=True."""
    r, c, n = 23, 31, 9
    for dtype in DTYPES:
        Ez, Hx, Hy, eps, mu = _state(r, c, dtype)
        amps = np.linspace(-1, 1, n)
        a = [x.copy() for x in (Ez, Hx, Hy)]
        corc.run(*a, eps, mu, DT, DX, n, 7, 30, amps=amps, fused=True)
        b = [x.copy() for x in (Ez, Hx, Hy)]
        for s in range(n):
            corc.update_h(*b, mu, eps, DT, DX, fused=True)
            corc.update_e(*b, mu, eps, DT, DX, fused=True)
            corc.add_point(b[0], 7, 30, amps[s])
        u = [x.copy() for x in (Ez, Hx, Hy)]
        corc.run(*u, eps, mu, DT, DX, n, 7, 30, amps=amps)
        for x, y, z in zip(a, b, u):
            assert np.array_equal(x, y) and not np.array_equal(x, z)


def _rel(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name,steps,bound", [("g4_config1_256x256", 500, 5e-6), ("g7_vacuum_96x96_2000", 2000, 1e-4)])
def test_fused_oracle_within_the_stated_tolerances_of_the_float64_goldens(name, steps, bound):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    r, c = int(g["rows"]), int(g["cols"])
    sr, sc = (int(v) for v in g["src"])
    for dtype, lim in ((np.float32, bound), (np.float64, 1e-12)):
        eps = np.full((r, c), float(g["eps_uniform"])).astype(dtype)
        mu = np.full((r, c), MU0).astype(dtype)
        f = [np.zeros((r, c), dtype), np.zeros((r, c - 1), dtype), np.zeros((r - 1, c), dtype)]
        corc.run(*f, eps, mu, DT, DX, steps, sr, sc, amps=g["amps"], fused=True)
        for a, k in zip(f, ("Ez", "Hx", "Hy")):
            e = _rel(a, g[f"{k}_f64_{steps}"])
            print(name, np.dtype(dtype).name, k, e)
            assert e <= lim, (name, np.dtype(dtype).name, k, e)
