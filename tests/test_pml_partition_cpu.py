"""The case table of tests/test_gpu_pml_passes.py and CPU-only checks of it.

The single-grid boundary="pml" engine advances a grid with one of three things: the float32 16-step pass, which is TWO
kernels that read the same buffers and write disjoint cells (k_bulk_split_pml on the tasks whose cone touches the layer,
the unchanged k_bulk_split on the rest; launch_pml_split in csrc/pass_f32_pml.hip derives the partition), the 8-step
k_pass_pml, whose waves decide one by one whether their cone touches the layer (float64 always, float32 at
max_pass_steps = 8 and for a take of exactly 8 steps inside a float32 run), and the single-step kernels.  Where the two
passes can go wrong depends on (L, R, C), the launch shape and the run length.  This module restates, in plain Python
and independently of the product code,
  * the strips: nstrips, x0_of(s) with the left-shifted last strip, the columns a strip stores;
  * launch_pml_split: n_left, n_right, inner, reach = L + 16, a_hi, c_lo (rounded up to 8), rows_tb, n_top, n_bot,
    rows_e, both (two streams from 256 rows), the task decode of k_bulk_split_pml and of the plain kernel (band by band,
    or dealt out XCD by XCD);
  * k_pass_pml: the three launch classes (a_hi, c_lo rounded up to 16 rows, reach = L + 1 + 16) and the per-wave
    `layer` predicate;
  * the columns both partitions count as layer columns: max(L, 4) -- the plain bodies' general form (grid edge or
    source in the cone) applies the Mur frame's rule to the columns < 5 and >= C - 5 of the strip it holds;
  * plan_pass for a PML handle, the band-height rules and which launch shape a pass of a run takes,
and asserts for every row of CASES that every cell is owned by exactly one task of exactly one kernel, that every cell
whose nlev-step cone reaches a layer update (or a column the plain body would treat as the Mur frame) is owned by a
layer task, and the property the row is in the table for."""
from collections import namedtuple

import numpy as np
import pytest

NT_PAIR, HC_PAIR, SW_PAIR, OW_PAIR = 16, 16, 256, 224
NT_P8, HC_P8 = 8, 8
V_OF = {"f32": 4, "f64": 2}
MUR_BAND = 5                # columns per side the plain bodies' general form treats as the Mur frame

Case = namedtuple("Case", "name dtype R C L n max_steps materials source opts ezx courant prop")


# ---- the rules, restated ---------------------------------------------------------------------------------------------------

def up(x, m):
    return (x + m - 1) // m * m


def nstrips(C, OW):
    return (C + OW - 1) // OW


def x0_of(s, ns, C, SW, OW, HC):
    x = s * OW - HC
    if s == ns - 1:
        x = min(x, (C - SW + 3) & ~3)
    return x


def stored_cols(s, ns, C, V, SW, OW, HC):
    """[lo, hi): the columns the 64 lanes of strip s store (V columns per lane from x0 + V lane, inside the grid and
    inside the strip's own OW columns)."""
    x0 = x0_of(s, ns, C, SW, OW, HC)
    cols = [j for lane in range(64) for j in range(x0 + V * lane, x0 + V * lane + V)
            if 0 <= x0 + V * lane < C and s * OW <= x0 + V * lane < (s + 1) * OW and j < C]
    assert cols and cols == list(range(cols[0], cols[-1] + 1)), (s, x0)
    return cols[0], cols[-1] + 1


def layer_cols(L):
    return max(L, MUR_BAND - 1)


def cycle_steps(c, max_steps):
    """Longest pass of a PML engine whose max_pass_steps option was set: the pair needs float32 and uniform mu."""
    if c.materials == "mu" or c.R < 64 or c.C < 64:
        return 0
    if max_steps >= 16 and c.dtype == "f32":
        return 16
    return 8 if max_steps >= 8 else 0


def planned(n, cycle):
    """[(kernel length, levels)] of fdtd2d_run(n) on a PML handle, (0, 1) for a single step: a take of exactly 8 runs
    k_pass_pml, any other take runs the pair with nlev = take where the pair exists, else one single step."""
    out = []
    while n > 0:
        take = 0
        if cycle > 0:
            take = cycle if n > 2 * cycle else (n + 1) // 2 if n > cycle else n
        if take == 8:
            out.append((8, 8))
        elif take and cycle == 16:
            out.append((16, take))
        else:
            out.append((0, 1))
        n -= out[-1][1]
    return out


def launch_shape(c, nt, cycle, ns):
    """(band rows, edge rows, xcd map) of an nt-step pass of a run whose longest pass is `cycle`: the band_rows option,
    else a shape given for the full-length passes, else the rule."""
    o = c.opts
    shape = o.get("shape") if nt == cycle else None
    if o.get("band_rows"):
        br = o["band_rows"]
        shape = None
    elif shape:
        br = shape[0]
    elif nt >= 16:
        br = min(max((c.R + 57) // 58, 64), 448)
    else:
        want = max(1, (3072 + ns - 1) // ns)
        br = min(max(c.R // want, 16), 128)
    xcd = o["xcd_map"] if o.get("xcd_map", -1) >= 0 else (shape[4] if shape and len(shape) > 4 else 0)
    return br, (shape[2] if shape else 0), xcd


def pair_geometry(c, cycle=16, mutate=None):
    """launch_pml_split for the whole grid (band_lo = 0, band_hi = R, the handle owns top and bottom)."""
    R, C, L = c.R, c.C, c.L
    ns = nstrips(C, OW_PAIR)
    x0 = [x0_of(s, ns, C, SW_PAIR, OW_PAIR, HC_PAIR) for s in range(ns)]
    Lc = layer_cols(L)
    n_left = n_right = 0
    while n_left < ns and x0[n_left] < Lc + 1:
        n_left += 1
    if mutate == "n_right_ge":
        while n_right < ns - n_left and x0[ns - 1 - n_right] + SW_PAIR >= C - 1 - Lc:
            n_right += 1
    else:
        while n_right < ns - n_left and x0[ns - 1 - n_right] + SW_PAIR > C - 1 - Lc:
            n_right += 1
    inner = ns - n_left - n_right
    reach = L + NT_PAIR - (8 if mutate == "reach" else 0)
    br, edge, xcd = launch_shape(c, 16, cycle, ns)
    rows_e = max(16, edge if edge > 0 else 64)
    a_hi, c_lo = 0, R
    if inner > 0:
        a_hi = min(R, up(max(0, reach), 8))
        c_lo = max(a_hi, R - up(max(0, R - (R - reach)), 8))
    rows_tb = max(8, min(128, max(a_hi, R - c_lo)))
    g = dict(ns=ns, x0=x0, x0_last=x0[-1], x0_last_past_flush=x0[-1] - (C - SW_PAIR) if ns > 1 else 0, n_left=n_left,
             n_right=n_right, inner=inner, reach=reach, a_hi=a_hi, c_lo=c_lo, rows_tb=rows_tb, rows_e=rows_e,
             n_all=(R + rows_e - 1) // rows_e, n_top=(a_hi + rows_tb - 1) // rows_tb,
             n_bot=(R - c_lo + rows_tb - 1) // rows_tb, band_rows=br, xcd=xcd,
             plain_rows=(c_lo - a_hi) if inner > 0 else 0)
    g["nbands"] = (max(0, c_lo - a_hi) + br - 1) // br
    g["layer_blocks"] = (n_left + n_right) * g["n_all"] + inner * (g["n_top"] + g["n_bot"])
    g["plain_tasks"] = g["nbands"] * inner
    g["plain_blocks"] = 8 * ((g["plain_tasks"] + 7) // 8) if xcd and g["plain_tasks"] > 0 else g["plain_tasks"]
    g["both"] = g["layer_blocks"] > 0 and g["plain_blocks"] > 0 and R >= 256
    return g


def pair_tasks(c, g):
    """[(kernel, strip, ra, rb)] as the two kernels decode their block indices."""
    R, out = c.R, []
    n_edge = g["n_left"] + g["n_right"]
    for b in range(g["layer_blocks"]):
        if b < n_edge * g["n_all"]:
            sidx, band = divmod(b, g["n_all"])
            strip = sidx if sidx < g["n_left"] else g["ns"] - n_edge + sidx
            ra = band * g["rows_e"]
            rb = min(ra + g["rows_e"], R)
        else:
            sidx, band = divmod(b - n_edge * g["n_all"], g["n_top"] + g["n_bot"])
            strip = g["n_left"] + sidx
            if band < g["n_top"]:
                ra = band * g["rows_tb"]
                rb = min(ra + g["rows_tb"], g["a_hi"])
            else:
                ra = g["c_lo"] + (band - g["n_top"]) * g["rows_tb"]
                rb = min(ra + g["rows_tb"], R)
        if ra < rb:
            out.append(("layer", strip, ra, rb))
    per = (g["plain_tasks"] + 7) // 8
    for b in range(g["plain_blocks"]):
        if g["xcd"]:
            x, q = b & 7, b >> 3
            t = x * per + q
            if q >= per or t >= g["plain_tasks"]:
                continue
            band, sidx = divmod(t, g["inner"])
        else:
            sidx, band = divmod(b, g["nbands"])
        ra = g["a_hi"] + band * g["band_rows"]
        rb = min(ra + g["band_rows"], g["c_lo"])
        if ra < rb:
            out.append(("plain", g["n_left"] + sidx, ra, rb))
    return out


def p8_geometry(c, cycle=8):
    R, C, L = c.R, c.C, c.L
    V = V_OF[c.dtype]
    SW, OW = 64 * V, 64 * V - 2 * HC_P8
    ns = nstrips(C, OW)
    reach = L + 1 + 2 * NT_P8
    a_hi = min(R, max(0, up(reach, 16)))
    c_lo = max(a_hi, min(R, R - up(R - (R - reach), 16)))
    br = launch_shape(c, 8, cycle, ns)[0]
    return dict(V=V, SW=SW, OW=OW, ns=ns, x0=[x0_of(s, ns, C, SW, OW, HC_P8) for s in range(ns)], reach=reach, a_hi=a_hi,
                c_lo=c_lo, n1=(R + 15) // 16, nA=(a_hi + 15) // 16, nC=(R - c_lo + 15) // 16,
                nB=(max(0, c_lo - a_hi) + br - 1) // br, band_rows=br, inner=max(0, ns - 2))


def p8_is_layer(c, g, strip, ra, rb, mutate=None):
    """k_pass_pml's per-wave choice: does the cone (rows [ra - 16, rb + 8), the strip's columns) touch the layer?"""
    x0, Lc = g["x0"][strip], layer_cols(c.L)
    left = x0 < (Lc if mutate == "p8_col_L" else Lc + 1)
    return left or x0 + g["SW"] > c.C - 1 - Lc or ra - 2 * NT_P8 < c.L + 1 or rb + NT_P8 > c.R - 1 - c.L


def p8_tasks(c, g, mutate=None):
    R, out = c.R, []
    blocks = 2 * g["n1"] + g["inner"] * (g["nA"] + g["nC"] + g["nB"])
    for b in range(blocks):
        if b < 2 * g["n1"]:
            sidx, band = divmod(b, g["n1"])
            if sidx == 1 and g["ns"] == 1:
                continue
            strip = 0 if sidx == 0 else g["ns"] - 1
            ra = band * 16
            rb = min(ra + 16, R)
        elif b - 2 * g["n1"] < g["inner"] * (g["nA"] + g["nC"]):
            sidx, band = divmod(b - 2 * g["n1"], g["nA"] + g["nC"])
            strip = sidx + 1
            if band < g["nA"]:
                ra = band * 16
                rb = min(ra + 16, g["a_hi"])
            else:
                ra = g["c_lo"] + (band - g["nA"]) * 16
                rb = min(ra + 16, R)
        else:
            sidx, band = divmod(b - 2 * g["n1"] - g["inner"] * (g["nA"] + g["nC"]), g["nB"])
            strip = sidx + 1
            ra = g["a_hi"] + band * g["band_rows"]
            rb = min(ra + g["band_rows"], g["c_lo"])
        if ra < rb:
            out.append(("layer" if p8_is_layer(c, g, strip, ra, rb, mutate) else "plain", strip, ra, rb))
    return out


def ownership(c, tasks, V, SW, OW, HC):
    """(how many tasks store each cell, the cells a layer task stores)."""
    ns = nstrips(c.C, OW)
    count = np.zeros((c.R, c.C), np.int32)
    layer = np.zeros((c.R, c.C), bool)
    cols = {}
    for kind, strip, ra, rb in tasks:
        if strip not in cols:
            cols[strip] = stored_cols(strip, ns, c.C, V, SW, OW, HC)
        lo, hi = cols[strip]
        count[ra:rb, lo:hi] += 1
        if kind == "layer":
            layer[ra:rb, lo:hi] = True
    return count, layer


def needs_layer(R, C, L, nlev):
    """Cells whose Ez, Hx or Hy after nlev steps depends on an update the plain body gets wrong: Ez of a layer cell
    (the outer edge included) or of a column the general plain body treats as the Mur frame, Hx of a row or Hy of a
    column whose H factors are not 1 (half-cell positions: rows < L and > R - 2 - L, columns likewise)."""
    i, j = np.arange(R)[:, None], np.arange(C)[None, :]
    bad_e = (i < L) | (i > R - 1 - L) | (j < L) | (j > C - 1 - L) | (j < MUR_BAND) | (j >= C - MUR_BAND)
    bad_x = np.broadcast_to((i < L) | (i > R - 2 - L), (R, C))
    bad_y = np.broadcast_to((j < L) | (j > C - 2 - L), (R, C))

    def shifted(a, di, dj):                 # a[i + di, j + dj], False outside the grid
        out = np.zeros_like(a)
        src = a[max(di, 0):R + min(di, 0), max(dj, 0):C + min(dj, 0)]
        out[max(-di, 0):R + min(-di, 0), max(-dj, 0):C + min(-dj, 0)] = src
        return out
    te, tx, ty = (np.zeros((R, C), bool) for _ in range(3))
    for _ in range(nlev):
        tx = bad_x | tx | te | shifted(te, 1, 0)
        ty = bad_y | ty | te | shifted(te, 0, 1)
        te = bad_e | te | tx | shifted(tx, -1, 0) | ty | shifted(ty, 0, -1)
    return te | tx | ty


# ---- the table ---------------------------------------------------------------------------------------------------------------

def _case(name, dtype="f32", R=120, C=505, L=40, n=16, max_steps=None, materials="uniform", source="centre", opts=None,
          ezx="b", courant=0.15, **prop):
    if source == "centre":
        source = (R // 2, C // 2, 1, 1)
    return Case(name, dtype, R, C, L, n, max_steps if max_steps is not None else (16 if dtype == "f32" else 8), materials,
                source, dict(opts or {}), ezx, courant, prop)


def _cases():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    # float32 pair, columns, L = 40 (120 rows: a_hi = 56, c_lo = 64)
    add("cols-504", C=504, n_right=2, inner=0, plain_rows=0)
    add("cols-505", C=505, materials="eps", n_right=1, inner=1, plain_rows=8)
    add("cols-505-a", C=505, ezx="a", n_right=1, inner=1)
    add("cols-728", C=728, materials="eps", ns=4, n_right=2, inner=1)
    add("cols-729", C=729, ns=4, n_right=1, inner=2)
    add("cols-729-a", C=729, ezx="a", materials="eps", inner=2)
    add("cols-448", C=448, ns=2, inner=0)
    add("cols-449", C=449, materials="eps", ns=3, inner=0, n_left=1, n_right=2)
    add("cols-506", C=506, ns=3, x0_last=252, x0_last_past_flush=2, inner=1)       # C - SW + 3 = 253
    add("cols-507", C=507, materials="eps", ns=3, x0_last=252, x0_last_past_flush=1, inner=1)     # 254
    add("cols-731", C=731, ns=4, x0_last=476, x0_last_past_flush=1, inner=2)       # 478
    add("cols-130", C=130, ns=1, x0_last=-124, n_left=1, n_right=0, inner=0)
    add("cols-83", C=83, materials="eps", ns=1, x0_last=-172, inner=0)          # 2 L + 3: the narrowest grid the layer fits
    # float32 pair, rows, L = 40 (reach 56), one inner strip
    add("rows-112", R=112, inner=1, a_hi=56, c_lo=56, plain_rows=0, plain_tasks=0)
    add("rows-113", R=113, materials="eps", inner=1, a_hi=56, c_lo=57, plain_rows=1, plain_tasks=1)
    add("rows-113-a", R=113, ezx="a", inner=1, plain_rows=1)
    add("rows-120", R=120, materials="eps", inner=1, plain_rows=8)
    add("rows-255", R=255, inner=1, both=False, plain_rows=143)
    add("rows-256", R=256, materials="eps", inner=1, both=True, plain_rows=144)
    add("rows-256-a", R=256, ezx="a", inner=1, both=True)
    add("rows-257", R=257, inner=1, both=True, plain_rows=145)
    add("rows-83", R=83, materials="eps", inner=1, a_hi=56, c_lo=56, n_top=1, n_bot=1, rows_tb=56)
    # other layers
    add("L37", L=37, inner=1, reach=53, a_hi=56, c_lo=64)           # rows 53..55 of the top task: plain-capable
    add("L37-a", L=37, ezx="a", materials="eps", reach=53, a_hi=56)
    add("L1-466", R=70, C=466, L=1, materials="eps", inner=0, n_right=2)    # strip 1 holds columns 461..463 >= C - 5
    add("L1-469", R=70, C=469, L=1, inner=1, a_hi=24, c_lo=46, reach=17)
    add("L2-467", R=70, C=467, L=2, inner=0, n_right=2)                     # ... 462, 463 >= C - 5
    add("L4-469", R=70, C=469, L=4, materials="eps", inner=1, a_hi=24)      # 464 = C - 1 - L: the first inner width
    add("L10-64x64", R=64, C=64, L=10, materials="eps", ns=1, inner=0)
    add("L10-63x64", R=63, C=64, L=10, plan=[(0, 1)] * 16)                  # one row short of any pass
    add("L207", R=470, C=897, L=207, ns=5, n_left=1, n_right=2, inner=2, reach=223, a_hi=224, c_lo=246, rows_tb=128,
        n_top=2, n_bot=2, both=True)
    add("L208", R=470, C=897, L=208, materials="eps", ns=5, n_left=2, n_right=2, inner=1, reach=224, a_hi=224, c_lo=246,
        rows_tb=128, n_top=2, n_bot=2, both=True)
    # launch shape: inner strips and two streams
    for br in (1, 7, 33, 1000):
        add(f"band-{br}", R=260, C=729, opts={"band_rows": br}, band_rows=br, inner=2, both=True,
            nbands=(148 + br - 1) // br)
    for e in (0, 16, 40, 300):
        add(f"edge-{e}", R=260, C=729, materials="eps", opts={"shape": (64, 0, e)}, rows_e=max(16, e or 64),
            n_all=(260 + max(16, e or 64) - 1) // max(16, e or 64), both=True)
    add("xcd-0", R=260, C=729, opts={"xcd_map": 0, "band_rows": 7}, xcd=0, plain_tasks=44, plain_blocks=44)
    add("xcd-1", R=260, C=729, opts={"xcd_map": 1, "band_rows": 7}, xcd=1, plain_tasks=44, plain_blocks=48)
    add("xcd-1-tall", R=260, C=729, materials="eps", opts={"xcd_map": 1}, xcd=1, plain_tasks=6, plain_blocks=8)
    # run lengths, float32: the pair at every nlev, k_pass_pml for a take of 8, odd and even numbers of passes
    plans = {1: [(16, 1)], 3: [(16, 3)], 7: [(16, 7)], 8: [(8, 8)], 9: [(16, 9)], 15: [(16, 15)], 16: [(16, 16)],
             17: [(16, 9), (8, 8)], 24: [(16, 12)] * 2, 32: [(16, 16)] * 2, 33: [(16, 16), (16, 9), (8, 8)],
             40: [(16, 16), (16, 12), (16, 12)]}
    for k, (n, plan) in enumerate(plans.items()):
        add(f"run-{n}", n=n, materials="eps" if k % 2 else "uniform", plan=plan, inner=1)
    for n in (9, 17, 40):
        add(f"run-{n}-a", n=n, ezx="a", plan=plans[n])
    for n in (2, 4, 5, 6, 10, 11, 12, 13, 14):      # the remaining nlev of the pair, on the two-stream shape
        add(f"nlev-{n}", R=260, C=729, n=n, materials="eps" if n % 2 else "uniform", plan=[(16, n)], both=True)
    # sources (130 x 729: a_hi = 56, strips 1 and 2 inner, strip 0 stores columns 0..223)
    S = dict(R=130, C=729)
    add("src-row-seam-above", source=(55, 300, 1, 1), src_row_minus_a_hi=-1, **S)
    add("src-row-seam-below", source=(56, 300, 1, 1), materials="eps", src_row_minus_a_hi=0, **S)
    add("src-col-seam-left", source=(60, 223, 1, 1), src_col_minus_seam=-1, **S)
    add("src-col-seam-right", source=(60, 224, 1, 1), materials="eps", src_col_minus_seam=0, **S)
    add("src-first-cell", source=(1, 1, 1, 1), src_in="corner", **S)
    add("src-last-cell", source=(128, 727, 1, 1), materials="eps", src_in="corner", **S)
    add("src-top-layer", source=(10, 300, 1, 1), src_in="top", **S)
    add("src-bottom-layer", source=(120, 300, 1, 1), materials="eps", src_in="bottom", **S)
    add("src-left-layer", source=(65, 10, 1, 1), src_in="left", **S)
    add("src-right-layer", source=(65, 719, 1, 1), materials="eps", src_in="right", **S)
    add("src-corner-block", source=(125, 5, 1, 1), src_in="corner", **S)
    add("src-line", source=(60, 0, 1, 729), materials="eps", src_strips=4, src_in="plain-rows", **S)
    add("src-line-two-streams", R=260, C=729, source=(130, 0, 1, 729), src_strips=4, both=True)
    add("src-patch", source=(53, 290, 6, 12), src_row_minus_a_hi=-3, src_rows_past_a_hi=3, **S)
    add("src-none", source=None, materials="eps", **S)
    add("src-none-a", source=None, ezx="a", **S)
    # materials: a mu array takes no pass at all
    add("mu-array", materials="mu", plan=[(0, 1)] * 16)
    # k_pass_pml: float64, and float32 at max_pass_steps = 8 (L = 40: a_hi = 64, c_lo = R - 64)
    add("p8-f64-272", dtype="f64", R=140, C=272, p8_plain_strips=[])
    add("p8-f64-273", dtype="f64", R=140, C=273, materials="eps", p8_plain_strips=[1], p8_plain_rows=12)
    add("p8-f64-273-a", dtype="f64", R=140, C=273, ezx="a", p8_plain_strips=[1])
    add("p8-f64-128", dtype="f64", R=128, C=273, p8_a_hi=64, p8_c_lo=64, p8_plain_rows=0)
    add("p8-f64-129", dtype="f64", R=129, C=273, materials="eps", p8_a_hi=64, p8_c_lo=65, p8_plain_rows=1)
    for n, plan in ((8, [(8, 8)]), (16, [(8, 8)] * 2), (19, [(8, 8)] + [(0, 1)] * 3 + [(8, 8)]), (24, [(8, 8)] * 3)):
        add(f"p8-f64-run-{n}", dtype="f64", R=140, C=385, n=n, materials="eps" if n % 16 else "uniform", plan=plan,
            p8_plain_strips=[1, 2])
    add("p8-f64-L104", dtype="f64", R=260, C=340, L=104, p8_x0_1_minus_L=0, p8_plain_strips=[])    # x0 of strip 1 == L
    add("p8-f64-L103", dtype="f64", R=260, C=340, L=103, materials="eps", p8_x0_1_minus_L=1, p8_plain_strips=[1])
    add("p8-f64-L1-234", dtype="f64", R=70, C=234, L=1, source=(35, 140, 1, 1), p8_plain_strips=[])   # holds 229..231 >= C - 5
    add("p8-f64-L1-237", dtype="f64", R=70, C=237, L=1, source=(35, 140, 1, 1), p8_plain_strips=[1])
    add("p8-f32-528", R=140, C=528, max_steps=8, p8_plain_strips=[])
    add("p8-f32-529", R=140, C=529, max_steps=8, materials="eps", p8_plain_strips=[1], p8_plain_rows=12)
    add("p8-f32-529-a", R=140, C=529, max_steps=8, ezx="a", p8_plain_strips=[1])
    add("p8-f32-128", R=128, C=529, max_steps=8, materials="eps", p8_plain_rows=0)
    add("p8-f32-129", R=129, C=529, max_steps=8, p8_plain_rows=1)
    add("p8-f32-run-19", R=140, C=529, n=19, max_steps=8, materials="eps", plan=[(8, 8)] + [(0, 1)] * 3 + [(8, 8)])
    add("p8-f32-run-24", R=140, C=529, n=24, max_steps=8, plan=[(8, 8)] * 3)
    add("p8-f32-L1-490", R=70, C=490, L=1, max_steps=8, source=(35, 300, 1, 1), p8_plain_strips=[])   # holds 485..487
    add("p8-f32-L1-493", R=70, C=493, L=1, max_steps=8, materials="eps", source=(35, 300, 1, 1), p8_plain_strips=[1])
    add("p8-band-rows-1", dtype="f64", R=140, C=273, opts={"band_rows": 1}, p8_plain_rows=12, p8_nB=12)
    add("p8-band-rows-1000", dtype="f64", R=140, C=273, materials="eps", opts={"band_rows": 1000}, p8_nB=1)
    # The same seams at Courant 0.65 in vacuum.  A cell that a task updates by the wrong rule k cells from a stored cell
    # reaches it k steps later scaled by (S^2 / eps_r)^k: at S = 0.15 that is 0.0225 per cell, below float32 rounding from
    # the fifth cell on, so there only wrong ownership, a wrong body near its seam and a stale Ezx show; at 0.65 it is
    # 0.42 per cell, and the outermost cells of a 16-step cone count (0.42^15 = 2e-6 against 6e-8).  L = 8: the layer
    # rises steeply enough (s(1) = 2e-3) for a plain row started 8 rows early to show.
    F = dict(courant=0.65, materials="vacuum")
    add("fast-L8", L=8, inner=1, reach=24, a_hi=24, c_lo=96, **F)
    add("fast-cols-505", inner=1, n_right=1, **F)
    add("fast-rows-113", R=113, plain_rows=1, **F)
    add("fast-L1-466", R=70, C=466, L=1, inner=0, n_right=2, **F)
    add("fast-L2-467", R=70, C=467, L=2, inner=0, n_right=2, **F)
    add("fast-L4-469", R=70, C=469, L=4, inner=1, **F)
    add("fast-run-17", n=17, plan=[(16, 9), (8, 8)], **F)
    add("fast-p8-f32-L1-490", R=70, C=490, L=1, max_steps=8, source=(35, 300, 1, 1), p8_plain_strips=[], **F)
    add("fast-p8-f64-L1-234", dtype="f64", R=70, C=234, L=1, source=(35, 140, 1, 1), p8_plain_strips=[], **F)
    add("fast-p8-f64-L104", dtype="f64", R=260, C=340, L=104, p8_x0_1_minus_L=0, **F)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name


def variants(c):
    """The max_pass_steps values a row runs with: the plan under test, 8-step passes, single steps."""
    return sorted({c.max_steps, 8, 0}, reverse=True)


def facts(c):
    """What a row reaches, from the restated rules: the figures its `prop` names."""
    cyc = cycle_steps(c, c.max_steps)
    f = {"plan": planned(c.n, cyc)}
    if cyc == 16:
        g = pair_geometry(c)
        f.update({k: v for k, v in g.items() if k != "x0"})
    if cyc >= 8:
        g8 = p8_geometry(c, cyc)
        tasks = p8_tasks(c, g8)
        plain = [t for t in tasks if t[0] == "plain"]
        f.update(p8_a_hi=g8["a_hi"], p8_c_lo=g8["c_lo"], p8_nB=g8["nB"], p8_plain_strips=sorted({t[1] for t in plain}),
                 p8_plain_rows=sum(t[3] - t[2] for t in plain if t[1] == 1))
        if g8["ns"] > 1:
            f["p8_x0_1_minus_L"] = g8["x0"][1] - c.L
    if c.source and cyc == 16:
        r, q, nr, nc = c.source
        g = pair_geometry(c)
        f["src_row_minus_a_hi"] = r - g["a_hi"]
        f["src_rows_past_a_hi"] = r + nr - g["a_hi"]
        f["src_col_minus_seam"] = q - g["n_left"] * OW_PAIR
        f["src_strips"] = len({s for s in range(g["ns"]) for j in range(q, q + nc)
                               if j in range(*stored_cols(s, g["ns"], c.C, 4, SW_PAIR, OW_PAIR, HC_PAIR))})
        top, bot = r < c.L, r > c.R - 1 - c.L
        left, right = nr * nc == 1 and q < c.L, nr * nc == 1 and q > c.C - 1 - c.L      # (of a point)
        f["src_in"] = ("corner" if (top or bot) and (left or right) else "top" if top else "bottom" if bot else
                       "left" if left else "right" if right else
                       "plain-rows" if g["a_hi"] <= r < g["c_lo"] else "interior")
    return f


# ---- the table against the rules --------------------------------------------------------------------------------------------

def test_names_are_unique_and_rows_are_sized_for_a_shared_gpu():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert c.R * c.C < 500_000 and 1 <= c.n <= 40, c.name
        assert c.L >= 1 and 2 * c.L + 3 <= min(c.R, c.C), c.name
        assert c.dtype in V_OF and c.materials in ("uniform", "eps", "mu", "vacuum") and c.ezx in ("a", "b"), c.name
        assert c.courant in (0.15, 0.65) and (c.courant == 0.15 or c.materials == "vacuum"), c.name
        assert c.max_steps == 16 if c.dtype == "f32" and "p8-" not in c.name else c.max_steps == 8, c.name
        if c.source:
            r, q, nr, nc = c.source
            assert 0 <= r and r + nr <= c.R and 0 <= q and q + nc <= c.C, c.name


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_row_has_the_property_it_is_in_the_table_for(c):
    f = facts(c)
    for k, want in c.prop.items():
        assert f[k] == want, (c.name, k, f[k], want)
    assert sum(lev for _, lev in f["plan"]) == c.n


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_cell_has_one_owner_and_every_cone_that_meets_the_layer_a_layer_task(c):
    """For every pass length a row's three runs take: the tasks of the pass store every cell exactly once, and a cell
    whose cone (as many levels as the pass advances) reaches a layer update belongs to a task that runs the layer body."""
    checked = set()
    for ms in variants(c):
        cyc = cycle_steps(c, ms)
        for nt, nlev in set(planned(c.n, cyc)):
            if nt == 16:
                g = pair_geometry(c, cyc)
                count, layer = ownership(c, pair_tasks(c, g), 4, SW_PAIR, OW_PAIR, HC_PAIR)
            elif nt == 8:
                g = p8_geometry(c, cyc)
                count, layer = ownership(c, p8_tasks(c, g), g["V"], g["SW"], g["OW"], HC_P8)
            else:
                continue
            assert count.min() == 1 and count.max() == 1, (c.name, nt, np.argwhere(count != 1)[:4].tolist())
            need = needs_layer(c.R, c.C, c.L, nlev)
            assert not (need & ~layer).any(), (c.name, nt, nlev, np.argwhere(need & ~layer)[:4].tolist())
            checked.add(nt)
    assert checked == {nt for ms in variants(c) for nt, _ in planned(c.n, cycle_steps(c, ms)) if nt}


def test_plan_restated():
    assert planned(27, 16) == [(16, 14), (16, 13)] and planned(27, 8) == [(8, 8)] * 2 + [(0, 1)] * 3 + [(8, 8)]
    assert planned(8, 16) == [(8, 8)] and planned(4, 16) == [(16, 4)] and planned(4, 8) == [(0, 1)] * 4
    assert planned(25, 16) == [(16, 13), (16, 12)] and planned(16, 8) == [(8, 8)] * 2 and planned(5, 0) == [(0, 1)] * 5
    assert planned(15, 8) == [(8, 8)] + [(0, 1)] * 7 and planned(48, 16) == [(16, 16)] * 3


def test_strips_restated():
    # 16-step strips: 256 columns held, 224 stored, the last one shifted left onto a multiple of 4
    assert [nstrips(C, OW_PAIR) for C in (224, 225, 448, 449)] == [1, 2, 2, 3]
    assert x0_of(2, 3, 506, 256, 224, 16) == 252 and x0_of(1, 3, 506, 256, 224, 16) == 208
    assert x0_of(0, 1, 130, 256, 224, 16) == -124 and x0_of(0, 1, 83, 256, 224, 16) == -172
    assert stored_cols(0, 3, 506, 4, 256, 224, 16) == (0, 224) and stored_cols(2, 3, 506, 4, 256, 224, 16) == (448, 506)
    assert stored_cols(0, 1, 83, 4, 256, 224, 16) == (0, 83)
    # 8-step strips: 240 of 256 columns in float32, 112 of 128 in float64
    assert [nstrips(C, 240) for C in (480, 481)] == [2, 3] and [nstrips(C, 112) for C in (224, 225)] == [2, 3]
    assert stored_cols(2, 3, 273, 2, 128, 112, 8) == (224, 273)


def test_table_reaches_every_seam_of_both_partitions():
    F = {c.name: facts(c) for c in CASES}
    pair = [c for c in CASES if cycle_steps(c, c.max_steps) == 16]
    # the column partition: each count on either side of each of its steps
    assert {F[c.name]["inner"] for c in pair} >= {0, 1, 2} and {F[c.name]["n_left"] for c in pair} == {1, 2}
    assert {F[c.name]["n_right"] for c in pair} >= {0, 1, 2} and {F[c.name]["ns"] for c in pair} >= {1, 2, 3, 4, 5}
    # (the last strip always starts left of its pitch position: flush with the right edge, rounded up to a multiple of 4)
    assert {F[c.name]["x0_last_past_flush"] for c in pair if F[c.name]["ns"] > 1} == {0, 1, 2, 3}
    # the row partition: no plain row, one, a multiple of 8; both stream arrangements; tall ends in two tasks
    rows = {F[c.name]["plain_rows"] for c in pair if F[c.name]["inner"] > 0}
    assert {0, 1, 8} <= rows and {F[c.name]["both"] for c in pair} == {False, True}
    assert {F[c.name]["n_top"] for c in pair} >= {0, 1, 2} and {F[c.name]["rows_tb"] for c in pair} >= {8, 24, 56, 128}
    assert {F[c.name]["rows_e"] for c in pair} >= {16, 40, 64, 300} and {F[c.name]["xcd"] for c in pair} == {0, 1}
    # every nlev of the pair, the 8-step kernel inside a float32 run, odd and even numbers of passes, both flavours
    levs = {lev for c in pair for nt, lev in F[c.name]["plan"] if nt == 16}
    assert levs == set(range(1, 17)) - {8}
    assert any((8, 8) in F[c.name]["plan"] and (16, 9) in F[c.name]["plan"] for c in pair)
    assert {len(F[c.name]["plan"]) % 2 for c in pair} == {0, 1}
    for fam in ("cols-", "rows-", "L", "run-", "src-", "p8-f64", "p8-f32"):
        assert {c.ezx for c in CASES if c.name.startswith(fam)} == {"a", "b"}, fam
    # k_pass_pml: plain waves in both dtypes, rows either side of the first plain band, single steps inside a plan
    for dtype in ("f32", "f64"):
        p8 = [c for c in CASES if c.name.startswith("p8-") and c.dtype == dtype]
        assert any(F[c.name]["p8_plain_strips"] for c in p8) and not all(F[c.name]["p8_plain_strips"] for c in p8)
        assert {0, 1} <= {F[c.name]["p8_plain_rows"] for c in p8}
        assert any((0, 1) in F[c.name]["plan"] and (8, 8) in F[c.name]["plan"] for c in p8)
    # sources: on both sides of both seams, in each layer, a corner, across every strip, none
    src = [F[c.name] for c in CASES if c.name.startswith("src-") and c.source]
    assert {-1, 0} <= {f["src_row_minus_a_hi"] for f in src} and {-1, 0} <= {f["src_col_minus_seam"] for f in src}
    assert {f["src_in"] for f in src} >= {"top", "bottom", "left", "right", "corner", "plain-rows"}
    assert any(f["src_strips"] == f["ns"] for f in src) and any(c.source is None for c in CASES)
    assert {c.materials for c in CASES} == {"uniform", "eps", "mu", "vacuum"}


def test_the_three_mutations_move_a_seam_of_the_table():
    """What DESIGN.md section 5.4 records about the three one-line mutations of the C++, restated: `reach = L + NT - 8`
    breaks the cone property on rows of the table; `>=` for `>` in the n_right loop and `L` for `L + 1` in k_pass_pml's
    column test each change the partition of a row of the table (the seam is there) but not the cone property: both
    bounds have a column to spare (a strip's outermost held column is level-0 data only)."""
    broken, moved_r, moved_p8 = [], [], []
    for c in CASES:
        if cycle_steps(c, c.max_steps) == 16:
            g, gm = pair_geometry(c), pair_geometry(c, mutate="reach")
            _, layer = ownership(c, pair_tasks(c, gm), 4, SW_PAIR, OW_PAIR, HC_PAIR)
            lev = max(lev for nt, lev in planned(c.n, 16) if nt == 16) if any(nt == 16 for nt, _ in planned(c.n, 16)) else 0
            if lev and (needs_layer(c.R, c.C, c.L, lev) & ~layer).any():
                broken.append(c.name)
            gr = pair_geometry(c, mutate="n_right_ge")
            if gr["n_right"] != g["n_right"]:
                moved_r.append(c.name)
                count, layer = ownership(c, pair_tasks(c, gr), 4, SW_PAIR, OW_PAIR, HC_PAIR)
                assert count.min() == count.max() == 1 and not (needs_layer(c.R, c.C, c.L, 16) & ~layer).any()
        if cycle_steps(c, 8) == 8:
            g8 = p8_geometry(c)
            if p8_tasks(c, g8, mutate="p8_col_L") != p8_tasks(c, g8):
                moved_p8.append(c.name)
                _, layer = ownership(c, p8_tasks(c, g8, mutate="p8_col_L"), g8["V"], g8["SW"], g8["OW"], HC_P8)
                assert not (needs_layer(c.R, c.C, c.L, 8) & ~layer).any()
    assert {"cols-505", "rows-113", "rows-256", "L37", "L207", "band-1", "run-16", "src-line", "fast-L8"} <= set(broken), broken
    assert "cols-505" in moved_r and "L4-469" in moved_r, moved_r
    assert moved_p8 == ["p8-f64-L104", "fast-p8-f64-L104"], moved_p8
