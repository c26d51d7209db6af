"""The rows of tests/test_gpu_batch_wide_lines.py and CPU-only checks of them: the four families that came after the
shapes table of tests/test_batch_shapes_cpu.py (flux lines, line sources on them, the Hz polarisation and its flux lines)
at the MAXC = 8 instances of their resident kernels, with lines, point cells, probes and a window at slots 4 and 5 of the
cell walk.

The rule is that module's (resident_threads, _seg, per_thread, maxc_of, field_bytes, table_bytes, LDS_LIMIT); this one adds
what batch.hip's lds_table_bytes and flux_part_bytes add for flux lines: 16 * nff for their phasor table, 32 * nff * cells
for their sums.  All rows are float32 without a pole: seven arrays (a lossless box with lines runs the lossy kernels).

    boundary   R x C      layer   cells/thread   1024 % C
    pml        61 x 89    6       6              45        the carry branch often; slot 5 (cells >= 5120) in the bottom
                                                           layer and the edge rows
    pml        163 x 33   4       6              1         slot 5 begins at row 155, column 5
    periodic   163 x 33   4       6              1         the same with the cyclic neighbour and the image column
    periodic   61 x 89    6       6              45        the carry branch, periodic

Every row carries, for all four families (slot = cell // 1024, owner thread = cell % 1024):
  lines    a row line at slot 5; a row line at slot 4 that crosses the next (one cell on two lines: a two-bit nibble); a
           column line at C - 2 across slots 3, 4 and 5; a column line at column 0 of a periodic row (column 1 of a box)
           across slots 4 and 5, longer at the bottom than the line at C - 2, so that Hy[:, C - 2] of a periodic row takes
           an H part for column 0 alone at slot 5
  points   one thread's slots wanted_slots(5) = [0, 3, 5] with the slot-5 cell on the first line; a lone slot-4 cell;
           another thread's slot 0; a slot-5 cell of the last line (column 0 of a periodic row, listed at its image too)
  probes   every point cell and a slot-5 cell of the last column (the image column of a periodic row)
  window   tab.window(): 3 x 6 at slot 4 or higher (slot 5 in a box; with the image column in a periodic row)
  sigma    a patch of interior cells, all at slot 4, inside conductivity_margin and the Hz polarisation's allowed set
The point cells come from wanted_slots; fixed_cells() chooses its threads away from any line, so the thread here is the
owner of a cell of the first line instead.

The runs start from a random uploaded state (a wave travels six cells in the 24 steps, so no source would reach the
lines): 24 steps as run(13), run(11), the lines set before the first and sampled every third step, so the sums cross a
launch.  The liveness checks below run every family's stand-in once per row and are what the GPU module compares with.

Mutants of the kernels that the GPU module's tests catch and these rows are for (each by hand, none committed):
fmask >> (4 * (q & 3)) in k_batch_resident_flux; hmask >> (2 * (q & 3)) in k_batch_resident_flux_src; pts >> (q & 3) & 1
in k_batch_resident_hz; fmask as unsigned short in k_batch_resident_hz_flux; the MAXC = 4 box instance in the flux table's
resident[0][1]; lw = l - 1 for slots >= 5 in the periodic MAXC = 8 flux body."""
from collections import namedtuple

import numpy as np
import pytest

from oracle import fdtd_numpy as onp
from oracle_batch_flux import flux_oracle_for
from oracle_batch_flux_adjoint import line_source_oracle_for
from oracle_batch_hz import HzPeriodicOracle, HzPmlOracle
from oracle_batch_hz_flux import hz_flux_oracle_for
import test_batch_shapes_cpu as tab
from test_batch_shapes_cpu import LDS_LIMIT, _seg, maxc_of, per_thread, resident_threads

DT, DX = 5e-14, 1e-4
N, SPLITS, EVERY, WIN_EVERY = 24, (13, 11), 3, 2
NF, NFF, K = 2, 2, 6                       # window frequencies, line frequencies, channels
FAMILIES = ("flux", "linesrc", "hz", "hzflux")
LINED = ("flux", "linesrc", "hzflux")

Row = namedtuple("Row", "boundary R C layer")
ROWS = [Row("pml", 61, 89, 6), Row("pml", 163, 33, 4), Row("periodic", 163, 33, 4), Row("periodic", 61, 89, 6)]
# per shape: the slot-5 row line (row, first column, cells), the slot-4 row line (row, first column; it runs to column
# C - 2: a box's edge column holds zeros), the line at C - 2 (first row, cells), the line at column 0 or 1 (first row, cells), the lone slot-4 point cell
# and the rows of the conductivity patch
_AT = {(61, 89): dict(row5=(58, 50, 20), row4=(50, 80), colC2=(44, 14), col_low=(52, 8), lone4=(52, 40), patch=(47, 54)),
       (163, 33): dict(row5=(157, 5, 20), row4=(140, 20), colC2=(122, 35), col_low=(150, 11), lone4=(130, 12),
                       patch=(126, 151))}


def row_id(r):
    return f"{r.boundary}{r.R}x{r.C}"


def members(family):
    """Three members with lines, five without, as the families' own modules have."""
    return 5 if family == "hz" else 3


def case_of(r):
    """The shapes module's Case with this row's seven arrays."""
    if r.boundary == "periodic":
        return tab.Case("periodic", "layer", "f32", "arrays", r.R, r.C, 6, 8, r.layer)
    return tab.Case("lossy", "pml", "f32", "arrays", r.R, r.C, 6, 8, r.layer)


def slot(r, cell):
    return (cell[0] * r.C + cell[1]) // resident_threads(r.R * r.C)


def owner(r, cell):
    return (cell[0] * r.C + cell[1]) % resident_threads(r.R * r.C)


# ---- what a row carries ---------------------------------------------------------------------------------------------------

def lines(r):
    at, periodic = _AT[r.R, r.C], r.boundary == "periodic"
    return [("row",) + at["row5"], ("row", at["row4"][0], at["row4"][1], r.C - 1 - at["row4"][1]),
            ("col", r.C - 2) + at["colC2"], ("col", 0 if periodic else 1) + at["col_low"]]


def line_cells(line):
    kind, at, first, n = line
    return [(at, first + k) if kind == "row" else (first + k, at) for k in range(n)]


def entries(r):
    """The lines' cells concatenated in the order given: the entries of the sums and of the line-source weights."""
    return [c for line in lines(r) for c in line_cells(line)]


def point_cells(r):
    """[(row, col)]: one thread's slots [0, 3, 5] (the last on the first line), the lone slot-4 cell, another thread's
    slot 0, and the last but one cell of the last line."""
    nthr = resident_threads(r.R * r.C)
    on_line = line_cells(lines(r)[0])[3]
    tid = owner(r, on_line)
    last = (r.R * r.C - 1 - tid) // nthr
    many = [divmod(q * nthr + tid, r.C) for q in tab.wanted_slots(last)]
    assert many[-1] == on_line
    return many + [_AT[r.R, r.C]["lone4"], (0, 7), line_cells(lines(r)[3])[-2]]


def table_entries(r):
    """Entries of the point-source table: a periodic batch lists the cells of column 0 at their images too."""
    pts = point_cells(r)
    return len(pts) + (r.boundary == "periodic") * sum(j == 0 for _, j in pts)


def probe_cells(r):
    return point_cells(r) + [(lines(r)[0][1], r.C - 1)]


def window(r):
    return tab.window(case_of(r))


def patch(r):
    """(rows, columns) of the conductivity patch: every column of a period, columns 8 .. C - 9 of a box."""
    r0, r1 = _AT[r.R, r.C]["patch"]
    return slice(r0, r1), (slice(0, r.C) if r.boundary == "periodic" else slice(8, r.C - 8))


def h_values(r):
    """({(i, j)} of the Hx, {(i, j)} of the Hy) that take an H part (fdtd2d_batch_flux_adjoint.h): a row line holds
    (i, j) or (i + 1, j), a column line holds (i, j) or its right neighbour, (i, 0) for j = C - 2 of a periodic row;
    only values that the update writes."""
    hx, hy = set(), set()
    for line in lines(r):
        for i, j in line_cells(line):
            if line[0] == "row":
                hx |= {(i, j), (i - 1, j)}
            else:
                hy |= {(i, j), (i, r.C - 2 if j == 0 else j - 1)}
    keep = {(i, j) for i in range(r.R - 1) for j in range(r.C - 1)}
    return hx & keep, hy & keep


# ---- the capacity rule with lines -------------------------------------------------------------------------------------------

def field_bytes(r):
    c = case_of(r)
    return tab.field_bytes(c.family, c.boundary, c.dtype, c.materials, r.R, r.C)


def lds_table_bytes(r, family):
    return tab.table_bytes(NF, table_entries(r)) + (16 * NFF if family in LINED else 0)


def flux_cells(r):
    return sum(line[3] for line in lines(r))


def is_resident(r, family):
    return field_bytes(r) + lds_table_bytes(r, family) <= LDS_LIMIT


def window_in_lds(r, family):
    return field_bytes(r) + lds_table_bytes(r, family) + 16 * NF * 18 <= LDS_LIMIT


def flux_in_lds(r, family, allowed=True):
    """The sums live in LDS behind the window's accumulators when they fit too and FDTD2D_BATCH_OPT_FLUX_LDS allows."""
    acc = 16 * NF * 18 if window_in_lds(r, family) else 0
    return (family in LINED and allowed and
            field_bytes(r) + lds_table_bytes(r, family) + acc + 32 * NFF * flux_cells(r) <= LDS_LIMIT)


def lds_bytes(r, family, allowed=True):
    return (field_bytes(r) + lds_table_bytes(r, family) + (16 * NF * 18 if window_in_lds(r, family) else 0) +
            (32 * NFF * flux_cells(r) if flux_in_lds(r, family, allowed) else 0))


# ---- the members of a row and the calls that drive them -----------------------------------------------------------------------

_cfgs, _refs = {}, {}


def config(family, r):
    """Members that differ in eps, mu, conductivity, rectangle sources, line frequencies, weights and channels, and a
    random state: Ez of order 1 with H of order 1/377, or Hz of order 1/377 with E of order 1."""
    B = members(family)
    key = (B, r)
    if key not in _cfgs:
        R, C, periodic = r.R, r.C, r.boundary == "periodic"
        rng = np.random.default_rng(R + 2 * C + periodic)
        t = np.arange(N) * DT
        cells = len(entries(r))
        rows, cols = patch(r)
        sigma = np.zeros((B, R, C))
        sigma[:, rows, cols] = 5.0 * (1 + rng.random(sigma[:, rows, cols].shape))
        shapes = ((B, R, C), (B, R, C - 1), (B, R - 1, C), (B, R, C))
        cfg = dict(R=R, C=C, boundary=r.boundary, layer=r.layer, sigma=sigma,
                   eps=(onp.EPS0 * (1 + 2 * rng.random((B, R, C)))).astype(np.float32),
                   mu=(onp.MU0 * (1 + 0.5 * rng.random((B, R, C)))).astype(np.float32),
                   rects=np.array([[R // 2 + m % 3 - 1, ((0, 2, C - 6, 1, 3) if periodic else (8, 12, C - 12, 10, 14))[m],
                                    1, ((C - 1, 3, 3, 2, 4) if periodic else (C - 20, 3, 2, 2, 4))[m]] for m in range(B)]),
                   amps=np.stack([np.sin(2 * np.pi * 50e9 * (1 + 0.1 * m) * t + m) for m in range(B)]),
                   omegas=2 * np.pi * np.array([[40e9, 85e9], [35e9, 75e9], [45e9, 90e9], [50e9, 70e9], [30e9, 95e9]])[:B],
                   win_omegas=2 * np.pi * np.array([50e9, 70e9]),
                   points=np.array(point_cells(r)), weights=0.2 * rng.standard_normal((B, len(point_cells(r)), K)),
                   probes=np.array(probe_cells(r)),
                   chan=np.stack([[np.sin(2 * np.pi * 45e9 * (1 + 0.2 * c + 0.05 * m) * t + c + 1) for c in range(K)]
                                  for m in range(B)]),
                   # the E parts are of the order of Ez, the H parts of the order of Ez / 377
                   we=0.3 * (1 + rng.random((B, cells, K))) * rng.choice([-1.0, 1.0], (B, cells, K)),
                   wh=1e-3 * (1 + rng.random((B, cells, K))) * rng.choice([-1.0, 1.0], (B, cells, K)),
                   state=[rng.standard_normal(s) for s in shapes])
        _cfgs[key] = cfg
    return _cfgs[key]


def state_of(family, cfg):
    """(Ez, Hx, Hy, Ezx) or (Hz, Ex, Ey, Hzx) of the random state."""
    s = cfg["state"]
    if family in ("hz", "hzflux"):
        return [s[0] / 377, s[1], s[2], s[3] / 377]
    return [s[0], s[1] / 377, s[2] / 377, s[3]]


def courant00(cfg):
    return np.array([(1 / np.sqrt(float(e) * float(u)) * DT) / DX for e, u in zip(cfg["eps"][:, 0, 0], cfg["mu"][:, 0, 0])])


def drive(b, family, r, cfg=None, splits=SPLITS, with_lines=True, channels=True, sigma=True, we=True, wh=True,
          points=True, state=None, line_list=None):
    """The same calls on a BatchEngine (in the family's polarisation) and on the stand-in.  with_lines False leaves the
    lines (and the line sources) out, channels False leaves every source but the rectangle's silent; cfg, state and
    line_list replace the row's own members, random state and lines."""
    cfg = cfg or config(family, r)
    b.set_materials(cfg["eps"], cfg["mu"]).set_sources(cfg["rects"])
    b.set_pml(r.layer, courant00=courant00(cfg))
    if sigma:
        b.set_conductivity(cfg["sigma"])
    b.set_dft_window(window(r), cfg["win_omegas"], every=WIN_EVERY).set_probes(cfg["probes"], N)
    if points:
        b.set_point_sources(cfg["points"], cfg["weights"])
    s = state or state_of(family, cfg)
    b.upload(s[0], s[1], s[2])
    b.upload_ezx(s[3])
    lined = with_lines and family in LINED
    if lined:
        setter = b.set_hz_flux_lines if family == "hzflux" else b.set_flux_lines
        setter(line_list or lines(r), cfg["omegas"], every=EVERY)
    if lined and family == "linesrc" and (we or wh):
        b.set_flux_line_sources(cfg["we"] if we else None, cfg["wh"] if wh else None)
    done, launches = 0, 0
    for k in splits:
        before = getattr(b, "launches", 0)
        b.run(k, cfg["amps"][:, done:done + k], cfg["chan"][:, :, done:done + k] if channels else None)
        launches += getattr(b, "launches", 0) - before
        done += k
    out = dict(fields=tuple(b.download()) + (b.download_ezx() if hasattr(b, "download_ezx") else b.Ezx.copy(),),
               dft=b.read_dft_window(), probes=b.read_probes(), launches=launches)
    if lined:
        out["E"], out["H"] = b.read_flux_lines(raw=True)
        out["P"] = b.flux()
        if hasattr(b, "flux_scale"):
            out["scale"] = b.flux_scale()
    return out


def oracle_class(family, boundary):
    if family == "flux":
        return flux_oracle_for(boundary)
    if family == "linesrc":
        return line_source_oracle_for(boundary)
    if family == "hzflux":
        return hz_flux_oracle_for(boundary)
    return HzPeriodicOracle if boundary == "periodic" else HzPmlOracle


def stand_in(family, r, **kw):
    """The stand-in's results of a (family, row), computed once per set of options and left unchanged."""
    key = (family, r) + tuple(sorted(kw.items()))
    if key not in _refs:
        ref = oracle_class(family, r.boundary)(members(family), r.R, r.C, DT, DX, dtype=np.float32, boundary=r.boundary)
        _refs[key] = drive(ref, family, r, **kw)
    return _refs[key]


CASES = [(f, r) for f in FAMILIES for r in ROWS]
CASE_IDS = [f"{f}-{row_id(r)}" for f, r in CASES]


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,r", CASES, ids=CASE_IDS)
def test_the_row_is_resident_at_six_cells_per_thread_with_its_sums_in_lds(family, r):
    cells, nthr = r.R * r.C, resident_threads(r.R * r.C)
    assert field_bytes(r) == {(61, 89): 154496, (163, 33): 153776}[r.R, r.C]
    assert is_resident(r, family)
    assert per_thread(cells) == 6 and maxc_of(per_thread(cells)) == 8
    assert nthr == 1024 and nthr % r.C == {89: 45, 33: 1}[r.C] != 0        # the walk's carry branch is taken
    assert r.R % 2 == 1 and r.C % 2 == 1 and 2 * r.layer + 3 <= min(r.R, r.C)
    assert table_entries(r) <= tab.MAX_POINTS and window(r)[2:] == (3, 6)
    assert window_in_lds(r, family)
    if family in LINED:
        assert flux_cells(r) <= 100
        assert flux_in_lds(r, family)                                   # beside everything else
        assert not flux_in_lds(r, family, allowed=False)                # "global": the option's doing alone
        assert lds_bytes(r, family) - lds_bytes(r, family, allowed=False) == 32 * NFF * flux_cells(r)
    else:
        assert not flux_in_lds(r, family) and lds_bytes(r, family) == field_bytes(r) + lds_table_bytes(r, family) + 576


def test_what_the_rule_cannot_reach():
    # MAXC = 16 needs more than 8 * 1024 cells and MAXC = 8 more than 4 * 1024: seven float32 arrays of 8193 cells take
    # 7 * 32784 = 229488 B, seven float64 arrays of 4097 cells 7 * 32784 B too, ten float32 arrays (a pole) of 4097 cells
    # 10 * 16400 = 164000 B, each above the 163840 B of LDS before any factor or table is counted
    assert resident_threads(8193) == resident_threads(4097) == 1024
    assert per_thread(8192) == 8 and per_thread(8193) == 9 and per_thread(4096) == 4 and per_thread(4097) == 5
    assert 7 * _seg(8193, 4) == 229488 > LDS_LIMIT
    assert 7 * _seg(4097, 8) == 229488 > LDS_LIMIT
    assert 10 * _seg(4097, 4) == 164000 > LDS_LIMIT and 12 * _seg(4097, 4) > LDS_LIMIT
    for esz, arrays in ((4, 7), (8, 7), (4, 10), (4, 12), (8, 10), (8, 12)):
        reached = {maxc_of(per_thread(R * C)) for R in range(3, 200) for C in (R, R + 1, R + 2, 33, 89)
                   if per_thread(R * C) <= 16 and arrays * _seg(R * C, esz) <= LDS_LIMIT}
        assert reached == ({4, 8} if (esz, arrays) == (4, 7) else {4}), (esz, arrays)


# ---- 2. what sits at the high slots -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_the_lines_sit_at_the_slots_the_row_is_for(r):
    periodic = r.boundary == "periodic"
    row5, row4, colC2, col_low = lines(r)
    assert len(lines(r)) == 4 and all(0 <= i < r.R and 0 <= j < r.C - periodic for i, j in entries(r))
    assert 1 <= row5[1] <= r.R - 2 and 1 <= row4[1] <= r.R - 2
    assert {slot(r, c) for c in line_cells(row5)} == {5}
    assert {slot(r, c) for c in line_cells(row4)} == {4}
    assert colC2[1] == r.C - 2 and {slot(r, c) for c in line_cells(colC2)} == {3, 4, 5}
    assert col_low[1] == (0 if periodic else 1) and {slot(r, c) for c in line_cells(col_low)} == {4, 5}
    # one cell on two lines, at slot 4: a nibble with two bits
    twice = [c for c in set(entries(r)) if entries(r).count(c) == 2]
    assert twice == [(row4[1], r.C - 2)] and slot(r, twice[0]) == 4
    assert len(set(entries(r))) == len(entries(r)) - 1
    # the conductivity patch: interior cells, all at slot 4, where the Ez and the Hz families may conduct
    rows, cols = patch(r)
    g = max(6, r.layer)
    assert g <= rows.start and rows.stop - 1 <= r.R - 2 - g
    assert periodic or (g <= cols.start and cols.stop - 1 <= r.C - 2 - g)
    assert {slot(r, (i, j)) for i in range(rows.start, rows.stop) for j in range(cols.start, cols.stop)} == {4}
    assert any(rows.start <= i < rows.stop and cols.start <= j < cols.stop for i, j in line_cells(row4))


@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_point_cells_probes_and_window_sit_at_the_slots_the_row_is_for(r):
    periodic = r.boundary == "periodic"
    pts = point_cells(r)
    assert len(set(pts)) == len(pts) == 6 and all(0 <= i < r.R and 0 <= j < r.C - periodic for i, j in pts)
    many, lone4, other0, low5 = pts[:3], pts[3], pts[4], pts[5]
    # one thread owns slots 0, 3 and 5 (not neighbours), the slot-5 cell on a line
    assert [slot(r, c) for c in many] == tab.wanted_slots(5) == [0, 3, 5] and len({owner(r, c) for c in many}) == 1
    assert many[2] in line_cells(lines(r)[0])
    # a slot-4 cell alone in its thread, off the lines; another thread's slot 0; a slot-5 cell of the last line
    assert slot(r, lone4) == 4 and lone4 not in entries(r)
    assert slot(r, other0) == 0 and slot(r, low5) == 5 and low5 in line_cells(lines(r)[3])
    assert low5[1] == (0 if periodic else 1)
    assert len({owner(r, c) for c in (many[0], lone4, other0, low5)}) == 4
    by_owner = {}
    for c in pts:
        by_owner.setdefault(owner(r, c), []).append(slot(r, c))
    assert sorted(by_owner.values()) == sorted([[0, 3, 5], [4], [0], [5]])
    assert table_entries(r) == 6 + periodic
    # probes: every point cell, and a slot-5 cell of the last column
    probes = probe_cells(r)
    assert probes[:6] == pts and probes[6][1] == r.C - 1 and slot(r, probes[6]) == 5
    # the window
    r0, c0, nr, nc = window(r)
    inside = [(i, j) for i in range(r0, r0 + nr) for j in range(c0, c0 + nc)]
    assert 0 <= r0 and r0 + nr <= r.R and 0 <= c0 and c0 + nc <= r.C
    assert min(slot(r, c) for c in inside) >= (4 if periodic else 5)
    assert not periodic or c0 + nc == r.C                               # the image column


@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_the_line_sources_put_both_parts_at_slot_5(r):
    periodic = r.boundary == "periodic"
    cfg = config("linesrc", r)
    assert cfg["we"].shape == cfg["wh"].shape == (3, len(entries(r)), K)
    assert np.all(cfg["we"] != 0) and np.all(cfg["wh"] != 0)
    hx, hy = h_values(r)
    assert any(slot(r, c) == 5 for c in hx) and any(slot(r, c) == 5 for c in hy)
    assert any(slot(r, c) == 4 for c in hx) and any(slot(r, c) == 3 for c in hy)
    # both of a row line's Hx and both of a column line's Hy at slot 5
    i5, j5 = line_cells(lines(r)[0])[0]
    assert {(i5, j5), (i5 - 1, j5)} <= hx and slot(r, (i5 - 1, j5)) == 5
    top = line_cells(lines(r)[2])[-1]
    assert {top, (top[0], top[1] - 1)} <= hy and slot(r, (top[0], top[1] - 1)) == 5
    if periodic:     # Hy[:, C - 2] serves column 0, at slot 5 for the last line alone
        served = [(i, r.C - 2) for i, _ in line_cells(lines(r)[3])]
        assert set(served) <= hy
        alone = [c for c in served if c not in line_cells(lines(r)[2]) and (c[0], r.C - 3) not in hy]
        assert alone and any(slot(r, c) == 5 for c in alone)
    # the stand-in agrees: one step with the H parts alone changes exactly these values (they are added before the H
    # update, which is linear in Ez, so the difference stays where it was put)
    with_h = stand_in("linesrc", r, splits=(1,), we=False, points=False)
    without = stand_in("linesrc", r, splits=(1,), channels=False, points=False)
    for name, a, b, want in (("Hx", with_h["fields"][1], without["fields"][1], hx),
                             ("Hy", with_h["fields"][2], without["fields"][2], hy)):
        for m in range(3):
            assert {tuple(c) for c in np.argwhere(a[m] != b[m])} == want, (name, m)


# ---- 3. liveness, on the stand-in alone -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,r", CASES, ids=CASE_IDS)
def test_everything_at_the_high_slots_is_live_in_the_stand_in(family, r):
    got = stand_in(family, r)
    assert all(np.all(np.isfinite(a)) for a in got["fields"]) and got["launches"] == 0
    B = members(family)
    assert got["probes"].shape == (B, 7, N) and np.all(np.abs(got["probes"]).max(axis=2) > 0)
    assert got["dft"].shape == (B, NF, 3, 6) and np.all(got["dft"] != 0)
    if family in LINED:
        for name in ("E", "H"):
            assert got[name].shape == (B, NFF, len(entries(r)))
            assert np.abs(got[name]).min() > 1e-6 * np.abs(got[name]).max(), name
        assert np.all(got["scale"] > 0) and got["P"].shape == (B, 4, NFF)
    # the sources act where they sit: against the same run with every channel silent
    silent = stand_in(family, r, channels=False)
    a, b = got["fields"][0], silent["fields"][0]
    for i, j in point_cells(r):
        assert np.all(a[:, i, j] != b[:, i, j]), (i, j)
    if family == "linesrc":
        for i, j in set(entries(r)):
            assert np.all(a[:, i, j] != b[:, i, j]), (i, j)
    if r.boundary == "periodic":
        assert np.array_equal(a[:, :, -1], a[:, :, 0])
    for name in ("probes",) + (("E", "H") if family in LINED else ()):
        assert not np.array_equal(got[name], silent[name]), name
    # the conductivity acts at slot 4: a run without it differs there
    lossless = stand_in(family, r, sigma=False)
    rows, cols = patch(r)
    assert np.any(got["fields"][0][:, rows, cols] != lossless["fields"][0][:, rows, cols])
