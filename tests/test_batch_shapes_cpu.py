"""The shape table of tests/test_gpu_batch_shapes.py and CPU-only checks of it.

The host instantiates every resident kernel of the batched engine for at most 4, 8 or 16 cells per thread (MAXC) and
picks one by ceil(R*C / resident_threads(R*C)).  CASES lists, per kernel family, members that are resident with their
monitor tables and take each MAXC the capacity rule can reach, at shapes with both dimensions odd and
resident_threads % C != 0, so that the cell walk's carry branch is taken.  This module restates resident_threads and the
capacity rule in plain Python and asserts, per row, that the member is resident, that its cells per thread are the stated
ones and fall in the bracket of the stated MAXC, and that nthr % C != 0; and that the table reaches every
(family, boundary, dtype, MAXC) the rule can reach.  Unreachable, since LDS_LIMIT / arrays / itemsize is too small:
MAXC = 16 for lossy, periodic and every float64 family, MAXC = 8 for float64 with 5, 6 or 7 arrays (point sources with
material arrays, lossy, periodic).

It also chooses the point cells, probes and window of every row (point_cells, window) and checks what the GPU tests
rely on: which slots of the cell walk the point cells occupy, that they are distinct, and where the window lies."""
from collections import namedtuple

import pytest

LDS_LIMIT = 163840
NF, MAX_POINTS = 10, 12           # window frequencies and the largest point-source table of the GPU tests
LAYER, SMALL_LAYER = 10, 4

# family "points": the monitored kernels with point sources (Mur or PML, material arrays or uniform); "lossy": the
# same with a conductivity; "periodic": periodic columns with the layer on the rows ("layer") or PEC there ("pec").
Case = namedtuple("Case", "family boundary dtype materials R C per_thread maxc layer")

_BIG = [
    ("points", "mur", "f32", "arrays", 67, 97, 7, 8),
    ("points", "mur", "f32", "arrays", 83, 97, 8, 8),        # the only shape whose walk reaches slot 7 of MAXC = 8
    ("points", "mur", "f32", "uniform", 101, 113, 12, 16),
    ("points", "pml", "f32", "arrays", 71, 89, 7, 8),
    ("points", "pml", "f32", "uniform", 97, 101, 10, 16),
    ("points", "mur", "f64", "uniform", 67, 97, 7, 8),
    ("points", "pml", "f64", "uniform", 59, 83, 5, 8),
    ("points", "mur", "f64", "arrays", 53, 71, 4, 4),
    ("lossy", "mur", "f32", "arrays", 71, 89, 7, 8),
    ("lossy", "pml", "f32", "arrays", 61, 89, 6, 8),
    ("lossy", "mur", "f64", "arrays", 47, 59, 4, 4),
    ("lossy", "pml", "f64", "arrays", 47, 59, 4, 4),
    ("periodic", "layer", "f32", "arrays", 61, 89, 6, 8),
    ("periodic", "pec", "f32", "arrays", 61, 89, 6, 8),
    ("periodic", "layer", "f64", "arrays", 47, 59, 4, 4),
]
_SMALL_THREADS = {(11, 11): 2, (13, 70): 4, (17, 19): 3}      # cells per thread


def _cases():
    out = [Case(*row, LAYER if row[1] in ("pml", "layer") else 0) for row in _BIG]
    for dtype in ("f32", "f64"):
        for R, C in ((11, 11), (13, 70), (17, 19)):
            per = _SMALL_THREADS[R, C]
            for family in ("points", "lossy"):
                if (R, C) == (17, 19) and family == "points":
                    continue
                out.append(Case(family, "mur", dtype, "arrays", R, C, per, 4, 0))
                out.append(Case(family, "pml", dtype, "arrays", R, C, per, 4, SMALL_LAYER))
            out.append(Case("periodic", "layer", dtype, "arrays", R, C, per, 4, SMALL_LAYER))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.family}-{c.boundary}-{c.dtype}-{c.materials}-{c.R}x{c.C}"


# ---- the rule, restated -------------------------------------------------------------------------------------------------

def resident_threads(cells):
    """A wave multiple, at least a quarter of the cells, at most 1024."""
    return min(1024, -(-(-(-cells // 4)) // 64) * 64)


def _seg(n, esz):
    return -(-n * esz // 16) * 16


def itemsize(dtype):
    return {"f32": 4, "f64": 8}[dtype]


def arrays(family, boundary, materials):
    """Ez, Hx, Hy (+ Ezx with a layer) (+ ce, ch unless uniform) (+ ca with a conductivity); a periodic batch always
    counts the lossy PML's seven."""
    if family == "periodic":
        return 7
    if family == "lossy":
        return 7 if boundary == "pml" else 6
    return (3 if materials == "uniform" else 5) + (boundary == "pml")


def field_bytes(family, boundary, dtype, materials, R, C):
    esz = itemsize(dtype)
    factors = _seg(4 * R, esz) + _seg(4 * C, esz) if family == "periodic" or boundary == "pml" else 0
    return arrays(family, boundary, materials) * _seg(R * C, esz) + factors


def table_bytes(nf, ntab):
    return 16 * nf + 8 * ntab


def is_resident(c, nf=NF, ntab=MAX_POINTS):
    return field_bytes(c.family, c.boundary, c.dtype, c.materials, c.R, c.C) + table_bytes(nf, ntab) <= LDS_LIMIT


def window_in_lds(c, ntab, window_cells, nf=NF):
    return (field_bytes(c.family, c.boundary, c.dtype, c.materials, c.R, c.C) + table_bytes(nf, ntab) +
            16 * nf * window_cells <= LDS_LIMIT)


def per_thread(cells):
    return -(-cells // resident_threads(cells))


def maxc_of(per):
    return 4 if per <= 4 else 8 if per <= 8 else 16 if per <= 16 else None


# ---- the monitors of a row ------------------------------------------------------------------------------------------------

def window(c):
    """3 x 6 cells around a point cell of a high slot (the waves of a 40-step run travel six cells): the lone cell, or
    in a periodic row the cell of column C - 2, with the image column."""
    fixed = fixed_cells(c)
    r, j = fixed["colC2" if c.family == "periodic" else "lone"]
    return (min(max(r - 1, 0), c.R - 3), c.C - 6 if c.family == "periodic" else min(max(j - 2, 0), c.C - 6), 3, 6)


def source_rows(c):
    """Rows that hold some member's line source (the drivers place it at R // 2 + m % 3 - 1)."""
    return range(c.R // 2 - 1, c.R // 2 + 2)


def source_cell(c, m):
    """A cell of member m's line source as the drivers place it: the middle column, or in a periodic row the second
    cell of a span that starts at column 0, 0, C - 6 or 3."""
    col = (0, 0, c.C - 6, 3)[m % 4] + 1 if c.family == "periodic" else c.C // 2
    return (c.R // 2 + m % 3 - 1, col)


def wanted_slots(last):
    """Slots of one thread's walk that are not neighbours: 0, 5, 7, 9 and the thread's last, as far as they exist."""
    s = {q for q in (0, 5, 7, 9) if q <= last} | {last}
    if len(s) < 3 and last >= 2:
        s.add(last - 2)
    return sorted(s)


def fixed_cells(c):
    """name -> (row, col) of the point cells that are the same for every member.  many / lone: the cells of two threads
    of the resident walk, one owning wanted_slots(), one owning only its last slot."""
    R, C, periodic = c.R, c.C, c.family == "periodic"
    cells, nthr = R * C, resident_threads(R * C)
    out = {"origin": 0, "last_row": (R - 1) * C + 5, "last": cells - 1 - periodic}
    if periodic:        # columns 0 and C - 2, at slot 4 or higher where the walk has one
        r = min(R - 2, -(-4 * nthr // C))
        out["col0"] = r * C
        out["colC2"] = (r + 1 if r + 1 < R - 1 else r) * C + C - 2
    busy = {l % nthr for l in out.values()} | {(r * C + j) % nthr for r in source_rows(c) for j in range(C)}

    def usable(ls):
        return all(l not in out.values() and l // C not in source_rows(c) and not (periodic and l % C == C - 1)
                   for l in ls)

    for tid in range(3, nthr):
        last = (cells - 1 - tid) // nthr
        ls = [q * nthr + tid for q in wanted_slots(last)]
        if tid not in busy and usable(ls):
            out.update({f"many{q}": l for q, l in zip(wanted_slots(last), ls)})
            busy.add(tid)
            break
    # the free thread with the highest last slot (the highest such thread)
    for tid in sorted(range(3, nthr), key=lambda t: ((cells - 1 - t) // nthr, t), reverse=True):
        l = (cells - 1 - tid) // nthr * nthr + tid
        if tid not in busy and usable([l]):
            out["lone"] = l
            break
    return {k: divmod(l, C) for k, l in out.items()}


def point_cells(c, members):
    """(B, P, 2) point cells: fixed_cells() and, last, a cell of member m's own line source."""
    fixed = list(fixed_cells(c).values())
    return [[list(rc) for rc in fixed] + [list(source_cell(c, m))] for m in range(members)]


def image_probe(c):
    """A cell of a periodic row's image column, in the bottom half."""
    return [3 * c.R // 4, c.C - 1]


# ---- the checks -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_the_row_is_resident_at_the_stated_cells_per_thread(c):
    cells, nthr = c.R * c.C, resident_threads(c.R * c.C)
    assert is_resident(c)
    assert per_thread(cells) == c.per_thread and maxc_of(c.per_thread) == c.maxc
    lo = {4: 0, 8: 4, 16: 8}[c.maxc]
    assert lo < c.per_thread <= c.maxc
    assert nthr % c.C != 0                                     # the walk's carry branch is taken
    assert c.R % 2 == 1 and (c.C % 2 == 1 or c.maxc == 4)      # odd, except the wide 13 x 70
    if c.boundary in ("pml", "layer"):
        assert c.layer >= 1 and 2 * c.layer + 3 <= (c.R if c.family == "periodic" else min(c.R, c.C))


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_the_point_cells_sit_in_the_slots_the_row_is_for(c):
    R, C = c.R, c.C
    cells, nthr = R * C, resident_threads(R * C)
    fixed = fixed_cells(c)
    lin = {k: r * C + j for k, (r, j) in fixed.items()}
    many = sorted(l for k, l in lin.items() if k.startswith("many"))
    assert "lone" in lin and len(many) >= 2
    # one thread owns the wanted slots and nothing else, whichever member's source cell is added
    tid = many[0] % nthr
    last = (cells - 1 - tid) // nthr
    assert [l // nthr for l in many] == wanted_slots(last) and {l % nthr for l in many} == {tid}
    if c.maxc == 16:
        assert last > 8 and sum(q > 8 for q in wanted_slots(last)) >= 1 and {0, 5, 7}.issubset(wanted_slots(last))
    if c.maxc == 8:
        assert last > 3 and any(q > 3 for q in wanted_slots(last))
    if c.per_thread == 8:
        assert wanted_slots(last) == [0, 5, 7]
    slots = wanted_slots(last)
    assert any(b - a > 1 for a, b in zip(slots, slots[1:])) or last < 2        # not all neighbours
    # another thread owns only its last slot
    lone = lin["lone"]
    assert lone % nthr != tid and lone // nthr == (cells - 1 - lone % nthr) // nthr
    if c.maxc > 4:
        assert lone // nthr >= 4
    assert fixed["origin"] == (0, 0) and fixed["last_row"][0] == R - 1
    assert fixed["last"] == ((R - 1, C - 2) if c.family == "periodic" else (R - 1, C - 1))
    ntab = 0
    for m in range(4):
        src = source_cell(c, m)[0] * C + source_cell(c, m)[1]
        every = list(lin.values()) + [src]
        ntab = max(ntab, len(every) + (c.family == "periodic") * sum(l % C == 0 for l in every))
        assert len(set(every)) == len(every) and all(0 <= l < cells for l in every)
        owners = {}
        for l in every:
            owners.setdefault(l % nthr, set()).add(l // nthr)
        assert owners[tid] == set(slots) and owners[lone % nthr] == {lone // nthr}
    if c.family == "periodic":
        assert all(j != C - 1 for _, j in fixed.values())
        assert fixed["col0"][1] == 0 and fixed["colC2"][1] == C - 2
        if c.maxc > 4:
            assert lin["col0"] // nthr >= 4 and lin["colC2"] // nthr >= 4
        r, j = image_probe(c)
        assert j == C - 1 and R // 2 <= r < R
    assert ntab <= MAX_POINTS          # a periodic row's table lists the cells of column 0 at their images too


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_the_window_lies_past_the_first_slots(c):
    r0, c0, nr, nc = window(c)
    nthr = resident_threads(c.R * c.C)
    assert 0 <= r0 and r0 + nr <= c.R and 0 <= c0 and c0 + nc <= c.C
    r, j = fixed_cells(c)["colC2" if c.family == "periodic" else "lone"]
    assert r0 <= r < r0 + nr and c0 <= j < c0 + nc             # a point source drives the window's cells
    inside = [i * c.C + k for i in range(r0, r0 + nr) for k in range(c0, c0 + nc)]
    if c.maxc >= 8:
        assert r * c.C + j >= 4 * nthr and sum(l >= 4 * nthr for l in inside) >= 6
    if c.maxc == 16:
        assert r * c.C + j >= 8 * nthr and sum(l >= 8 * nthr for l in inside) >= 6
    if c.family == "periodic":
        assert c0 + nc == c.C                                  # the image column


def _reachable():
    """(family, boundary, dtype, MAXC) that some resident member takes, with no tables at all (the most room)."""
    out = set()
    for family, boundaries in (("points", ("mur", "pml")), ("lossy", ("mur", "pml")), ("periodic", ("periodic",))):
        for boundary in boundaries:
            for dtype in ("f32", "f64"):
                for materials in ("arrays", "uniform") if family == "points" else ("arrays",):
                    for R in range(3, 130):               # squares and near-squares reach every cell count's bracket
                        for C in (R, R + 1, R + 2):
                            per = per_thread(R * C)
                            if per <= 16 and field_bytes(family, boundary, dtype, materials, R, C) <= LDS_LIMIT:
                                out.add((family, boundary, dtype, maxc_of(per)))
    return out


def _key(c):
    return (c.family, "periodic" if c.family == "periodic" else c.boundary, c.dtype, c.maxc)


def test_the_table_reaches_every_variant_the_rule_can_reach():
    reachable = _reachable()
    assert {_key(c) for c in CASES} == reachable
    # what the module docstring lists as unreachable
    for family, boundary in (("points", "mur"), ("points", "pml"), ("lossy", "mur"), ("lossy", "pml"),
                             ("periodic", "periodic")):
        assert (family, boundary, "f64", 16) not in reachable
        assert ((family, boundary, "f32", 16) in reachable) == (family == "points")
        assert ((family, boundary, "f64", 8) in reachable) == (family == "points")
    # float64 reaches MAXC = 8 with uniform materials alone
    for boundary in ("mur", "pml"):
        cells = LDS_LIMIT // arrays("points", boundary, "arrays") // 8
        assert per_thread(cells) <= 4
    # both placements of the accumulators occur in every family by the rule itself or are forced by the tests
    for family in ("points", "lossy", "periodic"):
        assert any(window_in_lds(c, MAX_POINTS, 18) for c in CASES if c.family == family and c.maxc > 4)
