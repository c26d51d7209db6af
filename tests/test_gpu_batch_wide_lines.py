"""GPU: flux lines, line sources, the Hz polarisation and its flux lines at the MAXC = 8 instances of their resident
kernels (k_batch_resident_flux, k_batch_resident_flux_src, k_batch_resident_hz, k_batch_resident_hz_flux), box and
periodic, with everything they carry at slots 4 and 5 of the cell walk.

The rows, lines, point cells, probes, window, members and the driver are those of tests/test_batch_wide_lines_cpu.py, which
proves on the CPU that each row is resident at 6 cells per thread with its sums in LDS, which slot and thread own every
item, and that every sum, trace and window value of the stand-in is live: "pml" 61x89 (layer 6) and 163x33 (layer 4),
periodic 163x33 (layer 4) and 61x89 (layer 6), float32, seven arrays.  Per row: a row line at slot 5, a row line at slot 4
that crosses the column line at C - 2 (slots 3, 4 and 5; one cell on two lines), a column line at column 0 of a periodic
row (column 1 of a box) across slots 4 and 5; point sources at one thread's slots 0, 3 and 5 (the last on a line), a lone
slot-4 cell, another thread's slot 0 and a slot-5 cell of the last line (column 0 and its image in a periodic row); probes
on all of them and on a slot-5 cell of the last column; a 3 x 6 window at slot 4 or higher; a conductivity patch at slot
4; line sources with both parts on every line cell.  Three members (five in the plain Hz family) run 24 steps from a
random uploaded state as run(13), run(11), the lines sampling every third step.

Tolerances, those of tests/test_gpu_batch_flux.py for its reasons: fields, Ezx or Hzx and probe traces bit-identical to the
stand-in (exact build); the window DFT and the raw line sums differ by the device's sin and cos against NumPy's alone, 1e-12
max|stand-in| per array; the flux is a sum of products of two such factors, 4e-12 dx sum|E||H| per line.

Launches of the box MAXC = 8 instances made here, per family: test_the_wide_row_matches_the_stand_in runs both box rows
in the modes "lds" and "global" (2 launches each; "streamed" runs the streamed pair); the placement test adds
steps_per_launch = 7 (4 launches) and the split (1, 12, 11) (3 launches) on 61x89; the Hz tests add the pole-free box
without conductivity against the Ez kernels' MAXC = 8 box instances; the line-source family adds the one-cell line.

Mutants (by hand on an MI355X, none committed).  Each fails test_the_wide_row_matches_the_stand_in of its family in the
resident modes (each run was stopped at four failures: both box rows, "lds" and "global", for 1 to 5, both periodic rows
for 6, while the streamed cases before them passed); "own module" is what the family's earlier module did with it:
  1. fmask >> (4 * (q & 3)) at the read in k_batch_resident_flux: the flux rows.  Own module: not
     run, since there the mutant indexes the sums of the 150x33 member past their end; its column-0 line at slot 4
     would take slot 0's nibble.
  2. hmask >> (2 * (q & 3)) in k_batch_resident_flux_src: the line-source rows.  Own module: its 150x33 member fails.
  3. pts >> (q & 3) & 1 in k_batch_resident_hz: the Hz rows.  Own module: the capacity test's largest seven-array
     member fails (its slot-0 point source acts at slot 4 too); nothing else does.
  4. fmask as unsigned short in k_batch_resident_hz_flux: the Hz-flux rows.  Own module: passes (the column-0 line of its
     130x33 member ends at slot 3).
  5. the MAXC = 4 box instance in resident[0][1] of batch_flux.hip's table: the flux box rows.  Own module: passes.
  6. lw = l - 1 at slots >= 5 of the periodic MAXC = 8 flux body: the flux periodic rows.  Own module: passes."""
import numpy as np
import pytest

import test_batch_wide_lines_cpu as wide
from test_batch_wide_lines_cpu import DT, DX, FAMILIES, LINED, N, ROWS, SPLITS, row_id

pytestmark = pytest.mark.gpu

LDS_LIMIT = wide.LDS_LIMIT
MODES = ("lds", "global", "streamed")
BOX, PERIODIC = ROWS[0], ROWS[2]                  # "pml" 61x89 and periodic 163x33
HZ = ("hz", "hzflux")
NAMES = {False: ("Ez", "Hx", "Hy", "Ezx"), True: ("Hz", "Ex", "Ey", "Hzx")}


@pytest.fixture(scope="module")
def fd():
    import fdtd2d_amd
    return fdtd2d_amd


def _exact_only(fd):
    if fd.ARITHMETIC != "exact":
        pytest.skip("the stand-in restates the exact build's arithmetic")


def _engine(fd, family, r, count=None):
    b = fd.BatchEngine(count or wide.members(family), r.R, r.C, DT, DX, dtype=np.float32, boundary=r.boundary)
    return b.set_polarization("hz") if family in HZ else b


def _expect_capacity(b, family, r, mode, lined):
    """The capacity rule as tests/test_batch_wide_lines_cpu.py restates it, against the library's own figures."""
    fam = family if lined else "hz"               # without lines: the tables of a line-free family
    resident = mode != "streamed"
    assert b.resident == resident
    assert b.lds_bytes == wide.lds_bytes(r, fam, allowed=mode != "global")
    factors = wide.field_bytes(r) - 7 * wide._seg(r.R * r.C, 4)
    assert b.resident_max_cells == (LDS_LIMIT - factors - wide.lds_table_bytes(r, fam)) // 7 // 16 * 16 // 4
    # six cells per thread, from the library's own capacity: the MAXC = 8 instance
    nthr = wide.resident_threads(r.R * r.C)
    assert 4 * nthr < r.R * r.C <= min(b.resident_max_cells, 8 * nthr) and -(-r.R * r.C // nthr) == 6
    assert b.window_in_lds == resident
    assert b.flux_lines_in_lds == (lined and mode in ("lds", "spl7", "split"))
    assert b.info(21) == (4 if lined else 0)
    assert b.polarization == ("hz" if family in HZ else "ez") and (family in HZ or b.lossy)


_runs = {}


def _device(fd, family, r, mode):
    """mode: "lds", "global", "streamed", "spl7" (resident, 7 steps per launch), "split" (resident, run(1), run(12),
    run(11)) or "nolines" (resident, the same members without the lines)."""
    key = (family, r, mode)
    if key not in _runs:
        lined = family in LINED and mode != "nolines"
        splits = (1, 12, 11) if mode == "split" else SPLITS
        with _engine(fd, family, r) as b:
            b.set_option(resident=0 if mode == "streamed" else None, steps_per_launch=7 if mode == "spl7" else None)
            b.set_flux_lds(mode != "global")
            out = wide.drive(b, family, r, splits=splits, with_lines=lined)
            _expect_capacity(b, family, r, "lds" if mode == "nolines" else mode, lined)
            if family == "linesrc":
                assert b.info(23) == (wide.K if lined else 0)
            # a resident run is one launch (per steps_per_launch), a streamed one two launches per step
            spl = 7 if mode == "spl7" else N
            assert out["launches"] == (2 * N if mode == "streamed" else sum(-(-k // spl) for k in splits))
        _runs[key] = out
    return _runs[key]


def _same(a, b, keys):
    for x, y in zip(a["fields"], b["fields"]):
        if not np.array_equal(x, y):
            return False
    return len(a["fields"]) == len(b["fields"]) and all(np.array_equal(a[k], b[k]) for k in keys)


def _keys(family):
    return ("dft", "probes") + (("E", "H", "P") if family in LINED else ())


ALL = [(f, r, m) for f in FAMILIES for r in ROWS for m in MODES]


# ---- 1. against the stand-in, on every path ------------------------------------------------------------------------------

@pytest.mark.parametrize("family,r,mode", ALL, ids=[f"{f}-{row_id(r)}-{m}" for f, r, m in ALL])
def test_the_wide_row_matches_the_stand_in(fd, family, r, mode):
    _exact_only(fd)
    got, want = _device(fd, family, r, mode), wide.stand_in(family, r)
    assert got["launches"] == (2 * N if mode == "streamed" else 2)
    assert len(got["fields"]) == len(want["fields"]) == 4
    for name, a, w in zip(NAMES[family in HZ], got["fields"], want["fields"]):
        assert a.dtype == w.dtype == np.float32 and np.array_equal(a, w), name
    assert np.array_equal(got["probes"], want["probes"])
    for name in ("dft",) + (("E", "H") if family in LINED else ()):
        err, top = np.abs(got[name] - want[name]).max(), np.abs(want[name]).max()
        print(f"{family} {row_id(r)} {mode} {name}: max error {err:.3e}, max |stand-in| {top:.3e}, ratio {err / top:.2e}")
        assert top > 0 and err <= 1e-12 * top, name
    if family in LINED:
        err = np.abs(got["P"] - want["P"])
        print(f"{family} {row_id(r)} {mode} P: worst error over its scale {np.max(err / want['scale']):.2e}")
        assert np.all(want["scale"] > 0) and np.all(err <= 4e-12 * want["scale"])
        # the crossing cell: one Ez (Hz) on two lines
        at = wide.entries(r)
        first, second = (k for k, c in enumerate(at) if c == (wide.lines(r)[1][1], r.C - 2))
        centre = "H" if family == "hzflux" else "E"
        assert np.array_equal(got[centre][:, :, first], got[centre][:, :, second])


# ---- 2. whatever the path, the placement and the launch split ----------------------------------------------------------------

CASES = [(f, r) for f in FAMILIES for r in ROWS]


@pytest.mark.parametrize("family,r", CASES, ids=wide.CASE_IDS)
def test_wide_rows_do_not_depend_on_path_placement_or_split(fd, family, r):
    first = _device(fd, family, r, "lds")
    assert all(np.abs(a).max() > 0 for a in first["fields"])
    for mode in MODES[1:] + (("spl7", "split") if r in (BOX, PERIODIC) else ()):
        assert _same(first, _device(fd, family, r, mode), _keys(family)), mode


# ---- 3. duality, device against device, between the two MAXC = 8 instances -----------------------------------------------------

@pytest.mark.parametrize("r", [BOX, PERIODIC], ids=row_id)
@pytest.mark.parametrize("family", HZ)
def test_a_wide_hz_row_equals_the_ez_kernels_with_exchanged_materials(fd, family, r):
    """Pole-free and without conductivity: Hz = Ez, Ex = -Hx, Ey = -Hy, Hzx = Ezx, and with lines Hz_hat = Ez_hat,
    Et_hat = -Ht_hat and P equal, bit for bit."""
    _exact_only(fd)
    cfg = wide.config(family, r)
    state = wide.state_of(family, cfg)
    with _engine(fd, family, r) as b:
        hz = wide.drive(b, family, r, sigma=False)
        assert b.resident and b.polarization == "hz" and not b.lossy
    dual = dict(cfg, eps=cfg["mu"], mu=cfg["eps"])
    with _engine(fd, "flux", r, count=wide.members(family)) as b:
        ez = wide.drive(b, "flux", r, cfg=dual, sigma=False, with_lines=family == "hzflux",
                        state=[state[0], -state[1], -state[2], state[3]])
        assert b.resident and b.polarization == "ez" and b.resident_max_cells > 4 * 1024
    for name, a, w, sign in zip(NAMES[True], hz["fields"], ez["fields"], (1, -1, -1, 1)):
        assert np.abs(a).max() > 0 and np.array_equal(a, sign * w), name
    assert np.array_equal(hz["dft"], ez["dft"]) and np.array_equal(hz["probes"], ez["probes"])
    if family == "hzflux":
        assert np.array_equal(hz["H"], ez["E"]) and np.abs(ez["E"]).min() > 0
        assert np.array_equal(hz["E"], -ez["H"]) and np.abs(ez["H"]).min() > 0
        assert np.array_equal(hz["P"], ez["P"]) and np.all(ez["P"] != 0)


# ---- 4. a one-cell line with an E part alone is a point source, at slot 5 -------------------------------------------------------

@pytest.mark.parametrize("resident", [None, 0], ids=["resident", "streamed"])
@pytest.mark.parametrize("r,cell", [(BOX, (58, 60)), (PERIODIC, (157, 0))], ids=[row_id(BOX), row_id(PERIODIC)])
def test_a_one_cell_electric_line_at_slot_5_equals_a_point_source(fd, r, cell, resident):
    assert wide.slot(r, cell) == 5
    cfg = wide.config("linesrc", r)
    w = cfg["we"][:, :1, :]
    one = dict(cfg, we=w, points=np.array([cell]), weights=w)
    outs = []
    for kind in ("line", "point"):
        with _engine(fd, "linesrc", r) as b:
            b.set_option(resident=resident)
            outs.append(wide.drive(b, "linesrc", r, cfg=one, line_list=[("row", cell[0], cell[1], 1)], we=kind == "line",
                                   wh=False, points=kind == "point"))
            assert b.resident == (resident is None) and b.info(23) == (wide.K if kind == "line" else 0)
    a, c = outs
    assert a["launches"] == c["launches"] == (2 if resident is None else 2 * N)
    silent = wide.stand_in("linesrc", r, channels=False)["fields"][0]
    assert np.all(a["fields"][0][:, cell[0], cell[1]] != silent[:, cell[0], cell[1]])      # the source acted
    assert _same(a, c, _keys("linesrc"))


# ---- 5. the lines never change anything ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", ROWS, ids=row_id)
@pytest.mark.parametrize("family", ["flux", "hzflux"])
def test_lines_at_high_slots_change_no_field(fd, family, r):
    """The flux instance's MAXC = 8 body against the family's plain one (the lossy PML or periodic kernels, the Hz
    kernels), on the same members."""
    with_lines, without = _device(fd, family, r, "lds"), _device(fd, family, r, "nolines")
    assert np.abs(with_lines["P"]).max() > 0 and "P" not in without
    assert _same(with_lines, without, ("dft", "probes"))
