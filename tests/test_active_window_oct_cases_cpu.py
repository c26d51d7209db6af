"""CPU-only: every row of tests/active_window_oct_cases.py keeps what it is listed for, from the C oracle and the restated
rules alone -- so that tests/test_gpu_active_window_oct.py compares non-zero cells where a wrongly skipped task would
have left zeros.

Per row: after every segment the oracle's non-zero cells lie inside the restated bounds and come within ONE cell of each
bounded side (the one cell is the source of a run, which commit_pass grows one too far; zero cells for add_point); every
pass launches a window (the half-grid cap, asserted by simulate); the restated count of skipped tasks is positive where
the row is listed for it, and zero once the bounds are dropped."""
import os
import re

import numpy as np
import pytest

import active_window_oct_cases as oc
import active_window_cases as awc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fdtd-2d_amd", "csrc")
IDS = [r["name"] for r in oc.ROWS]


def test_restated_rules_are_the_library_s():
    aw = open(os.path.join(CSRC, "active_window.hpp")).read()
    assert "static constexpr int BIG = 1 << 29;" in aw
    assert "return Oct{r.r0 + r.c0, r.r1 - 1 + r.c1 - 1, r.r0 - (r.c1 - 1), r.r1 - 1 - r.c0};" in aw
    assert "return r.empty() || (r.r0 >= MARGIN && r.r1 <= R - MARGIN && r.c0 >= MARGIN && r.c1 <= C - MARGIN);" in aw
    assert "support_oct = grow(hull(old_oct, Oct::of(clip(src))), nsteps);" in aw
    assert "return hull(grow(hull(support_oct, Oct::of(clip(src))), nsteps), dirty_oct);" in aw
    ks = open(os.path.join(CSRC, "kernels_stream.hpp")).read()
    assert ("return rb - 1 + cb - 1 >= p.oct_s0 && ra + ca <= p.oct_s1 && rb - 1 - ca >= p.oct_d0 && ra - (cb - 1) <= p.oct_d1;"
            in ks)
    assert oc.oct_of((500, 501, 990, 991)) == (1490, 1490, -490, -490)
    assert oc.grow_oct(oc.UNBOUNDED, 16) == oc.UNBOUNDED and oc.grow_oct((10, 20, -5, 5), 3) == (7, 23, -8, 8)
    assert oc.hull(None, (1, 2, 3, 4)) == (1, 2, 3, 4) and oc.hull((0, 9, 0, 9), (1, 12, -3, 4)) == (0, 12, -3, 9)
    # a task touching the s0 line with its last cell meets; one cell further out it does not
    assert oc.meets((100, 200, -50, 50), 0, 51, 0, 51) and not oc.meets((101, 200, -50, 50), 0, 51, 0, 51)


def test_new_info_ids_are_declared_and_bound():
    import inspect
    from fdtd2d_amd import _abi, engine
    txt = open(os.path.join(ROOT, "include", "fdtd2d.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"#define\s+FDTD2D_(OCT_INFO_\w+)\s+(\d+)", txt)}
    assert sorted(ids.values()) == list(range(42, 47))
    for k, v in ids.items():
        assert getattr(_abi, k) == v, k
    assert int(re.search(r"#define\s+FDTD2D_OPT_WINDOW_OCTAGON\s+(\d+)", txt).group(1)) == _abi.OPT_WINDOW_OCTAGON == 10
    src = inspect.getsource(engine.Engine.last_window_octagon.fget)
    assert re.findall(r'"(\w+)"', src.split("keys = ")[1].split(")")[0]) == ["sum_lo", "sum_hi", "diff_lo", "diff_hi", "skipped"]
    assert _abi.OCT_UNBOUNDED == oc.BIG


@pytest.mark.parametrize("name", IDS)
def test_the_field_touches_the_bounds_and_tasks_are_skipped(name):
    row = oc.by_name(name)
    sim = oc.simulate(row)
    ref = oc.reference(name)
    exact = any(s[0] == "add_point" for s in row["segments"])
    total = 0
    for k, (seg, s, state) in enumerate(zip(row["segments"], sim, ref)):
        o, got = s["oct"], oc.span(state)
        print(name, "segment", k, seg[:4], "window", s["window"], "bounds", o, "non-zero span", got,
              "skipped/tasks", [(len(l["skipped"]), len(l["tasks"])) for l in s["launches"]])
        assert got is not None and o is not None
        # the rectangle holds the field (what tests/test_active_window_cases_cpu.py proves for its own rows)
        box = awc.support_box(state)
        w = s["window"]
        assert w[0] <= box[0] and box[1] <= w[1] and w[2] <= box[2] and box[3] <= w[3]
        slack = 0 if exact else 1
        for side in range(4):
            if abs(o[side]) >= oc.BIG:
                continue
            inward = (got[side] - o[side]) * (1 if side % 2 == 0 else -1)
            assert 0 <= inward <= slack, f"segment {k}: bound {side} at {o[side]}, the field reaches {got[side]}"
        for l in s["launches"]:
            total += len(l["skipped"])
            if l["oct"] == oc.UNBOUNDED:
                assert not l["skipped"]
            # a skipped task never holds a cell of the final state of its segment's last pass
        last = s["launches"][-1] if s["launches"] else None
        if last and last["skipped"]:
            ow = awc.strip_ow(row["dtype"], last["nt"])
            for st, ra, rb in last["skipped"]:
                for a in state:
                    assert not a[ra:rb, st * ow:(st + 1) * ow].any(), f"skipped task {(st, ra, rb)} holds non-zero cells"
    if row["skips"]:
        assert total > 0
    if row["lost"]:
        assert sim[-1]["oct"] == oc.UNBOUNDED and not sim[-1]["launches"][-1]["skipped"]
        assert any(l["oct"] != oc.UNBOUNDED for l in sim[0]["launches"])
    if row["n_src"] is not None:
        assert sim[-1]["launches"][-1]["n_src"] == row["n_src"]


def test_stale_copy_skips_nothing_once():
    sim = oc.simulate(oc.by_name("stale_copy"))
    after = sim[2]["launches"]
    assert sim[0]["launches"][-1]["skipped"] and not after[0]["skipped"] and after[0]["oct"] == oc.UNBOUNDED
    assert after[1]["skipped"] and after[1]["oct"] != oc.UNBOUNDED


def test_a_bound_one_too_tight_would_drop_non_zero_cells():
    """The net bites: on the exact row, the last pass of a segment has a task that bounds one cell too tight would skip
    and that holds non-zero cells of the oracle's state -- the GPU comparison would see zeros there."""
    row = oc.by_name("exact_point_16")
    sim, ref = oc.simulate(row), oc.reference("exact_point_16")
    hits = 0
    for s, state in zip(sim[1:], ref[1:]):
        l = s["launches"][-1]
        o = l["oct"]
        tight = (o[0] + 1, o[1] - 1, o[2] + 1, o[3] - 1)
        ow = awc.strip_ow(row["dtype"], l["nt"])
        more = [t for t in oc.skipped(row, l, None, tight) if t not in l["skipped"]]
        hits += sum(1 for st, ra, rb in more if any(a[ra:rb, st * ow:(st + 1) * ow].any() for a in state))
        print("pass", l["nt"], "bounds", o, "tasks a tight bound would also skip", more)
    assert hits > 0


def test_the_table_covers_what_it_is_for():
    every = [(r, l) for r in oc.ROWS for s in oc.simulate(r) for l in s["launches"]]
    assert {l["nt"] for _, l in every} == {8, 16, 20}
    assert {r["dtype"] for r in oc.ROWS} == {oc.F32, oc.F64}
    assert {l["n_src"] for _, l in every if l["skipped"]} == {0, 1, 2}
    assert any(l["xcd_map"] and l["skipped"] for _, l in every)
    assert any(l["waves"] == 4 and l["skipped"] for _, l in every)
    assert any(l["edge_rows"] != l["band_rows"] and l["skipped"] for _, l in every)
    assert any(l["nlev"] < l["nt"] and l["skipped"] for _, l in every)
    assert any(r["kind"] == "eps" and l["skipped"] for r, l in every)
    # skipped tasks of all three kinds: edge strips, source strips, inner strips
    ns = lambda r, l: -(-r["shape"][1] // awc.strip_ow(r["dtype"], l["nt"]))
    assert any(t[0] in (0, ns(r, l) - 1) for r, l in every for t in l["skipped"])
