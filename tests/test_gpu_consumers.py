"""GPU: the device-side consumers next to the single-grid loop -- the probe tile k_probe at every instance, clip and Mur
class of tests/test_consumers_cpu.py, k_probe_copy, the probe's bookkeeping, the running transform k_dft at its edges,
both on a PML engine, k_reduce after passes and k_snapshot on a constructed field -- against oracle/fdtd_numpy.py and
oracle/pml_numpy.py: series and fields bit for bit, transforms to the project's relative 1e-12 of max|want|."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_consumers_cpu as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX = 5e-14, 1e-4
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
INFO_EPS_UNIFORM, INFO_MU_UNIFORM, INFO_PASSES = 9, 10, 16
OMEGA16 = 2 * np.pi * np.linspace(11e9, 83e9, 16)


# ---- states and references ---------------------------------------------------------------------------------------------------

def mur_state(R, C, dtype, materials, n=tc.STEPS):
    """Random fields, materials with the stated arrays (the other one constant), amplitudes; seeded by its arguments."""
    from oracle import fdtd_numpy as onp
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng([R, C, np.dtype(dtype).itemsize, tc.MATERIALS.index(materials)])
    st = {"Ez": rng.standard_normal((R, C)).astype(dtype),
          "Hx": (rng.standard_normal((R, C - 1)) * 1e-3).astype(dtype),
          "Hy": (rng.standard_normal((R - 1, C)) * 1e-3).astype(dtype),
          "amps": rng.standard_normal(n)}
    eps = onp.EPS0 * (rng.uniform(1, 10, (R, C)) if materials in ("eps", "both") else np.full((R, C), 2.0))
    mu = onp.MU0 * (rng.uniform(1, 3, (R, C)) if materials in ("mu", "both") else np.ones((R, C)))
    st["eps"], st["mu"] = eps.astype(dtype), mu.astype(dtype)
    return st


def mur_reference(st, n, src, keep=()):
    """The oracle's n steps from st with the patch source src = (row, col, rows, cols): the Ez sequence (n, R, C), the
    fields after the steps in `keep`, the final fields."""
    from oracle import fdtd_numpy as onp
    seq, kept = [], {}

    def on_step(i, E, Hx, Hy):
        seq.append(E.copy())
        if i + 1 in keep:
            kept[i + 1] = (E.copy(), Hx.copy(), Hy.copy())
    ref = [st[k].copy() for k in ("Ez", "Hx", "Hy")]
    onp.leapfrog(*ref, st["eps"], st["mu"], DT, DX, n, src[0], src[1], amps=st["amps"], extent=src[2:], on_step=on_step)
    return np.array(seq), kept, ref


@functools.lru_cache(maxsize=None)
def table_reference(R, C, dtype, materials):
    """One oracle run per (grid, dtype, materials) of the table, shared by its rows: Ez at the table's cells per step."""
    st = mur_state(R, C, NP_DTYPE[dtype], materials)
    seq, kept, ref = mur_reference(st, tc.STEPS, tc.SOURCE[R, C], keep=(37,))
    cells = {(c.row, c.col) for c in tc.CASES if (c.R, c.C) == (R, C)}
    series = {rc: seq[:, rc[0], rc[1]].astype(np.float64) for rc in cells}
    for a in list(st.values()) + list(ref) + [x for v in kept.values() for x in v]:
        a.setflags(write=False)
    return st, series, kept, ref


def dft_want(seq, window, omegas, every, step0=0):
    """The float64 sum over the oracle's Ez sequence (seq[k - 1] = Ez after step k): samples at the steps k > step0 with
    (k - step0) % every == 0, phases from the absolute step count."""
    r0, c0, nr, nc = window
    want = np.zeros((len(omegas), nr, nc), np.complex128)
    for k in range(step0 + 1, len(seq) + 1):
        if (k - step0) % every == 0:
            w = seq[k - 1][r0:r0 + nr, c0:c0 + nc].astype(np.float64)
            for f, om in enumerate(omegas):
                want[f] += w * np.cos(om * (k * DT)) + 1j * (w * -np.sin(om * (k * DT)))
    return want


def assert_dft(got, want):
    assert got.shape == want.shape and np.abs(want).max() > 0
    err = np.abs(got - want).max() / np.abs(want).max()
    print("transform: relative error", err)
    assert err <= 1e-12, err


def mur_engine(fd, st, max_pass_steps, src=None):
    R, C = st["Ez"].shape
    eng = fd.Engine(R, C, DT, DX, dtype=st["Ez"].dtype)
    eng.set_materials(st["eps"], st["mu"]).set_option(max_pass_steps=max_pass_steps)
    if src is not None:
        eng.set_source_extent(*src[2:])
    eng.upload(st["Ez"], st["Hx"], st["Hy"])
    return eng


def assert_fields(got, ref, names=("Ez", "Hx", "Hy")):
    for a, b, k in zip(got, ref, names):
        assert np.array_equal(a, b), f"{k} differs at {np.argwhere(a != b)[:4].tolist()}"


# ---- the probe tile: every row of the table ----------------------------------------------------------------------------------

@pytest.mark.parametrize("c", tc.CASES, ids=tc.case_id)
def test_probe_table_row_matches_oracle(c):
    """45 steps from a random state with a patch source, the probe set after 3 of them: the series and the final fields
    equal the oracle's bit for bit, the passes counted are the planned ones of the stated length (a row that falls back
    to single steps, or to another kernel length, fails), the material instance is the stated one."""
    import fdtd2d_amd as fd
    st, series, _, ref = table_reference(c.R, c.C, c.dtype, c.materials)
    cyc = tc.cycle_steps(c.dtype, c.max_pass_steps)
    plan = tc.planned_passes(tc.STEPS - tc.LEAD, cyc)
    _, ce_arr, ch_arr = tc.instance(c)
    with mur_engine(fd, st, c.max_pass_steps, c.source) as eng:
        assert (eng.info(INFO_EPS_UNIFORM), eng.info(INFO_MU_UNIFORM)) == (not ce_arr, not ch_arr)
        eng.run(tc.LEAD, c.source[0], c.source[1], st["amps"][:tc.LEAD])
        eng.set_probe(c.row, c.col, tc.STEPS)
        assert eng.cycle_steps == cyc
        p0 = eng.info(INFO_PASSES)
        eng.run(tc.STEPS - tc.LEAD, c.source[0], c.source[1], st["amps"][tc.LEAD:])
        assert eng.info(INFO_PASSES) - p0 == len(plan) and eng.last_pass_steps == plan[-1][0]
        got = eng.read_probe()
        whole = eng.read_probe(0, tc.STEPS)
        fields = eng.download()
    want = series[c.row, c.col][tc.LEAD:]
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert not whole[tc.STEPS - tc.LEAD:].any()
    assert_fields(fields, ref)


# ---- the probe's bookkeeping -------------------------------------------------------------------------------------------------

BOOK = [("f32", 16), ("f32", 8), ("f32", 0), ("f64", 16), ("f64", 0)]


@pytest.mark.parametrize("dtype,max_steps", BOOK)
def test_probe_capacity_shorter_than_the_run(dtype, max_steps):
    """Capacity 20, runs of 16 + 16 + 5 steps: the second run's pass crosses the capacity inside the tile's loop
    (q.base + step - 1 < q.cap), the third starts beyond it (q.base >= q.cap, idx >= probe_cap)."""
    import fdtd2d_amd as fd
    R, C, cell = 76, 64, (38, 31)
    st, series, kept, _ = table_reference(R, C, dtype, "both")
    src = tc.SOURCE[R, C]
    with mur_engine(fd, st, max_steps, src) as eng:
        eng.set_probe(cell[0], cell[1], 20)
        n, p0 = 0, eng.info(INFO_PASSES)
        for k in (16, 16, 5):
            eng.run(k, src[0], src[1], st["amps"][n:n + k])
            n += k
        assert (eng.info(INFO_PASSES) > p0) == (max_steps > 0)
        got = eng.read_probe(0, 20)
        with pytest.raises(fd.Fdtd2dError):
            eng.read_probe(0, 21)
        with pytest.raises(fd.Fdtd2dError):
            eng.read_probe(20, 1)
        fields = eng.download()
    assert np.array_equal(got, series[cell][:20])
    assert_fields(fields, kept[37])


@pytest.mark.parametrize("dtype,max_steps", BOOK + [("f32", 4)])
def test_probe_kept_over_uneven_runs_reset_and_removed(dtype, max_steps):
    """run(7), run(16), run(1) with one probe; re-set to another cell: its series starts at the re-set step and the
    buffer is zero beyond what was recorded; removed: read_probe is refused and the run goes on, equal to the oracle."""
    import fdtd2d_amd as fd
    R, C, a, b = 76, 64, (38, 31), (73, 20)
    st, series, _, ref = table_reference(R, C, dtype, "both")
    src = tc.SOURCE[R, C]
    with mur_engine(fd, st, max_steps, src) as eng:
        n = 0

        def run(k):
            nonlocal n
            eng.run(k, src[0], src[1], st["amps"][n:n + k])
            n += k
        eng.set_probe(a[0], a[1], 64)
        for k in (7, 16, 1):
            run(k)
        assert eng.read_probe().shape == (24,)
        got_a = eng.read_probe(0, 64)
        eng.set_probe(b[0], b[1], 30)
        assert not eng.read_probe(0, 30).any()
        run(13)
        got_b = eng.read_probe(0, 30)
        eng.set_probe(b[0], b[1], 0)
        with pytest.raises(fd.Fdtd2dError):
            eng.read_probe(0, 1)
        run(8)
        assert eng.step_count == tc.STEPS
        fields = eng.download()
    assert np.array_equal(got_a[:24], series[a][:24]) and not got_a[24:].any()
    assert np.array_equal(got_b[:13], series[b][24:37]) and not got_b[13:].any()
    assert_fields(fields, ref)


# ---- probe and transform together ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("every,max_steps", [(5, 16), (16, 16), (5, 8), (16, 8)])
@pytest.mark.parametrize("cell", [(20, 25), (2, 30)], ids=["in_window", "top_band"])
def test_probe_and_transform_together(dtype, every, max_steps, cell):
    """The passes are cut at the sampled steps and the tile records inside each short pass."""
    import fdtd2d_amd as fd
    R, C, win = 76, 64, (0, 10, 40, 40)
    st = mur_state(R, C, NP_DTYPE[dtype], "eps")
    src = tc.SOURCE[R, C]
    seq, _, ref = _together_reference(dtype)
    om = OMEGA16[[3, 9]]
    with mur_engine(fd, st, max_steps, src) as eng:
        eng.set_probe(cell[0], cell[1], tc.STEPS)
        eng.set_dft(win, om, every)
        eng.run(30, src[0], src[1], st["amps"][:30])
        eng.run(15, src[0], src[1], st["amps"][30:])
        assert eng.info(INFO_PASSES) > 0
        series, got, fields = eng.read_probe(), eng.read_dft(), eng.download()
    assert np.array_equal(series, seq[:, cell[0], cell[1]].astype(np.float64))
    assert_fields(fields, ref)
    assert_dft(got, dft_want(seq, win, om, every))


@functools.lru_cache(maxsize=None)
def _together_reference(dtype):
    st = mur_state(76, 64, NP_DTYPE[dtype], "eps")
    return mur_reference(st, tc.STEPS, tc.SOURCE[76, 64])


# ---- the transform's edges ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _edge_reference(R, C):
    st = mur_state(R, C, np.float32, "eps", n=40)
    return (st,) + mur_reference(st, 40, (R // 2, C // 2, 1, 1))


EDGES = [((76, 64), "whole", 16, 5), ((76, 64), "row", 3, 16), ((76, 64), "col", 16, 7),
         ((150, 300), "whole", 16, 16), ((150, 300), "row", 2, 5), ((150, 300), "col", 2, 1)]


@pytest.mark.parametrize("shape,kind,nfreq,every", EDGES)
def test_transform_window_shapes_and_sixteen_frequencies(shape, kind, nfreq, every):
    """The whole grid, one row, one column; 16 frequencies; a 17th is refused and changes nothing: the 16 go on."""
    import fdtd2d_amd as fd
    R, C = shape
    st, seq, _, ref = _edge_reference(R, C)
    win = {"whole": (0, 0, R, C), "row": (R - 1, 0, 1, C), "col": (0, C - 1, R, 1)}[kind]
    om = OMEGA16[:nfreq]
    with mur_engine(fd, st, 16) as eng:
        eng.set_dft(win, om, every)
        eng.run(25, R // 2, C // 2, st["amps"][:25])
        with pytest.raises(fd.Fdtd2dError):
            eng.set_dft(win, np.concatenate([OMEGA16, [2 * np.pi * 90e9]]), every)
        with pytest.raises(fd.Fdtd2dError):
            eng.set_dft((0, 0, R + 1, C), om, every)
        eng.run(15, R // 2, C // 2, st["amps"][25:])
        assert eng.info(INFO_PASSES) > 0
        got, fields = eng.read_dft(), eng.download()
    assert_fields(fields, ref)
    assert_dft(got, dft_want(seq, win, om, every))


@pytest.mark.parametrize("shape", [(76, 64), (150, 300)])
def test_transform_without_a_sample_and_set_again_mid_run(shape):
    """every = steps + 1: no sample, all zeros.  set_dft again after 20 steps: the sums restart from zero, the samples
    are counted from that step, the phases stay those of the absolute step count."""
    import fdtd2d_amd as fd
    R, C = shape
    st, seq, _, ref = _edge_reference(R, C)
    win, om = (3, 5, R - 20, C - 11), OMEGA16[[0, 15, 7]]
    with mur_engine(fd, st, 16) as eng:
        eng.set_dft(win, om, 41)
        eng.run(40, R // 2, C // 2, st["amps"])
        none = eng.read_dft()
        assert_fields(eng.download(), ref)
        assert none.shape == (3, win[2], win[3]) and not none.any()
    for every in (6, 16):
        with mur_engine(fd, st, 16) as eng:
            eng.set_dft(win, om, 4)
            eng.run(20, R // 2, C // 2, st["amps"][:20])
            assert np.abs(eng.read_dft()).max() > 0
            eng.set_dft(win, om, every)
            assert not eng.read_dft().any()
            eng.run(20, R // 2, C // 2, st["amps"][20:])
            got = eng.read_dft()
            assert_fields(eng.download(), ref)
        assert_dft(got, dft_want(seq, win, om, every, step0=20))


def test_transform_on_a_slab_that_owns_half_of_the_window():
    """A top slab (rows 0..69 of 130) whose bottom halo comes from the handle below it, no transport: the window's rows
    50..89 are half owned, read_dft has the owned rows' shape, and after one committed 16-step pass it holds the oracle's
    sample of step 16 at those rows."""
    import fdtd2d_amd as fd
    import hipmem
    R, C, H = 130, 200, 16
    st = mur_state(R, C, np.float32, "uniform", n=16)
    seq, _, _ = mur_reference(st, 16, (40, 90, 1, 1))
    win, om = (50, 20, 40, 150), OMEGA16[[2, 11]]
    eps, mu = float(st["eps"][0, 0]), float(st["mu"][0, 0])
    with fd.Engine(R, C, DT, DX, dtype=np.float32, slab=(0, 70, H)) as top, \
            fd.Engine(R, C, DT, DX, dtype=np.float32, slab=(70, 60, H)) as below:
        for eng, (a, b) in ((top, (0, 70)), (below, (70, 130))):
            eng.set_materials(eps, mu).set_option(max_pass_steps=16)
            eng.upload(st["Ez"][a:b], st["Hx"][a:b], st["Hy"][a:min(b, R - 1)])
        buf = hipmem.DevBuf(top.halo_bytes)
        below.halo_pack(0, buf.ptr)
        below.sync()
        top.halo_unpack(1, buf.ptr)
        top.set_dft(win, om, 16)
        assert top.read_dft().shape == (2, 20, 150)
        top.pass_rows(16, 0, 70, 40, 90, st["amps"])
        top.pass_commit()
        got = top.read_dft()
        Ez = top.download()[0]
        below.set_dft(win, om, 16)
        assert below.read_dft().shape == (2, 20, 150)
        buf.free()
    assert np.array_equal(Ez, seq[15][:70])
    assert_dft(got, dft_want(seq, (50, 20, 20, 150), om, 16))


# ---- the PML engine ---------------------------------------------------------------------------------------------------------------

PML_SHAPE, PML_L, PML_S, PML_SRC = (96, 130), 20, 0.15, (30, 50)


@functools.lru_cache(maxsize=None)
def pml_reference(dtype):
    from oracle import fdtd_numpy as onp
    from oracle import pml_numpy as pm
    r, c = PML_SHAPE
    dt_ = NP_DTYPE[dtype]
    rng = np.random.default_rng(96 + np.dtype(dt_).itemsize)
    st = {"Ez": rng.standard_normal((r, c)).astype(dt_), "Ezx": (0.3 * rng.standard_normal((r, c))).astype(dt_),
          "Hx": (rng.standard_normal((r, c - 1)) * 1e-3).astype(dt_), "Hy": (rng.standard_normal((r - 1, c)) * 1e-3).astype(dt_),
          "eps": (onp.EPS0 * rng.uniform(1, 4, (r, c))).astype(dt_), "mu": np.full((r, c), onp.MU0).astype(dt_),
          "amps": rng.standard_normal(tc.STEPS)}
    P = pm.profiles(r, c, PML_S, L=PML_L, dtype=dt_)
    seq, kept = [], {}

    def on_step(i, E, Ezx, Hx, Hy):
        seq.append(E.copy())
        if i + 1 == 37:
            kept[37] = (E.copy(), Ezx.copy(), Hx.copy(), Hy.copy())
    ref = [st[k].copy() for k in ("Ez", "Ezx", "Hx", "Hy")]
    pm.leapfrog(*ref, st["eps"], st["mu"], DT, DX, tc.STEPS, PML_SRC[0], PML_SRC[1], st["amps"], P, on_step=on_step)
    return st, np.array(seq), kept, ref


def pml_engine(fd, st, max_steps):
    r, c = PML_SHAPE
    eng = fd.Engine(r, c, DT, DX, dtype=st["Ez"].dtype, boundary="pml")
    eng.set_materials(st["eps"], st["mu"]).set_pml(L=PML_L, courant00=PML_S).set_option(max_pass_steps=max_steps)
    eng.upload(st["Ez"], st["Hx"], st["Hy"]).upload_ezx(st["Ezx"])
    return eng


def pml_fields(eng):
    got = eng.download()
    return got[0], eng.download_ezx(), got[1], got[2]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("max_steps", [16, 8, 0])
@pytest.mark.parametrize("cell", [(5, 60), (19, 64), (48, 110), (48, 65)], ids=["layer", "inner_edge_row", "inner_edge_col", "interior"])
def test_pml_probe_falls_back_to_single_steps(dtype, max_steps, cell):
    """With a probe set a PML engine has no probe tile: no pass is taken, every sample is k_probe_copy's, and
    cycle_steps says 8 or less; series and fields (Ez, Ezx, Hx, Hy) bit for bit."""
    import fdtd2d_amd as fd
    st, seq, _, ref = pml_reference(dtype)
    with pml_engine(fd, st, max_steps) as eng:
        eng.run(tc.LEAD, *PML_SRC, st["amps"][:tc.LEAD])
        eng.set_probe(cell[0], cell[1], tc.STEPS)
        assert eng.cycle_steps <= 8
        p0 = eng.info(INFO_PASSES)
        eng.run(tc.STEPS - tc.LEAD, *PML_SRC, st["amps"][tc.LEAD:])
        assert eng.info(INFO_PASSES) == p0
        got = eng.read_probe()
        fields = pml_fields(eng)
    assert np.array_equal(got, seq[tc.LEAD:, cell[0], cell[1]].astype(np.float64))
    assert_fields(fields, ref, ("Ez", "Ezx", "Hx", "Hy"))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("every,max_steps", [(5, 16), (16, 16), (5, 8), (16, 8)])
def test_pml_transform_over_layer_cells(dtype, every, max_steps):
    """No probe: the passes are cut at the sampled steps.  every = 16 runs full passes (the float32 16-step pair, else
    k_pass_pml's 8 steps); every = 5 runs 5-level short passes of the float32 16-step pair.  k_pass_pml has no short
    passes (launch_pass: "short passes run on the level-split kernels only"), so with every = 5 the configurations on
    the 8-step kernel (float64, or max_pass_steps = 8) cannot take a pass at all: asserted as such, their fields and
    transform are checked all the same."""
    import fdtd2d_amd as fd
    st, seq, _, ref = pml_reference(dtype)
    win, om = (10, 30, 40, 95), OMEGA16[[1, 14]]
    pair = dtype == "f32" and max_steps == 16
    with pml_engine(fd, st, max_steps) as eng:
        assert eng.cycle_steps == (16 if pair else 8)
        eng.set_dft(win, om, every)
        eng.run(30, *PML_SRC, st["amps"][:30])
        eng.run(15, *PML_SRC, st["amps"][30:])
        if every == 16:
            assert eng.info(INFO_PASSES) == 4 and eng.last_pass_steps == (16 if pair else 8)
        elif pair:
            assert eng.info(INFO_PASSES) == 9 and eng.last_pass_steps == 16
        else:
            assert eng.info(INFO_PASSES) == 0
        got = eng.read_dft()
        fields = pml_fields(eng)
    assert_fields(fields, ref, ("Ez", "Ezx", "Hx", "Hy"))
    assert_dft(got, dft_want(seq, win, om, every))


# ---- reductions ---------------------------------------------------------------------------------------------------------------------

def assert_reduce(eng, what):
    fields = eng.download()
    for name, a in zip(("Ez", "Hx", "Hy"), fields):
        s, m = eng.reduce(name)
        assert m == np.abs(a).max(), (what, name, m, np.abs(a).max())
        assert s == pytest.approx(np.sum(a.astype(np.float64) ** 2), rel=1e-12), (what, name)
    return fields


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", ["mur-130x470", "pml-96x130", "mur-76x64"])
def test_reduce_after_passes_reset_and_a_previous_life(dtype, grid):
    """reduce of Ez, Hx, Hy = the downloaded fields reduced in float64 on the host -- after 37 steps run as passes from
    1e3-scale fields (the spare column of Hx and the spare row of Hy, which download() never shows, must not enter), after
    reset(), and after small fields were uploaded over that previous life and advanced, in either buffer of the pair."""
    import fdtd2d_amd as fd
    if grid.startswith("pml"):
        st, _, kept, _ = pml_reference(dtype)
        src, make, want37 = PML_SRC + (1, 1), lambda: pml_engine(fd, st, 16), [kept[37][k] for k in (0, 2, 3)]
    else:
        R, C = (int(v) for v in grid[4:].split("x"))
        st, _, kept, _ = table_reference(R, C, dtype, "both")
        src, make, want37 = tc.SOURCE[R, C], lambda: mur_engine(fd, st, 16, tc.SOURCE[R, C]), kept[37]
    with make() as eng:
        eng.run(37, src[0], src[1], st["amps"])
        assert eng.info(INFO_PASSES) > 0
        assert_fields(assert_reduce(eng, "small, 37 steps"), want37)
        big = [st[k] * st[k].dtype.type(1e3) for k in ("Ez", "Hx", "Hy")]
        eng.upload(*big)
        assert_reduce(eng, "large, uploaded")
        eng.run(37, src[0], src[1], 1e3 * st["amps"])
        assert_reduce(eng, "large, 37 steps")
        eng.run(8, src[0], src[1], 1e3 * st["amps"])
        assert_reduce(eng, "large, 45 steps")
        eng.reset()
        for name in ("Ez", "Hx", "Hy"):
            assert eng.reduce(name) == (0.0, 0.0), name
        eng.upload(*(st[k] * st[k].dtype.type(1e-3) for k in ("Ez", "Hx", "Hy")))
        assert_reduce(eng, "small over large, uploaded")
        for k in (16, 21, 8):
            eng.run(k)
            assert_reduce(eng, f"small over large, {k} more steps")


SLAB = (37, 50, 16)


@pytest.fixture(scope="module")
def slab_engine():
    """The middle slab of a 130 x 200 grid, its owned rows uploaded, its halo rows filled with 1e3-scale values from
    the handles above and below it."""
    import fdtd2d_amd as fd
    import hipmem
    R, C = 130, 200
    r0, nr, H = SLAB
    rng = np.random.default_rng(37)
    Ez = rng.uniform(-1, 1, (R, C)).astype(np.float32)
    Hx = rng.uniform(-1, 1, (R, C - 1)).astype(np.float32)
    Hy = rng.uniform(-1, 1, (R - 1, C)).astype(np.float32)
    for a in (Ez, Hx, Hy):
        a[:r0] *= 1e3
        a[r0 + nr:] *= 1e3
    engs = [fd.Engine(R, C, DT, DX, dtype=np.float32, slab=s) for s in ((0, r0, H), SLAB, (r0 + nr, R - r0 - nr, H))]
    for eng in engs:
        a, b = eng.owned_rows
        eng.set_materials()
        eng.upload(Ez[a:b], Hx[a:b], Hy[a:min(b, R - 1)])
    buf = hipmem.DevBuf(engs[1].halo_bytes)
    for side, other in ((0, engs[0]), (1, engs[2])):
        other.halo_pack(1 - side, buf.ptr)
        other.sync()
        engs[1].halo_unpack(side, buf.ptr)
        engs[1].sync()
    assert (engs[1].info(11), engs[1].info(12)) == (r0 - H, r0 + nr + H)      # the halo rows are current
    yield engs[1], Ez, Hx, Hy
    for eng in engs:
        eng.close()
    buf.free()


def test_reduce_on_a_slab_counts_owned_rows_only(slab_engine):
    eng, Ez, Hx, Hy = slab_engine
    r0, nr, _ = SLAB
    for name, a in (("Ez", Ez), ("Hx", Hx), ("Hy", Hy)):
        own = a[r0:r0 + nr]
        s, m = eng.reduce(name)
        assert m == np.abs(own).max() and m < 10, name
        assert s == pytest.approx(np.sum(own.astype(np.float64) ** 2), rel=1e-12), name


@pytest.mark.parametrize("stride", [1, 2, 3, 7, 50, 64, 100])
def test_snapshot_on_a_slab_takes_global_multiples_of_the_stride(slab_engine, stride):
    """Owned rows 37..86: rows and columns at the global multiples of the stride (row 37 is none for any stride but 1:
    the first row taken is not the slab's first); stride 100 has no owned row and gives an empty result."""
    eng, Ez, _, _ = slab_engine
    r0, nr, _ = SLAB
    rows = [i for i in range(r0, r0 + nr) if i % stride == 0]
    want = snapshot_expected(Ez[rows][:, ::stride], -0.7, 0.9) if rows else np.empty((0, (200 - 1) // stride + 1), np.uint8)
    got = eng.snapshot_index(-0.7, 0.9, stride)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert (stride == 100) == (got.shape[0] == 0)
    assert np.array_equal(got, want)


# ---- snapshot on a constructed field ----------------------------------------------------------------------------------------------

def snapshot_expected(Ez, vmin, vmax):
    """main.py:155,167-168 restated: clip, subtract, divide, x 256, truncate, 256 -> 255, in Ez's dtype (the Python
    scalars are weak).  Observed here for the special values (NumPy 2.x, x86-64): -inf and values below vmin -> 0, +inf
    and values from vmax up -> 255, -0.0 and +0.0 -> the index of 0, NaN -> 0 (NaN stays NaN through clip; its cast to
    an integer is INT64_MIN here and 0 on platforms whose conversion saturates NaN to 0 -- the final clip to 0..255 makes
    both 0, so NaN stays in)."""
    with np.errstate(invalid="ignore"):
        x = (np.clip(Ez, vmin, vmax) - vmin) / (vmax - vmin)
        y = x * 256
        idx = y.astype(np.int64)
    idx[y == 256] = 255
    return np.clip(idx, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_snapshot_bin_edges_range_ends_and_special_values(dtype):
    """Every bin edge vmin + k (vmax - vmin) / 256, k = 0..256, with its two neighbouring representable numbers; vmin,
    vmax, values beyond both, +-0, +-inf, NaN; vmin and vmax neither symmetric nor powers of two."""
    import fdtd2d_amd as fd
    dt_ = NP_DTYPE[dtype]
    vmin, vmax = -0.37, 1.93
    edges = (vmin + np.arange(257) * ((vmax - vmin) / 256)).astype(dt_)
    inf = dt_(np.inf)
    vals = np.concatenate([edges, np.nextafter(edges, -inf), np.nextafter(edges, inf),
                           np.array([vmin, vmax, vmin - 1e-3, vmax + 1e-3, -50.0, 50.0, 0.0, -0.0, np.inf, -np.inf, np.nan,
                                     np.finfo(dt_).max, -np.finfo(dt_).max, np.finfo(dt_).tiny, -np.finfo(dt_).tiny], dtype=dt_),
                           (vmin + (np.arange(256) + 0.5) * ((vmax - vmin) / 256)).astype(dt_)])      # and the middle of every bin
    R, C = 30, 37
    rng = np.random.default_rng(5)
    Ez = rng.uniform(vmin - 0.2, vmax + 0.2, R * C).astype(dt_)
    Ez[:vals.size] = vals
    Ez = rng.permutation(Ez).reshape(R, C)
    want = snapshot_expected(Ez, vmin, vmax)
    assert set(np.unique(want[np.isfinite(Ez)])) == set(range(256))                   # every bin is hit
    assert want[np.isnan(Ez)].tolist() == [0] and want[Ez == inf].tolist() == [255] and want[Ez == -inf].tolist() == [0]
    assert np.all(want[Ez == 0] == want[Ez == 0][0]) and np.signbit(Ez[Ez == 0]).sum() == 1
    with fd.Engine(R, C, DT, DX, dtype=dt_) as eng:
        eng.set_materials()
        eng.upload(Ez, np.zeros((R, C - 1), dt_), np.zeros((R - 1, C), dt_))
        for stride in (1, 3):
            got = eng.snapshot_index(vmin, vmax, stride)
            bad = np.argwhere(got != want[::stride, ::stride])
            assert bad.size == 0, [(Ez[::stride, ::stride][tuple(b)], got[tuple(b)], want[::stride, ::stride][tuple(b)]) for b in bad[:6]]


# ---- the fused build ----------------------------------------------------------------------------------------------------------------

FUSED_ROWS = ["76x64-f32-both-max16-38_31", "76x64-f32-mu-max16-75_63", "76x64-f32-mu-max16-2_33", "130x470-f64-mu-max16-60_467",
              "130x470-f32-both-max16-129_200", "130x470-f32-eps-max16-70_0"]

FUSED_CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
import fdtd2d_amd as fd
from fdtd2d_amd import _abi
import test_consumers_cpu as tc
import test_gpu_consumers as tg
assert fd.ARITHMETIC == "fused" and _abi.LIB_PATH.endswith("libfdtd2d_fused.so")
out = {}
for c in tc.CASES:
    if tc.case_id(c) not in ROWS:
        continue
    st = tg.mur_state(c.R, c.C, tg.NP_DTYPE[c.dtype], c.materials)
    res = []
    for max_steps in (16, 8, 0):
        with tg.mur_engine(fd, st, max_steps, c.source) as eng:
            eng.run(tc.LEAD, c.source[0], c.source[1], st["amps"][:tc.LEAD])
            eng.set_probe(c.row, c.col, tc.STEPS)
            p0 = eng.info(16)
            eng.run(tc.STEPS - tc.LEAD, c.source[0], c.source[1], st["amps"][tc.LEAD:])
            res.append((eng.read_probe(), eng.download(), eng.info(16) - p0, eng.last_pass_steps))
    out[tc.case_id(c)] = {"series": [bool(np.array_equal(r[0], res[2][0])) for r in res[:2]],
                          "fields": [bool(all(np.array_equal(a, b) for a, b in zip(r[1], res[2][1]))) for r in res[:2]],
                          "passes": [r[2] for r in res], "last": [r[3] for r in res[:2]],
                          "moved": bool(np.abs(res[2][0]).max() > 0 and len(res[2][0]) == tc.STEPS - tc.LEAD)}
print("FUSED_CONSUMERS " + json.dumps(out))
'''


def test_fused_build_probe_series_do_not_depend_on_the_launch_shape():
    """FDTD2D_ARITHMETIC=fused in a child process: for one row per kind of Mur class (interior, corner, top band, side
    band, edge row, edge column; both dtypes) the series recorded by the probe tile inside 16- and 8-step passes equals,
    bit for bit, the series the same build records with max_pass_steps = 0 (k_probe_copy of the stored field)."""
    kinds = {tc.mur_class(c.R, c.C, c.row, c.col) for c in tc.CASES if tc.case_id(c) in FUSED_ROWS}
    assert kinds == {"interior", "corner_br", "band_top", "band_right", "edge_row_bottom", "edge_col_left"}, kinds
    rows = [c for c in tc.CASES if tc.case_id(c) in FUSED_ROWS]
    assert len(rows) == len(FUSED_ROWS) and {c.dtype for c in rows} == {"f32", "f64"}
    head = f"ROOT = {ROOT!r}\nTESTS = {os.path.join(ROOT, 'tests')!r}\nROWS = {FUSED_ROWS!r}\n"
    p = subprocess.run([sys.executable, "-c", head + FUSED_CHILD], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FDTD2D_ARITHMETIC="fused"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("FUSED_CONSUMERS ")][-1][16:])
    assert sorted(out) == sorted(FUSED_ROWS)
    for c in rows:
        o = out[tc.case_id(c)]
        want_last = [tc.cycle_steps(c.dtype, 16), 8]
        assert o["moved"] and o["last"] == want_last and o["passes"][2] == 0 and min(o["passes"][:2]) > 0, (tc.case_id(c), o)
        assert all(o["series"]) and all(o["fields"]), (tc.case_id(c), o)
