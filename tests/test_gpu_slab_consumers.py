"""GPU: the consumers of the single-grid loop -- running transform, point probe -- on row slabs: through fdtd2d_run_slab
(tests/local_slabs.py: one thread per rank) and through SlabRunner (tests/dist_harness.py: one process per rank), over
several cycles, with windows and cells next to and across the cuts, on ranks without window rows, in float64 and with the
PML.  Fields and series bit for bit against oracle/fdtd_numpy.py and oracle/pml_numpy.py, transforms to the project's
relative 1e-12 of max|want| against the float64 sum over the oracle's Ez sequence; in the fused build the reference is a
single Engine of the same build (its PML paths agree to rounding only: pml_bound).  And the refusals that keep a pass issued in pieces from running over a sampled step.

Shapes: 3 slabs x 37 rows x 300 columns are the shortest slabs that run overlapped 16-step cycles (two 16-row edge pieces
and a 21-row zone: 2 * 16 + 5), 3 x 40 x 300 run 8-step cycles on the 16-row halo, 220 x 260 in two slabs is the PML grid
of tests/test_gpu_slab.py (40-cell layer).  Every test asserts the cycle, the overlap flag and the passes counted."""
import functools
import os

import numpy as np
import pytest

from test_gpu_consumers import DT, DX, OMEGA16, assert_dft, assert_fields, dft_want, mur_reference, mur_state

pytestmark = pytest.mark.gpu

OM3 = OMEGA16[[1, 8, 14]]
MUR16, MUR8 = (111, 300), (120, 300)          # 3 x 37 rows (cuts at 37, 74), 3 x 40 rows (cuts at 40, 80)
NP_DTYPE = {"f32": np.float32, "f64": np.float64}


# ---- references -------------------------------------------------------------------------------------------------------------

def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _engine_sequence(fd, st, n, src, boundary="mur"):
    """The fused build's reference: a single Engine of the same build, step by step."""
    R, C = st["Ez"].shape
    seq = []
    with fd.Engine(R, C, DT, DX, dtype=st["Ez"].dtype, boundary=boundary) as eng:
        eng.set_materials(st["eps"], st["mu"])
        if boundary == "pml":
            eng.set_pml()
        eng.upload(st["Ez"], st["Hx"], st["Hy"])
        for k in range(n):
            eng.run(1, src[0], src[1], st["amps"][k:k + 1])
            seq.append(eng.download()[0])
        ref = list(eng.download())
    return np.array(seq), ref


@functools.lru_cache(maxsize=None)
def mur_case(shape, dtype, materials, n=50):
    """State (with dt, dx for run_local_slabs), source on the first cut, the Ez sequence and the final fields."""
    import fdtd2d_amd as fd
    R, C = shape
    st = mur_state(R, C, NP_DTYPE[dtype], materials, n=n)
    src = (R // 3, C // 2)
    if fd.ARITHMETIC == "exact":
        seq, _, ref = mur_reference(st, n, src + (1, 1))
    else:
        seq, ref = _engine_sequence(fd, st, n, src)
    assert np.abs(seq[-1]).max() > 0
    _freeze(seq, *ref, *(v for v in st.values() if isinstance(v, np.ndarray)))
    return dict(st, dt=DT, dx=DX), src, seq, ref


PML_SHAPE, PML_SRC = (220, 260), (110, 58)


@functools.lru_cache(maxsize=None)
def pml_case(n=50):
    """220 x 260, random fields (Ezx zero, as the slab upload leaves it), eps array, vacuum at [0, 0]; source on the cut."""
    import fdtd2d_amd as fd
    from oracle import fdtd_numpy as onp
    from oracle import pml_numpy as pm
    r, c = PML_SHAPE
    rng = np.random.default_rng(220)
    st = {"Ez": rng.standard_normal((r, c)).astype(np.float32), "Hx": (rng.standard_normal((r, c - 1)) * 1e-3).astype(np.float32),
          "Hy": (rng.standard_normal((r - 1, c)) * 1e-3).astype(np.float32),
          "eps": (onp.EPS0 * rng.uniform(1, 3, (r, c))).astype(np.float32), "mu": np.full((r, c), onp.MU0).astype(np.float32),
          "amps": rng.standard_normal(n)}
    st["eps"][0, 0] = np.float32(onp.EPS0)
    if fd.ARITHMETIC == "exact":
        S = (1 / np.sqrt(fd.EPS0 * fd.MU0) * DT) / DX
        seq = []
        full = [st["Ez"].copy(), np.zeros((r, c), np.float32), st["Hx"].copy(), st["Hy"].copy()]
        pm.leapfrog(*full, st["eps"], st["mu"], DT, DX, n, PML_SRC[0], PML_SRC[1], st["amps"], pm.profiles(r, c, S, dtype=np.float32),
                    on_step=lambda i, E, *_: seq.append(E.copy()))
        seq, ref = np.array(seq), [full[0], full[2], full[3]]
    else:
        seq, ref = _engine_sequence(fd, st, n, PML_SRC, "pml")
    assert np.abs(seq[-1]).max() > 0
    _freeze(seq, *ref, *(v for v in st.values() if isinstance(v, np.ndarray)))
    return dict(st, dt=DT, dx=DX), seq, ref


def pml_bound(n=50):
    """0 in the exact build.  The fused build's PML kernels do not contract the same multiply-add pairs (the single-step
    kernels leave the choice to the compiler, the passes write their fused forms out), so its slabs -- passes on one rank,
    single steps on the rank with a probe -- agree with its single engine to rounding only: tests/test_gpu_pml_passes.py's
    fused_bound, 16 n eps of the field's maximum (at most 8 roundings of eps / 2 of the largest term per step, adding
    linearly: the scheme does not amplify; a factor 4 for terms above the final maximum)."""
    import fdtd2d_amd as fd
    return 0.0 if fd.ARITHMETIC == "exact" else 16 * n * float(np.finfo(np.float32).eps)


def assert_pml_fields(got, ref):
    if pml_bound() == 0:
        return assert_fields(got, ref)
    for a, b, k in zip(got, ref, ("Ez", "Hx", "Hy")):
        assert np.abs(a.astype(np.float64) - b).max() <= pml_bound() * np.abs(b).max(), k


def assert_pml_series(series, seq, cell):
    want = seq[:, cell[0], cell[1]].astype(np.float64)
    assert series.shape == want.shape and np.abs(want).max() > 0
    if pml_bound() == 0:
        assert np.array_equal(series, want), np.flatnonzero(series != want)[:8]
    else:
        assert np.abs(series - want).max() <= pml_bound() * np.abs(seq).max()


def assert_pml_parts(parts, win, want, seq, nsamples=3):
    """Exact build: the project's 1e-12.  Fused build: each of the samples differs by at most pml_bound() of the field's
    maximum per cell, on top of it."""
    if pml_bound() == 0:
        return assert_parts(parts, PML_SHAPE, win, 3, want)
    got = np.concatenate(parts, axis=1)
    assert got.shape == want.shape and np.abs(want).max() > 0
    err = np.abs(got - want).max() / np.abs(want).max()
    print("transform: relative error", err)
    assert err <= 1e-12 + nsamples * pml_bound() * np.abs(seq).max() / np.abs(want).max(), err


def local_run(shape, dtype, st, src, chunks, *, cycle_opt, materials="array", boundary="mur", overlap=True, dft=None, dft_after=None,
              probe=None):
    """run_local_slabs with a transform set on EVERY rank (before the first chunk, or after chunk number dft_after) and a
    probe set on the rank that owns its row.  Returns fields, cycle, overlapped, launches, the ranks' read_dft() parts and
    the owner's series."""
    import fdtd2d_amd as fd
    from local_slabs import run_local_slabs

    def owner(eng):
        return probe is not None and eng.owned_rows[0] <= probe[0] < eng.owned_rows[1]

    def setup(k, eng):
        if owner(eng):
            eng.set_probe(probe[0], probe[1], sum(chunks))
        if dft is not None and dft_after is None:
            eng.set_dft(*dft)

    def between(k, eng, i):
        if dft is not None and i == dft_after:
            eng.set_dft(*dft)

    def collect(k, eng):
        return (eng.read_dft() if dft is not None else None, eng.read_probe() if owner(eng) else None, eng.step_count)

    got, cycle, overlapped, launches, hooks = run_local_slabs(
        fd, len(PLAN[shape]), shape, NP_DTYPE[dtype], boundary, st, sum(chunks), src, cycle_opt=cycle_opt, overlap=overlap,
        materials="uniform" if materials == "uniform" else "array", setup=setup, between=between, collect=collect, chunks=chunks)
    assert [c[2] for c in hooks["collect"]] == [sum(chunks)] * len(PLAN[shape])
    series = [c[1] for c in hooks["collect"] if c[1] is not None]
    return got, cycle, overlapped, launches, [c[0] for c in hooks["collect"]], series[0] if series else None


PLAN = {MUR16: [(0, 37), (37, 74), (74, 111)], MUR8: [(0, 40), (40, 80), (80, 120)], PML_SHAPE: [(0, 110), (110, 220)]}


def assert_parts(parts, shape, win, nfreq, want):
    """Each rank's part has the rows of the window it owns -- (F, 0, ncols) where it owns none --, and together, along the
    row axis, they are the whole window."""
    for (a, b), p in zip(PLAN[shape], parts):
        own = max(0, min(b, win[0] + win[2]) - max(a, win[0]))
        assert p.shape == (nfreq, own, win[3]), (a, b, p.shape)
    assert_dft(np.concatenate(parts, axis=1), want)


# ---- (a) window geometry over the cuts ----------------------------------------------------------------------------------------

WINDOWS = {"across_both_cuts": (30, 0, 50, 300),        # tail of rank 0, all of rank 1, head of rank 2, the Mur columns
           "two_rows_at_a_cut": (36, 7, 2, 250),        # the last owned row of rank 0 and the first one of rank 1
           "inside_rank_1": (45, 20, 20, 200),          # ranks 0 and 2 own nothing
           "top_zone": (0, 0, 21, 300)}                 # rows 0..20 of rank 0


@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("materials", ["both", "uniform"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_transform_window_over_the_cuts(dtype, materials, window):
    """The C loop, 50 steps = three overlapped 16-step cycles and a plain tail of 2, samples at 16, 32 and 48."""
    st, src, seq, ref = mur_case(MUR16, dtype, materials)
    win = WINDOWS[window]
    got, cycle, overlapped, launches, parts, _ = local_run(MUR16, dtype, st, src, [50], cycle_opt=16, materials=materials,
                                                           dft=(win, OM3, 16))
    assert cycle == 16 and overlapped and min(launches) > 0
    assert_fields(got, ref)
    assert_parts(parts, MUR16, win, 3, dft_want(seq, win, OM3, 16))


# ---- (b) the sampling grid against the cycle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,cycle_opt,every,chunks,dft_after", [
    (MUR16, 16, 32, [50], None), (MUR16, 16, 48, [50], None),
    (MUR8, None, 16, [50], None),                # two 8-step cycles per sample
    (MUR16, 16, 16, [16, 34], 0),                # set after the first chunk: counted from step 16
    (MUR16, 16, 16, [8, 40], 0),                 # ... from step 8: the cycles are aligned to that step, not to step 0
], ids=["every32", "every48", "cycle8_every16", "set_at_16", "set_at_8"])
def test_transform_sampling_grid_against_the_cycle(shape, cycle_opt, every, chunks, dft_after):
    st, src, seq, ref = mur_case(shape, "f32", "both")
    n = sum(chunks)
    step0 = 0 if dft_after is None else chunks[0]
    win = (shape[0] // 3 - 7, 3, shape[0] // 3 + 14, 290)       # from rank 0 over rank 1 into rank 2
    got, cycle, overlapped, launches, parts, _ = local_run(shape, "f32", st, src, chunks, cycle_opt=cycle_opt,
                                                           dft=(win, OM3, every), dft_after=dft_after)
    assert cycle == (16 if cycle_opt else 8) and overlapped and min(launches) > 0
    if n == 50:
        assert_fields(got, ref)
    else:
        assert np.array_equal(got[0], seq[n - 1])
    want = dft_want(seq[:n], win, OM3, every, step0=step0)
    assert_parts(parts, shape, win, 3, want)


# ---- (c) refusals ---------------------------------------------------------------------------------------------------------------

class TopSlab:
    """The first of three 37-row slabs as one handle with a transport that records its calls and moves nothing (the
    message buffers are zeros: the halo rows it 'receives' are zeros, which is a state like any other here)."""

    def __init__(self, fd, dtype=np.float32, boundary="mur"):
        import hipmem
        st = mur_state(MUR16[0], MUR16[1], dtype, "uniform", n=32)
        self.st, self.called = st, []
        self.eng = fd.Engine(MUR16[0], MUR16[1], DT, DX, dtype=dtype, boundary=boundary, slab=(0, 37, 16))
        self.eng.set_materials(float(st["eps"][0, 0]), float(st["mu"][0, 0]))
        if boundary == "pml":
            self.eng.set_pml()
        self.eng.set_option(max_pass_steps=16)
        self.eng.upload(st["Ez"][:37], st["Hx"][:37], st["Hy"][:37])
        self.bufs = hipmem.DevBuf(self.eng.halo_bytes), hipmem.DevBuf(self.eng.halo_bytes)
        self.eng.slab_attach({1: (self.bufs[0].ptr, self.bufs[1].ptr)}, lambda *a: self.called.append(a) or 0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()
        for b in self.bufs:
            b.free()


def assert_nothing_pending(eng):
    from fdtd2d_amd import _abi
    with pytest.raises(_abi.Fdtd2dError) as e:
        eng.pass_commit()
    assert e.value.code == _abi.E_STATE and "no partial pass is pending" in str(e.value)


@pytest.mark.parametrize("every", [5, 8])
def test_c_loop_refuses_a_transform_off_the_cycle(every):
    """every % cycle != 0: FDTD2D_E_ARG before anything is posted."""
    import fdtd2d_amd as fd
    from fdtd2d_amd import _abi
    with TopSlab(fd) as s:
        s.eng.set_dft((20, 0, 30, 300), OM3, every)
        with pytest.raises(_abi.Fdtd2dError) as e:
            s.eng.run_slab(16, 16, True, 37, 150, s.st["amps"])
        assert e.value.code == _abi.E_ARG and not s.called and s.eng.step_count == 0
        assert_nothing_pending(s.eng)


def test_c_loop_refuses_a_cycle_that_would_cross_a_sample():
    """every = 16, run_slab(8) and then run_slab(16): the second call's overlapped cycle would run from step 8 to step 24,
    over the sample at 16.  It returns FDTD2D_E_ARG and names the step count and the cycle; the transport is not called,
    the step count, the fields and the sums are what they were, nothing is pending -- and the run can go on with 8-step cycles up to the sample, then with 16-step ones."""
    import fdtd2d_amd as fd
    from fdtd2d_amd import _abi
    with TopSlab(fd) as s:
        eng = s.eng
        eng.set_dft((20, 0, 30, 300), OM3, 16)
        eng.run_slab(8, 16, True, 30, 150, s.st["amps"])
        calls = len(s.called)
        assert calls == 1 and eng.step_count == 8
        before = eng.download(), eng.read_dft()
        assert np.abs(before[0][0]).max() > 0 and before[1].shape == (3, 17, 300)
        with pytest.raises(_abi.Fdtd2dError) as e:
            eng.run_slab(16, 16, True, 30, 150, s.st["amps"][8:])
        assert e.value.code == _abi.E_ARG and "8 steps" in str(e.value) and "16-step cycle" in str(e.value), str(e.value)
        assert len(s.called) == calls and eng.step_count == 8
        after = eng.download(), eng.read_dft()
        assert_fields(after[0], before[0])
        assert np.array_equal(after[1], before[1])
        assert_nothing_pending(eng)
        eng.run_slab(8, 8, True, 30, 150, s.st["amps"][8:])           # an 8-step cycle is aligned here and ends on the sample
        assert eng.step_count == 16 and np.abs(eng.read_dft()).max() > 0
        eng.run_slab(16, 16, True, 30, 150, s.st["amps"][16:])        # aligned again: an overlapped cycle
        assert eng.step_count == 32


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pass_rows_refuses_a_pass_over_a_sampled_step(dtype):
    """A whole grid advanced by passes issued in pieces.  every = 5, and every = 16 from a misaligned step: a 16-step pass
    is refused with FDTD2D_E_ARG before anything is launched, nothing is pending, the fields are untouched.  Passes that
    end before the sampled step (4 of a gap of 8) or ON it (4 of a gap of 4) are accepted, and the commit of the latter
    takes the sample."""
    import fdtd2d_amd as fd
    from fdtd2d_amd import _abi
    R, C = MUR16
    st, src, seq, _ = mur_case(MUR16, dtype, "both")
    win = (10, 5, 90, 280)
    with fd.Engine(R, C, DT, DX, dtype=NP_DTYPE[dtype]) as eng:
        eng.set_materials(st["eps"], st["mu"]).set_option(max_pass_steps=16)
        eng.upload(st["Ez"], st["Hx"], st["Hy"])
        assert eng.cycle_steps == 16
        eng.set_dft(win, OM3, 5)
        with pytest.raises(_abi.Fdtd2dError) as e:
            eng.pass_rows(16, 0, R, src[0], src[1], st["amps"])
        assert e.value.code == _abi.E_ARG
        assert_nothing_pending(eng)
        assert_fields(eng.download(), [st[k] for k in ("Ez", "Hx", "Hy")])
        eng.set_dft(win, OM3, 16)
        eng.run(8, src[0], src[1], st["amps"])
        p0 = eng.info(16)
        with pytest.raises(_abi.Fdtd2dError) as e:
            eng.pass_rows(16, 0, R, src[0], src[1], st["amps"][8:])
        assert e.value.code == _abi.E_ARG and eng.step_count == 8 and eng.info(16) == p0
        assert_nothing_pending(eng)
        assert np.array_equal(eng.download()[0], seq[7]) and not eng.read_dft().any()
        for k in (8, 12):                              # gap 8, then gap 4: in two pieces each
            eng.pass_rows(4, 0, 60, src[0], src[1], st["amps"][k:])
            eng.pass_rows(4, 60, R, src[0], src[1], st["amps"][k:])
            eng.pass_commit()
        assert eng.step_count == 16 and eng.info(16) > p0
        assert np.array_equal(eng.download()[0], seq[15])
        assert_dft(eng.read_dft(), dft_want(seq[:16], win, OM3, 16))


def test_every_rank_refuses_a_misaligned_chunk():
    """Three ranks, every = 16, chunks of 8 and 16 steps: every rank's second call returns the same FDTD2D_E_ARG before it
    posts anything, so none is left waiting for a neighbour."""
    import fdtd2d_amd as fd
    from fdtd2d_amd import _abi
    from local_slabs import run_local_slabs
    st, src, _, _ = mur_case(MUR16, "f32", "both")
    with pytest.raises(_abi.Fdtd2dError) as e:
        run_local_slabs(fd, 3, MUR16, np.float32, "mur", st, 24, src, cycle_opt=16, chunks=[8, 16],
                        setup=lambda k, eng: eng.set_dft((30, 0, 50, 300), OM3, 16))
    per_rank = e.value.per_rank
    assert [k for k, _ in per_rank] == [0, 1, 2]
    assert all(isinstance(x, _abi.Fdtd2dError) and x.code == _abi.E_ARG for _, x in per_rank), per_rank
    assert len({str(x) for _, x in per_rank}) == 1 and "16-step cycle" in str(e.value)


# ---- (d) SlabRunner: the Python-sequenced loop and the C loop, one process per rank ---------------------------------------------

RUNNER_SHAPE, RUNNER_WIN, RUNNER_SRC = (170, 600), (70, 250, 31, 120), (80, 300)      # cut at row 85: window rows 70..100


@functools.lru_cache(maxsize=None)
def runner_case(dtype="f32"):
    import fdtd2d_amd as fd
    R, C = RUNNER_SHAPE
    st = mur_state(R, C, NP_DTYPE[dtype], "eps", n=50)
    if fd.ARITHMETIC == "exact":
        seq, _, ref = mur_reference(st, 50, RUNNER_SRC + (1, 1))
    else:
        seq, ref = _engine_sequence(fd, st, 50, RUNNER_SRC)
    _freeze(seq, *ref)
    return st, seq, ref


def runner_job(tmp_path, st, dtype="float32", **kw):
    from dist_harness import run_job
    path = os.path.join(str(tmp_path), "state.npz")
    np.savez(path, **st)
    job = dict(engine="hip", shape=RUNNER_SHAPE, dtype=dtype, dt=DT, dx=DX, state=path, src=RUNNER_SRC, chunks=[50],
               materials="array", overlap=True, options={"max_pass_steps": 16}, expect_cycle=16)
    job.update(kw)
    got = run_job(2, job, str(tmp_path))
    parts = [np.load(os.path.join(str(tmp_path), f"dft_rank{k}.npy")) for k in range(2)] if job.get("dft") else None
    probe = os.path.join(str(tmp_path), "probe.npy")
    return got, parts, np.load(probe) if os.path.exists(probe) else None


@pytest.mark.parametrize("loop,overlap,probe_row", [("python", True, 100), ("c", True, 85), ("python", False, None)],
                         ids=["python", "c_probe_85", "python_plain"])
def test_runner_transform_across_the_cut(tmp_path, loop, overlap, probe_row):
    """Two ranks, 170 x 600, cut at row 85, window rows 70..100, every = 16, 50 steps: overlapped 16-step cycles in the
    Python loop and in the C loop, and plain cycles; where a probe is set too, its series (capacity = the 50 steps)."""
    st, seq, ref = runner_case()
    got, parts, series = runner_job(tmp_path, st, loop=loop, overlap=overlap, expect_overlap=overlap,
                                    dft=(RUNNER_WIN, OM3, 16), probe=(probe_row, 301) if probe_row else None)
    assert_fields(got, ref)
    assert [p.shape for p in parts] == [(3, 15, 120), (3, 16, 120)]
    assert_dft(np.concatenate(parts, axis=1), dft_want(seq, RUNNER_WIN, OM3, 16))
    if probe_row:
        want = seq[:, probe_row, 301].astype(np.float64)
        assert series.shape == (50,) and np.abs(want).max() > 0 and np.array_equal(series, want)


def test_runner_refuses_a_misaligned_chunk_on_both_ranks(tmp_path):
    """Chunks of 24 and 16 steps with every = 16 (and an every = 8 that set_dft refuses first): the second run() raises
    ValueError on both ranks before it touches the engine, and what the first chunk left -- fields, transform with the
    sample of step 16 -- stays."""
    st, seq, _ = runner_case()
    got, parts, _ = runner_job(tmp_path, st, loop="python", chunks=[24, 16], refuse=[1], dft=(RUNNER_WIN, OM3, 16), dft_refused=8)
    for k in range(2):
        text = open(os.path.join(str(tmp_path), f"refused_rank{k}.txt")).read().splitlines()
        assert len(text) == 2 and text[0].startswith("set_dft: ") and text[1].startswith("chunk 1: "), text
    assert np.array_equal(got[0], seq[23]) and np.abs(seq[23]).max() > 0
    assert_dft(np.concatenate(parts, axis=1), dft_want(seq[:24], RUNNER_WIN, OM3, 16))


# ---- (e) the probe on slabs -------------------------------------------------------------------------------------------------------

def test_runner_probe_in_the_c_loop_on_the_last_row_before_the_cut(tmp_path):
    """Probe row 84 (rank 0's last owned row) in the C loop, transform set as well."""
    st, seq, ref = runner_case()
    got, parts, series = runner_job(tmp_path, st, loop="c", expect_overlap=True, dft=(RUNNER_WIN, OM3, 16), probe=(84, 301))
    assert_fields(got, ref)
    assert_dft(np.concatenate(parts, axis=1), dft_want(seq, RUNNER_WIN, OM3, 16))
    assert series.shape == (50,) and np.array_equal(series, seq[:, 84, 301].astype(np.float64))


def test_runner_agrees_on_8_step_cycles_for_a_float64_probe(tmp_path):
    """float64's 16-step kernel has no probe tile: the rank that holds the probe runs 8-step passes from set_probe on, so
    the runner must agree on the cycle again -- a runner that kept 16 asked that rank for 16-step pieces it cannot issue."""
    st, seq, ref = runner_case("f64")
    got, _, series = runner_job(tmp_path, st, dtype="float64", loop="python", expect_overlap=True, expect_cycle=8, probe=(85, 301))
    assert_fields(got, ref)
    assert np.array_equal(series, seq[:, 85, 301].astype(np.float64)) and np.abs(series).max() > 0


def test_float64_probe_handle_refuses_overlapped_16_step_cycles_before_the_transport():
    """The same on one handle: with a probe a float64 handle reports 8-step cycles, and run_slab(cycle = 16, overlap = 1)
    returns FDTD2D_E_ARG before anything is posted (it used to fail inside its first cycle, after the exchange)."""
    import fdtd2d_amd as fd
    from fdtd2d_amd import _abi
    with TopSlab(fd, dtype=np.float64) as s:
        assert s.eng.cycle_steps == 16
        s.eng.set_probe(20, 150, 16)
        assert s.eng.cycle_steps == 8
        with pytest.raises(_abi.Fdtd2dError) as e:
            s.eng.run_slab(16, 16, True, 30, 150, s.st["amps"])
        assert e.value.code == _abi.E_ARG and not s.called and s.eng.step_count == 0
        assert_nothing_pending(s.eng)


@pytest.mark.parametrize("where", ["first_owned", "last_owned", "interior"])
@pytest.mark.parametrize("shape,dtype,cycle_opt", [(MUR16, "f32", 16), (MUR16, "f64", 16), (MUR8, "f32", None)],
                         ids=["f32_cycle16", "f64_asked16", "f32_cycle8"])
def test_probe_on_the_middle_rank_of_three(shape, dtype, cycle_opt, where):
    """The middle rank's first owned row, its last one and one inside, a transform over the cuts set on the same run.
    float64 with 16-step passes asked for: the handle with the probe reports 8 (no probe tile in float64's 16-step
    kernel), so 8 is what the ranks agree on."""
    st, src, seq, ref = mur_case(shape, dtype, "both")
    a, b = PLAN[shape][1]
    cell = ({"first_owned": a, "last_owned": b - 1, "interior": (a + b) // 2}[where], 151)
    win = (a - 5, 100, b - a + 10, 100)
    got, cycle, overlapped, launches, parts, series = local_run(shape, dtype, st, src, [50], cycle_opt=cycle_opt, probe=cell,
                                                                dft=(win, OM3, 16))
    assert cycle == (16 if cycle_opt and dtype == "f32" else 8) and overlapped and min(launches) > 0
    want = seq[:, cell[0], cell[1]].astype(np.float64)
    assert series.shape == (50,) and np.abs(want).max() > 0
    assert np.array_equal(series, want), np.flatnonzero(series != want)[:8]
    assert_fields(got, ref)
    assert_parts(parts, shape, win, 3, dft_want(seq, win, OM3, 16))


# ---- (f) PML slabs ------------------------------------------------------------------------------------------------------------------

PML_WIN = (95, 0, 30, 61)         # rows 95..124 over the cut at 110, columns 0..60: the 40-cell column layer and beyond


def test_pml_transform_in_the_c_loop():
    """Overlapped 16-step cycles on the level-split PML pair, every = 16."""
    st, seq, ref = pml_case()
    got, cycle, overlapped, launches, parts, _ = local_run(PML_SHAPE, "f32", st, PML_SRC, [50], cycle_opt=16, boundary="pml",
                                                           dft=(PML_WIN, OM3, 16))
    assert cycle == 16 and overlapped and min(launches) > 0
    assert_pml_fields(got, ref)
    assert_pml_parts(parts, PML_WIN, dft_want(seq, PML_WIN, OM3, 16), seq)


def test_pml_transform_in_the_python_loop(tmp_path):
    st, seq, ref = pml_case()
    got, parts, _ = runner_job(tmp_path, {k: v for k, v in st.items() if k not in ("dt", "dx")}, shape=PML_SHAPE, src=PML_SRC,
                               boundary="pml", loop="python", expect_overlap=True, dft=(PML_WIN, OM3, 16))
    assert_pml_fields(got, ref)
    assert [p.shape for p in parts] == [(3, 15, 61), (3, 15, 61)]
    assert_pml_parts(parts, PML_WIN, dft_want(seq, PML_WIN, OM3, 16), seq)


@pytest.mark.parametrize("cell", [(109, 30), (110, 130)], ids=["rank0_in_the_layer", "rank1_first_row"])
def test_pml_probe_with_plain_cycles_on_every_rank(cell):
    """A PML handle with a probe takes no pass (no probe tile): overlap = 0 on every rank, as SlabRunner does; the rank
    with the probe reports 8-step cycles and advances by single steps (no pass counted), the other one runs passes."""
    st, seq, ref = pml_case()
    got, cycle, overlapped, launches, _, series = local_run(PML_SHAPE, "f32", st, PML_SRC, [50], cycle_opt=16, boundary="pml",
                                                            overlap=False, probe=cell)
    owner = 0 if cell[0] < 110 else 1
    assert cycle == 8 and not overlapped and launches[owner] == 0 and launches[1 - owner] > 0
    assert_pml_series(series, seq, cell)
    assert_pml_fields(got, ref)


def test_pml_probe_handle_refuses_overlapped_cycles_before_the_transport():
    """run_slab(overlap = 1) on the handle that holds a PML probe: an error before anything is posted."""
    import fdtd2d_amd as fd
    from fdtd2d_amd import _abi
    with TopSlab(fd, boundary="pml") as s:
        s.eng.set_probe(20, 150, 16)
        assert s.eng.cycle_steps == 8
        with pytest.raises(_abi.Fdtd2dError) as e:
            s.eng.run_slab(16, 8, True, 30, 150, s.st["amps"])
        assert e.value.code == _abi.E_ARG and "overlap = 0" in str(e.value) and not s.called and s.eng.step_count == 0
        assert_nothing_pending(s.eng)
        s.eng.run_slab(16, 8, False, 30, 150, s.st["amps"])
        assert len(s.called) == 2 and s.eng.step_count == 16 and s.eng.read_probe().shape == (16,)
