"""Case table and runner of tests/test_gpu_fused_parity.py -- TEST INFRASTRUCTURE.

Every case drives the single-grid Mur engine (an Engine, the drop-in half steps, tests/local_slabs.py) from seeded
inputs in one launch shape and compares Ez, Hx and Hy with the C oracle by np.array_equal:
    fused=False   libfdtd2d.so        against c_oracle.*(fused=False)   (proves the table and the runner)
    fused=True    libfdtd2d_fused.so  against c_oracle.*(fused=True)    (the fused build's arithmetic, stated exactly:
                                                                         oracle/fdtd_oracle.c)
and asserts that the launch it names really ran (pass count, kernel length, launch-shape entries, windowed launches).
Shapes are the smallest at which tests/test_gpu_parity.py, test_gpu_active_window.py and test_gpu_slab.py exercise the
same seams; all cases start from an uploaded random state with H scaled by 1e-3, the active-window cases from rest."""
import numpy as np

DT, DX, FC = 5e-14, 1e-4, 30e9
NAMES = ("Ez", "Hx", "Hy")
F32, F64 = "float32", "float64"

CASES = []


def _add(name, group, driver, **kw):
    assert all(c["name"] != name for c in CASES), name
    CASES.append(dict(name=name, group=group, driver=driver, **kw))


def _tag(dtype):
    return "f32" if dtype == F32 else "f64"


def plan(n, cycle, split, long_passes=False):
    """The passes run(n) is made of, as the library plans them (kernel length, levels): full passes while more than two
    remain, a remainder between one and two passes cut in halves, the last remainder on the shortest kernel that holds
    it -- which stops early only in its level-split form (`split`); else on the longest full pass below it."""
    out, rem = [], n
    lens = [c for c in (1, 2, 4, 8, 16) if c <= cycle]
    while rem > 0:
        take = rem
        if long_passes and rem <= 20:
            if rem > 16:
                out.append((20, rem))
                break
        elif rem > 2 * cycle:
            take = cycle
        elif rem > cycle:
            take = (rem + 1) // 2
        fit = [x for x in lens if x >= take and (x == take or (split and x >= 8))]
        if fit:
            c = fit[0]
        else:
            c = take = max(x for x in lens if x < take)
        out.append((c, take))
        rem -= take
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------

for _shape in ((11, 11), (12, 13), (48, 40)):
    for _dt in (F32, F64):
        _add(f"half_steps_{_shape[0]}x{_shape[1]}_{_tag(_dt)}", "small", "half", shape=_shape, dtype=_dt, kind="eps+mu",
             seed=_shape[0] * 100 + _shape[1])

for _dt in (F32, F64):
    _add(f"single_steps_64x80_{_tag(_dt)}", "small", "engine", shape=(64, 80), dtype=_dt, kind="eps+mu", n=50, src=(21, 40),
         seed=6480, options=dict(max_pass_steps=0), expect=dict(passes=0))

# every kernel variant of the 8-step pass on one grid (test_every_kernel_variant_matches_oracle)
for _dt in (F32, F64):
    for _ls in (0, 1, 8):
        for _zs in (0, 1):
            for _kind in ("uniform", "eps"):
                _split = _ls != 0 and not (_kind == "eps" and _zs == 1)
                _p = plan(19, 8, _split)
                _add(f"variant_ls{_ls}_zs{_zs}_{_kind}_{_tag(_dt)}", "small", "engine", shape=(150, 500), dtype=_dt, kind=_kind,
                     eps_r=1.3, n=19, src=(77, 241), seed=31,
                     options=dict(level_split=min(_ls, 1), zone_split=_zs, band_rows=20, split_waves=8 if _ls == 8 else 4),
                     expect=dict(passes=len(_p), last_nt=_p[-1][0], shape={1: (8 if _ls == 8 else 4) if _split else 1}))

# ragged 8-step shapes (test_blocked_passes_match_oracle): 23 = 8 + 8 + a short pass of 7
for _shape in ((44, 16), (64, 241), (70, 497), (257, 129)):
    for _dt in (F32, F64):
        for _kind in ("uniform", "eps+mu"):
            _add(f"ragged_{_shape[0]}x{_shape[1]}_{_kind}_{_tag(_dt)}", "small", "engine", shape=_shape, dtype=_dt, kind=_kind,
                 eps_r=2.5, n=23, src=(_shape[0] // 2 + 3, _shape[1] // 3), seed=77 * _shape[0] + _shape[1],
                 options=dict(max_pass_steps=8), expect=dict(passes=3, last_nt=8))

# float32 16-step passes (test_16_step_passes_match_oracle, test_16_step_passes_array_materials): 35 = 16 + 16 + 3
for _shape in ((76, 64), (100, 225), (130, 470), (200, 1000)):
    for _nw in (4, 8):
        for _src in ((0, 0), (21, 223)):
            _s = (min(_src[0], _shape[0] - 1), min(_src[1], _shape[1] - 1))
            _add(f"f32_16_{_shape[0]}x{_shape[1]}_nw{_nw}_src{_s[0]}_{_s[1]}", "passes32", "engine", shape=_shape, dtype=F32,
                 kind="uniform", eps_r=1.9, n=35, src=_s, seed=_shape[0] * _shape[1],
                 options=dict(max_pass_steps=16, split_waves=_nw, band_rows=48),
                 expect=dict(passes=3, last_nt=16, shape={1: _nw, 3: 1}))
for _shape in ((100, 225), (130, 470)):
    for _kind in ("eps", "mu", "eps+mu"):
        _add(f"f32_16_{_shape[0]}x{_shape[1]}_{_kind}", "passes32", "engine", shape=_shape, dtype=F32, kind=_kind, eps_r=2.2,
             n=35, src=(21, 223), seed=_shape[0] * _shape[1] + 1, allow_uniform=False,
             options=dict(max_pass_steps=16, band_rows=40), expect=dict(passes=3, last_nt=16))

# float32 20-step passes: one pass of 20, 16 + 5 (two halves: 11 + 10), 20 + 20 (16 + 12 + 12)
for _n in (20, 21, 40):
    for _kind in ("uniform", "eps+mu"):
        _p = plan(_n, 16, True, long_passes=True)
        _add(f"f32_20_n{_n}_{_kind}", "passes32", "engine", shape=(130, 470), dtype=F32, kind=_kind, eps_r=2.3, n=_n,
             src=(24, 228), seed=1000 + _n, options=dict(max_pass_steps=20, band_rows=40),
             expect=dict(passes=len(_p), last_nt=_p[-1][0]))

# short tails (test_short_tail_passes_match_oracle): one short pass of the shortest level-split kernel that holds the tail
for _n in (3, 7, 11, 13, 19, 23):
    for _dt in (F32, F64):
        for _kind in ("uniform", "eps+mu"):
            _L = 16 if _dt == F32 else 8
            _p = plan(_n, _L, True)
            _add(f"tail_n{_n}_{_kind}_{_tag(_dt)}", "passes32", "engine", shape=(130, 470), dtype=_dt, kind=_kind, eps_r=3.1,
                 n=_n, src=(1, 236), extent=(3, 2), seed=_n, options=dict(max_pass_steps=_L, band_rows=40),
                 expect=dict(passes=len(_p), last_nt=_p[-1][0]))

# strips of 2 / 4 waves side by side (test_strips_of_several_waves_side_by_side_match_oracle): 36 = 16 + 20
for _xcd in (0, 1):
    for _shape, _src in (((150, 4200), (24, 251)), ((131, 4096), (60, 4095))):
        for _kind in ("uniform", "eps", "eps+mu"):
            _add(f"side2_{_shape[0]}x{_shape[1]}_{_kind}_xcd{_xcd}", "wide", "engine", shape=_shape, dtype=F32, kind=_kind,
                 eps_r=2.3, n=36, src=_src, seed=_shape[0] * _shape[1] + 2,
                 options=dict(max_pass_steps=20, band_rows=40, side_waves=2, xcd_map=_xcd),
                 expect=dict(passes=2, last_nt=20, shape={3: 2, 4: _xcd}))
    _add(f"side4_140x8300_uniform_xcd{_xcd}", "wide", "engine", shape=(140, 8300), dtype=F32, kind="uniform", eps_r=2.3, n=36,
         src=(0, 0), seed=140 * 8300 + 4, options=dict(max_pass_steps=20, band_rows=40, side_waves=4, xcd_map=_xcd),
         expect=dict(passes=2, last_nt=20, shape={3: 4, 4: _xcd}))

# zone tiles of a 20-step pass as workgroups of the bulk launch (test_20_step_pass_with_fused_zone_tiles_matches_oracle)
for _shape, _band, _src in (((150, 4200), 40, (24, 251)), ((300, 700), 300, (150, 215))):
    for _kind in ("uniform", "eps+mu"):
        for _xcd in (0, 1):
            _add(f"zone_fused_{_shape[0]}x{_shape[1]}_{_kind}_xcd{_xcd}", "wide", "engine", shape=_shape, dtype=F32, kind=_kind,
                 eps_r=2.3, n=36, src=_src, seed=_shape[0] * _shape[1] + 7, options=dict(max_pass_steps=20),
                 set_shape=((_band, 4, 0, 1, _xcd, 0, 0, 1), 20), expect=dict(passes=2, last_nt=20, shape={7: 1, 4: _xcd}))

# filler bands (test_filler_bands_match_oracle): 35 steps, source on the seam between tall and filler bands
for _sh, _steps in (((60, 4, 0, 1, 0, 40, 2), 0), ((64, 0, 0, 1, 0, 32, 2), 8)):
    for _kind in ("uniform", "eps+mu"):
        _nt = _steps or 16
        _add(f"filler_{_sh[0]}_{_sh[5]}x{_sh[6]}_nt{_nt}_{_kind}", "passes32", "engine", shape=(300, 1100), dtype=F32, kind=_kind,
             eps_r=2.3, n=35, src=(300 - (5 + _nt) - _sh[5] * _sh[6], 500), seed=sum(_sh), options=dict(max_pass_steps=_nt),
             set_shape=(_sh, _steps), expect=dict(last_nt=_nt, shape={0: _sh[0], 5: _sh[5], 6: _sh[6]}))

# float64 passes: 16 steps (test_float64_16_step_passes_match_oracle), strip seams of the 8-step pass against the right
# band (test_f64_passes_strip_seams_vs_right_band), strips of several waves (test_float64_strips_of_several_waves_...)
for (_shape, _src) in (((76, 64), (0, 0)), ((100, 225), (21, 223)), ((130, 470), (60, 100)), ((200, 1000), (20, 30))):
    for _nw in (4, 8):
        for _kind in ("uniform", "eps+mu"):
            _add(f"f64_16_{_shape[0]}x{_shape[1]}_nw{_nw}_{_kind}", "passes64", "engine", shape=_shape, dtype=F64, kind=_kind,
                 eps_r=1.9, n=35, src=_src, seed=_shape[0] * _shape[1] + 64,
                 options=dict(max_pass_steps=16, split_waves=_nw, band_rows=48),
                 expect=dict(passes=3, last_nt=16, shape={1: _nw}))
for _cols in (225, 232, 241, 344, 460):
    _add(f"f64_seam_60x{_cols}", "passes64", "engine", shape=(60, _cols), dtype=F64, kind="eps", n=12, src=(30, _cols - 3),
         seed=_cols, expect=dict(passes=2, last_nt=8))
for _side, _shape in ((2, (150, 2100)), (4, (140, 4200))):
    _add(f"f64_side{_side}_{_shape[0]}x{_shape[1]}", "passes64", "engine", shape=_shape, dtype=F64, kind="uniform", eps_r=2.3,
         n=35, src=(60, 123), seed=sum(_shape) + _side, options=dict(max_pass_steps=16, band_rows=40, side_waves=_side),
         expect=dict(passes=3, last_nt=16, shape={3: _side}))

# sources on the frame, in the zones, at strip seams (test_blocked_passes_source_anywhere); one row line and one patch
# (test_line_and_patch_sources_match_oracle) through single steps, 8- and 16-step passes
for _src in ((0, 0), (3, 200), (12, 7), (13, 100), (20, 255), (99, 299), (95, 0), (50, 150)):
    for _dt in (F32, F64):
        _add(f"src_{_src[0]}_{_src[1]}_{_tag(_dt)}", "sources", "engine", shape=(100, 300), dtype=_dt, kind="eps", n=16, src=_src,
             seed=3, expect=dict(passes_min=1))
for _src, _ext in (((40, 3), (1, 420)), ((60, 236), (30, 40))):
    for _mp in (0, 8, 16):
        _add(f"extent_{_ext[0]}x{_ext[1]}_mp{_mp}", "sources", "engine", shape=(130, 470), dtype=F32, kind="eps", n=21, src=_src,
             extent=_ext, seed=_src[0] * 1000 + _src[1], options=dict(max_pass_steps=_mp),
             expect=dict(passes=0) if _mp == 0 else dict(passes_min=1, last_nt=_mp))

# the active window, from rest (test_gpu_active_window.py)
_add("window_700x1800_f32", "window", "window", shape=(700, 1800), dtype=F32, kind="uniform", eps_r=1.7,
     segments=((16, 350, 900, 1), (54, 350, 900, 2)), options=dict(active_window=1, max_pass_steps=16, band_rows=40),
     expect=dict(passes=5, windowed=5, last_nt=16))
_add("window_300x1000_f32_eps_20", "window", "window", shape=(300, 1000), dtype=F32, kind="eps",
     segments=((20, 141, 452, 6), (20, 141, 452, 7)), options=dict(active_window=1, max_pass_steps=20, band_rows=40),
     expect=dict(passes=2, windowed=2, last_nt=20))
_add("window_300x1000_f64", "window", "window", shape=(300, 1000), dtype=F64, kind="uniform", eps_r=1.7,
     segments=((20, 141, 452, 6), (20, 141, 452, 7)), options=dict(active_window=1, max_pass_steps=16, band_rows=40),
     expect=dict(passes_min=3, windowed="all", last_nt=16))

# 3 row slabs in one process (tests/local_slabs.py): 8-step cycles on the smallest grid test_gpu_slab.py runs them on
for _mat in ("uniform", "array"):
    _add(f"slabs_3x_320x300_{_mat}", "sources", "slabs", shape=(320, 300), dtype=F32, n=29, world=3, materials=_mat, seed=620)

# the library's own waveform
_add("waveform_ricker_130x470", "sources", "waveform", shape=(130, 470), dtype=F32, kind="eps", n=40, src=(60, 236), seed=40,
     options=dict(max_pass_steps=16), expect=dict(passes_min=1, last_nt=16))

GROUPS = ("small", "passes32", "passes64", "sources", "window", "wide")
assert {c["group"] for c in CASES} == set(GROUPS)


# ---- the runner ----------------------------------------------------------------------------------------------------------

def _onp():
    from oracle import fdtd_numpy
    return fdtd_numpy


def _corc():
    from oracle import c_oracle
    return c_oracle


def _state(case):
    """Seeded inputs of a case (tests/test_gpu_parity.py, _random_state): H scaled by 1e-3, eps in 1..10 eps0, mu in
    1..3 mu0 where the case has a mu array; a uniform case has eps_r * eps0 everywhere."""
    onp = _onp()
    r, c = case["shape"]
    dtype = np.dtype(case["dtype"]).type
    kind = case.get("kind", "eps")
    rng = np.random.default_rng(case.get("seed", 0))
    Ez = rng.standard_normal((r, c)).astype(dtype)
    Hx = (rng.standard_normal((r, c - 1)) * 1e-3).astype(dtype)
    Hy = (rng.standard_normal((r - 1, c)) * 1e-3).astype(dtype)
    eps = (onp.EPS0 * rng.uniform(1, 10, (r, c))).astype(dtype)
    mu = (onp.MU0 * (rng.uniform(1, 3, (r, c)) if "mu" in kind else np.ones((r, c)))).astype(dtype)
    if "eps" not in kind:
        eps = np.full((r, c), case.get("eps_r", 2.5) * onp.EPS0).astype(dtype)
    amps = rng.standard_normal(max(1, case.get("n", 1)))
    return Ez, Hx, Hy, eps, mu, amps


def oracle_steps(fields, eps, mu, n, src, amps, extent, fused):
    """n steps of the C oracle in place.  A point source runs inside orc_run; a line or patch is added in NumPy through
    double (fdtd_numpy.add_source) between the oracle's half steps."""
    corc, onp = _corc(), _onp()
    if tuple(extent) == (1, 1):
        corc.run(*fields, eps, mu, DT, DX, n, src[0], src[1], amps=amps, fused=fused)
        return
    corc.set_threads(*fields[0].shape)
    for s in range(n):
        corc.update_h(*fields, mu, eps, DT, DX, fused=fused)
        corc.update_e(*fields, mu, eps, DT, DX, fused=fused)
        onp.add_source(fields[0], src[0], src[1], amps[s], extent)


def _ulps(a, b):
    """Largest difference of two same-type arrays in units of the last place (distance of their ordered bit patterns)."""
    it = np.int32 if a.dtype == np.float32 else np.int64
    def key(x):
        v = np.ascontiguousarray(x).view(it).astype(np.int64)
        return np.where(v < 0, np.int64(np.iinfo(it).min) - v, v)
    d = np.abs(key(a) - key(b))                        # (int64: wraps only between huge values of opposite sign)
    return float(d.max()) if d.size else 0.0


def compare(got, ref):
    out = {}
    for a, b, k in zip(got, ref, NAMES):
        eq = bool(a.dtype == b.dtype and np.array_equal(a, b))
        rec = dict(equal=eq, ndiff=0, first=[], max_ulp=0.0)
        if not eq:
            bad = np.argwhere(a != b)
            rec.update(ndiff=int(len(bad)), first=bad[:4].tolist(), max_ulp=_ulps(a, b))
        out[k] = rec
    return out


def _check_launch(eng, case, dtype_name):
    """What the case names really ran; returns (error text or None, variant tuple or None)."""
    ex = case.get("expect", {})
    passes, errs = eng.info(16), []
    nt = eng.last_pass_steps if passes else 0
    shape = eng.last_shape if passes else (0,) * 8
    win = eng.windowed_launches
    if "passes" in ex and passes != ex["passes"]:
        errs.append(f"passes {passes} != {ex['passes']}")
    if "passes_min" in ex and passes < ex["passes_min"]:
        errs.append(f"passes {passes} < {ex['passes_min']}")
    if "last_nt" in ex and nt != ex["last_nt"]:
        errs.append(f"last_pass_steps {nt} != {ex['last_nt']}")
    for k, v in ex.get("shape", {}).items():
        if shape[k] != v:
            errs.append(f"last_shape[{k}] {shape[k]} != {v}")
    want_win = ex.get("windowed", 0)
    if want_win == "all":
        want_win = passes
    if win != want_win or (want_win and win <= 0):
        errs.append(f"windowed_launches {win} != {want_win}")
    variant = (dtype_name, nt, shape[1], shape[3], shape[4], shape[7], int(win > 0)) if passes else None
    return ("; ".join(errs) or None), variant


def _engine(fd, case, eps, mu):
    r, c = case["shape"]
    eng = fd.Engine(r, c, DT, DX, dtype=np.dtype(case["dtype"]))
    eng.set_materials(eps, mu, allow_uniform=case.get("allow_uniform", True))
    if case.get("options"):
        eng.set_option(**case["options"])
    if case.get("set_shape"):
        eng.set_shape(*case["set_shape"])
    if case.get("extent"):
        eng.set_source_extent(*case["extent"])
    return eng


def run_case(fd, case, fused):
    """Run one case on the loaded library and compare it with the C oracle at `fused`.  Returns
    {"fields": {name: {equal, ndiff, first (four positions), max_ulp}}, "launch": error text or None,
     "variant": (dtype, last pass steps, waves, side waves, xcd map, zone tiles fused, windowed) or None}."""
    corc, onp = _corc(), _onp()
    driver = case["driver"]
    dtype_name = case["dtype"]
    launch, variant = None, None
    if driver == "slabs":
        from local_slabs import run_local_slabs
        r, c = case["shape"]
        n = case["n"]
        rng = np.random.default_rng(case["seed"])
        st = dict(Ez=rng.standard_normal((r, c)), Hx=rng.standard_normal((r, c - 1)) * 1e-3,
                  Hy=rng.standard_normal((r - 1, c)) * 1e-3, eps=onp.EPS0 * rng.uniform(1, 10, (r, c)),
                  mu=onp.MU0 * np.ones((r, c)), amps=rng.standard_normal(n), dt=DT, dx=DX)
        st["eps"][0, 0] = onp.EPS0
        if case["materials"] == "uniform":
            st["eps"][:] = 2.5 * onp.EPS0
        src = (r // case["world"], c // 2)
        got, cycle, _, launches = run_local_slabs(fd, case["world"], (r, c), np.float32, "mur", st, n, src,
                                                  materials=case["materials"])
        if cycle != 8 or min(launches) <= 0:
            launch = f"slab cycle {cycle}, pass launches {launches}"
        ref = [st[k].astype(np.float32) for k in NAMES]
        oracle_steps(ref, st["eps"].astype(np.float32), st["mu"].astype(np.float32), n, src, st["amps"], (1, 1), fused)
        return dict(fields=compare(got, ref), launch=launch, variant=None)

    Ez, Hx, Hy, eps, mu, amps = _state(case)
    if driver == "half":
        ref = [a.copy() for a in (Ez, Hx, Hy)]
        corc.update_h(*ref, mu, eps, DT, DX, fused=fused)
        corc.update_e(*ref, mu, eps, DT, DX, fused=fused)
        got = [a.copy() for a in (Ez, Hx, Hy)]
        fd.update_Hx_Hy(*got, mu, eps, DT, DX)
        fd.update_Ez(*got, mu, eps, DT, DX)
        fd.invalidate_cache()
        return dict(fields=compare(got, ref), launch=None, variant=None)

    extent = case.get("extent", (1, 1))
    if driver == "window":
        ref = onp.grid_zeros(*case["shape"], np.dtype(dtype_name).type)
        with _engine(fd, case, eps, mu) as eng:
            eng.reset()
            for steps, row, col, seed in case["segments"]:
                a = np.random.default_rng(seed).standard_normal(steps)
                eng.run(steps, row, col, a)
                oracle_steps(ref, eps, mu, steps, (row, col), a, extent, fused)
            got = eng.download()
            launch, variant = _check_launch(eng, case, dtype_name)
        return dict(fields=compare(got, ref), launch=launch, variant=variant)

    n, src = case["n"], case["src"]
    if driver == "waveform":
        lib = fd._abi.load()
        amps = np.array([lib.fdtd2d_source_amplitude(fd._abi.SRC_RICKER, (0 + i) * DT, FC) for i in range(n)])
    ref = [a.copy() for a in (Ez, Hx, Hy)]
    oracle_steps(ref, eps, mu, n, src, amps, extent, fused)
    with _engine(fd, case, eps, mu) as eng:
        eng.upload(Ez, Hx, Hy)
        if driver == "waveform":
            eng.run_waveform(n, "ricker", src[0], src[1], FC, 0)
        else:
            eng.run(n, src[0], src[1], amps)
        got = eng.download()
        launch, variant = _check_launch(eng, case, dtype_name)
        if eng.step_count != n:
            launch = (launch + "; " if launch else "") + f"step_count {eng.step_count} != {n}"
    return dict(fields=compare(got, ref), launch=launch, variant=variant)


def run_group(fd, group, fused):
    """Every case of a group: {case name: result of run_case}."""
    return {c["name"]: run_case(fd, c, fused) for c in CASES if c["group"] == group}
