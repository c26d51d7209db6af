"""GPU: the boundary="pml" passes at the seams of their partitions -- every row of tests/test_pml_partition_cpu.py from a
random state, on the plan under test (the float32 16-step pair k_bulk_split / k_bulk_split_pml, or 8-step k_pass_pml),
on 8-step passes and on the single-step kernels, against oracle/pml_numpy.py: Ez, Ezx, Hx, Hy bit for bit in the exact
build; in the fused build the three device paths against each other, to a rounding bound (fused_bound: bit for bit they
differ on every row, in thousands to a million cells by up to 4e-7 of the largest value -- the kernels of that build do
not contract the same multiply-add pairs).  The passes counted, the single-step launches and `last_pass_steps` are the
planned ones, so a row cannot fall back to single steps unseen."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_pml_partition_cpu as tp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX = 5e-14, 1e-4             # Courant 0.15 in vacuum; the rows at 0.65 scale DT
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
INFO_EPS_UNIFORM, INFO_MU_UNIFORM, INFO_PASSES, INFO_STEP_LAUNCHES = 9, 10, 16, 17
FIELDS = ("Ez", "Ezx", "Hx", "Hy")
MAX_STEPS = 40


def state_key(c):
    return (c.dtype, c.R, c.C, c.L, c.materials, c.ezx, c.courant)


def time_step(courant):
    return DT * (courant / 0.15)


# the run lengths the rows that share a state and a source ask for: one oracle run serves them all
LENGTHS = {}
for _c in tp.CASES:
    LENGTHS.setdefault((state_key(_c), _c.source), set()).add(_c.n)


def layer_mask(R, C, L):
    i, j = np.arange(R)[:, None], np.arange(C)[None, :]
    return (i < L) | (i > R - 1 - L) | (j < L) | (j > C - 1 - L)


@functools.lru_cache(maxsize=None)
def pml_state(key):
    """Random Ez, Hx, Hy in every cell; Ezx random inside the layer and exactly 0 outside (flavour a: a state the engine
    can reach) or random in every cell (b: one upload_ezx accepts); eps in [1, 4] EPS0, 2 EPS0, or EPS0 ("vacuum"); seeded by the key."""
    from oracle import fdtd_numpy as onp
    dtype, R, C, L, materials, ezx, _ = key
    T = NP_DTYPE[dtype]
    rng = np.random.default_rng([R, C, L, np.dtype(T).itemsize, ("uniform", "eps", "mu", "vacuum").index(materials), ord(ezx)])
    st = {"Ez": rng.standard_normal((R, C)).astype(T),
          "Ezx": (0.3 * rng.standard_normal((R, C))).astype(T),
          "Hx": (rng.standard_normal((R, C - 1)) * 1e-3).astype(T),
          "Hy": (rng.standard_normal((R - 1, C)) * 1e-3).astype(T),
          "amps": rng.standard_normal(MAX_STEPS)}
    if ezx == "a":
        st["Ezx"][~layer_mask(R, C, L)] = 0
    st["eps"] = (onp.EPS0 * (rng.uniform(1, 4, (R, C)) if materials == "eps" else np.full((R, C), 1.0 if materials == "vacuum" else 2.0))).astype(T)
    st["mu"] = (onp.MU0 * (rng.uniform(1, 3, (R, C)) if materials == "mu" else np.ones((R, C)))).astype(T)
    for a in st.values():
        a.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def pml_reference(key, source):
    """The oracle's fields after each run length of LENGTHS[key, source]: its `step`, and a dense Ez += s over the
    source rectangle (the engine's rounding: float64 sum, rounded once)."""
    from oracle import pml_numpy as pm
    dtype, R, C, L, _, _, courant = key
    T = NP_DTYPE[dtype]
    st = pml_state(key)
    P = pm.profiles(R, C, courant, L=L, dtype=T)
    f = [st[k].copy() for k in FIELDS]
    out = {}
    for n in range(1, max(LENGTHS[key, source]) + 1):
        pm.step(*f, st["eps"], st["mu"], time_step(courant), DX, P)
        if source is not None:
            r, q, nr, nc = source
            f[0][r:r + nr, q:q + nc] = (f[0][r:r + nr, q:q + nc].astype(np.float64) + st["amps"][n - 1]).astype(T)
        if n in LENGTHS[key, source]:
            out[n] = [a.copy() for a in f]
            assert all(np.isfinite(a).all() for a in out[n]), (key, n)
            for a in out[n]:
                a.setflags(write=False)
    return out


def run_three_ways(fd, c):
    """[(fields, passes counted, single-step launches, last_pass_steps, max_pass_steps)] per variant of the row."""
    st = pml_state(state_key(c))
    outs = []
    for ms in tp.variants(c):
        with fd.Engine(c.R, c.C, time_step(c.courant), DX, dtype=NP_DTYPE[c.dtype], boundary="pml") as eng:
            eng.set_materials(st["eps"], st["mu"]).set_pml(L=c.L, courant00=c.courant)
            opts = {k: v for k, v in c.opts.items() if k != "shape"}
            eng.set_option(max_pass_steps=ms, **opts)
            if "shape" in c.opts:
                eng.set_shape(c.opts["shape"])
            assert (eng.info(INFO_EPS_UNIFORM), eng.info(INFO_MU_UNIFORM)) == (c.materials != "eps", c.materials != "mu")
            eng.upload(st["Ez"], st["Hx"], st["Hy"]).upload_ezx(st["Ezx"])
            p0, s0 = eng.info(INFO_PASSES), eng.info(INFO_STEP_LAUNCHES)
            if c.source is None:
                eng.run(c.n)
            else:
                eng.set_source_extent(*c.source[2:])
                eng.run(c.n, c.source[0], c.source[1], st["amps"][:c.n])
            got = eng.download()
            gx = eng.download_ezx()
            outs.append(((got[0], gx, got[1], got[2]), eng.info(INFO_PASSES) - p0, eng.info(INFO_STEP_LAUNCHES) - s0,
                         eng.last_pass_steps, ms))
    return outs


def check_plan(c, outs):
    for _, passes, steps, last, ms in outs:
        plan = tp.planned(c.n, tp.cycle_steps(c, ms))
        want = [nt for nt, _ in plan if nt]
        assert passes == len(want) and steps == 2 * (len(plan) - len(want)), (c.name, ms, passes, steps, plan)
        assert last == (want[-1] if want else 0), (c.name, ms, last, plan)


def check_not_vacuous(c, fields):
    st = pml_state(state_key(c))
    lay = layer_mask(c.R, c.C, c.L)
    assert all(np.abs(a).max() > 0 for a in fields)
    inside = lay.copy()
    inside[[0, -1], :] = inside[:, [0, -1]] = False             # (the outer edge cells are never updated)
    assert not inside.any() or (fields[1] != st["Ezx"])[inside].mean() > 0.9     # (L = 1: the layer is the edge itself)
    if c.ezx == "a":
        assert not fields[1][~lay].any()
    else:
        assert np.array_equal(fields[1][~lay], st["Ezx"][~lay]) and fields[1][~lay].any()


def mismatch(a, b):
    bad = np.argwhere(a != b)
    return f"{len(bad)} cells, first {bad[:4].tolist()}, rows {bad[:, 0].min()}..{bad[:, 0].max()}, " \
           f"columns {bad[:, 1].min()}..{bad[:, 1].max()}"


def fused_bound(c):
    """How far two paths of the tolerance build may differ after c.n steps, relative to the field's largest value.  A
    step forms each value with at most 8 rounded operations; the fused build contracts three multiply-add pairs of them,
    and not the same three in every kernel (the single-step PML kernels leave the choice to the compiler, the staged
    plain body writes its fused forms out), so per step two paths differ by at most 8 roundings of eps / 2 of the
    largest term.  The scheme does not amplify (Courant <= 0.65, layer factors <= 1), so the differences of n steps
    add at most linearly: 4 n eps; a factor 4 for a term larger than the field's final maximum.  A stale Ezx, a cell
    nobody wrote or a wrong body is of the order of the field itself."""
    return 16 * c.n * float(np.finfo(NP_DTYPE[c.dtype]).eps)


def path_differences(c, outs):
    """[(field, max_pass_steps, largest difference to the single-step path relative to the field's maximum)]."""
    base = outs[-1][0]
    return [(k, ms, float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()))
            for fields, _, _, _, ms in outs[:-1] for a, b, k in zip(fields, base, FIELDS)]


@pytest.mark.parametrize("c", tp.CASES, ids=tp.case_id)
def test_pml_table_row_matches_oracle(c):
    import fdtd2d_amd as fd
    outs = run_three_ways(fd, c)
    check_plan(c, outs)
    if fd.ARITHMETIC != "exact":        # the tolerance build: its three paths against each other (the test below)
        check_not_vacuous(c, outs[-1][0])
        bad = [d for d in path_differences(c, outs) if not d[2] <= fused_bound(c)]
        assert not bad, (c.name, bad, fused_bound(c))
        return
    ref = pml_reference(state_key(c), c.source)[c.n]
    check_not_vacuous(c, ref)
    names = {16: "16-step pair", 8: "8-step passes", 0: "single steps"}
    errors = [f"{k}: {names[ms]} vs oracle: {mismatch(a, b)}" for fields, _, _, _, ms in outs
              for a, b, k in zip(fields, ref, FIELDS) if not np.array_equal(a, b)]
    assert not errors, (c.name, errors)


# ---- the fused build ----------------------------------------------------------------------------------------------------------------

FUSED_CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
import fdtd2d_amd as fd
from fdtd2d_amd import _abi
import test_pml_partition_cpu as tp
import test_gpu_pml_passes as tg
assert fd.ARITHMETIC == "fused" and _abi.LIB_PATH.endswith("libfdtd2d_fused.so")
out = {}
for c in tp.CASES:
    outs = tg.run_three_ways(fd, c)
    tg.check_plan(c, outs)
    tg.check_not_vacuous(c, outs[-1][0])
    out[c.name] = {"worst": max([d[2] for d in tg.path_differences(c, outs)]), "bound": tg.fused_bound(c)}
print("FUSED_PML_PASSES " + json.dumps(out))
'''


def test_fused_build_pml_paths_agree_on_every_row():
    """FDTD2D_ARITHMETIC=fused in a child process: on every row the pass paths agree with the single-step kernels of the
    same build to fused_bound (rounding: the kernels do not contract the same multiply-add pairs), with the planned
    passes counted and the same non-vacuity checks (no oracle comparison: the tolerance build differs from it by
    rounding too)."""
    head = f"ROOT = {ROOT!r}\nTESTS = {os.path.join(ROOT, 'tests')!r}\n"
    p = subprocess.run([sys.executable, "-c", head + FUSED_CHILD], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FDTD2D_ARITHMETIC="fused"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("FUSED_PML_PASSES ")][-1][17:])
    assert sorted(out) == sorted(c.name for c in tp.CASES)
    print("fused build: largest path difference / bound:", max(v["worst"] / v["bound"] for v in out.values()))
    bad = {k: v for k, v in out.items() if not v["worst"] <= v["bound"]}
    assert not bad, bad
