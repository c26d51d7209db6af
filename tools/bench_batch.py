"""Batched engine: throughput of BatchEngine.run against the same members run one Engine at a time.

One JSON line per configuration (default: 1024 members of 60 x 60 and 64 members of 256 x 256, float32,
array eps with random binary permittivity, a ricker line source per member):
  ms / mcell_steps_per_s      one run(steps) of the whole batch, host call to stream sync (amplitude upload
                              included), median of --reps
  path, launches_per_run      resident (one launch per run) or streamed (two per step)
  lds_bytes_per_member        LDS a resident workgroup declares
  lds_bound_mcell_steps_per_s the resident kernel's LDS-traffic bound from its own access count per interior
                              cell-step (H: 5 reads + ch, 2 writes; E: 5 reads + ce, 1 write) at the per-CU
                              peaks of MI355X_MICROARCH.md section LDS (ds_read_b32 128 B/clk, ds_read_b64 256,
                              ds_write_b32 64, ds_write_b64 85) x 256 CUs x --clock-ghz; lds_bound_fraction =
                              achieved / bound
  loop_*                      the yardstick: --loop-members of the same members, each through its own Engine
                              (create, materials, run, download), timed alternately with the batch in this
                              process; loop_ms_extrapolated = per member x count
  --boundary pml              every member with a --pml-cells split-field layer (BatchEngine.set_pml); the loop
                              yardstick is then Engine(boundary="pml"), and the line adds mur_ms / pml_over_mur:
                              the same members as a Mur batch, timed alternately in this process
  --monitors                  instead: a window DFT (30 x 1 cells, 10 frequencies, every step) and 4 probes per
                              member (BatchEngine.set_dft_window / set_probes): mon_ms and plain_ms (the same batch
                              without monitors) timed alternately, mon_over_plain, launches_per_run, and
                              dft_runs_ms = the same 10 frequencies as 10 runs with the whole-grid set_dft, one
                              omega each (reset, set_dft, run, read_dft), dft_runs_over_mon
  --adjoint                   instead: one batch_eps_gradient (PML, 10 frequencies, 30 probes, a design window of
                              100 cells in 60 x 60 members or 100 x 100 cells in 250 x 250 ones, dt = 2e-13) against
                              two monitored runs of the same length with a rectangle source, timed alternately:
                              grad_ms (the whole helper: engine, both runs, probe reads, host algebra), two_runs_ms,
                              device_ms (forward run, hold, reset, adjoint run with channels, product, on a standing
                              engine) and device_over_two_runs = the cost of the channels and the product;
                              product_ms (dft_window_product) against download_ms (both windows read back and
                              multiplied in NumPy).  Default: 1024 members of 60 x 60 and 64 of 250 x 250.
                              Timed alternately with those, in the same process: session_ms (one value_and_grad of a
                              standing AdjointSession, the same objective) and session_over_two_runs / _over_device /
                              grad_over_session; spectra_device_ms (one BatchEngine.probe_spectra of all members with
                              the peaks; spectra_trace_bytes = B * P * n * 8 is what its kernel reads) against
                              spectra_host_ms (read_probes + adjoint.probe_spectra, the helper's way); eps_window_ms
                              (set_eps_window of the design window) against set_materials_ms (the full arrays);
                              launches_per_session_iteration.
  --lossy                     instead: the lossy step kernels (BatchEngine.set_conductivity, sigma random up to 20 S/m
                              on the cells that may conduct) against the point-source kernels they were copied from, on
                              the same members with the same one silent point source (weight 0, a zero channel), timed
                              alternately: lossy_ms, pts_ms, lossy_over_pts, both paths and LDS sizes, and
                              workgroups_per_cu of each from its LDS size (160 KiB per CU).  By this script's LDS count
                              the lossy update adds one read per interior cell-step (lds_reads_per_cell_step).  One
                              line for Mur and one for the PML.
  --periodic                  instead: the periodic step kernels (boundary="periodic", a layer on the rows) against the
                              lossy PML kernels they were copied from (boundary="pml", profiles= with the same row
                              factors and unit column factors), on the same members with the same conductivity and the
                              same one silent point source, timed alternately in one process: periodic_ms,
                              lossy_pml_ms, periodic_over_lossy_pml, both paths and LDS sizes.  Default: 1024 members
                              of 60 rows x 61 columns, a 10-cell layer, 1000 steps.
  --hz                        instead: the Hz polarisation (set_polarization("hz")) with a metal strip and its Drude pole
                              against the Ez polarisation's dispersive kernels on the same periodic members, layer and
                              strip, both resident, timed alternately in one process: hz_ms, ez_dispersive_ms,
                              hz_over_ez_dispersive, both paths and LDS sizes.  The Hz kernel does two pole updates per
                              cell in 12 LDS arrays against one in 10.  Default: 1024 members of 56 rows x 57 columns, a
                              10-cell layer, 2000 steps.
  --hz-bloch                  instead: a Bloch phase in the Hz polarisation (BatchEngine.set_hz_bloch_phase: a phase sweep
                              0..pi over the members, ramp weights) on 1024 periodic members of 40 x 41 with the metal strip
                              and the pole of --hz, so that the twenty arrays stay resident, against the real Hz kernels on
                              the same members (hz_bloch_over_hz) and against the Ez Bloch kernels with the same pole
                              (hz_bloch_over_ez_bloch): the three medians, paths and LDS bytes per member
  --hz-lattice                instead: the lattice mode of the Hz polarisation (BatchEngine.set_hz_lattice_phase: the k-path
                              Gamma-X-M-Gamma over the members, ramp weights) on 1024 members of 32 x 33 with a metal rod and
                              its pole (18 LDS arrays), against the Ez lattice kernels with the pole of
                              set_bloch_dispersion on the same members (14 arrays: hz_lattice_over_ez_lattice) and against
                              the same Hz lattice batch without the pole (9 arrays: hz_lattice_over_plain), all resident,
                              timed alternately in one process: the three medians, paths, LDS bytes per member and the
                              workgroups per CU they leave
  --hz-bloch-flux             instead: flux lines under that phase (BatchEngine.set_hz_bloch_flux_lines: two whole-period row
                              lines, 10 frequencies) on the member of --hz-bloch against the same batch without them, both
                              resident, timed alternately in one process: hz_bloch_ms, hz_bloch_flux_ms, their ratio,
                              where the sums live (LDS or global memory) and the LDS bytes per member
  --hz-flux                   instead: flux lines in the Hz polarisation (BatchEngine.set_hz_flux_lines: two whole-period
                              row lines, 10 frequencies) on the member of --hz (the metal strip with its pole) against the
                              same batch without them, and the lines of --flux on a lossless Ez batch of the same shape
                              against that batch without them, all resident, timed alternately in one process: hz_ms,
                              hz_flux_ms, hz_flux_over_hz, ez_ms, ez_flux_ms, ez_flux_over_ez, the ratio of the two
                              ratios, where each batch keeps its sums (LDS or global memory) and the LDS sizes; and
                              ez_flux_global_ms, the Ez lines with their sums kept in global memory (set_flux_lds(False)),
                              where the Hz member's live at this shape.
                              Default: 1024 members of 56 rows x 57 columns, a 10-cell layer, 2000 steps.
  --bloch                     instead: a Bloch batch (set_bloch_phase, a phase sweep over the members, ramp weights)
                              against the plain periodic batch of the same members, layer and conductivity, timed
                              alternately in one process: bloch_ms, periodic_ms, bloch_over_periodic, both paths and
                              LDS sizes.  A Bloch member carries two members' fields, so the number to beat is 2.
                              Default: 1024 members of 60 x 60, a 10-cell layer, 1000 steps.
  --bloch-adjoint             instead: the adjoint gradient of a Bloch batch (a phase sweep over the members, a
                              conductivity, ramp weights, 10 frequencies, 30 probes, 20 channels, a design window of 100
                              cells, dt = 2e-13), the columns of --adjoint: device_ms (forward run, hold_bloch_window,
                              reset, adjoint run with channels and the conjugate rotation, bloch_window_product, on a
                              standing engine) against two_runs_ms (two monitored Bloch runs of that length with the
                              rectangle source) and session_ms (one value_and_grad of a standing BlochAdjointSession),
                              timed alternately in one process: device_over_two_runs, session_over_two_runs, the path
                              and the LDS size.  Default: 1024 members of 60 x 60, a 10-cell layer, 1500 steps.
  --dispersive                instead: the dispersive step kernels (BatchEngine.set_dispersion: a Drude block, wp = 2 pi
                              70 GHz and gamma = 1e11, on the middle third of every member) against the lossy PML
                              kernels they were copied from, on the same members with the same layer, conductivity and
                              one silent point source, timed alternately in one process: dispersive_ms, lossy_pml_ms,
                              dispersive_over_lossy_pml, both paths and LDS sizes.  By this script's LDS count the pole
                              adds three reads and two writes per interior cell-step to the lossy PML kernel's 17 reads
                              and 3 writes.  Default: 1024 members of 60 x 60, a 10-cell layer, 1000 steps.
  --lattice                   instead: a lattice batch (boundary="lattice": Bloch conditions on both pairs of edges, a
                              k-path sweep Gamma-X-M-Gamma over the members, ramp weights) against the Bloch batch of the
                              same members without a layer (PEC rows, the members' column phases), with the same
                              conductivity (zero within 6 rows of the top and bottom, where the Bloch batch allows none),
                              timed alternately in one process: lattice_ms, bloch_ms, lattice_over_bloch, both paths and
                              LDS sizes.  The lattice kernel carries 9 arrays against 11 and has no layer branch, so
                              the number to beat is 1.  Default: 1024 members of 33 x 33, 1000 steps.
  --bloch-dispersive          instead: the Drude-Lorentz pole of complex batches (BatchEngine.set_bloch_dispersion: a Drude
                              block, wp = 2 pi 70 GHz and gamma = 1e11, on the middle third of every member) against the
                              same members without it, timed alternately in one process; two lines: a lattice batch
                              (the k-path sweep of --lattice) and a Bloch batch with a --pml-cells layer (the phase sweep
                              of --bloch): dispersive_ms, plain_ms, dispersive_over_plain, both paths, the LDS bytes per
                              workgroup and the workgroups per CU they admit (160 KiB per CU): 14 arrays against 9 and
                              16 against 11 may cost a workgroup per CU.  Default: 1024 members of 33 x 33, 1000 steps.
  --dispersive-adjoint        instead: the three gradients of a dispersive batch (a Drude block, wp = 2 pi 70 GHz and
                              gamma = 1e11, and a conductivity on the design window of 100 cells; PML, 10 frequencies, 30
                              probes, 20 channels, dt = 2e-13): dispersive_ms, one DispersiveAdjointSession.value_and_grad
                              + sigma_gradient + wp2_gradient, against lossy_ms, the same members without the pole as an
                              AdjointSession.value_and_grad + sigma_gradient, timed alternately in one process:
                              dispersive_over_lossy, both paths, LDS sizes and launches per iteration.  Also, on the
                              dispersive session's windows: multi_product_ms, one dispersive_window_product of three
                              coefficient sets, against three_products_ms, three calls of one set each (three launches,
                              three read-backs): multi_over_three.  Default: 1024 members of 60 x 60, a 10-cell layer,
                              1500 steps.
  --flux                      instead: flux lines (BatchEngine.set_flux_lines: two whole-period row lines, 10
                              frequencies, every step) on a periodic batch resident in LDS, against the same batch
                              without monitors and, for scale, with a window DFT of 16 frequencies over as many cells
                              (Ez alone), timed alternately in one process: plain_ms, flux_ms, window_ms,
                              flux_over_plain, window_over_plain, the LDS sizes and flux_call_ms (one BatchEngine.flux).
                              Default: 1024 members of 60 rows x 61 columns, a 10-cell layer, 2000 steps.
  --bloch-flux                instead: the same two lines and 10 frequencies on a Bloch batch
                              (BatchEngine.set_bloch_flux_lines, a phase sweep over the members, ramp weights) resident
                              in LDS, against the same Bloch batch without monitors, timed alternately in one process:
                              plain_ms, flux_ms, flux_over_plain, where the sums live (flux_lines_in_lds), the LDS sizes
                              and flux_call_ms.  Default: 1024 members of 60 rows x 61 columns, a 10-cell layer, 2000
                              steps.
  --flux-adjoint              instead: the adjoint of a flux objective on the members of --flux (periodic, two
                              whole-period row lines at 10 frequencies, dt = 2e-13, a design window of 100 cells between
                              them, 20 channels), timed alternately in one process: flux_ms (a run with the lines and a
                              window DFT over the design window), adjoint_run_ms (the same run driven through
                              set_flux_line_sources: E and H parts on both lines) and adjoint_run_over_flux;
                              flux_session_ms (one FluxAdjointSession.value_and_grad, the weights formed on the device)
                              against probe_session_ms (one AdjointSession.value_and_grad with 30 probes on the same
                              members) and flux_over_probe_session; weights_ms (one flux_adjoint_sources) and where
                              the weights live.  Default: 1024 members of 60 rows x 61 columns, a 10-cell layer, 2000
                              steps.
  --bloch-flux-adjoint        instead: the adjoint of a flux objective on the members of --bloch-flux (a phase sweep over
                              the members, ramp weights, two whole-period row lines at 10 frequencies; dt = 2e-13 and the
                              design window of --flux-adjoint, 20 channels), timed alternately in one process: flux_ms
                              (the --bloch-flux run of this batch, with a window DFT over the design window),
                              adjoint_run_ms (run_bloch_channels(conjugate=True) driven through
                              set_bloch_flux_line_sources: E and H parts on both lines) and adjoint_run_over_flux;
                              flux_session_ms (one BlochFluxAdjointSession.value_and_grad, the weights formed on the
                              device) against probe_session_ms (one BlochAdjointSession.value_and_grad with 30 probes on
                              the same members) and flux_over_probe_session; weights_ms (one
                              bloch_flux_adjoint_sources) and the launches per iteration.  Default: 1024 members of 60
                              rows x 61 columns, a 10-cell layer, 2000 steps.
Usage: python tools/bench_batch.py [--count 1024 --rows 60 --cols 60 --steps 1000] [--reps 5] [--loop-members 16]
                                   [--boundary {mur,pml} --pml-cells 10] [--monitors] [--adjoint] [--lossy]
                                   [--periodic] [--bloch] [--bloch-adjoint] [--dispersive] [--lattice]
                                   [--bloch-dispersive] [--dispersive-adjoint] [--flux] [--bloch-flux]
                                   [--flux-adjoint] [--bloch-flux-adjoint] [--hz-flux] [--hz-bloch] [--hz-bloch-flux] [--hz-lattice]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fdtd2d_amd as fd  # noqa: E402

DT, DX, FC = 5e-14, 1e-4, 30e9
CUS = 256
LDS_READ = {4: 128, 8: 256}     # B/clk/CU
LDS_WRITE = {4: 64, 8: 85}


def lds_bound(esz, arrays, clock_ghz, pml=False):
    """Cell-steps per second the resident kernel's LDS traffic allows (interior cells; the PML kernel reads the
    four H factors of its row and column in every H update)."""
    reads = 10 + (4 if pml else 0) + (2 if arrays else 0)
    writes = 3
    per_clk_read = LDS_READ[esz] * CUS * clock_ghz * 1e9
    per_clk_write = LDS_WRITE[esz] * CUS * clock_ghz * 1e9
    return 1.0 / (reads * esz / per_clk_read + writes * esz / per_clk_write)


def members(count, rows, cols, steps, seed=0):
    rng = np.random.default_rng(seed)
    eps = np.where(rng.random((count, rows, cols)) < 0.5, fd.EPS0, 5 * fd.EPS0)
    rr = rng.integers(6, rows - 6, count)
    rects = np.stack([rr, np.full(count, 5), np.ones(count, int), np.full(count, cols - 10)], axis=1)
    amps = np.array([fd.ricker_amplitude(i * DT, FC) for i in range(steps)])
    return eps, rects, np.ascontiguousarray(np.broadcast_to(amps, (count, steps)))


def courant00(eps, dtype):
    """Each member's Courant number at its [0,0] cell, as run_fdtd(boundary="pml") grades the layer."""
    return (1 / np.sqrt(eps[:, 0, 0].astype(dtype).astype(np.float64) * fd.MU0) * DT) / DX


def bench(count, rows, cols, steps, dtype, reps, loop_members, clock_ghz, boundary="mur", pml_cells=10):
    eps, rects, amps = members(count, rows, cols, steps)
    pml = boundary == "pml"
    c00 = courant00(eps, dtype)

    def batch(kind):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary=kind)
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        if kind == "pml":
            b.set_pml(pml_cells, courant00=c00)
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch(boundary) as b:
        mur = batch("mur") if pml else None
        l0 = b.launches
        b.reset().run(steps, amps).sync()
        launches = b.launches - l0
        batch_ms, loop_ms, mur_ms = [], [], []
        for _ in range(reps):
            batch_ms.append(timed(b))
            if mur is not None:
                mur_ms.append(timed(mur))
            if loop_members:
                t0 = time.perf_counter()
                for m in range(loop_members):
                    with fd.Engine(rows, cols, DT, DX, dtype=dtype, boundary=boundary) as e:
                        e.set_materials(eps[m].astype(dtype), np.full((rows, cols), fd.MU0, dtype))
                        if pml:
                            e.set_pml(pml_cells, courant00=c00[m])
                        e.set_source_extent(int(rects[m, 2]), int(rects[m, 3]))
                        e.run(steps, int(rects[m, 0]), int(rects[m, 1]), amps[m])
                        e.download()
                loop_ms.append((time.perf_counter() - t0) * 1e3 / loop_members)
        resident = b.resident
        lds = b.lds_bytes
        mur_resident = mur.resident if mur is not None else None
        if mur is not None:
            mur.close()
    ms = float(np.median(batch_ms))
    rate = count * rows * cols * steps / (ms * 1e-3)
    esz = np.dtype(dtype).itemsize
    bound = lds_bound(esz, True, clock_ghz, pml) if resident else None
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
           "materials": "arrays", "boundary": boundary, "pml_cells": pml_cells if pml else None,
           "path": "resident" if resident else "streamed", "reps": reps,
           "ms": round(ms, 4), "ms_min": round(min(batch_ms), 4), "mcell_steps_per_s": round(rate / 1e6, 1),
           "launches_per_run": launches, "lds_bytes_per_member": lds if resident else None,
           "lds_bound_mcell_steps_per_s": round(bound / 1e6, 1) if bound else None,
           "lds_bound_fraction": round(rate / bound, 4) if bound else None, "clock_ghz_assumed": clock_ghz}
    if mur_ms:
        out.update({"mur_path": "resident" if mur_resident else "streamed", "mur_ms": round(float(np.median(mur_ms)), 4),
                    "pml_over_mur": round(ms / float(np.median(mur_ms)), 3)})
    if loop_members:
        per = float(np.median(loop_ms))
        out.update({"loop_members_timed": loop_members, "loop_ms_per_member": round(per, 4),
                    "loop_ms_extrapolated": round(per * count, 2),
                    "loop_mcell_steps_per_s": round(rows * cols * steps / (per * 1e-3) / 1e6, 2),
                    "speedup_vs_loop": round(per * count / ms, 1)})
    return out


def bench_monitors(count, rows, cols, steps, dtype, reps, boundary="mur", pml_cells=10):
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    omegas = 2 * np.pi * np.linspace(10e9, 100e9, 10)
    window = ((rows - 30) // 2, (3 * cols) // 4, 30, 1)
    cells = [[rows // 2, cols // 2], [rows // 4, cols // 4], [3 * rows // 4, cols // 2], [rows // 2, 3 * cols // 4]]

    def batch():
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary=boundary)
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        if boundary == "pml":
            b.set_pml(pml_cells, courant00=c00)
        return b

    def timed(b, *reads):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        for r in reads:
            r()
        return (time.perf_counter() - t0) * 1e3

    with batch() as plain, batch() as mon, batch() as dft:
        mon.set_dft_window(window, omegas, 1).set_probes(cells, steps)
        for b in (plain, mon, dft):
            b.run(steps, amps).sync()                 # warm-up: code objects, clocks
        l0 = mon.launches
        mon.reset().run(steps, amps).sync()
        launches = mon.launches - l0
        plain_ms, mon_ms, dft_ms = [], [], []
        for _ in range(reps):
            plain_ms.append(timed(plain))
            mon_ms.append(timed(mon))
            total = 0.0
            for w in omegas:
                dft.set_dft(w, 1)
                total += timed(dft, dft.read_dft)
            dft_ms.append(total)
        mon_read_ms = timed(mon, mon.read_dft_window, mon.read_probes)
        resident, in_lds, lds = mon.resident, mon.window_in_lds, mon.lds_bytes
    med = {k: float(np.median(v)) for k, v in (("plain", plain_ms), ("mon", mon_ms), ("dft", dft_ms))}
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
            "materials": "arrays", "boundary": boundary, "pml_cells": pml_cells if boundary == "pml" else None,
            "monitors": {"window": list(window), "freqs": len(omegas), "every": 1, "probes": len(cells)},
            "path": "resident" if resident else "streamed", "window_in_lds": in_lds,
            "lds_bytes_per_member": lds if resident else None, "reps": reps,
            "mon_ms": round(med["mon"], 4), "mon_ms_min": round(min(mon_ms), 4),
            "plain_ms": round(med["plain"], 4), "plain_ms_min": round(min(plain_ms), 4),
            "mon_over_plain": round(med["mon"] / med["plain"], 3),
            "mon_with_reads_ms": round(mon_read_ms, 4),
            "dft_runs_ms": round(med["dft"], 4), "dft_runs_over_mon": round(med["dft"] / med["mon"], 2),
            "launches_per_run": launches}


def bench_lossy(count, rows, cols, steps, dtype, reps, boundary, pml_cells):
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    rng = np.random.default_rng(1)
    g = max(6, pml_cells) if boundary == "pml" else 6
    sigma = np.zeros((count, rows, cols))
    sigma[:, g:rows - g, g:cols - g] = 20.0 * rng.random((count, rows - 2 * g, cols - 2 * g))
    chan = np.zeros((1, steps))

    def batch(lossy):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary=boundary)
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        if boundary == "pml":
            b.set_pml(pml_cells, courant00=c00)
        b.set_point_sources([[rows // 2, cols // 2]], np.zeros((1, 1)))
        if lossy:
            b.set_conductivity(sigma)
        b.run(steps, amps, chan).sync()                # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps, chan).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch(False) as pts, batch(True) as lossy:
        assert lossy.lossy and not pts.lossy
        l0 = lossy.launches
        lossy.reset().run(steps, amps, chan).sync()
        launches = lossy.launches - l0
        pts_ms, lossy_ms = [], []
        for _ in range(reps):
            pts_ms.append(timed(pts))
            lossy_ms.append(timed(lossy))
        paths = ["resident" if b.resident else "streamed" for b in (pts, lossy)]
        lds = [b.lds_bytes for b in (pts, lossy)]
    med_p, med_l = float(np.median(pts_ms)), float(np.median(lossy_ms))
    reads = 12 + (4 if boundary == "pml" else 0)
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
            "materials": "arrays", "boundary": boundary, "pml_cells": pml_cells if boundary == "pml" else None,
            "reps": reps, "pts_path": paths[0], "lossy_path": paths[1],
            "pts_lds_bytes_per_member": lds[0], "lossy_lds_bytes_per_member": lds[1],
            "pts_workgroups_per_cu": 163840 // lds[0], "lossy_workgroups_per_cu": 163840 // lds[1],
            "lds_reads_per_cell_step": {"pts": reads, "lossy": reads + 1},
            "pts_ms": round(med_p, 4), "pts_ms_min": round(min(pts_ms), 4),
            "lossy_ms": round(med_l, 4), "lossy_ms_min": round(min(lossy_ms), 4),
            "lossy_over_pts": round(med_l / med_p, 3), "launches_per_run": launches,
            "lossy_mcell_steps_per_s": round(count * rows * cols * steps / (med_l * 1e-3) / 1e6, 1)}


def bench_periodic(count, rows, cols, steps, dtype, reps, pml_cells):
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    rng = np.random.default_rng(1)
    g = max(6, pml_cells)
    sigma = np.zeros((count, rows, cols))           # inside the PML batch's column margin too: the same for both
    sigma[:, g:rows - g, g:cols - g] = 20.0 * rng.random((count, rows - 2 * g, cols - 2 * g))
    chan = np.zeros((1, steps))
    rowf, _ = fd.batch.batch_pml_profiles(count, rows, 2 * pml_cells + 3, c00, pml_cells, dtype=dtype)
    prof = {k: rowf[:, i * rows:(i + 1) * rows] for i, k in enumerate(("ahr", "bhr", "aer", "ber"))}
    prof.update({k: np.ones(cols, dtype) for k in ("ahc", "bhc", "aec", "bec")})

    def batch(boundary):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary=boundary)
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, profiles=prof)
        b.set_point_sources([[rows // 2, cols // 2]], np.zeros((1, 1)))
        b.set_conductivity(sigma)
        b.run(steps, amps, chan).sync()                # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps, chan).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch("pml") as pml, batch("periodic") as per:
        assert per.periodic and per.lossy and pml.lossy and not pml.periodic
        l0 = per.launches
        per.reset().run(steps, amps, chan).sync()
        launches = per.launches - l0
        pml_ms, per_ms = [], []
        for _ in range(reps):
            pml_ms.append(timed(pml))
            per_ms.append(timed(per))
        paths = ["resident" if b.resident else "streamed" for b in (pml, per)]
        lds = [b.lds_bytes for b in (pml, per)]
    med_l, med_p = float(np.median(pml_ms)), float(np.median(per_ms))
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
            "materials": "arrays", "pml_cells": pml_cells, "reps": reps, "lossy_pml_path": paths[0],
            "periodic_path": paths[1], "lossy_pml_lds_bytes_per_member": lds[0], "periodic_lds_bytes_per_member": lds[1],
            "lossy_pml_ms": round(med_l, 4), "lossy_pml_ms_min": round(min(pml_ms), 4),
            "lossy_pml_ms_all": [round(v, 4) for v in pml_ms],
            "periodic_ms": round(med_p, 4), "periodic_ms_min": round(min(per_ms), 4),
            "periodic_ms_all": [round(v, 4) for v in per_ms],
            "periodic_over_lossy_pml": round(med_p / med_l, 3), "launches_per_run": launches,
            "periodic_mcell_steps_per_s": round(count * rows * cols * steps / (med_p * 1e-3) / 1e6, 1)}


def bench_flux(count, rows, cols, steps, dtype, reps, pml_cells):
    """Flux lines against the same periodic batch without monitors, and against a window DFT for scale."""
    eps, rects, amps = members(count, rows, cols, steps)
    rects[:, 1], rects[:, 3] = 0, cols - 1            # a line source over the period
    c00 = courant00(eps, dtype)
    lines = [("row", rows // 4, 0, cols - 1), ("row", 3 * rows // 4, 0, cols - 1)]
    om10 = 2 * np.pi * np.linspace(20e9, 65e9, 10)
    om16 = 2 * np.pi * np.linspace(20e9, 65e9, 16)

    def batch(kind):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="periodic")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00)
        if kind == "flux":
            b.set_flux_lines(lines, om10)
        if kind == "window":                          # as many cells as the two lines, 16 frequencies of Ez alone
            b.set_dft_window((rows // 4, 0, 2, cols - 1), om16)
        b.run(steps, amps).sync()                     # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch("plain") as plain, batch("flux") as flux, batch("window") as win:
        assert flux.resident and flux.flux_lines_in_lds and win.window_in_lds and plain.resident
        l0 = flux.launches
        flux.reset().run(steps, amps).sync()
        launches = flux.launches - l0
        t0 = time.perf_counter()
        P = flux.flux()
        flux_call_ms = (time.perf_counter() - t0) * 1e3
        ms = {"plain": [], "flux": [], "window": []}
        for _ in range(reps):
            for k, b in (("plain", plain), ("flux", flux), ("window", win)):
                ms[k].append(timed(b))
        lds = {k: b.lds_bytes for k, b in (("plain", plain), ("flux", flux), ("window", win))}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
           "materials": "arrays", "pml_cells": pml_cells, "reps": reps, "lines": 2, "line_cells": 2 * (cols - 1),
           "flux_freqs": 10, "window_freqs": 16, "launches_per_run": launches,
           "flux_call_ms": round(flux_call_ms, 4), "flux_finite": bool(np.all(np.isfinite(P)))}
    for k in ("plain", "flux", "window"):
        out.update({f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(ms[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in ms[k]], f"{k}_lds_bytes_per_member": lds[k]})
    out.update({"flux_over_plain": round(med["flux"] / med["plain"], 3),
                "window_over_plain": round(med["window"] / med["plain"], 3),
                "flux_mcell_steps_per_s": round(count * rows * cols * steps / (med["flux"] * 1e-3) / 1e6, 1)})
    return out


def bench_flux_adjoint(count, rows, cols, steps, dtype, reps, pml_cells):
    """The adjoint run with line sources against a flux run without them, and one FluxAdjointSession iteration against
    one AdjointSession iteration with 30 probes, on the same periodic members."""
    from fdtd2d_amd.adjoint import channel_system
    dt = 2e-13                                   # as --adjoint: the channels' envelope ends by step 1200
    rng = np.random.default_rng(0)
    side = 10
    design = ((rows - side) // 2, (cols - 1 - side) // 2, side, side)
    eps = np.full((count, rows, cols), fd.EPS0)
    eps[:, design[0]:design[0] + side, design[1]:design[1] + side] = np.where(
        rng.random((count, side, side)) < 0.5, fd.EPS0, 5 * fd.EPS0)
    sigma = np.zeros((count, rows, cols))        # damps the modes a periodic high-index block guides along the columns
    sigma[:, design[0]:design[0] + side, design[1]:design[1] + side] = 0.5
    rects = np.tile([pml_cells + 3, 0, 1, cols - 1], (count, 1))
    lines = [("row", rows // 4, 0, cols - 1), ("row", 3 * rows // 4, 0, cols - 1)]
    probes = np.array([[3 * rows // 4, 2 * k] for k in range(30)])
    omegas = 2 * np.pi * np.linspace(20e9, 65e9, 10)
    amps = np.tile(np.array([fd.ricker_amplitude(i * dt, FC) for i in range(steps)]), (count, 1))
    chan, A = channel_system(omegas, steps, dt, FC)
    c00 = (1 / np.sqrt(fd.EPS0 * fd.MU0) * dt) / DX
    cells = 2 * (cols - 1)
    common = dict(nsteps=steps, sources=rects, omegas=omegas, design=design, fc=FC, dt=dt, dx=DX, dtype=dtype,
                  boundary="periodic", pml_cells=pml_cells)

    def flux_objective(P):                       # the transmittance through the far line, summed over the frequencies
        g = np.zeros_like(P)
        g[:, 1, :] = 1.0
        return P[:, 1, :].sum(axis=1), g

    def probe_objective(spectra):
        mag = np.abs(spectra)
        return mag.mean(axis=1).sum(axis=1), spectra / np.maximum(mag, 1e-300) / spectra.shape[1]

    fs = fd.FluxAdjointSession(eps, sigma, flux_lines=lines, **common)
    ps = fd.AdjointSession(eps, probes=probes, **common)
    ps.set_conductivity(sigma)
    with fd.BatchEngine(count, rows, cols, dt, DX, dtype=dtype, boundary="periodic") as b:
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects).set_pml(pml_cells, courant00=c00)
        b.set_conductivity(sigma)
        b.set_dft_window(design, omegas).set_flux_lines(lines, omegas)
        b.set_flux_line_sources(1e-2 * rng.standard_normal((count, cells, 20)),
                                1e-5 * rng.standard_normal((count, cells, 20)))
        dJdP, solve = np.ones((count, 2, 10)), np.linalg.inv(A)

        def flux_run():
            b.reset().sync()
            t0 = time.perf_counter()
            b.run(steps, amps).sync()
            return (time.perf_counter() - t0) * 1e3

        def adjoint_run():
            b.reset().sync()
            t0 = time.perf_counter()
            b.run(steps, None, chan).sync()
            return (time.perf_counter() - t0) * 1e3

        def weights():
            t0 = time.perf_counter()
            b.flux_adjoint_sources(dJdP, solve)
            return (time.perf_counter() - t0) * 1e3

        def flux_session():
            t0 = time.perf_counter()
            out = fs.value_and_grad(flux_objective)
            return (time.perf_counter() - t0) * 1e3, out[3]

        def probe_session():
            t0 = time.perf_counter()
            ps.value_and_grad(probe_objective)
            return (time.perf_counter() - t0) * 1e3

        flux_run(), adjoint_run(), flux_session(), probe_session()    # warm-up: code objects, clocks
        assert b.resident and fs.engine.resident and ps.engine.resident
        l0 = fs.engine.launches
        info = flux_session()[1]
        session_launches = fs.engine.launches - l0
        t = {k: [] for k in ("flux", "adjoint_run", "weights", "flux_session", "probe_session")}
        for _ in range(reps):
            t["flux"].append(flux_run())
            t["adjoint_run"].append(adjoint_run())
            t["flux_session"].append(flux_session()[0])
            t["probe_session"].append(probe_session())
        for _ in range(reps):                        # last: they replace the timed run's weights
            t["weights"].append(weights())
        in_lds, lds = b.flux_lines_in_lds, b.lds_bytes
    fs.close()
    ps.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name, "dt": dt,
           "boundary": "periodic", "pml_cells": pml_cells, "design": list(design), "lines": 2, "line_cells": cells,
           "freqs": 10, "channels": 20, "probes": 30, "reps": reps, "weights_live_in": "global memory",
           "flux_sums_in_lds": in_lds, "lds_bytes_per_member": lds,
           "launches_per_flux_session_iteration": session_launches,
           "residual_forward_max": float(np.max(info["residual_forward"])),
           "residual_adjoint_max": float(np.max(info["residual_adjoint"]))}
    for k in t:
        out.update({f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(t[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in t[k]]})
    out.update({"adjoint_run_over_flux": round(med["adjoint_run"] / med["flux"], 3),
                "flux_over_probe_session": round(med["flux_session"] / med["probe_session"], 3)})
    return out


def bench_bloch_flux_adjoint(count, rows, cols, steps, dtype, reps, pml_cells):
    """The conjugated adjoint run with line sources against the Bloch flux run without them, and one
    BlochFluxAdjointSession iteration against one BlochAdjointSession iteration with 30 probes, on the same members."""
    from fdtd2d_amd.adjoint import channel_system
    dt = 2e-13                                   # as --flux-adjoint: the channels' envelope ends by step 1200
    rng = np.random.default_rng(0)
    side = 10
    design = ((rows - side) // 2, (cols - 1 - side) // 2, side, side)
    eps = np.full((count, rows, cols), fd.EPS0)
    eps[:, design[0]:design[0] + side, design[1]:design[1] + side] = np.where(
        rng.random((count, side, side)) < 0.5, fd.EPS0, 5 * fd.EPS0)
    sigma = np.zeros((count, rows, cols))
    sigma[:, design[0]:design[0] + side, design[1]:design[1] + side] = 0.5
    rects = np.tile([pml_cells + 3, 0, 1, cols - 1], (count, 1))
    lines = [("row", rows // 4, 0, cols - 1), ("row", 3 * rows // 4, 0, cols - 1)]
    probes = np.array([[3 * rows // 4, 2 * k] for k in range(30)])
    omegas = 2 * np.pi * np.linspace(20e9, 65e9, 10)
    phis = np.linspace(0.0, np.pi, count)
    amps = np.tile(np.array([fd.ricker_amplitude(i * dt, FC) for i in range(steps)]), (count, 1))
    camps = amps.astype(np.complex128)
    chan, A = channel_system(omegas, steps, dt, FC)
    c00 = (1 / np.sqrt(fd.EPS0 * fd.MU0) * dt) / DX
    cells = 2 * (cols - 1)
    common = dict(bloch_phase=phis, source_weights="ramp", nsteps=steps, sources=rects, omegas=omegas, design=design,
                  fc=FC, dt=dt, dx=DX, dtype=dtype, pml_cells=pml_cells)

    def flux_objective(P):                       # the transmittance through the far line, summed over the frequencies
        g = np.zeros_like(P)
        g[:, 1, :] = 1.0
        return P[:, 1, :].sum(axis=1), g

    def probe_objective(spectra):
        mag = np.abs(spectra)
        return mag.mean(axis=1).sum(axis=1), spectra / np.maximum(mag, 1e-300) / spectra.shape[1]

    fs = fd.BlochFluxAdjointSession(eps, sigma, flux_lines=lines, **common)
    ps = fd.BlochAdjointSession(eps, probes=probes, **common)
    ps.set_conductivity(sigma)
    with fd.BatchEngine(count, rows, cols, dt, DX, dtype=dtype, boundary="periodic") as b:
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects).set_pml(pml_cells, courant00=c00)
        b.set_conductivity(sigma)
        b.set_bloch_phase(phis).set_bloch_source("ramp")
        b.set_dft_window(design, omegas).set_bloch_flux_lines(lines, omegas)
        b.set_bloch_flux_line_sources(1e-2 * rng.standard_normal((count, cells, 20)),
                                      1e-5 * rng.standard_normal((count, cells, 20)))
        dJdP, solve = np.ones((count, 2, 10)), np.linalg.inv(A)

        def flux_run():
            b.reset().sync()
            t0 = time.perf_counter()
            b.run(steps, camps).sync()
            return (time.perf_counter() - t0) * 1e3

        def adjoint_run():
            b.reset().sync()
            t0 = time.perf_counter()
            b.run_bloch_channels(steps, None, chan, conjugate=True).sync()
            return (time.perf_counter() - t0) * 1e3

        def weights():
            t0 = time.perf_counter()
            b.bloch_flux_adjoint_sources(dJdP, solve)
            return (time.perf_counter() - t0) * 1e3

        def flux_session():
            t0 = time.perf_counter()
            out = fs.value_and_grad(flux_objective)
            return (time.perf_counter() - t0) * 1e3, out[3]

        def probe_session():
            t0 = time.perf_counter()
            ps.value_and_grad(probe_objective)
            return (time.perf_counter() - t0) * 1e3

        flux_run(), adjoint_run(), flux_session(), probe_session()    # warm-up: code objects, clocks
        assert b.resident and fs.engine.resident and ps.engine.resident and b.bloch
        l0, p0 = fs.engine.launches, ps.engine.launches
        info = flux_session()[1]
        probe_session()
        session_launches, probe_launches = fs.engine.launches - l0, ps.engine.launches - p0
        t = {k: [] for k in ("flux", "adjoint_run", "weights", "flux_session", "probe_session")}
        for _ in range(reps):
            t["flux"].append(flux_run())
            t["adjoint_run"].append(adjoint_run())
            t["flux_session"].append(flux_session()[0])
            t["probe_session"].append(probe_session())
        for _ in range(reps):                        # last: they replace the timed run's weights
            t["weights"].append(weights())
        in_lds, lds = b.flux_lines_in_lds, b.lds_bytes
    fs.close()
    ps.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name, "dt": dt,
           "boundary": "periodic+bloch", "pml_cells": pml_cells, "design": list(design), "lines": 2, "line_cells": cells,
           "freqs": 10, "channels": 20, "probes": 30, "reps": reps, "weights_live_in": "global memory",
           "flux_sums_in_lds": in_lds, "lds_bytes_per_member": lds,
           "launches_per_flux_session_iteration": session_launches,
           "launches_per_probe_session_iteration": probe_launches,
           "residual_forward_max": float(np.max(info["residual_forward"])),
           "residual_adjoint_max": float(np.max(info["residual_adjoint"]))}
    for k in t:
        out.update({f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(t[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in t[k]]})
    out.update({"adjoint_run_over_flux": round(med["adjoint_run"] / med["flux"], 3),
                "flux_over_probe_session": round(med["flux_session"] / med["probe_session"], 3)})
    return out


def bench_bloch_flux(count, rows, cols, steps, dtype, reps, pml_cells):
    """Flux lines on a Bloch batch against the same Bloch batch without monitors."""
    eps, rects, amps = members(count, rows, cols, steps)
    rects[:, 1], rects[:, 3] = 0, cols - 1            # a line source over the period
    c00 = courant00(eps, dtype)
    lines = [("row", rows // 4, 0, cols - 1), ("row", 3 * rows // 4, 0, cols - 1)]
    om10 = 2 * np.pi * np.linspace(20e9, 65e9, 10)
    phis = np.linspace(0.0, np.pi, count)
    camps = amps.astype(np.complex128)

    def batch(kind):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="periodic")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00).set_bloch_phase(phis).set_bloch_source("ramp")
        if kind == "flux":
            b.set_bloch_flux_lines(lines, om10)
        b.run(steps, camps).sync()                    # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, camps).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch("plain") as plain, batch("flux") as flux:
        assert flux.resident and plain.resident and flux.bloch and plain.bloch
        l0 = flux.launches
        flux.reset().run(steps, camps).sync()
        launches = flux.launches - l0
        t0 = time.perf_counter()
        P = flux.flux()
        flux_call_ms = (time.perf_counter() - t0) * 1e3
        ms = {"plain": [], "flux": []}
        for _ in range(reps):
            for k, b in (("plain", plain), ("flux", flux)):
                ms[k].append(timed(b))
        lds = {"plain": plain.lds_bytes, "flux": flux.lds_bytes}
        in_lds = flux.flux_lines_in_lds
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
           "materials": "arrays", "boundary": "periodic+bloch", "pml_cells": pml_cells, "reps": reps, "lines": 2,
           "line_cells": 2 * (cols - 1), "flux_freqs": 10, "flux_lines_in_lds": in_lds, "launches_per_run": launches,
           "flux_call_ms": round(flux_call_ms, 4), "flux_finite": bool(np.all(np.isfinite(P)))}
    for k in ("plain", "flux"):
        out.update({f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(ms[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in ms[k]], f"{k}_lds_bytes_per_member": lds[k]})
    out.update({"flux_over_plain": round(med["flux"] / med["plain"], 3),
                "flux_mcell_steps_per_s": round(count * rows * cols * steps / (med["flux"] * 1e-3) / 1e6, 1)})
    return out


def bench_dispersive(count, rows, cols, steps, dtype, reps, pml_cells):
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    rng = np.random.default_rng(1)
    g = max(6, pml_cells)
    sigma = np.zeros((count, rows, cols))
    sigma[:, g:rows - g, g:cols - g] = 20.0 * rng.random((count, rows - 2 * g, cols - 2 * g))
    wp2 = np.zeros((count, rows, cols))
    wp2[:, rows // 3:2 * rows // 3, cols // 3:2 * cols // 3] = (2 * np.pi * 70e9) ** 2
    chan = np.zeros((1, steps))

    def batch(pole):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="pml")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00)
        b.set_point_sources([[rows // 2, cols // 2]], np.zeros((1, 1)))
        b.set_conductivity(sigma)
        if pole:
            b.set_dispersion(wp2, 1e11, 0.0)
        b.run(steps, amps, chan).sync()                # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps, chan).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch(False) as pml, batch(True) as dis:
        assert dis.dispersive and dis.lossy and pml.lossy and not pml.dispersive
        l0 = dis.launches
        dis.reset().run(steps, amps, chan).sync()
        launches = dis.launches - l0
        pml_ms, dis_ms = [], []
        for _ in range(reps):
            pml_ms.append(timed(pml))
            dis_ms.append(timed(dis))
        paths = ["resident" if b.resident else "streamed" for b in (pml, dis)]
        lds = [b.lds_bytes for b in (pml, dis)]
    med_l, med_d = float(np.median(pml_ms)), float(np.median(dis_ms))
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
            "materials": "arrays", "pml_cells": pml_cells, "reps": reps, "lossy_pml_path": paths[0],
            "dispersive_path": paths[1], "lossy_pml_lds_bytes_per_member": lds[0],
            "dispersive_lds_bytes_per_member": lds[1],
            "lossy_pml_workgroups_per_cu": 163840 // lds[0], "dispersive_workgroups_per_cu": 163840 // lds[1],
            "lds_reads_per_cell_step": {"lossy_pml": 17, "dispersive": 20},
            "lds_writes_per_cell_step": {"lossy_pml": 3, "dispersive": 5},
            "lossy_pml_ms": round(med_l, 4), "lossy_pml_ms_min": round(min(pml_ms), 4),
            "lossy_pml_ms_all": [round(v, 4) for v in pml_ms],
            "dispersive_ms": round(med_d, 4), "dispersive_ms_min": round(min(dis_ms), 4),
            "dispersive_ms_all": [round(v, 4) for v in dis_ms],
            "dispersive_over_lossy_pml": round(med_d / med_l, 3), "launches_per_run": launches,
            "dispersive_mcell_steps_per_s": round(count * rows * cols * steps / (med_d * 1e-3) / 1e6, 1)}


def bench_hz(count, rows, cols, steps, dtype, reps, pml_cells):
    """The Hz polarisation with a metal strip and its pole against the Ez polarisation's dispersive kernels on the same
    periodic members, resident, timed alternately in one process."""
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    g = max(6, pml_cells)
    wp2 = np.zeros((count, rows, cols))
    wp2[:, rows // 2:rows // 2 + 2, :(cols - 1) // 2] = (2 * np.pi * 70e9) ** 2     # a strip over half the period
    rects = rects.copy()
    rects[:, 1] = np.minimum(rects[:, 1], cols - 1 - rects[:, 3])                  # off the image column

    def batch(pol):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="periodic").set_polarization(pol)
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00)
        b.set_dispersion(wp2, 1e11, 0.0)
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    assert g <= rows // 2 and rows // 2 + 2 <= rows - 1 - g
    with batch("ez") as ez, batch("hz") as hz:
        assert ez.dispersive and hz.dispersive and hz.polarization == "hz" and ez.polarization == "ez"
        l0 = hz.launches
        hz.reset().run(steps, amps).sync()
        launches = hz.launches - l0
        ez_ms, hz_ms = [], []
        for _ in range(reps):
            ez_ms.append(timed(ez))
            hz_ms.append(timed(hz))
        paths = ["resident" if b.resident else "streamed" for b in (ez, hz)]
        lds = [b.lds_bytes for b in (ez, hz)]
        finite = bool(np.all(np.isfinite(hz.download()[0])))
    med_e, med_h = float(np.median(ez_ms)), float(np.median(hz_ms))
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
            "materials": "arrays", "boundary": "periodic", "pml_cells": pml_cells, "reps": reps,
            "ez_dispersive_path": paths[0], "hz_path": paths[1], "ez_dispersive_lds_bytes_per_member": lds[0],
            "hz_lds_bytes_per_member": lds[1], "lds_arrays": {"ez_dispersive": 10, "hz": 12},
            "ez_dispersive_workgroups_per_cu": 163840 // lds[0], "hz_workgroups_per_cu": 163840 // lds[1],
            "ez_dispersive_ms": round(med_e, 4), "ez_dispersive_ms_min": round(min(ez_ms), 4),
            "ez_dispersive_ms_all": [round(v, 4) for v in ez_ms],
            "hz_ms": round(med_h, 4), "hz_ms_min": round(min(hz_ms), 4), "hz_ms_all": [round(v, 4) for v in hz_ms],
            "hz_over_ez_dispersive": round(med_h / med_e, 3), "launches_per_run": launches, "hz_finite": finite,
            "hz_mcell_steps_per_s": round(count * rows * cols * steps / (med_h * 1e-3) / 1e6, 1)}


def bench_hz_bloch(count, rows, cols, steps, dtype, reps, pml_cells):
    """A Bloch phase in the Hz polarisation (set_hz_bloch_phase, a phase sweep over the members, ramp weights) with a metal
    strip and its pole, against the real Hz kernels on the same members and against the Ez Bloch kernels with the same
    pole (--bloch-dispersive's family) on the same members; resident, timed alternately in one process."""
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    g = max(6, pml_cells)
    wp2 = np.zeros((count, rows, cols))
    wp2[:, rows // 2:rows // 2 + 2, :(cols - 1) // 2] = (2 * np.pi * 70e9) ** 2     # a strip over half the period
    rects = rects.copy()
    rects[:, 1] = np.minimum(rects[:, 1], cols - 1 - rects[:, 3])                  # off the image column
    phi = np.linspace(0.0, np.pi, count)

    def batch(kind):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="periodic")
        b.set_polarization("ez" if kind == "ez_bloch" else "hz")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00)
        if kind == "ez_bloch":
            b.set_bloch_phase(phi).set_bloch_source("ramp").set_bloch_dispersion(wp2, 1e11, 0.0)
        else:
            b.set_dispersion(wp2, 1e11, 0.0)
        if kind == "hz_bloch":
            b.set_hz_bloch_phase(phi).set_hz_bloch_source("ramp")
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    assert g <= rows // 2 and rows // 2 + 2 <= rows - 1 - g
    kinds = ("hz", "hz_bloch", "ez_bloch")
    with batch("hz") as hz, batch("hz_bloch") as hzb, batch("ez_bloch") as ezb:
        engines = (hz, hzb, ezb)
        assert all(b.dispersive for b in engines) and hzb.hz_bloch and not hz.hz_bloch and ezb.bloch and not hzb.bloch
        l0 = hzb.launches
        hzb.reset().run(steps, amps).sync()
        launches = hzb.launches - l0
        ms = {k: [] for k in kinds}
        for _ in range(reps):
            for k, b in zip(kinds, engines):
                ms[k].append(timed(b))
        paths = {k: "resident" if b.resident else "streamed" for k, b in zip(kinds, engines)}
        lds = {k: b.lds_bytes for k, b in zip(kinds, engines)}
        finite = bool(np.all(np.isfinite(hzb.download()[0])))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
           "materials": "arrays", "boundary": "periodic", "pml_cells": pml_cells, "sweep": "0..pi", "reps": reps,
           "arithmetic": fd.ARITHMETIC, "lds_arrays": {"hz": 12, "hz_bloch": 20, "ez_bloch": 16},
           "launches_per_run": launches, "hz_bloch_finite": finite}
    for k in kinds:
        out.update({f"{k}_path": paths[k], f"{k}_lds_bytes_per_member": lds[k], f"{k}_workgroups_per_cu": 163840 // lds[k],
                    f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(ms[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in ms[k]]})
    out.update({"hz_bloch_over_hz": round(med["hz_bloch"] / med["hz"], 3),
                "hz_bloch_over_ez_bloch": round(med["hz_bloch"] / med["ez_bloch"], 3),
                "hz_bloch_mcell_steps_per_s": round(count * rows * cols * steps / (med["hz_bloch"] * 1e-3) / 1e6, 1)})
    return out


def bench_hz_lattice(count, rows, cols, steps, dtype, reps):
    """The lattice mode of the Hz polarisation (set_hz_lattice_phase, the k-path Gamma-X-M-Gamma over the members, ramp
    weights) with a metal rod and its pole, against the Ez lattice kernels with the pole of set_bloch_dispersion on the
    same members and against the same Hz lattice batch without the pole; resident, timed alternately in one process."""
    eps, rects, amps = members(count, rows, cols, steps)
    wp2 = np.zeros((count, rows, cols))
    wp2[:, rows // 3:2 * rows // 3, cols // 3:2 * cols // 3] = (2 * np.pi * 70e9) ** 2       # the rod
    rects = rects.copy()
    rects[:, 0] = np.minimum(rects[:, 0], rows - 1 - rects[:, 2])                  # off the image row
    rects[:, 1] = np.minimum(rects[:, 1], cols - 1 - rects[:, 3])                  # off the image column
    phi_r, phi_c = k_path(count)

    def batch(kind):
        ez = kind == "ez_lattice"
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="lattice" if ez else "periodic")
        if not ez:
            b.set_polarization("hz")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        if ez:
            b.set_lattice_phase(phi_r, phi_c).set_bloch_source("ramp").set_bloch_dispersion(wp2, 1e11, 0.0)
        else:
            b.set_hz_lattice_phase(phi_r, phi_c).set_hz_bloch_source("ramp")
            if kind == "hz_lattice":
                b.set_dispersion(wp2, 1e11, 0.0)
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    kinds = ("hz_lattice", "ez_lattice", "hz_lattice_plain")
    with batch(kinds[0]) as hzl, batch(kinds[1]) as ezl, batch(kinds[2]) as pla:
        engines = (hzl, ezl, pla)
        assert hzl.hz_lattice and pla.hz_lattice and ezl.lattice and not hzl.lattice and not ezl.hz_lattice
        assert hzl.dispersive and ezl.dispersive and not pla.dispersive
        l0 = hzl.launches
        hzl.reset().run(steps, amps).sync()
        launches = hzl.launches - l0
        ms = {k: [] for k in kinds}
        for _ in range(reps):
            for k, b in zip(kinds, engines):
                ms[k].append(timed(b))
        paths = {k: "resident" if b.resident else "streamed" for k, b in zip(kinds, engines)}
        lds = {k: b.lds_bytes for k, b in zip(kinds, engines)}
        finite = bool(np.all(np.isfinite(hzl.download()[0])))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
           "materials": "arrays", "boundary": "periodic", "k_path": "Gamma-X-M-Gamma", "reps": reps,
           "arithmetic": fd.ARITHMETIC, "lds_arrays": {"hz_lattice": 18, "ez_lattice": 14, "hz_lattice_plain": 9},
           "launches_per_run": launches, "hz_lattice_finite": finite}
    for k in kinds:
        out.update({f"{k}_path": paths[k], f"{k}_lds_bytes_per_member": lds[k], f"{k}_workgroups_per_cu": 163840 // lds[k],
                    f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(ms[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in ms[k]]})
    out.update({"hz_lattice_over_ez_lattice": round(med["hz_lattice"] / med["ez_lattice"], 3),
                "hz_lattice_over_plain": round(med["hz_lattice"] / med["hz_lattice_plain"], 3),
                "hz_lattice_mcell_steps_per_s": round(count * rows * cols * steps / (med["hz_lattice"] * 1e-3) / 1e6, 1)})
    return out


def bench_hz_bloch_flux(count, rows, cols, steps, dtype, reps, pml_cells):
    """Two whole-period row lines at 10 frequencies on the member of --hz-bloch (a phase sweep, ramp weights, the metal
    strip with its pole) against the same member without them; resident, timed alternately in one process."""
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    g = max(6, pml_cells)
    wp2 = np.zeros((count, rows, cols))
    wp2[:, rows // 2:rows // 2 + 2, :(cols - 1) // 2] = (2 * np.pi * 70e9) ** 2     # a strip over half the period
    rects = rects.copy()
    rects[:, 1] = np.minimum(rects[:, 1], cols - 1 - rects[:, 3])                  # off the image column
    phi = np.linspace(0.0, np.pi, count)
    lines = [("row", rows // 4, 0, cols - 1), ("row", 3 * rows // 4, 0, cols - 1)]
    om10 = 2 * np.pi * np.linspace(20e9, 65e9, 10)
    assert g <= rows // 2 and rows // 2 + 2 <= rows - 1 - g

    def batch(kind):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="periodic")
        b.set_polarization("hz")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00)
        b.set_dispersion(wp2, 1e11, 0.0)
        b.set_hz_bloch_phase(phi).set_hz_bloch_source("ramp")
        if kind == "hz_bloch_flux":
            b.set_hz_bloch_flux_lines(lines, om10)
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    kinds = ("hz_bloch", "hz_bloch_flux")
    with batch("hz_bloch") as hzb, batch("hz_bloch_flux") as hzf:
        bs = dict(zip(kinds, (hzb, hzf)))
        assert all(b.resident and b.dispersive and b.hz_bloch for b in bs.values())
        l0 = hzf.launches
        hzf.reset().run(steps, amps).sync()
        launches = hzf.launches - l0
        t0 = time.perf_counter()
        P = hzf.flux()
        flux_call_ms = (time.perf_counter() - t0) * 1e3
        ms = {k: [] for k in kinds}
        for _ in range(reps):
            for k in kinds:
                ms[k].append(timed(bs[k]))
        lds = {k: b.lds_bytes for k, b in bs.items()}
        in_lds = hzf.flux_lines_in_lds
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
           "materials": "arrays", "boundary": "periodic", "pml_cells": pml_cells, "sweep": "0..pi", "reps": reps,
           "arithmetic": fd.ARITHMETIC, "lines": 2, "line_cells": 2 * (cols - 1), "flux_freqs": 10,
           "launches_per_run": launches, "flux_call_ms": round(flux_call_ms, 4),
           "flux_finite": bool(np.all(np.isfinite(P))), "hz_bloch_flux_lines_in_lds": in_lds,
           "hz_bloch_flux_sums": "lds" if in_lds else "global", "sums_bytes_per_member": 64 * 10 * 2 * (cols - 1)}
    for k in kinds:
        out.update({f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(ms[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in ms[k]], f"{k}_lds_bytes_per_member": lds[k]})
    out.update({"hz_bloch_flux_over_hz_bloch": round(med["hz_bloch_flux"] / med["hz_bloch"], 3),
                "hz_bloch_flux_mcell_steps_per_s": round(count * rows * cols * steps / (med["hz_bloch_flux"] * 1e-3) / 1e6, 1)})
    return out


def bench_hz_flux(count, rows, cols, steps, dtype, reps, pml_cells):
    """Two whole-period row lines at 10 frequencies on the Hz member of --hz against the same member without them, and
    the same lines on the lossless Ez member of --flux at this shape against that member without them."""
    eps, rects, amps = members(count, rows, cols, steps)
    rects[:, 1], rects[:, 3] = 0, cols - 1            # a line source over the period
    c00 = courant00(eps, dtype)
    g = max(6, pml_cells)
    wp2 = np.zeros((count, rows, cols))
    wp2[:, rows // 2:rows // 2 + 2, :(cols - 1) // 2] = (2 * np.pi * 70e9) ** 2     # a strip over half the period
    lines = [("row", rows // 4, 0, cols - 1), ("row", 3 * rows // 4, 0, cols - 1)]
    om10 = 2 * np.pi * np.linspace(20e9, 65e9, 10)
    assert g <= rows // 2 and rows // 2 + 2 <= rows - 1 - g

    def batch(kind):
        hz = kind.startswith("hz")
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="periodic")
        b.set_polarization("hz" if hz else "ez")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00)
        if hz:
            b.set_dispersion(wp2, 1e11, 0.0)
        if kind == "hz_flux":
            b.set_hz_flux_lines(lines, om10)
        if kind in ("ez_flux", "ez_flux_global"):     # the second with its sums in global memory, where the Hz member's
            b.set_flux_lines(lines, om10)             # live when the pole's twelve arrays leave them no room in LDS
            b.set_flux_lds(kind == "ez_flux")
        b.run(steps, amps).sync()                     # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    kinds = ("hz", "hz_flux", "ez", "ez_flux", "ez_flux_global")
    with batch("hz") as hz, batch("hz_flux") as hzf, batch("ez") as ez, batch("ez_flux") as ezf, \
            batch("ez_flux_global") as ezg:
        bs = dict(zip(kinds, (hz, hzf, ez, ezf, ezg)))
        assert all(b.resident for b in bs.values()) and hz.dispersive and hzf.dispersive
        assert hzf.polarization == "hz" and ezf.polarization == "ez"
        l0 = hzf.launches
        hzf.reset().run(steps, amps).sync()
        launches = hzf.launches - l0
        t0 = time.perf_counter()
        P = hzf.flux()
        flux_call_ms = (time.perf_counter() - t0) * 1e3
        ms = {k: [] for k in kinds}
        for _ in range(reps):
            for k in kinds:
                ms[k].append(timed(bs[k]))
        lds = {k: b.lds_bytes for k, b in bs.items()}
        in_lds = {k: b.flux_lines_in_lds for k, b in bs.items() if "flux" in k}
        assert not in_lds["ez_flux_global"]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
           "materials": "arrays", "boundary": "periodic", "pml_cells": pml_cells, "reps": reps, "lines": 2,
           "line_cells": 2 * (cols - 1), "flux_freqs": 10, "launches_per_run": launches,
           "flux_call_ms": round(flux_call_ms, 4), "flux_finite": bool(np.all(np.isfinite(P))),
           "hz_flux_lines_in_lds": in_lds["hz_flux"], "ez_flux_lines_in_lds": in_lds["ez_flux"]}
    for k in kinds:
        out.update({f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(ms[k]), 4),
                    f"{k}_ms_all": [round(v, 4) for v in ms[k]], f"{k}_lds_bytes_per_member": lds[k]})
    r_hz, r_ez = med["hz_flux"] / med["hz"], med["ez_flux"] / med["ez"]
    out.update({"hz_flux_over_hz": round(r_hz, 3), "ez_flux_over_ez": round(r_ez, 3),
                "ez_flux_global_over_ez": round(med["ez_flux_global"] / med["ez"], 3),
                "hz_ratio_over_ez_ratio": round(r_hz / r_ez, 3),
                "hz_flux_mcell_steps_per_s": round(count * rows * cols * steps / (med["hz_flux"] * 1e-3) / 1e6, 1)})
    return out


def bench_bloch(count, rows, cols, steps, dtype, reps, pml_cells):
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    rng = np.random.default_rng(1)
    g = max(6, pml_cells)
    sigma = np.zeros((count, rows, cols))
    sigma[:, g:rows - g, :] = 20.0 * rng.random((count, rows - 2 * g, cols))
    phis = np.linspace(0.0, np.pi, count)

    def batch(bloch):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="periodic")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        b.set_pml(pml_cells, courant00=c00).set_conductivity(sigma)
        if bloch:
            b.set_bloch_phase(phis).set_bloch_source("ramp")
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch(False) as per, batch(True) as blo:
        assert blo.bloch and blo.periodic and per.periodic and not per.bloch
        l0 = blo.launches
        blo.reset().run(steps, amps).sync()
        launches = blo.launches - l0
        per_ms, blo_ms = [], []
        for _ in range(reps):
            per_ms.append(timed(per))
            blo_ms.append(timed(blo))
        paths = ["resident" if b.resident else "streamed" for b in (per, blo)]
        lds = [b.lds_bytes for b in (per, blo)]
    med_p, med_b = float(np.median(per_ms)), float(np.median(blo_ms))
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
            "materials": "arrays", "pml_cells": pml_cells, "reps": reps, "periodic_path": paths[0], "bloch_path": paths[1],
            "periodic_lds_bytes_per_member": lds[0], "bloch_lds_bytes_per_member": lds[1],
            "periodic_ms": round(med_p, 4), "periodic_ms_min": round(min(per_ms), 4),
            "periodic_ms_all": [round(v, 4) for v in per_ms],
            "bloch_ms": round(med_b, 4), "bloch_ms_min": round(min(blo_ms), 4),
            "bloch_ms_all": [round(v, 4) for v in blo_ms],
            "bloch_over_periodic": round(med_b / med_p, 3), "launches_per_run": launches,
            "bloch_mcell_steps_per_s": round(count * rows * cols * steps / (med_b * 1e-3) / 1e6, 1)}


def k_path(count):
    """(phi_rows, phi_cols), each (count,): the path Gamma-X-M-Gamma of a rectangular lattice, a third of the members on
    each leg."""
    t = np.linspace(0.0, 3.0, count, endpoint=False)
    phi_r = np.pi * np.where(t < 1, t, np.where(t < 2, 1.0, 3.0 - t))
    phi_c = np.pi * np.where(t < 1, 0.0, np.where(t < 2, t - 1.0, 3.0 - t))
    return phi_r, phi_c


def bench_lattice(count, rows, cols, steps, dtype, reps):
    eps, rects, amps = members(count, rows, cols, steps)
    rng = np.random.default_rng(1)
    sigma = np.zeros((count, rows, cols))
    sigma[:, 6:rows - 6, :] = 20.0 * rng.random((count, rows - 12, cols))
    phi_r, phi_c = k_path(count)

    def batch(lattice):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="lattice" if lattice else "periodic")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects).set_conductivity(sigma)
        if lattice:
            b.set_lattice_phase(phi_r, phi_c).set_bloch_source("ramp")
        else:
            b.set_bloch_phase(phi_c).set_bloch_source("ramp")
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch(False) as blo, batch(True) as lat:
        assert lat.lattice and lat.periodic and blo.bloch and not blo.lattice and not blo.pml
        l0 = lat.launches
        lat.reset().run(steps, amps).sync()
        launches = lat.launches - l0
        blo_ms, lat_ms = [], []
        for _ in range(reps):
            blo_ms.append(timed(blo))
            lat_ms.append(timed(lat))
        paths = ["resident" if b.resident else "streamed" for b in (blo, lat)]
        lds = [b.lds_bytes for b in (blo, lat)]
    med_b, med_l = float(np.median(blo_ms)), float(np.median(lat_ms))
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name,
            "materials": "arrays", "k_path": "Gamma-X-M-Gamma", "reps": reps, "bloch_path": paths[0],
            "lattice_path": paths[1], "bloch_lds_bytes_per_member": lds[0], "lattice_lds_bytes_per_member": lds[1],
            "bloch_ms": round(med_b, 4), "bloch_ms_min": round(min(blo_ms), 4),
            "bloch_ms_all": [round(v, 4) for v in blo_ms],
            "lattice_ms": round(med_l, 4), "lattice_ms_min": round(min(lat_ms), 4),
            "lattice_ms_all": [round(v, 4) for v in lat_ms],
            "lattice_over_bloch": round(med_l / med_b, 3), "launches_per_run": launches,
            "lattice_mcell_steps_per_s": round(count * rows * cols * steps / (med_l * 1e-3) / 1e6, 1)}


def bench_bloch_dispersive(count, rows, cols, steps, dtype, reps, pml_cells, lattice):
    eps, rects, amps = members(count, rows, cols, steps)
    c00 = courant00(eps, dtype)
    rng = np.random.default_rng(1)
    g = 0 if lattice else max(6, pml_cells)
    sigma = np.zeros((count, rows, cols))
    sigma[:, g:rows - g, :] = 20.0 * rng.random((count, rows - 2 * g, cols))
    wp2 = np.zeros((count, rows, cols))
    wp2[:, rows // 3:2 * rows // 3, cols // 3:2 * cols // 3] = (2 * np.pi * 70e9) ** 2
    assert not wp2[:, :g].any() and not wp2[:, rows - g:].any(), "the block must keep clear of the layer"
    phi_r, phi_c = k_path(count)

    def batch(pole):
        b = fd.BatchEngine(count, rows, cols, DT, DX, dtype=dtype, boundary="lattice" if lattice else "periodic")
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects)
        if lattice:
            b.set_lattice_phase(phi_r, phi_c)
        else:
            b.set_pml(pml_cells, courant00=c00).set_bloch_phase(np.linspace(0.0, np.pi, count))
        b.set_conductivity(sigma).set_bloch_source("ramp")
        if pole:
            b.set_bloch_dispersion(wp2, 1e11, 0.0)
        b.run(steps, amps).sync()                      # warm-up: code objects, clocks
        return b

    def timed(b):
        b.reset().sync()
        t0 = time.perf_counter()
        b.run(steps, amps).sync()
        return (time.perf_counter() - t0) * 1e3

    with batch(False) as pla, batch(True) as dis:
        assert dis.dispersive and not pla.dispersive and dis.lattice == pla.lattice == lattice
        l0 = dis.launches
        dis.reset().run(steps, amps).sync()
        launches = dis.launches - l0
        pla_ms, dis_ms = [], []
        for _ in range(reps):
            pla_ms.append(timed(pla))
            dis_ms.append(timed(dis))
        paths = ["resident" if b.resident else "streamed" for b in (pla, dis)]
        lds = [b.lds_bytes for b in (pla, dis)]
    med_p, med_d = float(np.median(pla_ms)), float(np.median(dis_ms))
    return {"family": "lattice" if lattice else "bloch", "count": count, "rows": rows, "cols": cols, "steps": steps,
            "dtype": np.dtype(dtype).name, "materials": "arrays", "pml_cells": 0 if lattice else pml_cells,
            "sweep": "Gamma-X-M-Gamma" if lattice else "0..pi", "reps": reps, "arithmetic": fd.ARITHMETIC,
            "plain_path": paths[0], "dispersive_path": paths[1], "plain_lds_bytes_per_workgroup": lds[0],
            "dispersive_lds_bytes_per_workgroup": lds[1], "plain_workgroups_per_cu": 163840 // lds[0],
            "dispersive_workgroups_per_cu": 163840 // lds[1],
            "plain_ms": round(med_p, 4), "plain_ms_min": round(min(pla_ms), 4), "plain_ms_all": [round(v, 4) for v in pla_ms],
            "dispersive_ms": round(med_d, 4), "dispersive_ms_min": round(min(dis_ms), 4),
            "dispersive_ms_all": [round(v, 4) for v in dis_ms],
            "dispersive_over_plain": round(med_d / med_p, 3), "launches_per_run": launches,
            "dispersive_mcell_steps_per_s": round(count * rows * cols * steps / (med_d * 1e-3) / 1e6, 1)}


def bench_adjoint(count, rows, cols, steps, dtype, reps, pml_cells):
    from fdtd2d_amd.adjoint import channel_system, gradient_coefficients
    dt = 2e-13                                   # the Gaussian envelope of the channels (t0 = 4.5 / fc) ends by step 1200
    rng = np.random.default_rng(0)
    eps = np.where(rng.random((count, rows, cols)) < 0.5, fd.EPS0, 5 * fd.EPS0)
    side = 10 if min(rows, cols) < 200 else 100
    design = ((rows - side) // 2, (cols - side) // 2, side, side)
    rects = np.tile([rows // 2, design[1] - 8, 1, 1], (count, 1))
    probes = np.array([[rows // 2 - 15 + k, design[1] + side + 8] for k in range(30)])
    omegas = 2 * np.pi * np.linspace(10e9, 100e9, 10)
    amps = np.tile(np.array([fd.ricker_amplitude(i * dt, FC) for i in range(steps)]), (count, 1))
    c00 = (1 / np.sqrt(eps[:, 0, 0].astype(dtype).astype(np.float64) * fd.MU0) * dt) / DX

    def objective(spectra):
        mag = np.abs(spectra)
        return mag.mean(axis=1).sum(axis=1), spectra / np.maximum(mag, 1e-300) / spectra.shape[1]

    info = {}

    def gradient():
        t0 = time.perf_counter()
        out = fd.batch_eps_gradient(eps, nsteps=steps, sources=rects, probes=probes, omegas=omegas, design=design,
                                    objective=objective, fc=FC, dt=dt, dx=DX, dtype=dtype, boundary="pml",
                                    pml_cells=pml_cells)
        info.update(out[3])
        return (time.perf_counter() - t0) * 1e3

    from fdtd2d_amd.adjoint import probe_spectra as host_spectra
    chan, _ = channel_system(omegas, steps, dt, FC)
    session = fd.AdjointSession(eps, nsteps=steps, sources=rects, probes=probes, omegas=omegas, design=design, fc=FC,
                                dt=dt, dx=DX, dtype=dtype, boundary="pml", pml_cells=pml_cells)
    om = np.tile(omegas, (count, 1))
    new_window = np.where(rng.random((count, side, side)) < 0.5, fd.EPS0, 5 * fd.EPS0)
    weights = rng.standard_normal((count, 30, 20))
    coef = gradient_coefficients(omegas, dt)
    with fd.BatchEngine(count, rows, cols, dt, DX, dtype=dtype, boundary="pml") as b:
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects).set_pml(pml_cells, courant00=c00)
        b.set_dft_window(design, omegas).set_probes(probes, steps).set_point_sources(probes, weights)

        def two_runs():
            t0 = time.perf_counter()
            for _ in range(2):
                b.reset().run(steps, amps)
            b.sync()
            return (time.perf_counter() - t0) * 1e3

        def device():
            t0 = time.perf_counter()
            b.reset().run(steps, amps).hold_dft_window().reset().run(steps, None, chan)
            b.dft_window_product(coef)
            return (time.perf_counter() - t0) * 1e3

        def product():
            t0 = time.perf_counter()
            b.dft_window_product(coef)
            return (time.perf_counter() - t0) * 1e3

        def download():
            t0 = time.perf_counter()
            held, cur = b.read_dft_window(), b.read_dft_window()
            (coef[None, :, None, None] * held * cur).real.sum(axis=1)
            return (time.perf_counter() - t0) * 1e3

        def iteration():
            t0 = time.perf_counter()
            session.value_and_grad(objective)
            return (time.perf_counter() - t0) * 1e3

        def spectra_device():
            t0 = time.perf_counter()
            b.probe_spectra(om, 0, steps, peak=True)
            return (time.perf_counter() - t0) * 1e3

        def spectra_host():
            t0 = time.perf_counter()
            host_spectra(b.read_probes(0, steps), om, dt)
            return (time.perf_counter() - t0) * 1e3

        def eps_window():
            t0 = time.perf_counter()
            session.engine.set_eps_window(design, new_window)
            return (time.perf_counter() - t0) * 1e3

        def materials():
            t0 = time.perf_counter()
            b.set_materials(eps.astype(dtype), fd.MU0)
            return (time.perf_counter() - t0) * 1e3

        two_runs(), device(), gradient(), iteration()    # warm-up: code objects, clocks
        l0 = b.launches
        device()
        launches = b.launches - l0
        l0 = session.engine.launches
        iteration()
        session_launches = session.engine.launches - l0
        t = {k: [] for k in ("grad", "two", "device", "product", "download", "session", "spectra_device",
                             "spectra_host", "eps_window", "materials")}
        for _ in range(reps):
            t["two"].append(two_runs())
            t["device"].append(device())
            t["grad"].append(gradient())
            t["session"].append(iteration())
            t["product"].append(product())
            t["download"].append(download())
            t["spectra_device"].append(spectra_device())
            t["spectra_host"].append(spectra_host())
            t["eps_window"].append(eps_window())
            t["materials"].append(materials())
        resident, in_lds, lds = b.resident, b.window_in_lds, b.lds_bytes
    session.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name, "dt": dt,
            "boundary": "pml", "pml_cells": pml_cells, "design": list(design), "freqs": 10, "probes": 30, "channels": 20,
            "path": "resident" if resident else "streamed", "window_in_lds": in_lds,
            "lds_bytes_per_member": lds if resident else None, "reps": reps,
            "grad_ms": round(med["grad"], 3), "grad_ms_min": round(min(t["grad"]), 3),
            "two_runs_ms": round(med["two"], 3), "two_runs_ms_min": round(min(t["two"]), 3),
            "device_ms": round(med["device"], 3), "device_ms_min": round(min(t["device"]), 3),
            "grad_over_two_runs": round(med["grad"] / med["two"], 3),
            "device_over_two_runs": round(med["device"] / med["two"], 3), "launches_per_gradient": launches,
            "product_ms": round(med["product"], 3), "download_ms": round(med["download"], 3),
            "download_over_product": round(med["download"] / med["product"], 2),
            "session_ms": round(med["session"], 3), "session_ms_min": round(min(t["session"]), 3),
            "session_over_two_runs": round(med["session"] / med["two"], 3),
            "session_over_device": round(med["session"] / med["device"], 3),
            "grad_over_session": round(med["grad"] / med["session"], 2),
            "launches_per_session_iteration": session_launches,
            "spectra_device_ms": round(med["spectra_device"], 3), "spectra_host_ms": round(med["spectra_host"], 3),
            "spectra_trace_bytes": count * 30 * steps * 8,
            "eps_window_ms": round(med["eps_window"], 3), "set_materials_ms": round(med["materials"], 3),
            "condition": round(float(info["condition"]), 2),
            "residual_forward_max": float(np.max(info["residual_forward"])),
            "residual_adjoint_max": float(np.max(info["residual_adjoint"]))}


def bench_bloch_adjoint(count, rows, cols, steps, dtype, reps, pml_cells):
    from fdtd2d_amd.adjoint import channel_system, gradient_coefficients
    dt = 2e-13                                   # as --adjoint: the channels' envelope ends by step 1200
    rng = np.random.default_rng(0)
    eps = np.where(rng.random((count, rows, cols)) < 0.5, fd.EPS0, 5 * fd.EPS0)
    eps[:, :, -1] = eps[:, :, 0]
    side, g = 10, max(6, pml_cells)
    design = ((rows - side) // 2, (cols - side) // 2, side, side)
    rects = np.tile([g + 2, 0, 1, cols - 1], (count, 1))
    probes = np.array([[rows // 2 - 15 + k, design[1] + side + 8] for k in range(30)])
    sigma = np.zeros((count, rows, cols))
    sigma[:, g:rows - g, :] = 2.0 * rng.random((count, rows - 2 * g, cols))
    sigma[:, probes[:, 0], probes[:, 1]] = 0     # the probe cells do not conduct
    omegas = 2 * np.pi * np.linspace(10e9, 100e9, 10)
    phis = np.linspace(0.0, np.pi, count)
    amps = np.tile(np.array([fd.ricker_amplitude(i * dt, FC) for i in range(steps)]), (count, 1))
    c00 = (1 / np.sqrt(eps[:, 0, 0].astype(dtype).astype(np.float64) * fd.MU0) * dt) / DX

    def objective(spectra):
        mag = np.abs(spectra)
        return mag.mean(axis=1).sum(axis=1), spectra / np.maximum(mag, 1e-300) / spectra.shape[1]

    chan, _ = channel_system(omegas, steps, dt, FC)
    session = fd.BlochAdjointSession(eps, bloch_phase=phis, source_weights="ramp", nsteps=steps, sources=rects,
                                     probes=probes, omegas=omegas, design=design, fc=FC, dt=dt, dx=DX, dtype=dtype,
                                     pml_cells=pml_cells)
    session.set_conductivity(sigma)
    weights = rng.standard_normal((count, 30, 20))
    coef = gradient_coefficients(omegas, dt)
    info = {}
    with fd.BatchEngine(count, rows, cols, dt, DX, dtype=dtype, boundary="periodic") as b:
        b.set_materials(eps.astype(dtype), fd.MU0).set_sources(rects).set_pml(pml_cells, courant00=c00)
        b.set_conductivity(sigma).set_bloch_phase(phis).set_bloch_source("ramp")
        b.set_dft_window(design, omegas).set_probes(probes, steps).set_bloch_point_sources(probes, weights)

        def two_runs():
            t0 = time.perf_counter()
            for _ in range(2):
                b.reset().run(steps, amps)
            b.sync()
            return (time.perf_counter() - t0) * 1e3

        def device():
            t0 = time.perf_counter()
            b.reset().run(steps, amps).hold_bloch_window().reset().run_bloch_channels(steps, None, chan, conjugate=True)
            b.bloch_window_product(coef)
            return (time.perf_counter() - t0) * 1e3

        def iteration():
            t0 = time.perf_counter()
            info.update(session.value_and_grad(objective)[3])
            return (time.perf_counter() - t0) * 1e3

        two_runs(), device(), iteration()            # warm-up: code objects, clocks
        l0 = b.launches
        device()
        launches = b.launches - l0
        l0 = session.engine.launches
        iteration()
        session_launches = session.engine.launches - l0
        t = {k: [] for k in ("two", "device", "session")}
        for _ in range(reps):
            t["two"].append(two_runs())
            t["device"].append(device())
            t["session"].append(iteration())
        resident, in_lds, lds = b.resident, b.window_in_lds, b.lds_bytes
    session.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name, "dt": dt,
            "boundary": "periodic+bloch", "pml_cells": pml_cells, "design": list(design), "freqs": 10, "probes": 30,
            "channels": 20, "path": "resident" if resident else "streamed", "window_in_lds": in_lds,
            "lds_bytes_per_member": lds if resident else None, "reps": reps,
            "two_runs_ms": round(med["two"], 3), "two_runs_ms_min": round(min(t["two"]), 3),
            "two_runs_ms_all": [round(v, 3) for v in t["two"]],
            "device_ms": round(med["device"], 3), "device_ms_min": round(min(t["device"]), 3),
            "device_ms_all": [round(v, 3) for v in t["device"]],
            "device_over_two_runs": round(med["device"] / med["two"], 3), "launches_per_gradient": launches,
            "session_ms": round(med["session"], 3), "session_ms_min": round(min(t["session"]), 3),
            "session_over_two_runs": round(med["session"] / med["two"], 3),
            "session_over_device": round(med["session"] / med["device"], 3),
            "launches_per_session_iteration": session_launches,
            "residual_forward_max": float(np.max(info["residual_forward"])),
            "residual_adjoint_max": float(np.max(info["residual_adjoint"]))}


def bench_dispersive_adjoint(count, rows, cols, steps, dtype, reps, pml_cells):
    dt = 2e-13                                   # as --adjoint: the channels' envelope ends by step 1200
    rng = np.random.default_rng(0)
    eps = np.where(rng.random((count, rows, cols)) < 0.5, fd.EPS0, 5 * fd.EPS0)
    side, g = 10, max(6, pml_cells)
    r0, c0 = (rows - side) // 2, (cols - side) // 2
    design = (r0, c0, side, side)
    rects = np.tile([g + 2, g + 2, 1, 1], (count, 1))
    probes = np.array([[rows // 2 - 15 + k, c0 + side + 8] for k in range(30)])
    sigma, wp2 = np.zeros((count, rows, cols)), np.zeros((count, rows, cols))
    sigma[:, r0:r0 + side, c0:c0 + side] = 2.0 * rng.random((count, side, side))
    wp2[:, r0:r0 + side, c0:c0 + side] = (2 * np.pi * 70e9) ** 2 * (0.5 + rng.random((count, side, side)))
    omegas = 2 * np.pi * np.linspace(10e9, 100e9, 10)
    args = dict(nsteps=steps, sources=rects, probes=probes, omegas=omegas, design=design, fc=FC, dt=dt, dx=DX,
                dtype=dtype, boundary="pml", pml_cells=pml_cells)

    def objective(spectra):
        mag = np.abs(spectra)
        return mag.mean(axis=1).sum(axis=1), spectra / np.maximum(mag, 1e-300) / spectra.shape[1]

    info = {}
    with fd.DispersiveAdjointSession(eps, dispersion=(wp2, 1e11, 0.0), sigma=sigma, **args) as pole, \
            fd.AdjointSession(eps, **args) as lossy:
        lossy.set_conductivity(sigma)

        def dispersive():
            t0 = time.perf_counter()
            info.update(pole.value_and_grad(objective)[3])
            pole.sigma_gradient(), pole.wp2_gradient()
            return (time.perf_counter() - t0) * 1e3

        def plain():
            t0 = time.perf_counter()
            lossy.value_and_grad(objective)
            lossy.sigma_gradient()
            return (time.perf_counter() - t0) * 1e3

        eng, coefs, scales = pole.engine, pole._coefs, pole._scales

        def multi():
            t0 = time.perf_counter()
            eng.dispersive_window_product(coefs, scales)
            return (time.perf_counter() - t0) * 1e3

        def three():
            t0 = time.perf_counter()
            for k in range(3):
                eng.dispersive_window_product(coefs[k:k + 1], scales[:, k:k + 1])
            return (time.perf_counter() - t0) * 1e3

        dispersive(), plain(), multi(), three()      # warm-up: code objects, clocks
        launches = {}
        for name, s, call in (("dispersive", pole, dispersive), ("lossy", lossy, plain)):
            l0 = s.engine.launches
            call()
            launches[name] = s.engine.launches - l0
        t = {k: [] for k in ("dispersive", "lossy", "multi", "three")}
        for _ in range(reps):
            t["dispersive"].append(dispersive())
            t["lossy"].append(plain())
            t["multi"].append(multi())
            t["three"].append(three())
        paths = {k: "resident" if s.engine.resident else "streamed" for k, s in (("dispersive", pole), ("lossy", lossy))}
        lds = {k: s.engine.lds_bytes for k, s in (("dispersive", pole), ("lossy", lossy))}
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"count": count, "rows": rows, "cols": cols, "steps": steps, "dtype": np.dtype(dtype).name, "dt": dt,
            "boundary": "pml", "pml_cells": pml_cells, "design": list(design), "freqs": 10, "probes": 30, "channels": 20,
            "reps": reps, "dispersive_path": paths["dispersive"], "lossy_path": paths["lossy"],
            "dispersive_lds_bytes": lds["dispersive"], "lossy_lds_bytes": lds["lossy"],
            "dispersive_ms": round(med["dispersive"], 3), "dispersive_ms_all": [round(v, 3) for v in t["dispersive"]],
            "lossy_ms": round(med["lossy"], 3), "lossy_ms_all": [round(v, 3) for v in t["lossy"]],
            "dispersive_over_lossy": round(med["dispersive"] / med["lossy"], 3),
            "launches_per_dispersive_iteration": launches["dispersive"],
            "launches_per_lossy_iteration": launches["lossy"],
            "multi_product_ms": round(med["multi"], 3), "multi_product_ms_all": [round(v, 3) for v in t["multi"]],
            "three_products_ms": round(med["three"], 3), "three_products_ms_all": [round(v, 3) for v in t["three"]],
            "multi_over_three": round(med["multi"] / med["three"], 3),
            "residual_forward_max": float(np.max(info["residual_forward"])),
            "residual_adjoint_max": float(np.max(info["residual_adjoint"]))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--count", type=int)
    ap.add_argument("--rows", type=int)
    ap.add_argument("--cols", type=int)
    ap.add_argument("--steps", type=int)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-members", type=int, default=16, help="members timed one Engine at a time (0: none)")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="shader clock of the LDS bound")
    ap.add_argument("--boundary", default="mur", choices=["mur", "pml"])
    ap.add_argument("--pml-cells", type=int, default=10, help="layer depth with --boundary pml")
    ap.add_argument("--monitors", action="store_true", help="time the window DFT and probes (see above)")
    ap.add_argument("--adjoint", action="store_true", help="time batch_eps_gradient (see above)")
    ap.add_argument("--lossy", action="store_true", help="time the lossy kernels against the point-source ones")
    ap.add_argument("--periodic", action="store_true", help="time the periodic kernels against the lossy PML ones")
    ap.add_argument("--bloch", action="store_true", help="time a Bloch batch against the plain periodic one")
    ap.add_argument("--bloch-adjoint", action="store_true", help="time the adjoint gradient of a Bloch batch")
    ap.add_argument("--dispersive", action="store_true", help="time the dispersive kernels against the lossy PML ones")
    ap.add_argument("--lattice", action="store_true", help="time a lattice batch against the Bloch batch without a layer")
    ap.add_argument("--bloch-dispersive", action="store_true",
                    help="time the pole of a lattice and of a Bloch batch against the same batches without it")
    ap.add_argument("--dispersive-adjoint", action="store_true",
                    help="time the three gradients of a dispersive batch against the two of the same lossy batch")
    ap.add_argument("--flux", action="store_true", help="time flux lines against the same batch without monitors")
    ap.add_argument("--bloch-flux", action="store_true",
                    help="time flux lines on a Bloch batch against the same batch without monitors")
    ap.add_argument("--bloch-flux-adjoint", action="store_true",
                    help="time the adjoint of a flux objective on a Bloch batch (line sources, conjugated run, session)")
    ap.add_argument("--flux-adjoint", action="store_true",
                    help="time the adjoint run with line sources and a FluxAdjointSession iteration")
    ap.add_argument("--hz-flux", action="store_true",
                    help="time flux lines in the Hz polarisation against the same batch without them, beside the Ez lines")
    ap.add_argument("--hz", action="store_true",
                    help="time the Hz polarisation with a pole against the Ez dispersive kernels on periodic members")
    ap.add_argument("--hz-bloch", action="store_true",
                    help="time a Bloch phase in the Hz polarisation with a pole against the real Hz and the Ez Bloch kernels")
    ap.add_argument("--hz-bloch-flux", action="store_true",
                    help="time flux lines under the Bloch phase of the Hz polarisation against the same batch without them")
    ap.add_argument("--hz-lattice", action="store_true",
                    help="time the lattice mode of the Hz polarisation with a pole against the Ez lattice with its pole")
    a = ap.parse_args()
    if a.hz_lattice:
        print(json.dumps(bench_hz_lattice(a.count or 1024, a.rows or 32, a.cols or 33, a.steps or 2000, np.dtype(a.dtype),
                                          a.reps)), flush=True)
        return
    if a.hz_bloch_flux:
        print(json.dumps(bench_hz_bloch_flux(a.count or 1024, a.rows or 40, a.cols or 41, a.steps or 2000,
                                             np.dtype(a.dtype), a.reps, a.pml_cells)), flush=True)
        return
    if a.hz_bloch:
        print(json.dumps(bench_hz_bloch(a.count or 1024, a.rows or 40, a.cols or 41, a.steps or 2000, np.dtype(a.dtype),
                                        a.reps, a.pml_cells)), flush=True)
        return
    if a.hz_flux:
        print(json.dumps(bench_hz_flux(a.count or 1024, a.rows or 56, a.cols or 57, a.steps or 2000, np.dtype(a.dtype),
                                       a.reps, a.pml_cells)), flush=True)
        return
    if a.hz:
        print(json.dumps(bench_hz(a.count or 1024, a.rows or 56, a.cols or 57, a.steps or 2000, np.dtype(a.dtype),
                                  a.reps, a.pml_cells)), flush=True)
        return
    if a.flux_adjoint:
        print(json.dumps(bench_flux_adjoint(a.count or 1024, a.rows or 60, a.cols or 61, a.steps or 2000,
                                            np.dtype(a.dtype), a.reps, a.pml_cells)), flush=True)
        return
    if a.bloch_flux_adjoint:
        print(json.dumps(bench_bloch_flux_adjoint(a.count or 1024, a.rows or 60, a.cols or 61, a.steps or 2000,
                                                  np.dtype(a.dtype).type, a.reps, a.pml_cells)))
        return
    if a.bloch_flux:
        print(json.dumps(bench_bloch_flux(a.count or 1024, a.rows or 60, a.cols or 61, a.steps or 2000,
                                          np.dtype(a.dtype), a.reps, a.pml_cells)), flush=True)
        return
    if a.flux:
        print(json.dumps(bench_flux(a.count or 1024, a.rows or 60, a.cols or 61, a.steps or 2000, np.dtype(a.dtype),
                                    a.reps, a.pml_cells)), flush=True)
        return
    if a.dispersive_adjoint:
        print(json.dumps(bench_dispersive_adjoint(a.count or 1024, a.rows or 60, a.cols or 60, a.steps or 1500,
                                                  np.dtype(a.dtype), a.reps, a.pml_cells)), flush=True)
        return
    if a.bloch_dispersive:
        for lattice in (True, False):
            print(json.dumps(bench_bloch_dispersive(a.count or 1024, a.rows or 33, a.cols or a.rows or 33, a.steps or 1000,
                                                    np.dtype(a.dtype), a.reps, a.pml_cells, lattice)), flush=True)
        return
    if a.lattice:
        print(json.dumps(bench_lattice(a.count or 1024, a.rows or 33, a.cols or a.rows or 33, a.steps or 1000,
                                       np.dtype(a.dtype), a.reps)), flush=True)
        return
    if a.dispersive:
        print(json.dumps(bench_dispersive(a.count or 1024, a.rows or 60, a.cols or 60, a.steps or 1000,
                                          np.dtype(a.dtype), a.reps, a.pml_cells)), flush=True)
        return
    if a.bloch_adjoint:
        print(json.dumps(bench_bloch_adjoint(a.count or 1024, a.rows or 60, a.cols or 60, a.steps or 1500,
                                             np.dtype(a.dtype), a.reps, a.pml_cells)), flush=True)
        return
    if a.bloch:
        print(json.dumps(bench_bloch(a.count or 1024, a.rows or 60, a.cols or 60, a.steps or 1000, np.dtype(a.dtype),
                                     a.reps, a.pml_cells)), flush=True)
        return
    if a.periodic:
        print(json.dumps(bench_periodic(a.count or 1024, a.rows or 60, a.cols or 61, a.steps or 1000, np.dtype(a.dtype),
                                        a.reps, a.pml_cells)), flush=True)
        return
    if a.lossy:
        for boundary in ("mur", "pml"):
            print(json.dumps(bench_lossy(a.count or 1024, a.rows or 60, a.cols or a.rows or 60, a.steps or 1000,
                                         np.dtype(a.dtype), a.reps, boundary, a.pml_cells)), flush=True)
        return
    if a.adjoint:
        if a.count or a.rows or a.cols or a.steps:
            configs = [(a.count or 1024, a.rows or 60, a.cols or a.rows or 60, a.steps or 1500, a.pml_cells)]
        else:
            configs = [(1024, 60, 60, 1500, 10), (64, 250, 250, 1500, 40)]
        for count, rows, cols, steps, layer in configs:
            print(json.dumps(bench_adjoint(count, rows, cols, steps, np.dtype(a.dtype), a.reps, layer)), flush=True)
        return
    if a.count or a.rows or a.cols or a.steps:
        configs = [(a.count or 1024, a.rows or 60, a.cols or a.rows or 60, a.steps or 1000)]
    else:
        configs = [(1024, 60, 60, 1000), (64, 256, 256, 500)]
    if a.monitors:
        configs = [(a.count or 1024, a.rows or 60, a.cols or a.rows or 60, a.steps or 1000)]
    for count, rows, cols, steps in configs:
        if a.monitors:
            print(json.dumps(bench_monitors(count, rows, cols, steps, np.dtype(a.dtype), a.reps, a.boundary,
                                            a.pml_cells)), flush=True)
            continue
        print(json.dumps(bench(count, rows, cols, steps, np.dtype(a.dtype), a.reps,
                               min(a.loop_members, count), a.clock_ghz, a.boundary, a.pml_cells)), flush=True)


if __name__ == "__main__":
    main()
