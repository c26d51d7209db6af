"""Adjoint gradients of probe spectra with respect to the permittivity, for batches.

``batch_eps_gradient`` gives dJ/d eps of every cell of a design window for an objective J on the spectra of up to 64
probe cells at up to 16 frequencies, for all members of a batch at once, at the cost of two runs per member.

The leapfrog scheme is reciprocal in the discrete frequency domain.  With z_k = exp(i omega_k dt), D = eps dx / dt per
cell and X_k = sum_n x[n] exp(-i omega_k (n + 1) dt), eliminating H from one step gives
(D (z - 2 + 1/z) - L) E = D (z - 1) S with a symmetric L.  So the adjoint field is an ordinary run of the same engine
whose sources are the probe cells, and

    dJ/d eps[i] = (dx / dt) * sum_k Re( -(z_k - 2 + 1/z_k) / (z_k - 1) * E_k[i] * Eadj_k[i] )

where E_k, Eadj_k are the window DFTs of the two runs over the design window.  No field history is stored and no
transposed kernel exists: the forward run records a window DFT and the probes, ``hold_dft_window`` keeps the window on
the device, the adjoint run injects at every probe cell a time series whose DFT at omega_k is conj(g[p, k]) / D[p]
through ``set_point_sources`` / ``run(channels=...)``, and ``dft_window_product`` forms the sum above on the device.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .batch import _probe_cells, _waveform_amps, _window_omegas, pml_fits

# cells between the design window and every edge: the Mur frame is 5 cells deep, and cell [0, 0] sets the Mur factor
# and the PML grading
EDGE_MARGIN = 6
# largest condition number of the channel system (frequencies closer than the run can resolve are beyond it)
MAX_CONDITION = 1e8


def channel_system(omegas, nsteps, dt, fc):
    """The 2F channels of one member and their DFT matrix: a[2k] = env cos(omega_k n dt), a[2k + 1] = env sin(omega_k
    n dt) with the Gaussian envelope exp(-((t - t0) / tau)^2), t0 = 4.5 / fc, tau = 0.9 / fc; A = [Re M; Im M] with
    M[k, c] = sum_n a_c[n] exp(-i omega_k (n + 1) dt).  Returns (channels (2F, nsteps), A (2F, 2F))."""
    w = np.asarray(omegas, dtype=np.float64)
    t = np.arange(nsteps) * dt
    env = np.exp(-((t - 4.5 / fc) / (0.9 / fc)) ** 2)
    chan = np.empty((2 * w.size, nsteps))
    chan[0::2] = np.cos(w[:, None] * t) * env
    chan[1::2] = np.sin(w[:, None] * t) * env
    M = np.exp(-1j * w[:, None] * ((np.arange(nsteps) + 1) * dt)) @ chan.T
    return chan, np.vstack([M.real, M.imag])


def probe_spectra(traces, omegas, dt):
    """(B, P, F) complex: sum_n traces[b, p, n] exp(-i omegas[b, k] (n + 1) dt)."""
    n = np.arange(traces.shape[2]) + 1
    phasors = {}                                  # one pair of real (n, F) matrices per distinct set of frequencies
    for w in omegas:
        if w.tobytes() not in phasors:
            ph = np.exp(-1j * np.outer(n * dt, w))
            phasors[w.tobytes()] = (np.ascontiguousarray(ph.real), np.ascontiguousarray(ph.imag))
    out = np.empty((traces.shape[0], traces.shape[1], omegas.shape[1]), np.complex128)
    for b, (tr, w) in enumerate(zip(traces, omegas)):
        re, im = phasors[w.tobytes()]
        out[b].real = tr @ re
        out[b].imag = tr @ im
    return out


def gradient_coefficients(omegas, dt):
    """-(z - 2 + 1/z) / (z - 1) for z = exp(i omega dt): the factor of E_k * Eadj_k in the gradient."""
    z = np.exp(1j * np.asarray(omegas, dtype=np.float64) * dt)
    return -(z - 2 + 1 / z) / (z - 1)


def _check_design(design, rects, R, Cc, margin, why):
    d = np.asarray(design)
    if d.shape != (4,) or not np.issubdtype(d.dtype, np.integer):
        raise ValueError(f"design must be 4 integers (row0, col0, nrows, ncols), got {design!r}")
    r0, c0, nr, nc = (int(v) for v in d)
    if nr < 1 or nc < 1:
        raise ValueError(f"design window {(r0, c0, nr, nc)} is empty")
    if r0 < margin or c0 < margin or r0 + nr > R - margin or c0 + nc > Cc - margin:
        raise ValueError(f"member 0 (and every other): design window {(r0, c0, nr, nc)} must keep {margin} cells from "
                         f"every edge of the {R}x{Cc} grid ({why})")
    for b, (sr, sc, snr, snc) in enumerate(rects):
        if snr and snc and sr < r0 + nr and sr + snr > r0 and sc < c0 + nc and sc + snc > c0:
            raise ValueError(f"member {b}: the design window {(r0, c0, nr, nc)} holds cells of the forward source "
                             f"{(int(sr), int(sc), int(snr), int(snc))}, whose direct term the gradient leaves out")
    return r0, c0, nr, nc


def batch_eps_gradient(eps, mu=None, *, nsteps, sources, probes, omegas, design, objective, fc=30e9,
                       waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml", pml_cells=40, device=0,
                       engine=None):
    """Gradient of an objective on probe spectra with respect to eps over a design window, for B members at once.

    eps: (B, R, C); mu: None (vacuum), a scalar or (B, R, C).  sources: (B, 2) or (B, 4) rectangles of the forward
    run, driven by `waveform` ("ricker" or "sinusoidal") at fc (scalar or (B,)) with t = n * dt.  probes: (P, 2) or
    (B, P, 2) observation cells, P <= 64.  omegas: (F,) or (B, F) angular frequencies, F <= 16.  design = (row0, col0,
    nrows, ncols), shared by all members.  objective(spectra) takes the complex (B, P, F) spectra
    Eobs[b, p, k] = sum_n Ez[p](after step n) exp(-i omega_k (n + 1) dt) and returns (J (B,), g (B, P, F)) with
    g = dJ/dRe(Eobs) + i dJ/dIm(Eobs).  boundary "pml" (a pml_cells-deep layer) or "mur"; a closed box never rings
    down, so "none" is refused.  engine: the engine class (BatchEngine by default).

    Conditions, checked on the host before any device work (ValueError): the design window holds no cell of a member's
    forward source, lies outside the PML layer and at least 6 cells from every edge; the channel system's condition
    number is at most 1e8.  The fields must have died away by the end of both runs: info["residual_forward"] and
    info["residual_adjoint"] give, per member, the end-of-run max|Ez| of each run divided by its largest probe sample.

    Returns (J (B,), grad (B, nrows, ncols) float64, spectra (B, P, F) complex128, info)."""
    from .api import MU0
    if engine is None:
        from .batch import BatchEngine as engine
    if boundary not in ("pml", "mur"):
        raise ValueError(f'boundary must be "pml" or "mur" (a closed box never rings down), not {boundary!r}')
    eps = np.asarray(eps)
    if eps.ndim != 3:
        raise ValueError(f"eps must have shape (B, R, C), got {eps.shape}")
    B, R, Cc = eps.shape
    nsteps = int(nsteps)
    if nsteps < 1:
        raise ValueError(f"nsteps must be >= 1, got {nsteps}")
    mu = MU0 if mu is None else mu
    mu_arr = np.asarray(mu)
    if mu_arr.ndim not in (0, 3) or (mu_arr.ndim == 3 and mu_arr.shape != eps.shape):
        raise ValueError(f"mu must be a scalar or have shape {eps.shape}, got {mu_arr.shape}")
    mu_min = mu_arr.reshape(B, -1).min(axis=1) if mu_arr.ndim == 3 else np.full(B, float(mu_arr))
    courant = (1 / np.sqrt(eps.reshape(B, -1).min(axis=1) * mu_min) * dt) / dx
    if not np.all(courant <= 1.0):
        raise ValueError(f"Courant stability condition not met: members {np.nonzero(~(courant <= 1.0))[0].tolist()}")

    rects = np.asarray(sources)
    if rects.ndim != 2 or rects.shape[0] != B or rects.shape[1] not in (2, 4):
        raise ValueError(f"sources must have shape ({B}, 2) or ({B}, 4), got {rects.shape}")
    if rects.shape[1] == 2:
        rects = np.concatenate([rects, np.ones_like(rects)], axis=1)
    L = int(pml_cells)
    if boundary == "pml" and not pml_fits(R, Cc, L):
        raise ValueError(f"a {L}-cell PML does not fit {R}x{Cc} members (2L + 3 <= min(rows, cols))")
    margin = max(EDGE_MARGIN, L) if boundary == "pml" else EDGE_MARGIN
    win = _check_design(design, rects, R, Cc, margin,
                        f"the {L}-cell PML layer" if margin > EDGE_MARGIN else "the boundary frame and cell [0, 0]")

    cells = _probe_cells(probes, B)
    P = cells.shape[1]
    if not 1 <= P <= _abi.BATCH_MAX_PROBES:
        raise ValueError(f"probes must hold 1..{_abi.BATCH_MAX_PROBES} cells per member, got {P}")
    if np.any(cells < 0) or np.any(cells[..., 0] >= R) or np.any(cells[..., 1] >= Cc):
        raise ValueError(f"probe cells must lie in the {R}x{Cc} grid")
    for b in range(B):
        if len({(int(r), int(c)) for r, c in cells[b]}) != P:
            raise ValueError(f"member {b}: a probe cell is listed twice")
    om = _window_omegas(omegas, B)
    F = om.shape[1]
    if not 1 <= F <= _abi.BATCH_MAX_DFT_FREQS:
        raise ValueError(f"omegas must hold 1..{_abi.BATCH_MAX_DFT_FREQS} frequencies, got {F}")
    if not np.all(np.isfinite(om)) or np.any(om <= 0):
        raise ValueError("omegas must be finite and positive")
    fcs = np.ascontiguousarray(np.broadcast_to(np.asarray(fc, dtype=np.float64), (B,)))

    # the channel systems, one per distinct (frequencies, fc)
    systems, which = {}, []
    for b in range(B):
        key = (om[b].tobytes(), float(fcs[b]))
        if key not in systems:
            chan, A = channel_system(om[b], nsteps, dt, float(fcs[b]))
            cond = float(np.linalg.cond(A))
            if not cond <= MAX_CONDITION:
                raise ValueError(f"member {b}: the channel system's condition number {cond:.3g} exceeds "
                                 f"{MAX_CONDITION:g}: {nsteps} steps cannot tell these frequencies apart")
            systems[key] = (chan, A, cond)
        which.append(key)
    shared = len(systems) == 1

    amps = _waveform_amps(waveform, fcs, nsteps, dt)
    with engine(B, R, Cc, dt, dx, dtype=dtype, boundary=boundary, device=device) as eng:
        eng.set_materials(eps, mu)
        if boundary == "pml":
            m00 = mu_arr[:, 0, 0] if mu_arr.ndim == 3 else np.full(B, float(mu_arr))
            eng.set_pml(L, courant00=np.array([(1 / np.sqrt(float(e) * float(u)) * dt) / dx
                                               for e, u in zip(eps[:, 0, 0], m00)]))
        # 1. forward: the member's own source; window DFT over the design region, probes at the observation cells
        eng.set_sources(rects)
        eng.set_dft_window(win, om).set_probes(cells, nsteps)
        eng.run(nsteps, amps)
        traces = eng.read_probes(0, nsteps)
        end_fwd = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)
        eng.hold_dft_window()
        spectra = probe_spectra(traces, om, dt)

        # 2. the cotangent
        J, g = objective(spectra)
        J = np.asarray(J, dtype=np.float64)
        g = np.asarray(g, dtype=np.complex128)
        if J.shape != (B,) or g.shape != (B, P, F):
            raise ValueError(f"objective must return J of shape ({B},) and g of shape ({B}, {P}, {F}), got {J.shape} "
                             f"and {g.shape}")

        # 3. adjoint: same materials, fields zero, step 0; the probe cells inject conj(g) / D at every frequency
        D = np.asarray(eps, dtype=dtype).astype(np.float64)[np.arange(B)[:, None], cells[..., 0], cells[..., 1]] * dx / dt
        c = np.conj(g) / D[:, :, None]
        weights = np.empty((B, P, 2 * F))
        for b in range(B):
            weights[b] = np.linalg.solve(systems[which[b]][1], np.concatenate([c[b].real, c[b].imag], axis=1).T).T
        eng.reset()
        eng.set_point_sources(cells, weights)
        channels = systems[which[0]][0] if shared else np.stack([systems[k][0] for k in which])
        eng.run(nsteps, None, channels)      # amps None: no rectangle source
        adj_traces = eng.read_probes(0, nsteps)
        end_adj = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)

        # 4. the gradient, formed on the device from the two windows
        coef = np.stack([gradient_coefficients(w, dt) for w in om])
        grad = eng.dft_window_product(coef) * (dx / dt)

    def ratio(end, tr):
        flat = tr.reshape(B, -1)
        peak = np.maximum(flat.max(axis=1), -flat.min(axis=1))
        return np.divide(end, peak, out=np.full(B, np.inf), where=peak > 0)
    info = {"condition": max(s[2] for s in systems.values()),
            "residual_forward": ratio(end_fwd, traces), "residual_adjoint": ratio(end_adj, adj_traces),
            "channels_shared": shared}
    return J, grad, spectra, info
