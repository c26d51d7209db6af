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

With an electric conductivity sigma per cell (``BatchEngine.set_conductivity``) the one-step operator becomes
D (z - 2 + 1/z) + G (z - 1/z) - L with G = sigma dx / 2.  It is still symmetric and eps still enters through D alone,
so dJ/d eps keeps its formula, and ``batch_material_gradient`` adds

    dJ/d sigma[i] = (dx / 2) * sum_k Re( -(z_k + 1) / z_k * E_k[i] * Eadj_k[i] )

from the same two windows: one more product, no new run.

With periodic columns (``boundary="periodic"``) the column difference of L is cyclic, which leaves L symmetric, so nothing
in the method changes; only the column margins go (the design window and a conductivity may span the whole period).

With a Bloch phase (``batch_bloch_gradient``, ``BlochAdjointSession``) the fields are complex and the seam couples with
conj(rho) k in the row of column 0 and rho k in the row of column C-2, rho = (cos phi, sin phi): L is no longer symmetric,
and its transpose is the same operator with rho replaced by conj(rho), exactly (also with rho rounded to the batch dtype).
So the adjoint field is a Bloch run of the same member with the rotation conjugated (``run_bloch_channels(conjugate=
True)``) and sources at the probe cells, and the gradients are the formulas above with the plain, unconjugated product of
the two complex window DFTs.  The injected series stay real (added to the real part of Ez alone, the seam carries them into
the imaginary part), so the channel systems and their real weights are unchanged.

With a Drude-Lorentz pole per member (``BatchEngine.set_dispersion``; ``batch_dispersive_gradient``,
``DispersiveAdjointSession``) and the member's a, bq, ck of include/fdtd2d_batch_dispersive.h (cj = dx bq EPS0 wp2) the
operator gains the diagonal term cj (z - 1)^2 / ((z - a)(z - 1) + ck z).  It stays symmetric, so the adjoint field is an
ordinary dispersive run of the same member with sources at the probe cells, dJ/d eps and dJ/d sigma keep their formulas,
and

    dJ/d wp2[i] = dx * bq * EPS0 * sum_k Re( -(z_k - 1) / ((z_k - a)(z_k - 1) + ck z_k) * E_k[i] * Eadj_k[i] )

from the same two windows.  The held window and the product are calls of their own (``hold_dispersive_window``,
``dispersive_window_product``: up to three coefficient sets in one pass); the helpers above and ``AdjointSession`` keep
refusing an engine with a pole.

Flux objectives (``batch_flux_gradient``, ``FluxAdjointSession``): J depends on the power P = s dx sum_cells Re(E conj(H g))
through the lines of ``BatchEngine.set_flux_lines``, E and H the raw sums of a line cell, g = exp(i omega dt / 2),
s = +1 (row line) or -1 (column line).  Then dJ = sum Re(aE dE + aH dH) with aE = dJ/dP s dx conj(H g) and
aH = dJ/dP s dx conj(E) g per line cell.  Eliminating H as above, from rest and with ring-down, gives H on a line as a
fixed linear map of E: the H update with the member's own ch = dt / (mu dx), H = ch C E / (z - 1) with C the difference
of the update, averaged over the two H values of the cell (T).  A source that adds M to H before the H update of a step
and S to Ez after the E update enters as (D (z - 2 + 1/z) - L) E = D (z - 1) S - z C^T M, the update of Ez being the
negative transpose of C.  So the adjoint field, scaled by (z - 1) like the probes' so that the coefficients above stay,
solves the same system with

    S = aE / D = dJ/dP s dx conj(H g) / D                    on the line cells (D of the cell, sigma = 0 there)
    M = -(1/z) ch T^T aH:   0.5 * (-ch dJ/dP s dx conj(E g))   on each of the two H values of the cell

which is what ``BatchEngine.set_flux_line_sources`` injects: the transpose of the monitor, driven by the 2F channels of
the probe helpers with weights from the same channel systems.  The two H values of a cell take one weight, so mu must
agree on them; eps still enters through D alone, so ``dft_window_product`` with ``gradient_coefficients`` and
``sigma_coefficients`` forms dJ/d eps and dJ/d sigma as before.  ``FluxAdjointSession`` forms the weights on the device
(``flux_adjoint_sources``), ``batch_flux_gradient`` on the host (``flux_adjoint_weights``); they agree to rounding.
Checked against central finite differences of the stand-in's flux(): tests/test_batch_flux_adjoint_cpu.py.
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


def sigma_coefficients(omegas, dt):
    """-(z + 1) / z for z = exp(i omega dt): the factor of E_k * Eadj_k in the conductivity gradient."""
    z = np.exp(1j * np.asarray(omegas, dtype=np.float64) * dt)
    return -(z + 1) / z


def _check_sigma(p, sigma, window=None, name="sigma", may="conduct",
                 probe_why="would be conj(g) / (D + G), which is not implemented"):
    """The host checks of a conductivity (ValueError naming the first offending member): (B, R, C), or (B, nrows, ncols)
    for window = (row0, col0, nrows, ncols); >= 0 and finite; zero in the boundary frame or the PML layer and at every
    probe cell.  Returns it as a float64 array.  name, may, probe_why: the wording for another quantity under the same
    rules (_check_wp2)."""
    r0, c0, nr, nc = (0, 0, p.R, p.Cc) if window is None else window
    s = np.asarray(sigma, dtype=np.float64)
    if s.ndim == 0 and window is None:
        full = np.zeros((p.B, p.R, p.Cc))
        if p.periodic:
            full[:, p.margin:p.R - p.margin, :] = s
        else:
            full[:, p.margin:p.R - p.margin, p.margin:p.Cc - p.margin] = s
        if not s >= 0:
            full[...] = s
        s = full
    if s.shape != (p.B, nr, nc):
        raise ValueError(f"{name} must have shape ({p.B}, {nr}, {nc}), got {s.shape}")
    bad = ~(np.isfinite(s) & (s >= 0))
    if bad.any():
        raise ValueError(f"member {int(np.nonzero(bad.reshape(p.B, -1).any(axis=1))[0][0])}: {name} must be >= 0 and "
                         f"finite")
    rows, cols = np.arange(r0, r0 + nr), np.arange(c0, c0 + nc)
    if p.periodic:       # no column margin; the image column C-1 is accepted and never read
        edge = ((rows < p.margin) | (rows > p.R - 1 - p.margin))[:, None] & (cols < p.Cc - 1)[None, :]
    else:
        edge = ((rows < p.margin) | (rows > p.R - 1 - p.margin))[:, None] | \
            ((cols < p.margin) | (cols > p.Cc - 1 - p.margin))[None, :]
    out = (s != 0) & edge[None]
    if out.any():
        b = int(np.nonzero(out.reshape(p.B, -1).any(axis=1))[0][0])
        i, j = (int(v[0]) for v in np.nonzero(out[b]))
        raise ValueError(f"member {b}: {name} is non-zero at cell ({r0 + i}, {c0 + j}), within {p.margin} cells of an "
                         f"edge ({p.margin_why}): only cells that take the plain update may {may}")
    for b in range(p.B):
        for r, c in p.cells[b]:
            r, c = int(r) - r0, int(c) - c0
            if 0 <= r < nr and 0 <= c < nc and s[b, r, c] != 0:
                raise ValueError(f"member {b}: {name} is non-zero at the probe cell ({r + r0}, {c + c0}); the adjoint "
                                 f"injection there {probe_why}")
    return s


def _check_design(design, rects, R, Cc, margin, why, periodic=False):
    d = np.asarray(design)
    if d.shape != (4,) or not np.issubdtype(d.dtype, np.integer):
        raise ValueError(f"design must be 4 integers (row0, col0, nrows, ncols), got {design!r}")
    r0, c0, nr, nc = (int(v) for v in d)
    if nr < 1 or nc < 1:
        raise ValueError(f"design window {(r0, c0, nr, nc)} is empty")
    if periodic:
        if c0 < 0 or c0 + nc > Cc - 1:
            raise ValueError(f"member 0 (and every other): design window {(r0, c0, nr, nc)} must lie in columns 0..{Cc - 2}"
                             f" of the {R}x{Cc} grid: column {Cc - 1} is the image of column 0")
        if r0 < margin or r0 + nr > R - margin:
            raise ValueError(f"member 0 (and every other): design window {(r0, c0, nr, nc)} must keep {margin} rows from "
                             f"the top and bottom edges of the {R}x{Cc} grid ({why})")
    elif r0 < margin or c0 < margin or r0 + nr > R - margin or c0 + nc > Cc - margin:
        raise ValueError(f"member 0 (and every other): design window {(r0, c0, nr, nc)} must keep {margin} cells from "
                         f"every edge of the {R}x{Cc} grid ({why})")
    for b, (sr, sc, snr, snc) in enumerate(rects):
        if snr and snc and sr < r0 + nr and sr + snr > r0 and sc < c0 + nc and sc + snc > c0:
            raise ValueError(f"member {b}: the design window {(r0, c0, nr, nc)} holds cells of the forward source "
                             f"{(int(sr), int(sc), int(snr), int(snc))}, whose direct term the gradient leaves out")
    return r0, c0, nr, nc


class _Plan:
    """What batch_eps_gradient and AdjointSession work out on the host before any device work: the checked arguments,
    the channel systems and the forward amplitudes."""


def _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, boundary, pml_cells):
    """The host checks of batch_eps_gradient (ValueError), then the channel systems and the amplitudes."""
    from .api import MU0
    p = _Plan()
    if boundary not in ("pml", "mur", "periodic"):
        raise ValueError(f'boundary must be "pml", "mur" or "periodic" (a closed box never rings down), not {boundary!r}')
    periodic = boundary == "periodic"
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
    if periodic and not pml_fits(R, Cc, L, True):
        raise ValueError(f"member 0 (and every other): a {L}-cell PML does not fit the rows of {R}x{Cc} periodic members "
                         f"(2L + 3 <= rows, at least one cell: PEC rows never ring down)")
    margin = max(EDGE_MARGIN, L) if boundary in ("pml", "periodic") else EDGE_MARGIN
    p.margin, p.periodic = margin, periodic
    p.margin_why = f"the {L}-cell PML layer" if margin > EDGE_MARGIN else "the boundary frame and cell [0, 0]"
    if periodic:
        for b, (sr, sc, snr, snc) in enumerate(rects):
            if snr and snc and sc + snc > Cc - 1:
                raise ValueError(f"member {b}: the source {(int(sr), int(sc), int(snr), int(snc))} reaches column "
                                 f"{Cc - 1}, the image of column 0")
    win = _check_design(design, rects, R, Cc, margin, p.margin_why, periodic)

    cells = _probe_cells(probes, B)
    P = cells.shape[1]
    if not 1 <= P <= _abi.BATCH_MAX_PROBES:
        raise ValueError(f"probes must hold 1..{_abi.BATCH_MAX_PROBES} cells per member, got {P}")
    if np.any(cells < 0) or np.any(cells[..., 0] >= R) or np.any(cells[..., 1] >= Cc):
        raise ValueError(f"probe cells must lie in the {R}x{Cc} grid")
    if periodic and np.any(cells[..., 1] >= Cc - 1):
        b = int(np.nonzero((cells[..., 1] >= Cc - 1).any(axis=1))[0][0])
        raise ValueError(f"member {b}: a probe cell lies in column {Cc - 1}, the image of column 0, where the adjoint run "
                         f"cannot inject")
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
    p.eps, p.mu, p.mu_arr, p.mu_min = eps, mu, mu_arr, mu_min
    p.B, p.R, p.Cc, p.nsteps, p.dt, p.dx, p.boundary = B, R, Cc, nsteps, dt, dx, boundary
    p.rects, p.L, p.win, p.cells, p.P, p.om, p.F = rects, L, win, cells, P, om, F
    p.systems, p.which, p.shared = systems, which, len(systems) == 1
    p.channels = systems[which[0]][0] if p.shared else np.stack([systems[k][0] for k in which])
    p.amps = _waveform_amps(waveform, fcs, nsteps, dt)
    p.coef = np.stack([gradient_coefficients(w, dt) for w in om])
    p.coef_sigma = np.stack([sigma_coefficients(w, dt) for w in om])
    return p


def _setup(eng, p):
    """Materials, PML, the forward source, the window DFT over the design region and the probes."""
    eng.set_materials(p.eps, p.mu)
    if p.boundary in ("pml", "periodic"):
        m00 = p.mu_arr[:, 0, 0] if p.mu_arr.ndim == 3 else np.full(p.B, float(p.mu_arr))
        eng.set_pml(p.L, courant00=np.array([(1 / np.sqrt(float(e) * float(u)) * p.dt) / p.dx
                                             for e, u in zip(p.eps[:, 0, 0], m00)]))
    eng.set_sources(p.rects)
    eng.set_dft_window(p.win, p.om).set_probes(p.cells, p.nsteps)


def _refuse_bloch(eng):
    """The adjoint of complex fields is not implemented: an engine with a Bloch phase (an engine factory that sets one,
    or set_bloch_phase on a session's engine) is refused before any run."""
    if getattr(eng, "_bloch", None) is not None:
        from ._abi import E_STATE, Fdtd2dError
        raise Fdtd2dError(E_STATE, "adjoint gradients are not available while a Bloch phase is set (complex fields)")
    _refuse_dispersion(eng)


def _refuse_hz(eng):
    """The adjoint of the Hz polarisation is not implemented: an engine in it (an engine factory that calls
    set_polarization("hz"), or the call on a session's engine) is refused before any run."""
    if getattr(eng, "polarization", "ez") == "hz":
        from ._abi import E_STATE, Fdtd2dError
        raise Fdtd2dError(E_STATE, "adjoint gradients are not available in the Hz polarisation "
                          '(set_polarization("hz")): its adjoint is not implemented')


def _refuse_dispersion(eng):
    """The adjoint of a dispersive medium is not implemented: an engine with a Drude-Lorentz pole (an engine factory
    that sets one, or set_dispersion / set_bloch_dispersion on a session's engine) is refused before any run."""
    _refuse_hz(eng)
    if getattr(eng, "dispersive", False):
        from ._abi import E_STATE, Fdtd2dError
        raise Fdtd2dError(E_STATE, "adjoint gradients are not available while a dispersive pole is set: the adjoint of a "
                          "dispersive medium is not implemented")


def _cotangent(p, objective, spectra):
    J, g = objective(spectra)
    J = np.asarray(J, dtype=np.float64)
    g = np.asarray(g, dtype=np.complex128)
    if J.shape != (p.B,) or g.shape != (p.B, p.P, p.F):
        raise ValueError(f"objective must return J of shape ({p.B},) and g of shape ({p.B}, {p.P}, {p.F}), got {J.shape} "
                         f"and {g.shape}")
    return J, g


def _injections(p, g, eps, dtype):
    """conj(g) / D at the probe cells, D = eps dx / dt with eps as the engine stores it."""
    D = np.asarray(eps, dtype=dtype).astype(np.float64)[np.arange(p.B)[:, None], p.cells[..., 0], p.cells[..., 1]]
    return np.conj(g) / (D * p.dx / p.dt)[:, :, None]


def _residual(end, peak):
    return np.divide(end, peak, out=np.full(end.shape, np.inf), where=peak > 0)


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

    boundary "periodic": periodic columns with a pml_cells-deep layer on the top and bottom rows.  The column margins
    go: the design window may span columns 0..C-2, the whole period, and keeps max(6, pml_cells) rows from the top and
    bottom edges; sources and probe cells lie in columns 0..C-2.  Nothing else in the method changes.  Mind the ring-down
    there: a lossless high-index periodic layer guides modes along the columns that never reach the layer on the rows.
    On a 64x17 member (8-cell layer, eps_r in [1, 3] on 12 rows, 5000 steps) they left residuals of 3-7 % and gradient
    errors of up to 0.9 of max|gradient|; with a conductivity of 0.2-0.7 S/m on the same rows
    (batch_material_gradient) the residuals fell below 5e-5 and the errors to 2e-7.  info["residual_*"] reports the
    condition; the helper does not try to cure it.

    Conditions, checked on the host before any device work (ValueError): the design window holds no cell of a member's
    forward source, lies outside the PML layer and at least 6 cells from every edge; the channel system's condition
    number is at most 1e8.  The fields must have died away by the end of both runs: info["residual_forward"] and
    info["residual_adjoint"] give, per member, the end-of-run max|Ez| of each run divided by its largest probe sample.

    One call builds its engine and reads every probe trace back; a loop that calls it again and again is what
    AdjointSession is for.

    Returns (J (B,), grad (B, nrows, ncols) float64, spectra (B, P, F) complex128, info)."""
    p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, boundary, pml_cells)
    J, grad, _, spectra, info = _two_runs(p, None, objective, dtype, device, engine)
    return J, grad, spectra, info


def _two_runs(p, sigma, objective, dtype, device, engine):
    """The forward and the adjoint run of batch_eps_gradient and batch_material_gradient on a fresh engine; sigma: the
    checked conductivity, or None for a lossless batch.  Returns (J, grad_eps, grad_sigma or None, spectra, info)."""
    if engine is None:
        from .batch import BatchEngine as engine
    B, nsteps, dt, dx, boundary = p.B, p.nsteps, p.dt, p.dx, p.boundary
    with engine(B, p.R, p.Cc, dt, dx, dtype=dtype, boundary=boundary, device=device) as eng:
        _refuse_bloch(eng)
        # 1. forward: the member's own source; window DFT over the design region, probes at the observation cells
        _setup(eng, p)
        if sigma is not None:
            eng.set_conductivity(sigma)
        eng.run(nsteps, p.amps)
        traces = eng.read_probes(0, nsteps)
        end_fwd = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)
        eng.hold_dft_window()
        spectra = probe_spectra(traces, p.om, dt)

        # 2. the cotangent
        J, g = _cotangent(p, objective, spectra)

        # 3. adjoint: same materials, fields zero, step 0; the probe cells inject conj(g) / D at every frequency
        c = _injections(p, g, p.eps, dtype)
        weights = np.empty((B, p.P, 2 * p.F))
        for b in range(B):
            weights[b] = np.linalg.solve(p.systems[p.which[b]][1], np.concatenate([c[b].real, c[b].imag], axis=1).T).T
        eng.reset()
        eng.set_point_sources(p.cells, weights)
        eng.run(nsteps, None, p.channels)      # amps None: no rectangle source
        adj_traces = eng.read_probes(0, nsteps)
        end_adj = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)

        # 4. the gradients, formed on the device from the two windows
        grad = eng.dft_window_product(p.coef) * (dx / dt)
        grad_sigma = None if sigma is None else eng.dft_window_product(p.coef_sigma) * (dx / 2)

    def peak(tr):
        flat = tr.reshape(B, -1)
        return np.maximum(flat.max(axis=1), -flat.min(axis=1))
    info = {"condition": max(s[2] for s in p.systems.values()),
            "residual_forward": _residual(end_fwd, peak(traces)), "residual_adjoint": _residual(end_adj, peak(adj_traces)),
            "channels_shared": p.shared}
    return J, grad, grad_sigma, spectra, info


def batch_material_gradient(eps, sigma, mu=None, *, nsteps, sources, probes, omegas, design, objective, fc=30e9,
                            waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml", pml_cells=40,
                            device=0, engine=None):
    """batch_eps_gradient for lossy members: the gradients of the objective with respect to eps and to the electric
    conductivity sigma over the design window, from the same two runs.

    sigma: (B, R, C) in S/m (BatchEngine.set_conductivity), a scalar for every cell that may conduct, or None for
    zero.  The other arguments, the conditions and their checks are batch_eps_gradient's.  In addition, checked on the
    host with a ValueError that names the member: sigma is >= 0 and finite, zero within 6 cells of every edge and
    inside the PML layer (only cells that take the plain update may conduct), and zero at every probe cell (the
    injection there would be conj(g) / (D + G); only the sigma = 0 case is implemented).

    Returns (J (B,), grad_eps (B, nrows, ncols), grad_sigma (B, nrows, ncols) float64, spectra (B, P, F) complex128,
    info)."""
    p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, boundary, pml_cells)
    s = _check_sigma(p, 0.0 if sigma is None else sigma)
    return _two_runs(p, s, objective, dtype, device, engine)


class AdjointSession:
    """batch_eps_gradient as a loop: the engine stands between iterations, and an iteration moves only what it needs.

    The constructor takes batch_eps_gradient's arguments (without the objective), makes its host checks with its
    messages and does once what the helper does per call: the channel systems, the amplitudes, the engine with its
    materials, PML, source rectangles, window DFT and probes.  value_and_grad(objective) returns what the helper
    returns; it transforms the probe traces and takes the fields' maxima on the device (BatchEngine.probe_spectra,
    field_absmax), so B * P * F spectra and B * nrows * ncols gradients come down and B * P * 2F weights go up, and no
    trace, field or window is read back.  set_design_eps(eps_window) replaces the permittivity of the design window
    (BatchEngine.set_eps_window).  The spectra are summed in ascending step order, where the helper's host transform
    sums as its matrix product does: they agree to rounding (1e-14 of their maximum), not bit for bit.

        with AdjointSession(eps, nsteps=..., sources=..., probes=..., omegas=..., design=win) as s:
            for it in range(100):
                J, grad, spectra, info = s.value_and_grad(objective)
                s.set_design_eps(np.clip(s.eps[:, r0:r0 + nr, c0:c0 + nc] + step * grad, lo, hi))
    """

    def __init__(self, eps, mu=None, *, nsteps, sources, probes, omegas, design, fc=30e9, waveform="ricker", dt=5e-14,
                 dx=1e-4, dtype=np.float64, boundary="pml", pml_cells=40, device=0, engine=None):
        self._eng = None
        p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, boundary, pml_cells)
        self._open(p, dtype, engine, device)

    def _open(self, p, dtype, engine, device):
        """What the constructor does after the host checks: the session's state and the standing engine."""
        if engine is None:
            from .batch import BatchEngine as engine
        self._p = p
        p.eps = np.array(p.eps)                 # the session's own copy: set_design_eps keeps it current
        self._dtype = dtype
        # one solve per distinct channel system, for all of its members' probes at once
        self._groups = [(A, np.array([b for b, k in enumerate(p.which) if k == key]))
                        for key, (_, A, _) in p.systems.items()]
        self._condition = max(s[2] for s in p.systems.values())
        r0, c0, nr, nc = p.win
        outside = p.eps.astype(np.float64)
        outside[:, r0:r0 + nr, c0:c0 + nc] = np.inf
        self._eps_min_outside = outside.reshape(p.B, -1).min(axis=1)
        self._sigma = None                      # the conductivity as the session holds it (None: lossless)
        self._ran = False                       # the windows of a value_and_grad are on the device
        eng = engine(p.B, p.R, p.Cc, p.dt, p.dx, dtype=dtype, boundary=p.boundary, device=device)
        try:
            self._check_engine(eng)
            self._setup_engine(eng)
        except BaseException:
            eng.__exit__(None, None, None)
            raise
        self._eng = eng

    # -- lifetime -------------------------------------------------------------------
    def close(self):
        eng, self._eng = self._eng, None
        if eng is not None:
            eng.__exit__(None, None, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def engine(self):
        """The standing engine (None once closed)."""
        return self._eng

    @property
    def eps(self):
        """The members' permittivity as the session holds it, (B, R, C), read-only."""
        v = self._p.eps.view()
        v.flags.writeable = False
        return v

    # -- one iteration ----------------------------------------------------------------
    def value_and_grad(self, objective):
        """(J (B,), grad (B, nrows, ncols) float64, spectra (B, P, F) complex128, info) of the current permittivity,
        as batch_eps_gradient returns them."""
        p, eng = self._p, self._eng
        if eng is None:
            raise RuntimeError("the session is closed")
        self._check_engine(eng)
        none = np.empty((p.B, 0))
        # 1. forward
        eng.reset()
        eng.run(p.nsteps, p.amps)
        spectra, peak_fwd = self._spectra(eng, p.om)
        end_fwd = self._absmax(eng)
        self._hold(eng)
        # 2. the cotangent
        J, g = _cotangent(p, objective, spectra)
        # 3. adjoint
        c = _injections(p, g, p.eps, self._dtype)
        rhs = np.concatenate([c.real, c.imag], axis=2)              # (B, P, 2F)
        weights = np.empty((p.B, p.P, 2 * p.F))
        for A, members in self._groups:
            w = np.linalg.solve(A, rhs[members].reshape(-1, 2 * p.F).T)
            weights[members] = w.T.reshape(len(members), p.P, 2 * p.F)
        eng.reset()
        self._run_adjoint(eng, weights)
        _, peak_adj = self._spectra(eng, none)
        end_adj = self._absmax(eng)
        # 4. the gradient
        grad = self._product(eng, p.coef) * (p.dx / p.dt)
        self._ran = True
        info = {"condition": self._condition, "residual_forward": _residual(end_fwd, peak_fwd),
                "residual_adjoint": _residual(end_adj, peak_adj), "channels_shared": p.shared}
        return J, grad, spectra, info

    # the engine calls of an iteration (BlochAdjointSession takes their complex counterparts)
    _check_engine = staticmethod(_refuse_bloch)

    def _setup_engine(self, eng):
        _setup(eng, self._p)

    def _spectra(self, eng, omegas):
        return eng.probe_spectra(omegas, 0, self._p.nsteps, peak=True)

    def _absmax(self, eng):
        return eng.field_absmax("Ez")

    def _hold(self, eng):
        eng.hold_dft_window()

    def _run_adjoint(self, eng, weights):
        eng.set_point_sources(self._p.cells, weights)
        eng.run(self._p.nsteps, None, self._p.channels)

    def _product(self, eng, coef):
        return eng.dft_window_product(coef)

    # -- lossy members ------------------------------------------------------------------
    @property
    def sigma(self):
        """The members' conductivity as the session holds it, (B, R, C) float64, read-only (None: lossless)."""
        if self._sigma is None:
            return None
        v = self._sigma.view()
        v.flags.writeable = False
        return v

    def set_conductivity(self, sigma):
        """The conductivity of every member, (B, R, C) in S/m (a scalar: every cell that may conduct; None removes
        it), before the first iteration or between iterations.  Checked on the host as batch_material_gradient checks
        it (ValueError, nothing changed)."""
        if self._eng is None:
            raise RuntimeError("the session is closed")
        if sigma is None:
            self._eng.set_conductivity(None)
            self._sigma = None
            return self
        s = _check_sigma(self._p, sigma)
        self._eng.set_conductivity(s)
        self._sigma = s.copy()
        return self

    def set_design_sigma(self, sigma_window):
        """New conductivity of the design window for every member: (B, nrows, ncols).  Checked on the host
        (ValueError, nothing changed): the shape, values >= 0 and finite, zero at probe cells."""
        p = self._p
        if self._eng is None:
            raise RuntimeError("the session is closed")
        r0, c0, nr, nc = p.win
        s = _check_sigma(p, sigma_window, p.win)
        self._eng.set_conductivity_window(p.win, s)
        if self._sigma is None:
            self._sigma = np.zeros((p.B, p.R, p.Cc))
        self._sigma[:, r0:r0 + nr, c0:c0 + nc] = s
        return self

    def sigma_gradient(self):
        """dJ/d sigma over the design window, (B, nrows, ncols) float64, for the latest value_and_grad: one more
        product of the two windows that are still on the device, and one read-back."""
        if self._eng is None:
            raise RuntimeError("the session is closed")
        if not self._ran:
            raise RuntimeError("no gradient yet: call value_and_grad first")
        return self._product(self._eng, self._p.coef_sigma) * (self._p.dx / 2)

    def set_design_eps(self, eps_window):
        """New permittivity of the design window for every member: (B, nrows, ncols).  Checked on the host
        (ValueError, nothing changed): the shape, positive finite values, the Courant condition of the updated
        members."""
        p = self._p
        if self._eng is None:
            raise RuntimeError("the session is closed")
        r0, c0, nr, nc = p.win
        new = np.asarray(eps_window)
        if new.shape != (p.B, nr, nc):
            raise ValueError(f"eps_window must have shape ({p.B}, {nr}, {nc}), got {new.shape}")
        new = new.astype(p.eps.dtype)
        ok = np.isfinite(new) & (new > 0)
        if not np.all(ok):
            raise ValueError(f"eps_window must be positive and finite: members "
                             f"{np.nonzero(~ok.reshape(p.B, -1).all(axis=1))[0].tolist()}")
        eps_min = np.minimum(self._eps_min_outside, new.reshape(p.B, -1).min(axis=1))
        courant = (1 / np.sqrt(eps_min * p.mu_min) * p.dt) / p.dx
        if not np.all(courant <= 1.0):
            raise ValueError(f"Courant stability condition not met: members {np.nonzero(~(courant <= 1.0))[0].tolist()}")
        self._eng.set_eps_window(p.win, new)
        p.eps[:, r0:r0 + nr, c0:c0 + nc] = new
        return self


# ---- Bloch batches: complex fields, one phase per member ----------------------------------------------------------------

def _bloch_phases(phi, B):
    """(B,) float64 phases from a scalar or (B,) (ValueError naming the member)."""
    if phi is None:
        raise ValueError("member 0 (and every other): bloch_phase is required (a scalar or (B,) in radians); without a "
                         "phase use batch_material_gradient(boundary=\"periodic\")")
    ph = np.asarray(phi, dtype=np.float64)
    if ph.shape not in ((), (B,)):
        raise ValueError(f"bloch_phase must be a scalar or have shape ({B},), got {ph.shape}")
    ph = np.ascontiguousarray(np.broadcast_to(ph, (B,)))
    if not np.all(np.isfinite(ph)):
        raise ValueError(f"member {int(np.nonzero(~np.isfinite(ph))[0][0])}: bloch_phase is not finite")
    return ph


def _check_weights(source_weights, B, Cc):
    """source_weights as set_bloch_source takes them: "ramp", None or a complex (C-1,) or (B, C-1) array."""
    if source_weights is None or (isinstance(source_weights, str) and source_weights == "ramp"):
        return source_weights
    if isinstance(source_weights, str):
        raise ValueError(f'source_weights must be "ramp", None or an array, not {source_weights!r}')
    w = np.asarray(source_weights, dtype=np.complex128)
    if w.shape not in ((Cc - 1,), (B, Cc - 1)):
        raise ValueError(f"source_weights must have shape ({Cc - 1},) or ({B}, {Cc - 1}), got {w.shape}")
    if not np.all(np.isfinite(w)):
        raise ValueError("source_weights must be finite")
    return w


def _bloch_setup(eng, p, sigma, phi, weights):
    """_setup, the conductivity, then the phase and the source weights."""
    _setup(eng, p)
    if sigma is not None:
        eng.set_conductivity(sigma)
    eng.set_bloch_phase(phi)
    if weights is not None:
        eng.set_bloch_source(weights)


def _part_peak(z):
    """The larger of the largest |real part| and the largest |imaginary part| per member, as bloch_field_absmax and
    bloch_probe_spectra(peak=True) report them."""
    flat = z.reshape(z.shape[0], -1)
    return np.maximum(np.abs(flat.real).max(axis=1, initial=0.0), np.abs(flat.imag).max(axis=1, initial=0.0))


def batch_bloch_gradient(eps, sigma=None, mu=None, *, bloch_phase, source_weights=None, nsteps, sources, probes, omegas,
                         design, objective, fc=30e9, waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64,
                         pml_cells=40, device=0, engine=None):
    """batch_material_gradient(boundary="periodic") for Bloch batches: complex fields that repeat as F(x + period) =
    F(x) exp(1j * phi), one phase per member.

    bloch_phase: a scalar or (B,) in radians (BatchEngine.set_bloch_phase).  source_weights: "ramp", a complex (C-1,) or
    (B, C-1) array, or None for ones, as in run_fdtd_batch (BatchEngine.set_bloch_source).  The boundary is always
    periodic, with a pml_cells-deep layer on the top and bottom rows.  The objective receives the complex (B, P, F)
    spectra of the complex field, Eobs[b, p, k] = sum_n Ez[p](after step n) exp(-i omega_k (n + 1) dt), and returns
    (J (B,), g (B, P, F)) with g = dJ/dRe(Eobs) + i dJ/dIm(Eobs), as for the real helpers.  The other arguments, the
    conditions and their host checks (ValueError naming the member) are batch_material_gradient's with
    boundary="periodic": sources, probes and the design window lie in columns 0..C-2, the window and a conductivity keep
    max(6, pml_cells) rows from the top and bottom edges, sigma is zero at every probe cell.

    The method: the forward run with the member's phase; hold_bloch_window; reset; the real weights from the unchanged
    channel systems; the adjoint run with the rotation conjugated (run_bloch_channels(conjugate=True)), the probe cells
    injecting into the real part of Ez; two plain products of the complex windows (bloch_window_product).

    Mind the ring-down: under a Bloch phase it depends on phi.  On the stand-in (64x17, 8-cell layer, eps_r in [1, 3] and
    sigma in [0.2, 0.7] S/m on 12 rows, 0.1 S/m on the other rows outside the layer, 5000 steps, frequencies 25 / 40 /
    55 GHz) phi = 2.4 and 3.0 rang down (forward end field 3e-8 of the peak) and the gradients matched central finite
    differences to 2e-7 of max|gradient|; phi = 0.7 and 1.5 kept an end field of 2e-3, whatever the conductivity of the
    conducting rows, and gradient errors of 3e-3 to 9e-3.  info["residual_*"] report the condition per member; the helper
    does not try to cure it.

    One call builds its engine and reads every probe trace back; a loop is what BlochAdjointSession is for.

    Returns (J (B,), grad_eps (B, nrows, ncols), grad_sigma (B, nrows, ncols) or None without sigma, spectra (B, P, F)
    complex128, info) with batch_eps_gradient's info keys; the residuals compare the larger of max|Re Ez| and max|Im Ez|
    over columns 0..C-2 with the larger part's largest probe sample."""
    p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, "periodic", pml_cells)
    phi = _bloch_phases(bloch_phase, p.B)
    weights = _check_weights(source_weights, p.B, p.Cc)
    s = None if sigma is None else _check_sigma(p, sigma)
    if engine is None:
        from .batch import BatchEngine as engine
    B, nsteps = p.B, p.nsteps
    with engine(B, p.R, p.Cc, dt, dx, dtype=dtype, boundary="periodic", device=device) as eng:
        # 1. forward: the member's own source and phase
        _bloch_setup(eng, p, s, phi, weights)
        _refuse_dispersion(eng)                 # an engine factory that sets the pole of set_bloch_dispersion
        eng.run(nsteps, p.amps)
        traces = eng.read_probes(0, nsteps)
        end_fwd = _part_peak(eng.download()[0][:, :, :-1])
        eng.hold_bloch_window()
        sr = probe_spectra(np.ascontiguousarray(traces.real), p.om, dt)
        si = probe_spectra(np.ascontiguousarray(traces.imag), p.om, dt)
        spectra = (sr.real - si.imag) + 1j * (sr.imag + si.real)

        # 2. the cotangent
        J, g = _cotangent(p, objective, spectra)

        # 3. adjoint: the rotation conjugated, fields zero, step 0; the probe cells inject the real series whose spectrum is
        # conj(g) / D into the real part
        c = _injections(p, g, p.eps, dtype)
        w = np.empty((B, p.P, 2 * p.F))
        for b in range(B):
            w[b] = np.linalg.solve(p.systems[p.which[b]][1], np.concatenate([c[b].real, c[b].imag], axis=1).T).T
        eng.reset()
        eng.set_bloch_point_sources(p.cells, w)
        eng.run_bloch_channels(nsteps, None, p.channels, conjugate=True)
        adj_traces = eng.read_probes(0, nsteps)
        end_adj = _part_peak(eng.download()[0][:, :, :-1])

        # 4. the gradients: the plain products of the two complex windows
        grad = eng.bloch_window_product(p.coef) * (dx / dt)
        grad_sigma = None if s is None else eng.bloch_window_product(p.coef_sigma) * (dx / 2)
    info = {"condition": max(v[2] for v in p.systems.values()),
            "residual_forward": _residual(end_fwd, _part_peak(traces)),
            "residual_adjoint": _residual(end_adj, _part_peak(adj_traces)), "channels_shared": p.shared}
    return J, grad, grad_sigma, spectra, info


class BlochAdjointSession(AdjointSession):
    """AdjointSession for Bloch batches: batch_bloch_gradient as a loop on a standing engine.

    The constructor takes batch_bloch_gradient's arguments (without the objective and sigma), makes its host checks and
    sets the engine up once, phase and source weights included.  value_and_grad(objective) returns (J, grad_eps, spectra,
    info); sigma_gradient(), set_design_eps, set_design_sigma and set_conductivity are AdjointSession's, and
    set_bloch_phase(phi) changes the phases between iterations ("ramp" weights follow them).  An iteration transforms
    the complex probe traces and takes the fields' maxima on the device (bloch_probe_spectra, bloch_field_absmax) and
    reads no trace, field or window back.  Ring-down under a Bloch phase depends on phi (batch_bloch_gradient): watch
    info["residual_*"] when the phase changes."""

    def __init__(self, eps, mu=None, *, bloch_phase, source_weights=None, nsteps, sources, probes, omegas, design,
                 fc=30e9, waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, pml_cells=40, device=0, engine=None):
        self._eng = None
        p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, "periodic", pml_cells)
        self._phi = _bloch_phases(bloch_phase, p.B)
        self._weights = _check_weights(source_weights, p.B, p.Cc)
        self._open(p, dtype, engine, device)

    # the engine calls of an iteration: the complex counterparts
    @staticmethod
    def _check_engine(eng):
        _refuse_dispersion(eng)                 # the engine's own calls refuse a batch without a phase

    def _setup_engine(self, eng):
        _bloch_setup(eng, self._p, None, self._phi, self._weights)

    def _spectra(self, eng, omegas):
        return eng.bloch_probe_spectra(omegas, 0, self._p.nsteps, peak=True)

    def _absmax(self, eng):
        return eng.bloch_field_absmax("Ez")

    def _hold(self, eng):
        eng.hold_bloch_window()

    def _run_adjoint(self, eng, weights):
        eng.set_bloch_point_sources(self._p.cells, weights)
        eng.run_bloch_channels(self._p.nsteps, None, self._p.channels, conjugate=True)

    def _product(self, eng, coef):
        return eng.bloch_window_product(coef)

    @property
    def bloch_phase(self):
        """The members' phases as the session holds them, (B,) float64, read-only."""
        v = self._phi.view()
        v.flags.writeable = False
        return v

    def set_bloch_phase(self, phi):
        """New phases for the following iterations: a scalar or (B,) in radians (ValueError naming the member for a value
        that is not finite, nothing changed).  "ramp" source weights are formed again from the new phases; the point
        sources, the window and the probes stay."""
        if self._eng is None:
            raise RuntimeError("the session is closed")
        ph = _bloch_phases(phi, self._p.B)
        self._eng.set_bloch_phase(ph)
        if isinstance(self._weights, str):
            self._eng.set_bloch_source(self._weights)
        self._phi = ph
        self._ran = False                       # the windows on the device belong to the old phases
        return self


# ---- dispersive batches: one Drude-Lorentz pole per member ----------------------------------------------------------------

def pole_coefficients(omegas, dt, gamma, omega0):
    """The factor of E_k * Eadj_k in the gradient with respect to the pole strength, and its scale's member part.

    omegas: (F,) or (B, F); gamma, omega0: scalars or (B,).  With z = exp(i omega dt), g = gamma dt / 2,
    a = (1 - g) / (1 + g), bq = dt / (1 + g) and ck = bq omega0^2 dt (include/fdtd2d_batch_dispersive.h, in float64)
    returns (-(z - 1) / ((z - a)(z - 1) + ck z) as complex (B, F), bq as (B,)):
    dJ/d wp2[i] = dx * bq * EPS0 * sum_k Re(factor_k * E_k[i] * Eadj_k[i])."""
    gam, om0 = np.atleast_1d(np.asarray(gamma, dtype=np.float64)), np.atleast_1d(np.asarray(omega0, dtype=np.float64))
    w = np.asarray(omegas, dtype=np.float64)
    B = max(gam.size, om0.size, w.shape[0] if w.ndim == 2 else 1)
    w = np.broadcast_to(w, (B, w.shape[-1]))
    g = np.broadcast_to(gam, (B,)) * dt / 2
    a, bq = (1 - g) / (1 + g), dt / (1 + g)
    ck = bq * np.broadcast_to(om0, (B,)) ** 2 * dt
    z = np.exp(1j * w * dt)
    return -(z - 1) / ((z - a[:, None]) * (z - 1) + ck[:, None] * z), bq


def _refuse_phase(eng):
    """_refuse_bloch without its refusal of a pole: complex fields are refused, the pole is what these calls are for."""
    _refuse_hz(eng)
    if getattr(eng, "_bloch", None) is not None:
        from ._abi import E_STATE, Fdtd2dError
        raise Fdtd2dError(E_STATE, "adjoint gradients are not available while a Bloch phase is set (complex fields)")


def _check_pole_boundary(boundary):
    if boundary not in ("pml", "periodic"):
        raise ValueError(f'boundary must be "pml" or "periodic", not {boundary!r}: a dispersive pole needs the PML layer '
                         f'or periodic columns')


def _check_wp2(p, wp2, window=None):
    """_check_sigma's rules for the strength of a pole: the shape, >= 0 and finite, zero in the margin and the layer and
    at every probe cell."""
    return _check_sigma(p, wp2, window, name="wp2", may="carry a pole",
                        probe_why="assumes conj(g) / D, which a pole at the cell would change")


def _check_dispersion(p, dispersion):
    """The host checks of dispersion = (wp2, gamma, omega0) (ValueError naming the member).  Returns the three as float64
    arrays (B, R, C), (B,), (B,)."""
    if dispersion is None or len(dispersion) != 3:
        raise ValueError("dispersion must be (wp2, gamma, omega0)")
    wp2, gamma, omega0 = dispersion
    per = []
    for v, nm in ((gamma, "gamma"), (omega0, "omega0")):
        a = np.asarray(v, dtype=np.float64)
        if a.shape not in ((), (p.B,)):
            raise ValueError(f"{nm} must be a scalar or have shape ({p.B},), got {a.shape}")
        a = np.ascontiguousarray(np.broadcast_to(a, (p.B,)))
        bad = ~(np.isfinite(a) & (a >= 0))
        if bad.any():
            raise ValueError(f"member {int(np.nonzero(bad)[0][0])}: {nm} must be >= 0 and finite")
        per.append(a)
    if wp2 is None:
        raise ValueError("member 0 (and every other): wp2 is required (a scalar or (B, R, C)); without a pole use "
                         "batch_material_gradient")
    return _check_wp2(p, wp2), per[0], per[1]


def _pole_products(p, gamma, omega0):
    """The three coefficient sets (3, B, F) and their scales (B, 3): eps, sigma, wp2."""
    from .api import EPS0
    cw, bq = pole_coefficients(p.om, p.dt, gamma, omega0)
    scales = np.stack([np.full(p.B, p.dx / p.dt), np.full(p.B, p.dx / 2), p.dx * bq * EPS0], axis=1)
    return np.stack([p.coef, p.coef_sigma, cw]), scales


def batch_dispersive_gradient(eps, sigma, dispersion, mu=None, *, nsteps, sources, probes, omegas, design, objective,
                              fc=30e9, waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml",
                              pml_cells=40, device=0, engine=None):
    """batch_material_gradient for members with a Drude-Lorentz pole: the gradients of the objective with respect to eps,
    to the conductivity sigma and to the pole strength wp2 over the design window, from the same two runs.

    dispersion = (wp2, gamma, omega0) as run_fdtd_batch(dispersion=) and BatchEngine.set_dispersion take them: wp2
    (B, R, C) in rad^2/s^2 (a scalar: every cell that may carry it), gamma and omega0 scalars or (B,) in rad/s.  sigma:
    as batch_material_gradient takes it (None: zero).  boundary "pml" or "periodic": a pole needs the layer or periodic
    columns.  The other arguments, the conditions and their checks are batch_material_gradient's.  In addition, checked
    on the host with a ValueError that names the member, before any engine work: wp2 under the rules of sigma (the shape,
    >= 0 and finite, zero in the margin and the layer) and zero at every probe cell (the injection assumes
    conj(g) / D); gamma and omega0 >= 0 and finite.  The library adds its stability refusal (E_ARG, set_dispersion).

    The method is batch_material_gradient's: the pole adds a diagonal term to the one-step operator, which stays
    symmetric, so the adjoint run is a dispersive run of the same member with sources at the probe cells.  The forward
    window is held with hold_dispersive_window, and one dispersive_window_product forms the three gradients in one pass
    over the two windows.  gamma and omega0 are not differentiated.

    Returns (J (B,), grad_eps, grad_sigma, grad_wp2 (B, nrows, ncols) float64 each, spectra (B, P, F) complex128,
    info)."""
    _check_pole_boundary(boundary)
    p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, boundary, pml_cells)
    s = _check_sigma(p, 0.0 if sigma is None else sigma)
    wp2, gamma, omega0 = _check_dispersion(p, dispersion)
    coefs, scales = _pole_products(p, gamma, omega0)
    if engine is None:
        from .batch import BatchEngine as engine
    B = p.B
    with engine(B, p.R, p.Cc, dt, dx, dtype=dtype, boundary=boundary, device=device) as eng:
        _refuse_phase(eng)
        # 1. forward: the member's own source; the pole after the materials, the layer and the conductivity
        _setup(eng, p)
        eng.set_conductivity(s)
        eng.set_dispersion(wp2, gamma, omega0)
        eng.run(nsteps, p.amps)
        traces = eng.read_probes(0, nsteps)
        end_fwd = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)
        eng.hold_dispersive_window()
        spectra = probe_spectra(traces, p.om, dt)

        # 2. the cotangent
        J, g = _cotangent(p, objective, spectra)

        # 3. adjoint: same materials and pole, fields and pole state zero, step 0
        c = _injections(p, g, p.eps, dtype)
        weights = np.empty((B, p.P, 2 * p.F))
        for b in range(B):
            weights[b] = np.linalg.solve(p.systems[p.which[b]][1], np.concatenate([c[b].real, c[b].imag], axis=1).T).T
        eng.reset()
        eng.set_point_sources(p.cells, weights)
        eng.run(nsteps, None, p.channels)
        adj_traces = eng.read_probes(0, nsteps)
        end_adj = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)

        # 4. the three gradients: one pass over the two windows
        grads = eng.dispersive_window_product(coefs, scales)

    def peak(tr):
        flat = tr.reshape(B, -1)
        return np.maximum(flat.max(axis=1), -flat.min(axis=1))
    info = {"condition": max(v[2] for v in p.systems.values()),
            "residual_forward": _residual(end_fwd, peak(traces)), "residual_adjoint": _residual(end_adj, peak(adj_traces)),
            "channels_shared": p.shared}
    return J, grads[0], grads[1], grads[2], spectra, info


class DispersiveAdjointSession(AdjointSession):
    """AdjointSession for members with a Drude-Lorentz pole: batch_dispersive_gradient as a loop on a standing engine.

    The constructor takes batch_dispersive_gradient's arguments (without the objective; dispersion and sigma by keyword),
    makes its host checks and sets the engine up once, conductivity and pole included.  value_and_grad(objective)
    returns (J, grad_eps, spectra, info) as the base class does and keeps the windows; sigma_gradient() and
    wp2_gradient() belong to the latest value_and_grad.  The three gradients come from one dispersive_window_product, one
    launch and one read-back per iteration, and are kept until the next value_and_grad.  set_design_eps,
    set_design_sigma and set_conductivity are AdjointSession's; set_design_wp2(wp2_window) replaces the strengths of the
    design window.  A set_design_eps or set_design_wp2 that the library's stability check refuses (E_ARG) leaves the
    engine and the session as they were.

        with DispersiveAdjointSession(eps, dispersion=(wp2, gamma, omega0), nsteps=..., ..., design=win) as s:
            for it in range(100):
                J, g_eps, spectra, info = s.value_and_grad(objective)
                s.set_design_wp2(np.clip(s.wp2[:, r0:r0 + nr, c0:c0 + nc] + step * s.wp2_gradient(), 0, hi))
    """

    def __init__(self, eps, mu=None, *, dispersion, sigma=None, nsteps, sources, probes, omegas, design, fc=30e9,
                 waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml", pml_cells=40, device=0,
                 engine=None):
        self._eng = None
        _check_pole_boundary(boundary)
        p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, boundary, pml_cells)
        self._sigma0 = None if sigma is None else _check_sigma(p, sigma)
        self._wp2, self._gamma, self._omega0 = _check_dispersion(p, dispersion)
        self._wp2 = self._wp2.copy()
        self._coefs, self._scales = _pole_products(p, self._gamma, self._omega0)
        self._scales[:, 0] = 1.0                # value_and_grad scales the eps gradient itself, as the base class does
        self._grads = None                      # the three products of the latest value_and_grad
        self._pole_set = False
        self._open(p, dtype, engine, device)

    def _check_engine(self, eng):
        """A Bloch phase is refused as for AdjointSession; the pole, once set, is required."""
        _refuse_phase(eng)
        if self._pole_set and not eng.dispersive:
            from ._abi import E_STATE, Fdtd2dError
            raise Fdtd2dError(E_STATE, "DispersiveAdjointSession needs its dispersive pole: it was removed from the "
                              "session's engine (a batch without one takes AdjointSession)")

    def _setup_engine(self, eng):
        _setup(eng, self._p)
        if self._sigma0 is not None:
            eng.set_conductivity(self._sigma0)
            self._sigma = self._sigma0.copy()
        eng.set_dispersion(self._wp2, self._gamma, self._omega0)
        self._pole_set = True

    def _hold(self, eng):
        eng.hold_dispersive_window()

    def _product(self, eng, coef):
        # the base class asks for the eps product; the other two ride along in the same pass
        self._grads = eng.dispersive_window_product(self._coefs, self._scales)
        return self._grads[0]

    def _latest(self, k):
        if self._eng is None:
            raise RuntimeError("the session is closed")
        if not self._ran or self._grads is None:
            raise RuntimeError("no gradient yet: call value_and_grad first")
        return self._grads[k].copy()

    def sigma_gradient(self):
        """dJ/d sigma over the design window, (B, nrows, ncols) float64, for the latest value_and_grad (formed with it:
        no further launch)."""
        return self._latest(1)

    def wp2_gradient(self):
        """dJ/d wp2 over the design window, (B, nrows, ncols) float64, for the latest value_and_grad (formed with it: no
        further launch)."""
        return self._latest(2)

    @property
    def wp2(self):
        """The members' pole strengths as the session holds them, (B, R, C) float64, read-only."""
        v = self._wp2.view()
        v.flags.writeable = False
        return v

    def set_design_wp2(self, wp2_window):
        """New pole strengths of the design window for every member: (B, nrows, ncols).  Checked on the host (ValueError,
        nothing changed): the shape, values >= 0 and finite, zero at probe cells; the library's stability refusal
        (E_ARG) changes nothing either."""
        p = self._p
        if self._eng is None:
            raise RuntimeError("the session is closed")
        r0, c0, nr, nc = p.win
        w = _check_wp2(p, wp2_window, p.win)
        self._eng.set_dispersion_window(p.win, w)
        self._wp2[:, r0:r0 + nr, c0:c0 + nc] = w
        return self


# ---- flux objectives: the adjoint of the flux monitor -----------------------------------------------------------------

def _line_entries(lines):
    """(rows, cols, line index, column-line flag) of the lines' cells concatenated in the order given."""
    i, j, k, col = [], [], [], []
    for n, (kind, at, first, count) in enumerate(lines):
        run = np.arange(int(first), int(first) + int(count))
        c = kind == "col"
        i.append(run if c else np.full(len(run), int(at)))
        j.append(np.full(len(run), int(at)) if c else run)
        k.append(np.full(len(run), n))
        col.append(np.full(len(run), c))
    return tuple(np.concatenate(a) for a in (i, j, k, col))


def flux_adjoint_weights(E, H, dJdP, lines, omegas, dt, dx, solve, scale_e=None, scale_h=None):
    """The line sources of the adjoint of a flux objective, on the host: what BatchEngine.flux_adjoint_sources forms on
    the device.  E, H: the raw sums of read_flux_lines(raw=True), (B, F, cells).  dJdP: (B, N, F).  solve: (2F, 2F) or
    (B, 2F, 2F), the inverse of the channel system.  scale_e, scale_h: (B, cells) or None for ones.  Returns (we, wh),
    each (B, cells, 2F), for set_flux_line_sources."""
    B, F, cells = E.shape
    w = _window_omegas(omegas, B)
    g = np.exp(0.5j * w * dt)[:, :, None]
    _, _, k, col = _line_entries(lines)
    c = np.asarray(dJdP, dtype=np.float64)[:, k, :].transpose(0, 2, 1) * (np.where(col, -1.0, 1.0) * dx)[None, None, :]
    return _target_weights(c * np.conj(H * g), c * np.conj(E * g), solve, scale_e, scale_h)


def _target_weights(ae, ah, solve, scale_e=None, scale_h=None):
    """The core of flux_adjoint_weights: per-entry complex targets ae (the coefficient of dE in dJ = Re sum ae dE + ...)
    and ah (that of dH, in the header's convention: times conj(g)^2, the H part being injected a step earlier), each
    (B, F, cells); weights = solve @ [Re (scale * target); Im (scale * target)]."""
    B, F, cells = ae.shape
    one = np.ones((B, cells))
    te = (one if scale_e is None else np.asarray(scale_e, dtype=np.float64))[:, None, :] * ae
    th = (one if scale_h is None else np.asarray(scale_h, dtype=np.float64))[:, None, :] * ah
    s = np.broadcast_to(np.asarray(solve, dtype=np.float64), (B, 2 * F, 2 * F))
    return tuple(np.ascontiguousarray(np.einsum("bck,bkw->bwc", s, np.concatenate([t.real, t.imag], axis=1)))
                 for t in (te, th))


def _gap(lo, n, x, period=None):
    """Cells between coordinate(s) x and the run [lo, lo + n): 0 inside; cyclic with a period."""
    d = np.maximum(np.maximum(lo - x, x - (lo + n - 1)), 0)
    if period:
        for s in (-period, period):
            d = np.minimum(d, np.maximum(np.maximum(lo - (x + s), (x + s) - (lo + n - 1)), 0))
    return d


def _flux_plan(eps, sigma, mu, nsteps, sources, flux_lines, omegas, design, fc, waveform, dt, dx, dtype, boundary,
               pml_cells):
    """The host checks of batch_flux_gradient (ValueError naming the reason), the plan of _plan with one residual probe
    per line (its first cell), the checked conductivity, the lines and the per-entry scales of the adjoint sources."""
    from .api import MU0
    from .batch import _flux_lines
    if boundary not in ("pml", "periodic"):
        raise ValueError(f'boundary must be "pml" or "periodic" (flux lines live on those batches), not {boundary!r}')
    eps = np.asarray(eps)
    if eps.ndim != 3:
        raise ValueError(f"eps must have shape (B, R, C), got {eps.shape}")
    B, R, Cc = eps.shape
    periodic = boundary == "periodic"
    lines = [tuple(l) for l in flux_lines]
    _flux_lines(lines, omegas, 1, B, R, Cc, periodic)
    li, lj, _, lcol = _line_entries(lines)
    probes = np.array([[li[o], lj[o]] for o in np.cumsum([0] + [int(l[3]) for l in lines[:-1]])])
    p = _plan(eps, mu, nsteps, sources, probes, omegas, design, fc, waveform, dt, dx, boundary, pml_cells)
    L, Q = p.L, Cc - 1
    in_layer = (li < L) | (li > R - 1 - L) | (False if periodic else (lj < L) | (lj > Cc - 1 - L))
    if in_layer.any():
        o = int(np.nonzero(in_layer)[0][0])
        raise ValueError(f"member 0 (and every other): the flux line cell ({li[o]}, {lj[o]}) lies in the {L}-cell PML "
                         f"layer, where the sums are the layer's split fields', not a flux")
    edge = (li < 1) | (li > R - 2) | (False if periodic else (lj < 1) | (lj > Cc - 2))
    if edge.any():
        o = int(np.nonzero(edge)[0][0])
        raise ValueError(f"member 0 (and every other): the flux line cell ({li[o]}, {lj[o]}) lies on the edge of the grid")
    r0, c0, nr, nc = p.win
    near = np.maximum(_gap(r0, nr, li), _gap(c0, nc, lj, Q if periodic else None)) < 2
    if near.any():
        o = int(np.nonzero(near)[0][0])
        raise ValueError(f"member 0 (and every other): the flux line cell ({li[o]}, {lj[o]}) is closer than 2 cells to the "
                         f"design window {p.win}: the adjoint sources take the permittivity there as fixed")
    for b, (sr, sc, snr, snc) in enumerate(p.rects):
        if snr and snc:
            near = np.maximum(_gap(sr, snr, li), _gap(sc, snc, lj, Q if periodic else None)) < 2
            if near.any():
                o = int(np.nonzero(near)[0][0])
                raise ValueError(f"member {b}: the flux line cell ({li[o]}, {lj[o]}) is closer than 2 cells to the forward "
                                 f"source {(int(sr), int(sc), int(snr), int(snc))}, whose direct term the monitor would "
                                 f"read")
    s = None if sigma is None else _check_sigma(p, sigma)
    if s is not None and np.any(s[:, li, lj] != 0):
        b = int(np.nonzero((s[:, li, lj] != 0).any(axis=1))[0][0])
        raise ValueError(f"member {b}: sigma is non-zero at a flux line cell; the adjoint injection there would be "
                         f"conj(g) / (D + G), which is not implemented")
    # the two H values of an entry take the same 0.5 s_h, so the H update's ch = dt / (mu dx) must agree on them
    mu_e = np.broadcast_to(np.asarray(MU0 if mu is None else mu), eps.shape).astype(dtype).astype(np.float64)
    before = mu_e[:, np.where(lcol, li, li - 1), np.where(lcol, np.where(lj == 0, Q - 1, lj - 1), lj)]
    if np.any(mu_e[:, li, lj] != before):
        b = int(np.nonzero((mu_e[:, li, lj] != before).any(axis=1))[0][0])
        raise ValueError(f"member {b}: mu differs between the two H values of a flux line cell; the adjoint's magnetic "
                         f"sheet drives both with one weight")
    D = eps.astype(dtype).astype(np.float64)[:, li, lj] * dx / dt
    p.lines, p.sigma = lines, s
    p.scale_e, p.scale_h = 1.0 / D, -dt / (mu_e[:, li, lj] * dx)
    p.solve = np.stack([np.linalg.inv(p.systems[k][1]) for k in p.which])
    return p


def _flux_cotangent(p, objective, P):
    J, g = objective(P)
    J = np.asarray(J, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    if J.shape != (p.B,) or g.shape != P.shape:
        raise ValueError(f"objective must return J of shape ({p.B},) and dJ/dP of shape {P.shape}, got {J.shape} and "
                         f"{g.shape}")
    return J, g


def batch_flux_gradient(eps, sigma=None, mu=None, *, nsteps, sources, flux_lines, omegas, design, objective, fc=30e9,
                        waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml", pml_cells=40, device=0,
                        engine=None):
    """Gradient of an objective on the power through flux lines with respect to eps (and sigma) over a design window,
    for B members at once, at the cost of two runs per member.

    flux_lines: up to 4 lines as BatchEngine.set_flux_lines takes them, shared by all members; omegas: (F,) or (B, F).
    objective(P) takes the float64 (B, N, F) array of BatchEngine.flux() and returns (J (B,), dJ/dP (B, N, F)).  The
    other arguments are batch_material_gradient's; boundary is "pml" or "periodic".

    The method (module docstring): the forward run records the window DFT over the design
    window and the lines' sums; the cotangent of P on a line cell has an electric part, dJ/dP s dx conj(H g) / D, and a
    magnetic part, -dJ/dP s dx conj(E g) dt / (mu dx); the adjoint run drives the same member through
    set_flux_line_sources with the 2F channels of the probe helpers, and dft_window_product with the unchanged
    coefficients forms the gradients.

    Conditions, checked on the host before any device work (ValueError naming the reason), beside those of
    batch_material_gradient: every line cell lies outside the PML layer and off the grid's edge, at least 2 cells from the
    design window and from every forward source; sigma is zero at the line cells; mu agrees on the two H values of every
    line cell.  info["residual_forward"] and info["residual_adjoint"] compare the end-of-run max|Ez| with the largest
    sample at the first cell of each line.

    Out of scope: Bloch batches (batch_bloch_flux_gradient serves them) and lattice batches, dJ/d wp2 of a dispersive
    member, gradients with respect to mu.

    Returns (J (B,), grad_eps (B, nrows, ncols), grad_sigma (the same shape, or None without sigma), P (B, N, F), info)."""
    p = _flux_plan(eps, sigma, mu, nsteps, sources, flux_lines, omegas, design, fc, waveform, dt, dx, dtype, boundary,
                   pml_cells)
    if engine is None:
        from .batch import BatchEngine as engine
    B = p.B
    with engine(B, p.R, p.Cc, dt, dx, dtype=dtype, boundary=boundary, device=device) as eng:
        _refuse_bloch(eng)
        _setup(eng, p)
        if p.sigma is not None:
            eng.set_conductivity(p.sigma)
        eng.set_flux_lines(p.lines, p.om)
        eng.run(p.nsteps, p.amps)
        traces = eng.read_probes(0, p.nsteps)
        end_fwd = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)
        eng.hold_dft_window()
        P = eng.flux()
        J, g = _flux_cotangent(p, objective, P)
        E, H = eng.read_flux_lines(raw=True)
        we, wh = flux_adjoint_weights(E, H, g, p.lines, p.om, dt, dx, p.solve, p.scale_e, p.scale_h)
        eng.reset()
        eng.set_flux_line_sources(we, wh)
        eng.run(p.nsteps, None, p.channels)
        adj_traces = eng.read_probes(0, p.nsteps)
        end_adj = np.abs(eng.download()[0].astype(np.float64)).reshape(B, -1).max(axis=1)
        grad = eng.dft_window_product(p.coef) * (dx / dt)
        grad_sigma = None if p.sigma is None else eng.dft_window_product(p.coef_sigma) * (dx / 2)

    def peak(tr):
        return np.abs(tr.reshape(B, -1)).max(axis=1)
    info = {"condition": max(s[2] for s in p.systems.values()),
            "residual_forward": _residual(end_fwd, peak(traces)), "residual_adjoint": _residual(end_adj, peak(adj_traces)),
            "channels_shared": p.shared}
    return J, grad, grad_sigma, P, info


class FluxAdjointSession(AdjointSession):
    """batch_flux_gradient as a loop: AdjointSession for objectives on the power through flux lines.

    The constructor takes batch_flux_gradient's arguments (without the objective) and makes its host checks.
    value_and_grad(objective) returns (J, grad_eps, P, info); it forms the adjoint sources on the device
    (BatchEngine.flux_adjoint_sources), so B * N * F powers and B * nrows * ncols gradients come down, B * N * F
    derivatives go up, and no line spectrum, trace, field or window is read back.  set_design_eps, set_design_sigma,
    set_conductivity, sigma_gradient and info["residual_*"] behave as in AdjointSession; a conductivity must stay zero on
    the line cells."""

    def __init__(self, eps, sigma=None, mu=None, *, nsteps, sources, flux_lines, omegas, design, fc=30e9,
                 waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64, boundary="pml", pml_cells=40, device=0,
                 engine=None):
        self._eng = None
        p = _flux_plan(eps, sigma, mu, nsteps, sources, flux_lines, omegas, design, fc, waveform, dt, dx, dtype, boundary,
                       pml_cells)
        self._open(p, dtype, engine, device)
        if p.sigma is not None:
            self._sigma = p.sigma.copy()

    def _setup_engine(self, eng):
        p = self._p
        _setup(eng, p)
        if p.sigma is not None:
            eng.set_conductivity(p.sigma)
        eng.set_flux_lines(p.lines, p.om)

    def _check_line_sigma(self, s, r0=0, c0=0):
        li, lj, _, _ = _line_entries(self._p.lines)
        inside = (li >= r0) & (li < r0 + s.shape[1]) & (lj >= c0) & (lj < c0 + s.shape[2])
        if np.any(s[:, li[inside] - r0, lj[inside] - c0] != 0):
            raise ValueError("member 0 (or another): sigma is non-zero at a flux line cell; the adjoint injection there "
                             "would be conj(g) / (D + G), which is not implemented")

    def set_conductivity(self, sigma):
        if sigma is not None and self._eng is not None:
            self._check_line_sigma(_check_sigma(self._p, sigma))
        return super().set_conductivity(sigma)

    def value_and_grad(self, objective):
        """(J (B,), grad_eps (B, nrows, ncols) float64, P (B, N, F) float64, info) of the current materials."""
        p, eng = self._p, self._eng
        if eng is None:
            raise RuntimeError("the session is closed")
        self._check_engine(eng)
        none = np.empty((p.B, 0))
        eng.reset()
        eng.run(p.nsteps, p.amps)
        _, peak_fwd = self._spectra(eng, none)
        end_fwd = self._absmax(eng)
        self._hold(eng)
        P = eng.flux()
        J, g = _flux_cotangent(p, objective, P)
        eng.flux_adjoint_sources(g, p.solve[0] if p.shared else p.solve, p.scale_e, p.scale_h)
        eng.reset()
        eng.run(p.nsteps, None, p.channels)
        _, peak_adj = self._spectra(eng, none)
        end_adj = self._absmax(eng)
        grad = self._product(eng, p.coef) * (p.dx / p.dt)
        self._ran = True
        info = {"condition": self._condition, "residual_forward": _residual(end_fwd, peak_fwd),
                "residual_adjoint": _residual(end_adj, peak_adj), "channels_shared": p.shared}
        return J, grad, P, info


# ---- flux objectives on Bloch batches: the adjoint of the complex flux monitor ------------------------------------------

def _orders_targets(E, H, dJdPm, phi, first, omegas, dt, dx):
    """The per-entry targets of an objective on flux_orders of a whole-period row line whose entries start at `first`:
    (ae, ah), each (B, F, cells), zero off that line.  dJdPm: (B, F, Q) in np.fft.fftfreq order."""
    B, F, cells = E.shape
    Q = dJdPm.shape[2]
    g = np.exp(0.5j * _window_omegas(omegas, B) * dt)[:, :, None]
    m = np.fft.fftfreq(Q, 1 / Q)
    ker = np.exp(-1j * (phi[:, None, None] + 2 * np.pi * m[None, :, None]) * np.arange(Q)[None, None, :] / Q)   # (B, m, j)
    sl = slice(first, first + Q)
    Em = np.einsum("bfj,bmj->bfm", E[:, :, sl] * g, ker) / Q
    Hm = np.einsum("bfj,bmj->bfm", H[:, :, sl] * g, ker) / Q
    ae, ah = np.zeros((B, F, cells), np.complex128), np.zeros((B, F, cells), np.complex128)
    ae[:, :, sl] = dx * np.einsum("bfm,bmj->bfj", dJdPm * np.conj(Hm), ker)
    ah[:, :, sl] = dx * np.einsum("bfm,bmj->bfj", dJdPm * np.conj(Em), ker)
    return ae, ah


def bloch_flux_adjoint_weights(E, H, dJdP, lines, omegas, dt, dx, solve, scale_e=None, scale_h=None, orders=None):
    """The line sources of the adjoint of a flux objective on a Bloch batch, on the host: what
    BatchEngine.bloch_flux_adjoint_sources forms on the device.  E, H: the raw sums of the complex fields,
    read_flux_lines(raw=True), (B, F, cells); the other arguments are flux_adjoint_weights'.  orders: None, or
    (line, dJdPm (B, F, Q), phi (B,)) for an objective that also depends on flux_orders(line); its cotangent is mapped
    back to the line's cells (batch_bloch_flux_gradient has the map) and added to the targets.  Returns real (we, wh),
    each (B, cells, 2F), for set_bloch_flux_line_sources: a real series on the real part carries any complex spectrum at
    omega > 0, and the rotated seam term of the sources supplies the rest."""
    B, F, cells = E.shape
    g = np.exp(0.5j * _window_omegas(omegas, B) * dt)[:, :, None]
    _, _, k, col = _line_entries(lines)
    c = np.asarray(dJdP, dtype=np.float64)[:, k, :].transpose(0, 2, 1) * (np.where(col, -1.0, 1.0) * dx)[None, None, :]
    ae, ah = c * np.conj(H * g), c * np.conj(E * g)
    if orders is not None:
        line, dJdPm, phi = orders
        first = sum(int(l[3]) for l in lines[:int(line)])
        oe, oh = _orders_targets(E, H, np.asarray(dJdPm, dtype=np.float64), np.asarray(phi, dtype=np.float64), first,
                                 omegas, dt, dx)
        ae, ah = ae + oe, ah + oh
    return _target_weights(ae, ah, solve, scale_e, scale_h)


def _bloch_flux_plan(eps, sigma, mu, bloch_phase, source_weights, nsteps, sources, flux_lines, omegas, design, fc,
                     waveform, dt, dx, dtype, pml_cells, orders_line):
    """The host checks of batch_bloch_flux_gradient: _flux_plan's with periodic columns, the Bloch helpers' checks of phase
    and source weights, positive frequencies, and orders_line a whole-period row line."""
    om = np.asarray(omegas, dtype=np.float64)
    if om.size and not np.all(om > 0):
        raise ValueError("omegas must be positive: the flux monitors of a Bloch batch take either sign, the channel "
                         "system of the gradient helpers does not (a real series carries omega and -omega together)")
    p = _flux_plan(eps, sigma, mu, nsteps, sources, flux_lines, omegas, design, fc, waveform, dt, dx, dtype, "periodic",
                   pml_cells)
    phi = _bloch_phases(bloch_phase, p.B)
    weights = _check_weights(source_weights, p.B, p.Cc)
    if orders_line is not None:
        k = int(orders_line)
        if not 0 <= k < len(p.lines):
            raise ValueError(f"orders_line {orders_line} outside 0..{len(p.lines) - 1}")
        kind, _, first, n = p.lines[k]
        if kind != "row" or int(first) != 0 or int(n) != p.Cc - 1:
            raise ValueError(f"orders_line {k} must be a row line over the whole period (columns 0..{p.Cc - 2}), not "
                             f"{p.lines[k]}")
    return p, phi, weights


def _refuse_bloch_flux_pole(eng):
    """An engine with the pole of set_bloch_dispersion (an engine factory that sets one, or the call on a session's
    engine) is refused before any run: hold_bloch_window does not serve it, and dJ/d wp2 under a phase is out of scope."""
    _refuse_hz(eng)
    if getattr(eng, "dispersive", False):
        raise ValueError("the engine carries a dispersive pole (set_bloch_dispersion): gradients of flux under a Bloch "
                         "phase are not available with the pole")


def _bloch_flux_cotangent(p, objective, P, Pm):
    """(J, dJ/dP, dJ/dPm or None) of objective(P) or objective(P, Pm), shapes checked."""
    if Pm is None:
        J, g = _flux_cotangent(p, objective, P)
        return J, g, None
    J, g, gm = objective(P, Pm)
    J, g, gm = (np.asarray(a, dtype=np.float64) for a in (J, g, gm))
    if J.shape != (p.B,) or g.shape != P.shape or gm.shape != Pm.shape:
        raise ValueError(f"objective must return J of shape ({p.B},), dJ/dP of shape {P.shape} and dJ/dPm of shape "
                         f"{Pm.shape}, got {J.shape}, {g.shape} and {gm.shape}")
    return J, g, gm


def _bloch_flux_lines_setup(eng, p):
    """The lines, then silent line sources with the 2F channels of the adjoint run: with them the engine accepts
    hold_bloch_window and run_bloch_channels beside the lines."""
    eng.set_bloch_flux_lines(p.lines, p.om)
    cells = sum(int(l[3]) for l in p.lines)
    zero = np.zeros((cells, 2 * p.F))
    eng.set_bloch_flux_line_sources(zero, zero)


def batch_bloch_flux_gradient(eps, sigma=None, mu=None, *, bloch_phase, source_weights=None, nsteps, sources, flux_lines,
                              omegas, design, objective, orders_line=None, fc=30e9, waveform="ricker", dt=5e-14,
                              dx=1e-4, dtype=np.float64, pml_cells=40, device=0, engine=None):
    """batch_flux_gradient for Bloch batches: the gradient of an objective on the power through flux lines of complex
    fields, and on its split over the diffraction orders, with respect to eps (and sigma) over a design window.

    bloch_phase, source_weights: as in batch_bloch_gradient.  flux_lines: as BatchEngine.set_bloch_flux_lines takes them;
    omegas must be positive (ValueError: the monitors take either sign, the channel system of the adjoint does not).
    Without orders_line, objective(P) takes flux() (B, N, F) and returns (J (B,), dJ/dP).  With orders_line = k, a row
    line over the whole period, objective(P, Pm) also takes flux_orders(k) (B, F, Q) and returns (J, dJ/dP, dJ/dPm).
    The other arguments and host checks are batch_flux_gradient's with boundary="periodic" (line cells outside the layer,
    2 cells from the design window and the sources, sigma zero on them) and batch_bloch_gradient's; an engine with the
    pole of set_bloch_dispersion is refused.

    The method: set_bloch_flux_lines; silent line sources with K = 2F (set_bloch_flux_line_sources), which make the
    engine accept the next calls beside the lines; the forward run; hold_bloch_window; flux() and the orders; the
    cotangent and the weights (bloch_flux_adjoint_weights); reset; run_bloch_channels(conjugate=True), which drives the
    line sources with the rotation conjugated, the seam term with it; two bloch_window_products with the unchanged
    coefficients.

    The orders.  With ker[m, j] = exp(-1j * (phi + 2 pi m) * j / Q), E_m = (1/Q) sum_j ker[m, j] E_j and H_m likewise (H
    with the half-step factor g), Pm = dx Q Re(E_m conj(H_m)) is bilinear in the harmonics, which are linear in the line
    spectra, so dJ = Re sum_j (ae_j dE_j + ...) with
        ae_j = dx sum_m dJ/dPm conj(H_m) ker[m, j]        ah_j = dx sum_m dJ/dPm conj(E_m g) ker[m, j]
    added to the line's own targets dJ/dP dx conj(H_j), dJ/dP dx conj(E_j g).  sum_m conj(ker[m, j']) ker[m, j] = Q
    delta(j, j'), so dJ/dPm = 1 gives exactly the targets of dJ/dP = 1 on that line (Parseval).

    Mind the ring-down, as in batch_bloch_gradient: it depends on phi.

    Returns (J (B,), grad_eps (B, nrows, ncols), grad_sigma or None, P (B, N, F), info) with batch_eps_gradient's info
    keys; the residuals compare the end fields with the largest sample at the first cell of each line."""
    p, phi, weights = _bloch_flux_plan(eps, sigma, mu, bloch_phase, source_weights, nsteps, sources, flux_lines, omegas,
                                       design, fc, waveform, dt, dx, dtype, pml_cells, orders_line)
    if engine is None:
        from .batch import BatchEngine as engine
    B = p.B
    with engine(B, p.R, p.Cc, dt, dx, dtype=dtype, boundary="periodic", device=device) as eng:
        _bloch_setup(eng, p, p.sigma, phi, weights)
        _refuse_bloch_flux_pole(eng)
        _bloch_flux_lines_setup(eng, p)
        eng.run(p.nsteps, p.amps)
        traces = eng.read_probes(0, p.nsteps)
        end_fwd = _part_peak(eng.download()[0][:, :, :-1])
        eng.hold_bloch_window()
        P = eng.flux()
        Pm = None if orders_line is None else eng.flux_orders(int(orders_line))
        J, g, gm = _bloch_flux_cotangent(p, objective, P, Pm)
        E, H = eng.read_flux_lines(raw=True)
        we, wh = bloch_flux_adjoint_weights(E, H, g, p.lines, p.om, dt, dx, p.solve, p.scale_e, p.scale_h,
                                            None if gm is None else (int(orders_line), gm, phi))
        eng.reset()
        eng.set_bloch_flux_line_sources(we, wh)
        eng.run_bloch_channels(p.nsteps, None, p.channels, conjugate=True)
        adj_traces = eng.read_probes(0, p.nsteps)
        end_adj = _part_peak(eng.download()[0][:, :, :-1])
        grad = eng.bloch_window_product(p.coef) * (dx / dt)
        grad_sigma = None if p.sigma is None else eng.bloch_window_product(p.coef_sigma) * (dx / 2)
    info = {"condition": max(v[2] for v in p.systems.values()),
            "residual_forward": _residual(end_fwd, _part_peak(traces)),
            "residual_adjoint": _residual(end_adj, _part_peak(adj_traces)), "channels_shared": p.shared}
    return J, grad, grad_sigma, P, info


class BlochFluxAdjointSession(FluxAdjointSession, BlochAdjointSession):
    """batch_bloch_flux_gradient as a loop: BlochAdjointSession's standing engine with FluxAdjointSession's objective.

    The constructor takes batch_bloch_flux_gradient's arguments (without the objective) and makes its host checks.
    value_and_grad(objective) returns (J, grad_eps, P, info).  For an objective on P it forms the adjoint sources on
    the device (BatchEngine.bloch_flux_adjoint_sources) and reads no line spectrum, trace, field or window back.  With
    orders_line it reads the line spectra back (flux_orders and the weights are host arithmetic over them) and installs
    the weights from the host.  set_design_eps, set_design_sigma, set_conductivity (zero on the line cells) and
    sigma_gradient are FluxAdjointSession's; set_bloch_phase is BlochAdjointSession's and keeps the lines."""

    def __init__(self, eps, sigma=None, mu=None, *, bloch_phase, source_weights=None, nsteps, sources, flux_lines,
                 omegas, design, orders_line=None, fc=30e9, waveform="ricker", dt=5e-14, dx=1e-4, dtype=np.float64,
                 pml_cells=40, device=0, engine=None):
        self._eng = None
        p, self._phi, self._weights = _bloch_flux_plan(eps, sigma, mu, bloch_phase, source_weights, nsteps, sources,
                                                       flux_lines, omegas, design, fc, waveform, dt, dx, dtype,
                                                       pml_cells, orders_line)
        self._orders_line = None if orders_line is None else int(orders_line)
        self._open(p, dtype, engine, device)
        if p.sigma is not None:
            self._sigma = p.sigma.copy()

    _check_engine = staticmethod(_refuse_bloch_flux_pole)

    def _setup_engine(self, eng):
        p = self._p
        _bloch_setup(eng, p, p.sigma, self._phi, self._weights)
        _bloch_flux_lines_setup(eng, p)

    def value_and_grad(self, objective):
        """(J (B,), grad_eps (B, nrows, ncols) float64, P (B, N, F) float64, info) of the current materials and phases."""
        p, eng = self._p, self._eng
        if eng is None:
            raise RuntimeError("the session is closed")
        self._check_engine(eng)
        none = np.empty((p.B, 0))
        eng.reset()
        eng.run(p.nsteps, p.amps)
        _, peak_fwd = self._spectra(eng, none)
        end_fwd = self._absmax(eng)
        self._hold(eng)
        P = eng.flux()
        k = self._orders_line
        J, g, gm = _bloch_flux_cotangent(p, objective, P, None if k is None else eng.flux_orders(k))
        if gm is None:
            eng.bloch_flux_adjoint_sources(g, p.solve[0] if p.shared else p.solve, p.scale_e, p.scale_h)
        else:
            E, H = eng.read_flux_lines(raw=True)
            eng.set_bloch_flux_line_sources(*bloch_flux_adjoint_weights(E, H, g, p.lines, p.om, p.dt, p.dx, p.solve,
                                                                        p.scale_e, p.scale_h, (k, gm, self._phi)))
        eng.reset()
        eng.run_bloch_channels(p.nsteps, None, p.channels, conjugate=True)
        _, peak_adj = self._spectra(eng, none)
        end_adj = self._absmax(eng)
        grad = self._product(eng, p.coef) * (p.dx / p.dt)
        self._ran = True
        info = {"condition": self._condition, "residual_forward": _residual(end_fwd, peak_fwd),
                "residual_adjoint": _residual(end_adj, peak_adj), "channels_shared": p.shared}
        return J, grad, P, info
