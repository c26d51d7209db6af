"""Line sources on the flux lines of the Bloch stand-ins, restating in NumPy what
include/fdtd2d_batch_bloch_flux_adjoint.h fixes.  Two mixins around oracle_batch_bloch_flux.BlochFluxLines, as in
oracle_batch_flux_adjoint.py: `BlochLineSources` (the calls) above it and `_BlochLineSourceStep` (the step) below it, so
that the lines' own sums see the step's injection.  The class underneath is BlochDispersiveOracle: the Bloch adjoint
stand-in, with the pole once set_bloch_dispersion is called.

Entries are the lines' cells concatenated in the order given.  The weights are complex, kept as four float64 arrays
(we_re, we_im, wh_re, wh_im), each (B, cells, K) or None: a real array given to set_bloch_flux_line_sources leaves its
imaginary part absent.  In step n of run_bloch_channels(nsteps, amps, channels, conjugate), per member, entry w and
array, in float64 with one rounding per operation:

    s(w) = 0.0;  for c ascending:  s = s + weights[w, c] * channels[c, n]          (0.0 for an absent array)

H part, BEFORE the H update of step n, while wh_re or wh_im is present.  Every H value the update writes gathers
a = (0.0, 0.0); lines of its orientation ascending, own cell before neighbour cell: t = (0.5 * s_h_re, 0.5 * s_h_im); the
neighbour term of Hy[i, C-2] (its neighbour cell is column 0, across the seam) is rotated by the rotation (c, s) the run
steps with, widened from the batch dtype, (c, -s) in a conjugated run: t = (c*tr - s*ti, c*ti + s*tr); a = a + t per part.
Then H_re = (T)((double)H_re + a_re) and H_im likewise.

E part, after the E half-step and the rectangle source: a cell on at least one line takes, per part whose array is
present, a = 0.0; lines ascending: a = a + s_e(entry); Ez_part = (T)((double)Ez_part + a).  The image column is
refreshed (here it is stored rotated; the device keeps the unrotated copy and rotates when it reads).  The window DFT,
the probes and the lines' sums sample afterwards.  The lines' seam read uses the run's rotation, like the step.

Three refusals of the stand-ins underneath are overridden: run_bloch_channels and hold_bloch_window beside Bloch lines
(accepted once line sources are installed) and run_bloch_channels with the pole (accepted when it drives line sources).
bloch_flux_adjoint_sources restates fdtd2d_batch_bloch_flux_line_weights.  No device, no library."""
import numpy as np

from oracle_batch import point_sums
from oracle_batch_bloch import rotate
from oracle_batch_bloch_adjoint import BlochAdjointOracle
from oracle_batch_bloch_dispersive import BlochDispersiveOracle
from oracle_batch_bloch_flux import BlochFluxLines

MAX_CHANNELS = 32


class _BlochLineSourceStep:
    """Below BlochFluxLines in the method resolution order: one step of the class underneath with the injection."""
    blinesrc = None            # (we_re, we_im, wh_re, wh_im)
    _bline_run = None          # (channels of the run, the step count at its start)
    drop_seam_rotation = False     # tests alone: the mutant that leaves the seam term unrotated

    def _bh_terms(self, hy):
        """[(i, j, [(entry, rotated), ...])] for every H value of one kind that takes an H part, the terms in the order
        of the additions: lines ascending, own cell before neighbour cell."""
        f, R, C = self.bfluxmon, self.rows, self.cols
        terms = {}
        o = 0
        for k, (kind, at, first, n) in enumerate(f["lines"]):
            if (kind == "col") == hy:
                for c in range(n):
                    i, j = (first + c, at) if hy else (at, first + c)
                    before = (i, (C - 2 if j == 0 else j - 1)) if hy else (i - 1, j)
                    for slot, rank in (((i, j), 0), (before, 1)):
                        if 0 <= slot[0] <= R - 2 and 0 <= slot[1] <= C - 2:      # a value the update writes
                            terms.setdefault(slot, []).append((k, rank, o + c, bool(hy and rank and j == 0)))
            o += n
        return [(i, j, [(e, rot) for _, _, e, rot in sorted(t)]) for (i, j), t in terms.items()]

    def _run_bloch_member(self, b, nsteps, amps):
        src, run = self.blinesrc, self._bline_run
        if src is None or run is None or self.bfluxmon is None:
            return super()._run_bloch_member(b, nsteps, amps)
        f, T = self.bfluxmon, self.dtype.type
        chan, start = run
        chan = chan[b] if chan.ndim == 3 else chan
        we_re, we_im, wh_re, wh_im = src
        have_h = wh_re is not None or wh_im is not None
        hx_terms = self._bh_terms(False) if have_h else []
        hy_terms = self._bh_terms(True) if have_h else []
        rc, rs = np.float64(T(self.rho[0][b])), np.float64(T(self.rho[1][b]))
        zero = np.zeros(len(f["i"]))
        base = self.step
        try:
            for n in range(nsteps):
                self.step = base + n
                k = self.step - start                                  # the run's step
                col = chan[:, k:k + 1]
                if have_h:
                    sr = zero if wh_re is None else point_sums(wh_re[b], col)[:, 0]
                    si = zero if wh_im is None else point_sums(wh_im[b], col)[:, 0]
                    for Hr, Hi, terms in ((self.Hx[b], self.Hx_i[b], hx_terms), (self.Hy[b], self.Hy_i[b], hy_terms)):
                        for i, j, entries in terms:
                            ar = ai = 0.0
                            for e, rot in entries:
                                tr, ti = 0.5 * sr[e], 0.5 * si[e]
                                if rot and not self.drop_seam_rotation:
                                    tr, ti = rc * tr - rs * ti, rc * ti + rs * tr
                                ar = ar + tr
                                ai = ai + ti
                            Hr[i, j] = T(np.float64(Hr[i, j]) + ar)
                            Hi[i, j] = T(np.float64(Hi[i, j]) + ai)
                win, probes = self.win, self.probes
                self.win = self.probes = None                          # they sample after the E part
                try:
                    super()._run_bloch_member(b, 1, None if amps is None else amps[n:n + 1])
                finally:
                    self.win, self.probes = win, probes
                Er, Ei = self.Ez[b], self.Ez_i[b]
                for Ez, w in ((Er, we_re), (Ei, we_im)):
                    if w is None:
                        continue
                    se = point_sums(w[b], col)[:, 0]
                    total = {}
                    for e, (i, j) in enumerate(zip(f["i"], f["j"])):   # entries ascend with the lines
                        total[int(i), int(j)] = total.get((int(i), int(j)), 0.0) + se[e]
                    for (i, j), a in total.items():
                        Ez[i, j] = T(np.float64(Ez[i, j]) + a)
                Er[:, -1], Ei[:, -1] = rotate(T(self.rho[0][b]), T(self.rho[1][b]), Er[:, 0], Ei[:, 0])
                s = base + n + 1
                if win is not None and (s - win["step0"]) % win["every"] == 0:
                    r0, c0, wr, wc = win["win"]
                    t = float(s) * self.dt
                    for Ez, kr, ki in ((Er, "re", "im"), (Ei, "re_i", "im_i")):
                        e = Ez[r0:r0 + wr, c0:c0 + wc].astype(np.float64)
                        win[kr][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                        win[ki][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
                if probes is not None:
                    kk = s - 1 - probes["step0"]
                    if 0 <= kk < probes["trace"].shape[2]:
                        cells = probes["cells"][b]
                        probes["trace"][b, :, kk] = Er[cells[:, 0], cells[:, 1]]
                        probes["trace_i"][b, :, kk] = Ei[cells[:, 0], cells[:, 1]]
        finally:
            self.step = base


class BlochLineSources:
    """Above BlochFluxLines: the calls of BatchEngine that concern line sources on Bloch lines."""

    def set_bloch_flux_lines(self, lines, omegas, every=1):
        self.blinesrc = None                        # line sources belong to the lines they were set on
        return super().set_bloch_flux_lines(lines, omegas, every)

    def set_flux_line_sources(self, we, wh):
        raise AssertionError("line sources of this kind live on the lines of set_flux_lines, not on a Bloch batch")

    def set_bloch_flux_line_sources(self, we, wh):
        if we is None and wh is None:
            self.blinesrc = None
            return self
        assert self.bfluxmon is not None, "Bloch line sources live on Bloch flux lines"
        cells = len(self.bfluxmon["i"])
        parts = []
        for w in (we, wh):
            if w is None:
                parts += [None, None]
                continue
            w = np.asarray(w)
            cplx = np.iscomplexobj(w)
            w = np.broadcast_to(w, (self.count,) + w.shape[-2:])
            assert w.shape[:2] == (self.count, cells) and 1 <= w.shape[2] <= MAX_CHANNELS
            assert np.all(np.isfinite(w))
            parts.append(np.ascontiguousarray(w.real, dtype=np.float64))
            parts.append(np.ascontiguousarray(w.imag, dtype=np.float64) if cplx else None)
        assert len({w.shape[2] for w in parts if w is not None}) == 1
        self.blinesrc = tuple(parts)
        return self

    def read_bloch_flux_line_sources(self):
        assert self.blinesrc is not None, "no line sources are set"
        shape = next(w.shape for w in self.blinesrc if w is not None)
        a = [np.zeros(shape) if w is None else w for w in self.blinesrc]
        return a[0] + 1j * a[1], a[2] + 1j * a[3]

    def line_source_channels(self):
        return 0 if self.blinesrc is None else next(w.shape[2] for w in self.blinesrc if w is not None)

    # -- the refusals that line sources lift ---------------------------------------------------------------------------
    def run(self, nsteps, amps=None, channels=None):
        if self.rho is not None and self.conj_last and self.dispersive:
            self._pole_images()                           # with the images of Ez that BlochAdjointOracle.run refreshes
        return super().run(nsteps, amps, channels)

    def run_bloch_channels(self, nsteps, amps=None, channels=None, conjugate=False):
        if self.bfluxmon is None:                         # no lines: the Bloch adjoint stand-in's own rules
            return BlochDispersiveOracle.run_bloch_channels(self, nsteps, amps, channels, conjugate)
        assert self.blinesrc is not None, "a run with channels is not available while the lines are set"
        ch = np.asarray(channels, dtype=np.float64)
        assert ch.shape[-2] == self.line_source_channels() and ch.shape[-1] >= nsteps
        a = None if amps is None else np.asarray(amps, dtype=np.complex128)
        rho = self.rho
        if conjugate:
            self.rho = (rho[0], (-rho[1]).astype(self.dtype))
        self._images()                                    # this run's rotation from its first step on
        if self.dispersive:
            self._pole_images()
        self._bline_run = (ch, self.step)
        try:
            for b in range(self.count):
                self._run_bloch_member(b, nsteps, None if a is None else a[b])
        finally:
            self.rho = rho
            self._bline_run = None
        self.step += nsteps
        self.conj_last = bool(conjugate)
        return self

    def hold_bloch_window(self):
        assert self.bfluxmon is None or self.blinesrc is not None, \
            "the held window is not available while the lines are set"
        return BlochDispersiveOracle.hold_bloch_window(self)      # which keeps refusing the pole

    # -- the weights ---------------------------------------------------------------------------------------------------
    def bloch_flux_adjoint_sources(self, dJdP, solve, scale_e=None, scale_h=None):
        """fdtd2d_batch_bloch_flux_line_weights: with X the raw sum of the complex field, x = X g, cf = scale * (dJdP *
        (sign * dx)): tr = cf * xr, ti = -(cf * xi); weight[c] = sum_k solve[c, k] * tr_k, then + sum_k solve[c, F + k] *
        ti_k, k ascending from 0.0.  we reads H, wh reads E; the weights are real."""
        f = self.bfluxmon
        E, H = self.read_flux_lines(raw=True)
        B, F, cells = E.shape
        dJdP = np.asarray(dJdP, dtype=np.float64)
        solve = np.broadcast_to(np.asarray(solve, dtype=np.float64), (B, 2 * F, 2 * F))
        half = f["omega"] * self.dt * 0.5
        gc, gs = np.cos(half)[:, :, None], np.sin(half)[:, :, None]
        cf = np.empty((B, F, cells))
        o = 0
        for k, (kind, _, _, n) in enumerate(f["lines"]):
            cf[:, :, o:o + n] = (dJdP[:, k, :] * ((1.0 if kind == "row" else -1.0) * self.dx))[:, :, None]
            o += n
        out = []
        for X, scale in ((H, scale_e), (E, scale_h)):
            sc = np.ones((B, cells)) if scale is None else np.asarray(scale, dtype=np.float64)
            xr, xi = X.real * gc - X.imag * gs, X.real * gs + X.imag * gc
            c = sc[:, None, :] * cf
            tr, ti = c * xr, -(c * xi)
            w = np.zeros((B, cells, 2 * F))
            for k in range(F):
                w = w + solve[:, None, :, k] * tr[:, k, :, None]
            for k in range(F):
                w = w + solve[:, None, :, F + k] * ti[:, k, :, None]
            out.append(w)
        return self.set_bloch_flux_line_sources(*out)


class BlochLineSourceOracle(BlochLineSources, BlochFluxLines, _BlochLineSourceStep, BlochDispersiveOracle):
    """A periodic batch with a Bloch phase, the lines and their sources; with the pole after set_bloch_dispersion."""


assert issubclass(BlochLineSourceOracle, BlochAdjointOracle)
