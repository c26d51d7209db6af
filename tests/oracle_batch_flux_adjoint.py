"""Line sources for the stand-ins of tests/oracle_batch_flux.py, restating in NumPy what
include/fdtd2d_batch_flux_adjoint.h fixes.  Two mixins around FluxLines: `LineSources` (the calls) above it and
`_LineSourceStep` (the step) below it, so that the lines' own sums see the step's injection.

Entries are the lines' cells concatenated in the order given (a cell on two lines has two entries); we, wh are
(B, cells, K).  In step n of run(nsteps, amps, channels), per member and entry w, in float64 with one rounding per
operation:

    s_e(w) = 0.0;  for c ascending:  s_e = s_e + we[w, c] * channels[c, n]          s_h(w) likewise with wh

H part, BEFORE the H update of step n.  Every H value the update writes (Hx[i, j], Hy[i, j] with i <= R-2, j <= C-2)
gathers a = 0.0; for line k ascending: the own cell (i, j) on line k adds 0.5 * s_h(entry), then the neighbour cell on line
k adds 0.5 * s_h(entry); Hx counts row lines and its neighbour cell is (i+1, j), Hy counts column lines and its neighbour
cell is (i, j+1), (i, 0) for j = C-2 of a periodic member.  An H value with at least one term becomes
H = (T)((double)H + a).  Values that no update writes take nothing.

E part, after the E half-step, the rectangle source and the point sources of step n: a cell on at least one line takes
a = 0.0; for line k ascending that holds it: a = a + s_e(entry); Ez = (T)((double)Ez + a); a periodic member's image column
repeats column 0.  The window DFT, the probes and the lines' sums sample afterwards.

flux_adjoint_sources restates fdtd2d_batch_flux_line_weights.  No device, no library."""
import numpy as np

from oracle_batch import point_sums
from oracle_batch_dispersive import DispersivePeriodicOracle, DispersivePmlOracle
from oracle_batch_flux import FluxLines
from oracle_batch_lossy import LossyOracle
from oracle_batch_periodic import PeriodicOracle

MAX_CHANNELS = 32


class _LineSourceStep:
    """Below FluxLines in the method resolution order: one step of the class underneath with the injection."""
    linesrc = None
    _line_run = None           # (channels of the run, the step count at its start)

    def _h_terms(self, hy):
        """[(i, j, [entry, ...])] for every H value of one kind that takes an H part, the entries in the order of the
        additions: lines ascending, own cell before neighbour cell."""
        f, R, C = self.fluxmon, self.rows, self.cols
        periodic = self.boundary == "periodic"
        terms = {}
        o = 0
        for k, (kind, at, first, n) in enumerate(f["lines"]):
            if (kind == "col") == hy:
                for c in range(n):
                    i, j = (first + c, at) if hy else (at, first + c)
                    # the two H values the monitor averages for this cell: (i, j), whose own cell it is (rank 0), and
                    # the one before it, whose neighbour cell it is (rank 1)
                    before = (i, (C - 2 if periodic and j == 0 else j - 1)) if hy else (i - 1, j)
                    for slot, rank in (((i, j), 0), (before, 1)):
                        if 0 <= slot[0] <= R - 2 and 0 <= slot[1] <= C - 2:      # a value the update writes
                            terms.setdefault(slot, []).append((k, rank, o + c))
            o += n
        return [(i, j, [e for _, _, e in sorted(t)]) for (i, j), t in terms.items()]

    def _run_member(self, b, nsteps, amps, sums):
        src, run = self.linesrc, self._line_run
        if src is None or run is None or self.fluxmon is None:
            return super()._run_member(b, nsteps, amps, sums)
        f, T = self.fluxmon, self.dtype
        chan, start = run
        chan = chan[b] if chan.ndim == 3 else chan
        we, wh = src
        hx_terms = self._h_terms(False) if wh is not None else []
        hy_terms = self._h_terms(True) if wh is not None else []
        periodic = self.boundary == "periodic"
        base = self.step
        try:
            for n in range(nsteps):
                self.step = base + n
                k = self.step - start                                  # the run's step
                if wh is not None:
                    sh = point_sums(wh[b], chan[:, k:k + 1])[:, 0]
                    for H, terms in ((self.Hx[b], hx_terms), (self.Hy[b], hy_terms)):
                        for i, j, entries in terms:
                            a = 0.0
                            for e in entries:
                                a = a + 0.5 * sh[e]
                            H[i, j] = T.type(np.float64(H[i, j]) + a)
                win, probes = self.win, self.probes
                self.win = self.probes = None                          # they sample after the E part
                try:
                    super()._run_member(b, 1, None if amps is None else amps[n:n + 1],
                                        None if sums is None else sums[:, n:n + 1])
                finally:
                    self.win, self.probes = win, probes
                Ez = self.Ez[b]
                if we is not None:
                    se = point_sums(we[b], chan[:, k:k + 1])[:, 0]
                    total = {}
                    for e, (i, j) in enumerate(zip(f["i"], f["j"])):   # entries ascend with the lines
                        total[int(i), int(j)] = total.get((int(i), int(j)), 0.0) + se[e]
                    for (i, j), a in total.items():
                        Ez[i, j] = T.type(np.float64(Ez[i, j]) + a)
                    if periodic:
                        Ez[:, -1] = Ez[:, 0]
                s = base + n + 1
                if win is not None and (s - win["step0"]) % win["every"] == 0:
                    r0, c0, wr, wc = win["win"]
                    e = Ez[r0:r0 + wr, c0:c0 + wc].astype(np.float64)
                    t = float(s) * self.dt
                    win["re"][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                    win["im"][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
                if probes is not None:
                    kk = s - 1 - probes["step0"]
                    if 0 <= kk < probes["trace"].shape[2]:
                        cells = probes["cells"][b]
                        probes["trace"][b, :, kk] = Ez[cells[:, 0], cells[:, 1]]
        finally:
            self.step = base


class LineSources:
    """Above FluxLines: the calls of BatchEngine that concern line sources."""

    def set_flux_lines(self, lines, omegas, every=1):
        self.linesrc = None                         # line sources belong to the lines they were set on
        return super().set_flux_lines(lines, omegas, every)

    def set_flux_line_sources(self, we, wh):
        if we is None and wh is None:
            self.linesrc = None
            return self
        assert self.fluxmon is not None, "line sources live on flux lines"
        cells = len(self.fluxmon["i"])
        parts = []
        for w in (we, wh):
            if w is not None:
                w = np.asarray(w, dtype=np.float64)
                w = np.ascontiguousarray(np.broadcast_to(w, (self.count,) + w.shape[-2:]))
                assert w.shape[:2] == (self.count, cells) and 1 <= w.shape[2] <= MAX_CHANNELS and np.all(np.isfinite(w))
            parts.append(w)
        K = {w.shape[2] for w in parts if w is not None}
        assert len(K) == 1 and (self.points is None or self.points[1].shape[2] in K)
        self.linesrc = tuple(parts)
        return self

    def read_flux_line_sources(self):
        cells = len(self.fluxmon["i"])
        K = next(w.shape[2] for w in self.linesrc if w is not None)
        return tuple(np.zeros((self.count, cells, K)) if w is None else w.copy() for w in self.linesrc)

    def run(self, nsteps, amps=None, channels=None):
        if channels is None or self.linesrc is None:
            return super().run(nsteps, amps, channels)
        self._line_run = (np.asarray(channels, dtype=np.float64), self.step)
        try:
            return super().run(nsteps, amps, channels if self.points is not None else None)
        finally:
            self._line_run = None

    def flux_adjoint_sources(self, dJdP, solve, scale_e=None, scale_h=None):
        """fdtd2d_batch_flux_line_weights: te = scale_e c conj(H g), th = scale_h c conj(E g) with c = dJdP s dx per
        line and g = exp(+i omega dt / 2); weights = solve @ [Re target; Im target]."""
        f = self.fluxmon
        E, H = self.read_flux_lines()                 # H with the half-step factor g
        g = np.exp(0.5j * f["omega"] * self.dt)[:, :, None]
        B, F, cells = E.shape
        dJdP = np.asarray(dJdP, dtype=np.float64)
        solve = np.broadcast_to(np.asarray(solve, dtype=np.float64), (B, 2 * F, 2 * F))
        c = np.empty((B, F, cells))
        o = 0
        for k, (kind, _, _, n) in enumerate(f["lines"]):
            c[:, :, o:o + n] = (dJdP[:, k, :] * ((1.0 if kind == "row" else -1.0) * self.dx))[:, :, None]
            o += n
        one = np.ones((B, cells))
        te = (one if scale_e is None else np.asarray(scale_e))[:, None, :] * c * np.conj(H)
        th = (one if scale_h is None else np.asarray(scale_h))[:, None, :] * c * np.conj(E * g)
        out = []
        for t in (te, th):
            rhs = np.concatenate([t.real, t.imag], axis=1)            # (B, 2F, cells)
            out.append(np.ascontiguousarray(np.einsum("bck,bkw->bwc", solve, rhs)))
        return self.set_flux_line_sources(*out)


class LineSourceLossyOracle(LineSources, FluxLines, _LineSourceStep, LossyOracle):
    pass


class LineSourcePeriodicOracle(LineSources, FluxLines, _LineSourceStep, PeriodicOracle):
    pass


class LineSourceDispersivePmlOracle(LineSources, FluxLines, _LineSourceStep, DispersivePmlOracle):
    pass


class LineSourceDispersivePeriodicOracle(LineSources, FluxLines, _LineSourceStep, DispersivePeriodicOracle):
    pass


def line_source_oracle_for(boundary, dispersive=False):
    if dispersive:
        return LineSourceDispersivePeriodicOracle if boundary == "periodic" else LineSourceDispersivePmlOracle
    return LineSourcePeriodicOracle if boundary == "periodic" else LineSourceLossyOracle
