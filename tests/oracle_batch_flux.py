"""Flux lines for the stand-ins of the lossy, periodic and dispersive batches, restating in NumPy the definitions that
include/fdtd2d_batch_flux.h fixes.  A mixin: it runs the class it is mixed into one step at a time and, after the source
of every sampled step n (every `every`-th step counted from set_flux_lines), adds in float64 on every line cell

    E_k += Ez * exp(-1j * omega_k * n * dt)          Ez as stored, widened to double
    H_k += Ht * exp(-1j * omega_k * n * dt)          the same phasor

with the tangential H of the step's H half-step centred on the cell:

    row line    ("row", i, c0, nc), power towards increasing row:       Ht = 0.5 * (Hx[i-1, j] + Hx[i, j])
    column line ("col", j, r0, nr), power towards increasing column:    Ht = 0.5 * (Hy[i, j-1] + Hy[i, j])

(a periodic member's column 0 has column C-2 as its left neighbour; the slots Hx[:, C-1] and Hy[R-1, :], which no update
writes, read as zero).  That H lives at (n - 1/2) dt, so read_flux_lines() multiplies H_k by exp(+1j * omega_k * dt / 2)
unless raw, and flux() forms, per member, line and frequency,

    P = s * dx * sum over the line's cells of Re(E_k * conj(H_k * exp(+1j * omega_k * dt / 2)))

with s = +1 for a row line and -1 for a column line (S_y = Ez Hx, S_x = -Ez Hy: columns are x, rows are y).  No factor
1/2 and no normalisation.  No device, no library."""
import numpy as np

from oracle_batch_dispersive import DispersivePeriodicOracle, DispersivePmlOracle
from oracle_batch_lossy import LossyOracle
from oracle_batch_periodic import PeriodicOracle

MAX_LINES, MAX_FREQS = 4, 16


class FluxLines:
    fluxmon = None

    def set_flux_lines(self, lines, omegas, every=1):
        if lines is None or len(lines) == 0:
            self.fluxmon = None
            return self
        periodic = self.boundary == "periodic"
        R, C = self.rows, self.cols
        assert self.boundary in ("pml", "periodic") and 1 <= len(lines) <= MAX_LINES and every >= 1
        w = np.asarray(omegas, dtype=np.float64)
        w = np.ascontiguousarray(np.broadcast_to(w, (self.count, w.shape[-1])))
        assert 1 <= w.shape[1] <= MAX_FREQS
        rows, cols, colline = [], [], []
        for kind, at, first, n in lines:
            assert kind in ("row", "col") and n >= 1 and first >= 0
            if kind == "row":
                assert 1 <= at <= R - 2 and first + n <= (C - 1 if periodic else C)
                rows.append(np.full(n, at))
                cols.append(np.arange(first, first + n))
            else:
                assert (0 if periodic else 1) <= at <= C - 2 and first + n <= R
                rows.append(np.arange(first, first + n))
                cols.append(np.full(n, at))
            colline.append(np.full(n, kind == "col"))
        cells = sum(len(r) for r in rows)
        z = np.zeros((self.count, w.shape[1], cells), np.complex128)
        self.fluxmon = dict(lines=[tuple(l) for l in lines], omega=w, every=int(every), step0=self.step,
                            i=np.concatenate(rows), j=np.concatenate(cols), col=np.concatenate(colline),
                            E=z, H=z.copy())
        return self

    def reset(self):
        super().reset()
        f = getattr(self, "fluxmon", None)
        if f is not None:
            f["E"][...] = 0
            f["H"][...] = 0
            f["step0"] = 0
        return self

    def _tangential_h(self, b):
        """Ht on every line cell of member b, float64."""
        f, R, C = self.fluxmon, self.rows, self.cols
        hx = np.zeros((R, C))
        hx[:, :C - 1] = self.Hx[b]
        hy = np.zeros((R, C))
        hy[:R - 1, :] = self.Hy[b]
        i, j = f["i"], f["j"]
        left = np.where(j == 0, C - 2, j - 1)          # column 0 lies on a line of a periodic member alone
        return np.where(f["col"], 0.5 * (hy[i, left] + hy[i, j]), 0.5 * (hx[np.maximum(i - 1, 0), j] + hx[i, j]))

    def _run_member(self, b, nsteps, amps, sums):
        f = self.fluxmon
        if f is None:
            return super()._run_member(b, nsteps, amps, sums)
        base = self.step
        try:
            for n in range(nsteps):
                self.step = base + n
                super()._run_member(b, 1, None if amps is None else amps[n:n + 1],
                                    None if sums is None else sums[:, n:n + 1])
                s = base + n + 1
                if (s - f["step0"]) % f["every"] == 0:
                    t = float(s) * self.dt
                    ph = np.cos(f["omega"][b] * t) + 1j * (-np.sin(f["omega"][b] * t))
                    e = self.Ez[b][f["i"], f["j"]].astype(np.float64)
                    f["E"][b] += e[None, :] * ph[:, None]
                    f["H"][b] += self._tangential_h(b)[None, :] * ph[:, None]
        finally:
            self.step = base

    def read_flux_lines(self, raw=False):
        f = self.fluxmon
        half = 1.0 if raw else np.exp(0.5j * f["omega"] * self.dt)[:, :, None]
        return f["E"].copy(), f["H"] * half

    def flux(self):
        f = self.fluxmon
        E, H = self.read_flux_lines()
        out = np.empty((self.count, len(f["lines"]), f["omega"].shape[1]))
        o = 0
        for k, (kind, _, _, n) in enumerate(f["lines"]):
            s = 1.0 if kind == "row" else -1.0
            out[:, k, :] = s * self.dx * np.real(E[:, :, o:o + n] * np.conj(H[:, :, o:o + n])).sum(axis=2)
            o += n
        return out

    def flux_scale(self):
        """dx * sum |E_k| |H_k| per member, line and frequency: what the flux's rounding error is measured against."""
        f = self.fluxmon
        E, H = self.read_flux_lines()
        out = np.empty((self.count, len(f["lines"]), f["omega"].shape[1]))
        o = 0
        for k, (_, _, _, n) in enumerate(f["lines"]):
            out[:, k, :] = self.dx * (np.abs(E[:, :, o:o + n]) * np.abs(H[:, :, o:o + n])).sum(axis=2)
            o += n
        return out


class FluxLossyOracle(FluxLines, LossyOracle):
    pass


class FluxPeriodicOracle(FluxLines, PeriodicOracle):
    pass


class FluxDispersivePmlOracle(FluxLines, DispersivePmlOracle):
    pass


class FluxDispersivePeriodicOracle(FluxLines, DispersivePeriodicOracle):
    pass


def flux_oracle_for(boundary, dispersive=False):
    if dispersive:
        return FluxDispersivePeriodicOracle if boundary == "periodic" else FluxDispersivePmlOracle
    return FluxPeriodicOracle if boundary == "periodic" else FluxLossyOracle
