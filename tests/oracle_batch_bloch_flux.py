"""Flux lines for the stand-ins of the Bloch batches (with and without the pole), restating in NumPy the definitions that
include/fdtd2d_batch_bloch_flux.h fixes.  A mixin in the style of oracle_batch_flux.FluxLines: it runs the class it is
mixed into one step at a time and, after the source of every sampled step n (every `every`-th step counted from
set_bloch_flux_lines), adds in float64 on every line cell, for the real part and for the imaginary part of the fields,

    E_k += Ez * exp(-1j * omega_k * n * dt)          Ez of that part as stored, widened to double
    H_k += Ht * exp(-1j * omega_k * n * dt)          the same phasor

with the tangential H of the step's H half-step centred on the cell, on each part:

    row line    ("row", i, c0, nc), power towards increasing row:       Ht = 0.5 * (Hx[i-1, j] + Hx[i, j])
    column line ("col", j, r0, nr), power towards increasing column:    Ht = 0.5 * (Hy[i, j-1] + Hy[i, j])

Column 0's left neighbour lies across the seam: it is conj(rho) * Hy[i, C-2], `unrotate` in the batch dtype (what the E
half-step itself subtracts), then widened; rows 0 and R-1 evaluate it the same way.  The slot Hy[R-1, :], which no update
writes, reads as zero.  The spectra of the complex fields are E_k = Er_k + 1j * Ei_k and H_k likewise;
read_flux_lines() multiplies H_k by exp(+1j * omega_k * dt / 2) unless raw, and flux() forms

    P = s * dx * sum over the line's cells of Re(E_k * conj(H_k * exp(+1j * omega_k * dt / 2)))

with s = +1 for a row line and -1 for a column line.  flux_orders(line) splits P of a whole-period row line over the
diffraction orders.  No device, no library."""
import numpy as np

from oracle_batch_bloch import BlochOracle, unrotate
from oracle_batch_bloch_dispersive import BlochDispersiveOracle
from oracle_batch_flux import MAX_FREQS, MAX_LINES


class BlochFluxLines:
    bfluxmon = None

    def set_bloch_flux_lines(self, lines, omegas, every=1):
        if lines is None or len(lines) == 0:
            self.bfluxmon = None
            return self
        R, C = self.rows, self.cols
        assert self.boundary == "periodic" and self.rho is not None, "Bloch flux lines need a Bloch phase"
        assert getattr(self, "bpoints", None) is None and getattr(self, "held_b", None) is None, \
            "Bloch point sources and the held window exclude the lines"
        assert 1 <= len(lines) <= MAX_LINES and every >= 1
        w = np.asarray(omegas, dtype=np.float64)
        w = np.ascontiguousarray(np.broadcast_to(w, (self.count, w.shape[-1])))
        assert 1 <= w.shape[1] <= MAX_FREQS
        rows, cols, colline = [], [], []
        for kind, at, first, n in lines:
            assert kind in ("row", "col") and n >= 1 and first >= 0
            if kind == "row":
                assert 1 <= at <= R - 2 and first + n <= C - 1
                rows.append(np.full(n, at))
                cols.append(np.arange(first, first + n))
            else:
                assert 0 <= at <= C - 2 and first + n <= R
                rows.append(np.arange(first, first + n))
                cols.append(np.full(n, at))
            colline.append(np.full(n, kind == "col"))
        cells = sum(len(r) for r in rows)
        z = np.zeros((self.count, w.shape[1], cells), np.complex128)
        self.bfluxmon = dict(lines=[tuple(l) for l in lines], omega=w, every=int(every), step0=self.step,
                             i=np.concatenate(rows), j=np.concatenate(cols), col=np.concatenate(colline),
                             E=(z, z.copy()), H=(z.copy(), z.copy()))     # (real part's, imaginary part's)
        return self

    # -- what the lines exclude while they are set ----------------------------------------------------------------------
    def set_bloch_phase(self, phi, rotation=None):
        assert self.bfluxmon is None or phi is not None or rotation is not None, "the lines need the phase"
        return super().set_bloch_phase(phi, rotation)

    def set_bloch_point_sources(self, cells, weights=None):
        assert cells is None or self.bfluxmon is None, "a Bloch point source is not available while the lines are set"
        return super().set_bloch_point_sources(cells, weights)

    def run_bloch_channels(self, *a, **k):
        assert self.bfluxmon is None, "a run with channels is not available while the lines are set"
        return super().run_bloch_channels(*a, **k)

    def hold_bloch_window(self):
        assert self.bfluxmon is None, "the held window is not available while the lines are set"
        return super().hold_bloch_window()

    def reset(self):
        super().reset()
        f = self.bfluxmon
        if f is not None:
            for a in f["E"] + f["H"]:
                a[...] = 0
            f["step0"] = 0
        return self

    # -- the sums ---------------------------------------------------------------------------------------------------------
    def _tangential_h(self, b):
        """(Ht of the real part, Ht of the imaginary part) on every line cell of member b, float64."""
        f, R, C, T = self.bfluxmon, self.rows, self.cols, self.dtype.type
        i, j = f["i"], f["j"]
        hy = [np.zeros((R, C), self.dtype), np.zeros((R, C), self.dtype)]
        hy[0][:R - 1, :], hy[1][:R - 1, :] = self.Hy[b], self.Hy_i[b]
        left = [h[i, np.maximum(j - 1, 0)] for h in hy]
        seam = unrotate(T(self.rho[0][b]), T(self.rho[1][b]), hy[0][i, C - 2], hy[1][i, C - 2])     # in the batch dtype
        out = []
        for hx, h, lw, sw in zip((self.Hx[b], self.Hx_i[b]), hy, left, seam):
            lw = np.where(j == 0, sw, lw).astype(np.float64)
            up = hx[np.maximum(i - 1, 0), np.minimum(j, C - 2)].astype(np.float64)
            own = hx[i, np.minimum(j, C - 2)].astype(np.float64)
            out.append(np.where(f["col"], 0.5 * (lw + h[i, j].astype(np.float64)), 0.5 * (up + own)))
        return out

    def _run_bloch_member(self, b, nsteps, amps):
        f = self.bfluxmon
        if f is None:
            return super()._run_bloch_member(b, nsteps, amps)
        base = self.step
        try:
            for n in range(nsteps):
                self.step = base + n
                super()._run_bloch_member(b, 1, None if amps is None else amps[n:n + 1])
                s = base + n + 1
                if (s - f["step0"]) % f["every"] == 0:
                    t = float(s) * self.dt
                    ph = np.cos(f["omega"][b] * t) + 1j * (-np.sin(f["omega"][b] * t))
                    for part, Ez, ht in zip((0, 1), (self.Ez[b], self.Ez_i[b]), self._tangential_h(b)):
                        e = Ez[f["i"], f["j"]].astype(np.float64)
                        f["E"][part][b] += e[None, :] * ph[:, None]
                        f["H"][part][b] += ht[None, :] * ph[:, None]
        finally:
            self.step = base

    # -- reading -------------------------------------------------------------------------------------------------------------
    def read_bloch_flux_parts(self):
        f = self.bfluxmon
        return tuple((f["E"][k].copy(), f["H"][k].copy()) for k in (0, 1))

    def read_flux_lines(self, raw=False):
        f = self.bfluxmon
        half = 1.0 if raw else np.exp(0.5j * f["omega"] * self.dt)[:, :, None]
        return f["E"][0] + 1j * f["E"][1], (f["H"][0] + 1j * f["H"][1]) * half

    def _per_line(self, term):
        f = self.bfluxmon
        out = np.empty((self.count, len(f["lines"]), f["omega"].shape[1]))
        o = 0
        for k, (kind, _, _, n) in enumerate(f["lines"]):
            out[:, k, :] = (1.0 if kind == "row" else -1.0) * self.dx * term(slice(o, o + n)).sum(axis=2)
            o += n
        return out

    def flux(self):
        E, H = self.read_flux_lines()
        return self._per_line(lambda c: np.real(E[:, :, c] * np.conj(H[:, :, c])))

    def flux_scale(self):
        """dx * sum (|Er_k| + |Ei_k|) (|Hr_k| + |Hi_k|) per member, line and frequency: what the flux's rounding error
        is measured against."""
        f = self.bfluxmon
        e = np.abs(f["E"][0]) + np.abs(f["E"][1])
        h = np.abs(f["H"][0]) + np.abs(f["H"][1])
        return np.abs(self._per_line(lambda c: e[:, :, c] * h[:, :, c]))

    def flux_orders(self, line=0):
        """(B, F, Q), Q = C - 1, in np.fft.fftfreq(Q, 1 / Q) order: P_m = dx * Q * Re(E_m conj(H_m)) with
        E_m = (1 / Q) sum_j E_j exp(-1j * (phi + 2 pi m) * j / Q) and H_m likewise.  Written as the sum it is, not as an
        FFT."""
        f, Q = self.bfluxmon, self.cols - 1
        kind, _, first, n = f["lines"][line]
        if kind != "row" or first != 0 or n != Q:
            raise ValueError("flux_orders needs a row line over the whole period")
        assert self.phi is not None
        o = sum(l[3] for l in f["lines"][:line])
        E, H = (a[:, :, o:o + Q] for a in self.read_flux_lines())
        m = np.fft.fftfreq(Q, 1 / Q)
        jj = np.arange(Q)
        ker = np.exp(-1j * (self.phi[:, None, None] + 2 * np.pi * m[None, :, None]) * jj[None, None, :] / Q)   # (B, m, j)
        Em = np.einsum("bfj,bmj->bfm", E, ker) / Q
        Hm = np.einsum("bfj,bmj->bfm", H, ker) / Q
        return self.dx * Q * np.real(Em * np.conj(Hm))


class BlochFluxOracle(BlochFluxLines, BlochOracle):
    """A periodic batch with a Bloch phase and the lines."""


class BlochDispersiveFluxOracle(BlochFluxLines, BlochDispersiveOracle):
    """The same with the adjoint helpers and the pole (set_bloch_dispersion) of BlochDispersiveOracle."""
