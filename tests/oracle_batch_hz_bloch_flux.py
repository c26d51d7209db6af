"""Flux lines for the stand-in of the Hz Bloch batches (tests/oracle_batch_hz_bloch.py), restating in NumPy the definition
that include/fdtd2d_batch_hz_bloch_flux.h fixes.  A mixin in the manner of oracle_batch_bloch_flux.BlochFluxLines and
oracle_batch_hz_flux.HzFluxLines: it runs HzBlochOracle one step at a time and, after the source and the image column of
every sampled step n (every `every`-th step counted from set_hz_bloch_flux_lines), adds in float64 on every line cell, for
the real part and for the imaginary part of the fields,

    H_k += Hz * exp(-1j * omega_k * n * dt)          Hz of that part as stored, widened to double
    E_k += Et * exp(-1j * omega_k * n * dt)          the same phasor

with the tangential E of the step's E half-step centred on the cell, on each part:

    row line    ("row", i, c0, nc), power towards increasing row:       Et = 0.5 * (Ex[i-1, j] + Ex[i, j])
    column line ("col", j, r0, nr), power towards increasing column:    Et = 0.5 * (Ey[i, j-1] + Ey[i, j])

Column 0's left neighbour lies across the seam: it is conj(rho) * Ey[i, C-2], `unrotate` in the batch dtype (what the H
half-step itself subtracts), then widened; rows 0 and R-1 evaluate it the same way.  The slot Ey[R-1, :], which no update
writes, reads as zero (the device stores zero there).  The spectra of the complex fields are H_k = Hr_k + 1j * Hi_k and E_k
likewise; read_flux_lines() returns (Et_hat, Hz_hat), the electric transform first, with Et_hat multiplied by
exp(+1j * omega_k * dt / 2) unless raw, and flux() forms

    P = s * dx * sum over the line's cells of Re(H_k * conj(E_k * exp(+1j * omega_k * dt / 2)))

with s = -1 for a row line and +1 for a column line (S_y = -Ex Hz, S_x = Ey Hz).  flux_orders(line) splits P of a
whole-period row line over the diffraction orders.  No device, no library."""
import numpy as np

from oracle_batch_bloch import unrotate
from oracle_batch_flux import MAX_FREQS, MAX_LINES
from oracle_batch_hz_bloch import HzBlochOracle


class HzBlochFluxLines:
    hzbfluxmon = None

    def set_hz_bloch_flux_lines(self, lines, omegas, every=1):
        if lines is None or len(lines) == 0:
            self.hzbfluxmon = None
            return self
        R, C = self.rows, self.cols
        assert self.boundary == "periodic" and self.rho is not None, "the lines need the phase of set_hz_bloch_phase"
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
        self.hzbfluxmon = dict(lines=[tuple(l) for l in lines], omega=w, every=int(every), step0=self.step,
                               i=np.concatenate(rows), j=np.concatenate(cols), col=np.concatenate(colline),
                               H=(z, z.copy()), E=(z.copy(), z.copy()))     # (real part's, imaginary part's)
        return self

    # -- what the lines exclude while they are set ----------------------------------------------------------------------
    def set_hz_bloch_phase(self, phi, rotation=None):
        assert self.hzbfluxmon is None or phi is not None or rotation is not None, "the lines need the phase"
        return super().set_hz_bloch_phase(phi, rotation)

    def reset(self):
        super().reset()
        f = self.hzbfluxmon
        if f is not None:
            for a in f["H"] + f["E"]:
                a[...] = 0
            f["step0"] = 0
        return self

    # -- the sums ---------------------------------------------------------------------------------------------------------
    def _seam(self, c, s, re, im):
        """Ey of column C-2 as column 0 sees it: conj(rho) * Ey, in the batch dtype."""
        return unrotate(c, s, re, im)

    def _tangential_e(self, b):
        """(Et of the real part, Et of the imaginary part) on every line cell of member b, float64."""
        f, R, C, T = self.hzbfluxmon, self.rows, self.cols, self.dtype.type
        i, j = f["i"], f["j"]
        ey = [np.zeros((R, C), self.dtype), np.zeros((R, C), self.dtype)]
        ey[0][:R - 1, :], ey[1][:R - 1, :] = self.Hy[b], self.Hy_i[b]       # the Hy slot holds Ey
        left = [e[i, np.maximum(j - 1, 0)] for e in ey]
        seam = self._seam(T(self.rho[0][b]), T(self.rho[1][b]), ey[0][i, C - 2], ey[1][i, C - 2])   # in the batch dtype
        out = []
        for ex, e, lw, sw in zip((self.Hx[b], self.Hx_i[b]), ey, left, seam):                       # the Hx slot holds Ex
            lw = np.where(j == 0, sw, lw).astype(np.float64)
            up = ex[np.maximum(i - 1, 0), np.minimum(j, C - 2)].astype(np.float64)
            own = ex[i, np.minimum(j, C - 2)].astype(np.float64)
            out.append(np.where(f["col"], 0.5 * (lw + e[i, j].astype(np.float64)), 0.5 * (up + own)))
        return out

    def _run_bloch_member(self, b, nsteps, amps):
        f = self.hzbfluxmon
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
                    for part, Hz, et in zip((0, 1), (self.Ez[b], self.Ez_i[b]), self._tangential_e(b)):
                        h = Hz[f["i"], f["j"]].astype(np.float64)                                   # the Ez slot holds Hz
                        f["H"][part][b] += h[None, :] * ph[:, None]
                        f["E"][part][b] += et[None, :] * ph[:, None]
        finally:
            self.step = base

    # -- reading -------------------------------------------------------------------------------------------------------------
    def read_hz_bloch_flux_parts(self):
        f = self.hzbfluxmon
        return tuple((f["H"][k].copy(), f["E"][k].copy()) for k in (0, 1))

    def read_flux_lines(self, raw=False):
        f = self.hzbfluxmon
        half = 1.0 if raw else np.exp(0.5j * f["omega"] * self.dt)[:, :, None]
        return (f["E"][0] + 1j * f["E"][1]) * half, f["H"][0] + 1j * f["H"][1]

    def _per_line(self, term):
        f = self.hzbfluxmon
        out = np.empty((self.count, len(f["lines"]), f["omega"].shape[1]))
        o = 0
        for k, (kind, _, _, n) in enumerate(f["lines"]):
            out[:, k, :] = (-1.0 if kind == "row" else 1.0) * self.dx * term(slice(o, o + n)).sum(axis=2)
            o += n
        return out

    def flux(self):
        E, H = self.read_flux_lines()
        return self._per_line(lambda c: np.real(H[:, :, c] * np.conj(E[:, :, c])))

    def flux_scale(self):
        """dx * sum (|Hr_k| + |Hi_k|) (|Er_k| + |Ei_k|) per member, line and frequency: what the flux's rounding error
        is measured against."""
        f = self.hzbfluxmon
        h = np.abs(f["H"][0]) + np.abs(f["H"][1])
        e = np.abs(f["E"][0]) + np.abs(f["E"][1])
        return np.abs(self._per_line(lambda c: h[:, :, c] * e[:, :, c]))

    def flux_orders(self, line=0):
        """(B, F, Q), Q = C - 1, in np.fft.fftfreq(Q, 1 / Q) order: P_m = -dx * Q * Re(H_m conj(E_m)) with
        H_m = (1 / Q) sum_j H_j exp(-1j * (phi + 2 pi m) * j / Q) and E_m likewise.  Written as the sum it is, not as an
        FFT."""
        f, Q = self.hzbfluxmon, self.cols - 1
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
        return -self.dx * Q * np.real(Hm * np.conj(Em))


class HzBlochFluxOracle(HzBlochFluxLines, HzBlochOracle):
    """A periodic batch in the Hz polarisation with a Bloch phase (conductivity and pole as set) and the lines."""
