"""Flux lines for the stand-ins of the Hz polarisation, restating in NumPy the definitions that
include/fdtd2d_batch_hz_flux.h fixes: the FluxLines mixin of tests/oracle_batch_flux.py over the stand-ins of
tests/oracle_batch_hz.py.

The Hz stand-ins keep Hz in the ``Ez`` slot, Ex in the ``Hx`` slot and Ey in the ``Hy`` slot, so the mixin's sums are, after
the sources and the image column of every sampled step n,

    H_k += Hz * exp(-1j * omega_k * n * dt)          Hz as stored, widened to double
    E_k += Et * exp(-1j * omega_k * n * dt)          the same phasor

    row line    ("row", i, c0, nc), power towards increasing row:       Et = 0.5 * (Ex[i-1, j] + Ex[i, j])
    column line ("col", j, r0, nr), power towards increasing column:    Et = 0.5 * (Ey[i, j-1] + Ey[i, j])

(a periodic member's column 0 has column C-2 as its left neighbour).  That E lives at (n - 1/2) dt, so read_flux_lines()
returns (Et_hat, Hz_hat), the electric transform first, with Et_hat multiplied by exp(+1j * omega_k * dt / 2) unless raw,
and flux() forms

    P = s * dx * sum over the line's cells of Re(H_k * conj(E_k * exp(+1j * omega_k * dt / 2)))

with s = -1 for a row line and +1 for a column line (S_y = -Ex Hz, S_x = Ey Hz): the mixin's flux negated.  No device, no
library."""
import numpy as np

from oracle_batch_flux import FluxLines
from oracle_batch_hz import HzPeriodicOracle, HzPmlOracle


class HzFluxLines(FluxLines):
    def set_hz_flux_lines(self, lines, omegas, every=1):
        return FluxLines.set_flux_lines(self, lines, omegas, every)

    def set_flux_lines(self, *a, **k):
        raise AssertionError("flux lines (the sign and the averaged component differ) are not available in the Hz "
                             "polarisation")

    def read_flux_lines(self, raw=False):
        hz, et = FluxLines.read_flux_lines(self, raw)      # the mixin's "Ez" is Hz and its "Ht" is Et
        return et, hz

    def _per_line(self, term):
        """term(Hz_hat, Et_hat) summed over each line's cells: (B, N, F)."""
        f = self.fluxmon
        hz, et = FluxLines.read_flux_lines(self)
        out = np.empty((self.count, len(f["lines"]), f["omega"].shape[1]))
        o = 0
        for k, (_, _, _, n) in enumerate(f["lines"]):
            out[:, k, :] = term(hz[:, :, o:o + n], et[:, :, o:o + n]).sum(axis=2)
            o += n
        return out

    def flux(self):
        s = np.array([-1.0 if kind == "row" else 1.0 for kind, _, _, _ in self.fluxmon["lines"]])
        return s[None, :, None] * (self.dx * self._per_line(lambda h, e: np.real(h * np.conj(e))))

    def flux_scale(self):
        """dx * sum |H_k| |E_k| per member, line and frequency: what the flux's rounding error is measured against."""
        return self.dx * self._per_line(lambda h, e: np.abs(h) * np.abs(e))


class HzFluxPmlOracle(HzFluxLines, HzPmlOracle):
    pass


class HzFluxPeriodicOracle(HzFluxLines, HzPeriodicOracle):
    pass


def hz_flux_oracle_for(boundary):
    return HzFluxPeriodicOracle if boundary == "periodic" else HzFluxPmlOracle
