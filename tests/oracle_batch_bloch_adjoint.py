"""The stand-in of tests/oracle_batch_bloch.py plus what include/fdtd2d_batch_bloch_adjoint.h adds, restated in NumPy:

    point sources   after the E half-step and the rectangle source of step n, point cell p takes s = 0.0;
                    s = s + w[p][c] * chan[c][n] for c ascending in float64, then Ez_re = (T)((f64)Ez_re + s); the
                    imaginary part takes nothing; then the image columns are refreshed and the monitors sample
    conjugate       the run steps with (c, -s) in place of (c, s), image columns included
    held window     a copy of the complex window W(re) + 1j * W(im)
    the product     oracle_batch.window_product on the complex windows: hr = ar - bi, hi = ai + br are exactly the
                    real and imaginary part that read_dft_window forms, one rounding each
    probe spectra   SessionOracle.probe_spectra's sums of the real and of the imaginary traces, X = S(re) + 1j * S(im)
                    formed as X_re = S(re)_re - S(im)_im, X_im = S(re)_im + S(im)_re; the peak is the larger part's
    field maxima    the larger of the two parts' maxima, of Ez over columns 0..C-2

``BlochOracle`` itself keeps refusing the plain point sources, channels and held window.  No device, no library."""
import numpy as np

from oracle_batch import point_sums, window_product
from oracle_batch_bloch import BlochOracle, bloch_step, rotate
from oracle_batch_lossy import lossy_coefficients
from test_batch_session_cpu import SessionOracle


class BlochAdjointOracle(BlochOracle):
    bpoints = held_b = None
    conj_last = False     # the image columns hold conj(rho) * column 0 (the last run was a conjugate one)

    def _need_bloch(self):
        assert self.rho is not None, "no Bloch phase is set"

    def set_bloch_phase(self, phi, rotation=None):
        if phi is None and rotation is None:
            self.bpoints = self.held_b = None
        self.conj_last = False
        return BlochOracle.set_bloch_phase(self, phi, rotation)

    def set_dft_window(self, window, omegas, every=1):
        self.held_b = None
        return BlochOracle.set_dft_window(self, window, omegas, every)

    def run(self, nsteps, amps=None, channels=None):
        if self.rho is not None and self.conj_last:
            self._images()                                # a plain run reads rho * column 0 from its first step on
            self.conj_last = False
        return BlochOracle.run(self, nsteps, amps, channels)

    # -- the six calls ---------------------------------------------------------------------------------------------
    def set_bloch_point_sources(self, cells, weights=None):
        self._need_bloch()
        if cells is None:
            self.bpoints = None
            return self
        c = np.asarray(cells)
        w = np.asarray(weights, dtype=np.float64)
        assert np.all(c[..., 1] < self.cols - 1), "a point source lies in the image column"
        self.bpoints = (np.broadcast_to(c, (self.count,) + c.shape[-2:]), np.broadcast_to(w, (self.count,) + w.shape[-2:]))
        return self

    def run_bloch_channels(self, nsteps, amps=None, channels=None, conjugate=False):
        self._need_bloch()
        assert self.bpoints is not None, "no point sources are set"
        ch = np.asarray(channels, dtype=np.float64)
        a = None if amps is None else np.asarray(amps, dtype=np.complex128)
        for b in range(self.count):
            sums = point_sums(self.bpoints[1][b], ch[b] if ch.ndim == 3 else ch)
            self._run_member_points(b, nsteps, None if a is None else a[b], sums, conjugate)
        self.step += nsteps
        self.conj_last = bool(conjugate)
        return self

    def _window(self):
        """The complex window W(re) + 1j * W(im), (B, F, nrows, ncols)."""
        return BlochOracle.read_dft_window(self)

    def hold_bloch_window(self):
        self._need_bloch()
        self.held_b = self._window().copy()
        return self

    def bloch_window_product(self, coef):
        self._need_bloch()
        k = np.asarray(coef, dtype=np.complex128)
        k = np.broadcast_to(k, (self.count, k.shape[-1]))
        cur = self._window()
        return np.stack([window_product(k[b], self.held_b[b], cur[b]) for b in range(self.count)])

    def bloch_probe_spectra(self, omegas, first=0, count=None, peak=False):
        self._need_bloch()
        both = []
        for key in ("trace", "trace_i"):
            part = SessionOracle.__new__(SessionOracle)
            part.count, part.step, part.dt = self.count, self.step, self.dt
            part.probes = dict(trace=self.probes[key], step0=self.probes["step0"])
            both.append(SessionOracle.probe_spectra(part, omegas, first, count, peak=True))
        (sr, pr), (si, pi) = both
        out = (sr.real - si.imag) + 1j * (sr.imag + si.real)
        return (out, np.maximum(pr, pi)) if peak else out

    def bloch_field_absmax(self, which="Ez"):
        self._need_bloch()
        re, im = {"Ez": (self.Ez[:, :, :-1], self.Ez_i[:, :, :-1]), "Hx": (self.Hx, self.Hx_i),
                  "Hy": (self.Hy, self.Hy_i)}[which]
        top = lambda f: np.abs(f.astype(np.float64)).reshape(self.count, -1).max(axis=1)
        return np.maximum(top(re), top(im))

    # -- the loop: BlochOracle._run_bloch_member with the point sources and the run's rotation -----------------------
    def _run_member_points(self, b, nsteps, amps, sums, conjugate):
        T = self.dtype.type
        parts = ((self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b]), (self.Ez_i[b], self.Ezx_i[b], self.Hx_i[b], self.Hy_i[b]))
        eps, mu = self.eps[b], self.mu[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        c, s = T(self.rho[0][b]), T(self.rho[1][b])
        if conjugate:
            s = T(-s)
        # the image columns hold the rotation of the run before (or of set_bloch_phase): this run's from its first step on
        for k in (0, 1):
            parts[0][k][:, -1], parts[1][k][:, -1] = rotate(c, s, parts[0][k][:, 0], parts[1][k][:, 0])
        r, c0, nr, nc = (int(v) for v in self.rects[b])
        wr, wi = self.weights[b].real[c0:c0 + nc], self.weights[b].imag[c0:c0 + nc]
        pr, pc = self.bpoints[0][b][:, 0], self.bpoints[0][b][:, 1]
        win, probes = self.win, self.probes
        for n in range(nsteps):
            bloch_step(parts, eps, mu, self.dt, self.dx, self.profiles[b], ca, cb, c, s)
            if amps is not None and nr and nc:
                ar, ai = amps[n].real, amps[n].imag
                for (Ez, _, _, _), add in zip(parts, (ar * wr - ai * wi, ar * wi + ai * wr)):
                    Ez[r:r + nr, c0:c0 + nc] = (Ez[r:r + nr, c0:c0 + nc].astype(np.float64) + add[None, :]).astype(T)
            Ez = parts[0][0]
            Ez[pr, pc] = (Ez[pr, pc].astype(np.float64) + sums[:, n]).astype(T)      # the real part alone
            for k in (0, 1):                              # Ez, then Ezx
                parts[0][k][:, -1], parts[1][k][:, -1] = rotate(c, s, parts[0][k][:, 0], parts[1][k][:, 0])
            st = self.step + n + 1
            if win is not None and (st - win["step0"]) % win["every"] == 0:
                r0, w0, wnr, wnc = win["win"]
                t = float(st) * self.dt
                for (Ez, _, _, _), kr, ki in zip(parts, ("re", "re_i"), ("im", "im_i")):
                    e = Ez[r0:r0 + wnr, w0:w0 + wnc].astype(np.float64)
                    win[kr][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                    win[ki][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
            if probes is not None:
                k = st - 1 - probes["step0"]
                if 0 <= k < probes["trace"].shape[2]:
                    cells = probes["cells"][b]
                    probes["trace"][b, :, k] = parts[0][0][cells[:, 0], cells[:, 1]]
                    probes["trace_i"][b, :, k] = parts[1][0][cells[:, 0], cells[:, 1]]
