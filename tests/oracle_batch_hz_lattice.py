"""The stand-in of an Hz lattice batch, restating in NumPy the definition that include/fdtd2d_batch_hz_lattice.h fixes: the
unit cell of a rectangular 2D lattice in the Hz polarisation, with a conductivity and one Drude-Lorentz pole on Ex and Ey.
The member shape is (R, C), the period (R-1) x (C-1); row R-1 of Hz is the image of row 0 and column C-1 the image of
column 0.  Every field is a real part (the HzPeriodicOracle's arrays: ``Ez`` holds Hz, ``Hx`` Ex, ``Hy`` Ey, and Jx, Qx,
Jy, Qy) and an imaginary part (the HzBlochOracle's ``*_i`` arrays) of the batch dtype T; member b has the rotations
rho_r = (cr, sr) across the row seam and rho_c = (cc, sc) across the column seam, float64 cos and sin rounded to T.  One
step, operation for operation:

    E      ``hz_e_half`` on each part with every cell a material cell (no layer): the images are stored rotated here, so
           the seam cells read rho_r * Hz[0, j] and rho_c * Hz[i, 0] as they stand
    H      for i <= R-2, j <= C-2, per part: dey = Ey[i, j] - Ey[i, j-1], dex = Ex[i, j] - Ex[i-1, j],
           Hz = Hz - (dey - dex) * ch, with Ey[i, -1] = conj(rho_c) * Ey[i, C-2] and Ex[-1, j] = conj(rho_r) * Ex[R-2, j]
    then   the Hz Bloch rectangle source, the images Hz[i, C-1] = rho_c * Hz[i, 0] and Hz[R-1, :] = rho_r * Hz[0, :] (the
           corner therefore rho_r * (rho_c * Hz[0, 0])), the monitors of each part.

``rotate`` and ``unrotate`` are oracle_batch_bloch's, ``hz_e_half`` oracle_batch_hz's, the source weights, the monitors,
upload, download and reset the HzBlochOracle's.  There is no Hzx and no margin for sigma and wp2.  Without the mode
(``set_hz_lattice_phase(None, None)``) it is the HzPeriodicOracle.  No device, no library."""
import numpy as np

from oracle_batch_bloch import rotate, unrotate
from oracle_batch_dispersive import pole_coefficients
from oracle_batch_hz import hz_e_half
from oracle_batch_hz_bloch import HzBlochOracle
from oracle_batch_lossy import lossy_coefficients


def hz_lattice_h_half(parts, mu, dt, dx, rho_r, rho_c):
    """The H half-step of both parts of one member in place; the images are not yet refreshed.
    parts = ((Hz, Ex, Ey) real, (Hz, Ex, Ey) imaginary)."""
    ch = dt / (mu[:-1, :-1] * dx)
    left = unrotate(rho_c[0], rho_c[1], parts[0][2][:, -2], parts[1][2][:, -2])      # conj(rho_c) * Ey[i, C-2]
    up = unrotate(rho_r[0], rho_r[1], parts[0][1][-2, :], parts[1][1][-2, :])        # conj(rho_r) * Ex[R-2, j]
    for (Hz, Ex, Ey), lw, uw in zip(parts, left, up):
        ey, ex = Ey[:, :-1], Ex[:-1, :]
        west = np.roll(ey, 1, axis=1)
        west[:, 0] = lw
        north = np.roll(ex, 1, axis=0)
        north[0, :] = uw
        dey = ey - west
        dex = ex - north
        Hz[:-1, :-1] = Hz[:-1, :-1] - (dey - dex) * ch


class HzLatticeOracle(HzBlochOracle):
    rho_r = None          # (c (B,), s (B,)) across the row seam while the mode is on; HzBlochOracle.rho holds the column seam's

    @property
    def hz_lattice(self):
        return self.rho_r is not None

    @property
    def hz_bloch(self):
        return False      # BatchEngine.hz_bloch stays false in the lattice mode

    lattice = False       # and so do BatchEngine.lattice and .bloch

    # -- the phases ------------------------------------------------------------------------------------------------
    def set_hz_lattice_phase(self, phi_rows, phi_cols, rotation=None):
        B = self.count
        if phi_rows is None and phi_cols is None and rotation is None:
            if self.rho_r is None:
                return self
            assert not np.any(self._outside_periodic()), "sigma or wp2 where a periodic Hz batch allows none"
            self.rho_r = None
            HzBlochOracle.set_hz_bloch_phase(self, None)          # the column slots: unrotated copies of column 0
            self.Ez[:, -1, :] = self.Ez[:, 0, :]                  # the row slots: unrotated copies of row 0
            return self
        if self.rho_r is None:
            assert self.rho is None, "the phase of set_hz_bloch_phase excludes the lattice mode"
            assert self.profiles[0]["L"] == 0, "a layer excludes the lattice mode"
            if self.win is not None:
                assert self.win["win"][0] + self.win["win"][2] <= self.rows - 1, "the window touches the image row"
            if self.probes is not None:
                assert np.all(self.probes["cells"][..., 0] < self.rows - 1), "a probe lies in the image row"
            r = self.rects
            assert np.all((r[:, 2] == 0) | (r[:, 0] + r[:, 2] <= self.rows - 1)), "a source reaches the image row"
        if rotation is not None:
            (cr, sr), (cc, sc) = rotation
            self.phi_r = None
        else:
            self.phi_r = np.broadcast_to(np.asarray(phi_rows, dtype=np.float64), (B,))
            cr, sr = np.cos(self.phi_r), np.sin(self.phi_r)
        cr, sr = (np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)).astype(self.dtype) for v in (cr, sr))
        self.rho_r = (cr, sr)
        # the column seam's rotation, the imaginary parts, the weights and the monitors: the Hz Bloch phase's
        HzBlochOracle.set_hz_bloch_phase(self, None if rotation is not None else phi_cols,
                                         rotation=None if rotation is None else (cc, sc))
        return self

    def set_hz_bloch_phase(self, phi, rotation=None):
        assert self.rho_r is None, "set_hz_bloch_phase is refused in the lattice mode"
        return HzBlochOracle.set_hz_bloch_phase(self, phi, rotation)

    def _images(self):
        """Hz[:, C-1] = rho_c * Hz[:, 0], then Hz[R-1, :] = rho_r * Hz[0, :], every member."""
        if self.rho_r is None:
            return HzBlochOracle._images(self)
        re, im = self.Ez, self.Ez_i
        c, s = (v[:, None] for v in self.rho)
        re[:, :, -1], im[:, :, -1] = rotate(c, s, re[:, :, 0], im[:, :, 0])
        c, s = (v[:, None] for v in self.rho_r)
        re[:, -1, :], im[:, -1, :] = rotate(c, s, re[:, 0, :], im[:, 0, :])

    # -- where a cell may conduct or carry a pole --------------------------------------------------------------------
    def allowed(self):
        if self.rho_r is None:
            return HzBlochOracle.allowed(self)
        ok = np.zeros((self.rows, self.cols), bool)
        ok[:self.rows - 1, :] = True          # no margin: there is no edge (column C-1 is accepted and never read)
        return ok

    def _outside_periodic(self):
        """(B, R, C) bool: sigma or wp2 non-zero where the plain periodic Hz batch allows none."""
        keep, self.rho_r = self.rho_r, None
        ok = HzBlochOracle.allowed(self)
        self.rho_r = keep
        bad = np.zeros((self.count, self.rows, self.cols), bool)
        for a in (self.sigma, self.wp2):
            if a is not None:
                bad |= (np.asarray(a) != 0) & ~ok[None]
        return bad

    # -- what the images exclude -----------------------------------------------------------------------------------
    def set_pml(self, *a, **kw):
        assert self.rho_r is None, "a layer is refused in the lattice mode"
        return HzBlochOracle.set_pml(self, *a, **kw)

    def upload_ezx(self, Ezx):
        assert self.rho_r is None, "there is no Hzx in the lattice mode"
        return HzBlochOracle.upload_ezx(self, Ezx)

    def download_ezx(self):
        assert self.rho_r is None, "there is no Hzx in the lattice mode"
        return HzBlochOracle.download_ezx(self)

    def set_sources(self, rects):
        HzBlochOracle.set_sources(self, rects)
        if self.rho_r is not None:
            r = self.rects
            assert np.all((r[:, 2] == 0) | (r[:, 0] + r[:, 2] <= self.rows - 1)), "a source reaches the image row"
        return self

    def set_dft_window(self, window, omegas, every=1):
        if self.rho_r is not None:
            assert int(window[0]) + int(window[2]) <= self.rows - 1, "the window touches the image row"
        return HzBlochOracle.set_dft_window(self, window, omegas, every)

    def set_probes(self, cells, capacity):
        if self.rho_r is not None:
            assert np.all(np.asarray(cells)[..., 0] < self.rows - 1), "a probe lies in the image row"
        return HzBlochOracle.set_probes(self, cells, capacity)

    # -- the loop ------------------------------------------------------------------------------------------------
    def run(self, nsteps, amps=None, channels=None):
        if self.rho_r is None:
            return HzBlochOracle.run(self, nsteps, amps, channels)
        assert channels is None, "channels are refused in the lattice mode"
        a = None if amps is None else np.asarray(amps, dtype=np.complex128)
        for b in range(self.count):
            self._run_lattice_member(b, nsteps, None if a is None else a[b])
        self.step += nsteps
        return self

    def _run_lattice_member(self, b, nsteps, amps):
        T = self.dtype.type
        parts = ((self.Ez[b], self.Hx[b], self.Hy[b]), (self.Ez_i[b], self.Hx_i[b], self.Hy_i[b]))
        state = ((self.Jx[b], self.Qx[b], self.Jy[b], self.Qy[b]), (self.Jx_i[b], self.Qx_i[b], self.Jy_i[b], self.Qy_i[b]))
        eps, mu, P = self.eps[b], self.mu[b], self.profiles[b]
        assert P["L"] == 0
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        coef = None
        if self.dispersive:
            coef = pole_coefficients(self.wp2[b], self.gamma[b], self.omega0[b], self.dt, self.dx, self.dtype)
        rho_c = (T(self.rho[0][b]), T(self.rho[1][b]))
        rho_r = (T(self.rho_r[0][b]), T(self.rho_r[1][b]))
        r, c0, nr, nc = (int(v) for v in self.rects[b])
        wr, wi = self.weights[b].real[c0:c0 + nc], self.weights[b].imag[c0:c0 + nc]
        win, probes = self.win, self.probes
        for n in range(nsteps):
            for (Hz, Ex, Ey), st in zip(parts, state):        # the images hold the rotated copies
                hz_e_half(Hz, Ex, Ey, eps, self.dt, self.dx, P, ca, cb, True, None if coef is None else st + tuple(coef))
            hz_lattice_h_half(parts, mu, self.dt, self.dx, rho_r, rho_c)
            if amps is not None and nr and nc:
                ar, ai = amps[n].real, amps[n].imag
                for (Hz, _, _), add in zip(parts, (ar * wr - ai * wi, ar * wi + ai * wr)):
                    Hz[r:r + nr, c0:c0 + nc] = (Hz[r:r + nr, c0:c0 + nc].astype(np.float64) + add[None, :]).astype(T)
            hr, hi = parts[0][0], parts[1][0]
            hr[:, -1], hi[:, -1] = rotate(rho_c[0], rho_c[1], hr[:, 0], hi[:, 0])
            hr[-1, :], hi[-1, :] = rotate(rho_r[0], rho_r[1], hr[0, :], hi[0, :])
            st = self.step + n + 1
            if win is not None and (st - win["step0"]) % win["every"] == 0:
                r0, w0, wnr, wnc = win["win"]
                t = float(st) * self.dt
                for (Hz, _, _), kr, ki in zip(parts, ("re", "re_i"), ("im", "im_i")):
                    e = Hz[r0:r0 + wnr, w0:w0 + wnc].astype(np.float64)
                    win[kr][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                    win[ki][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
            if probes is not None:
                k = st - 1 - probes["step0"]
                if 0 <= k < probes["trace"].shape[2]:
                    cells = probes["cells"][b]
                    probes["trace"][b, :, k] = hr[cells[:, 0], cells[:, 1]]
                    probes["trace_i"][b, :, k] = hi[cells[:, 0], cells[:, 1]]
