"""The stand-in of tests/oracle_batch_hz.py's HzPeriodicOracle with a Bloch phase, restating in NumPy the definition that
include/fdtd2d_batch_hz_bloch.h fixes.  Every complex field is a real part (the HzPeriodicOracle's own arrays: ``Ez`` holds
Hz, ``Hx`` Ex, ``Hy`` Ey, ``Ezx`` Hzx, and Jx, Qx, Jy, Qy) and an imaginary part (the ``*_i`` arrays) of the batch dtype T;
member b has the rotation (c_b, s_b), float64 cos and sin rounded to T.  One step is the Hz step on each part -- the E
half-step is ``hz_e_half`` itself, ``hz_bloch_h_half`` restates ``hz_h_half`` because column 0 reads the other part -- and
the parts meet at the seam only:

    E half-step, j = C-2    the right neighbour of Hz is rho * column 0: re' = c*re - s*im, im' = s*re + c*im.  The
                            image column is stored rotated, so ``hz_e_half`` reads it as it stands.
    H half-step, column 0   the left neighbour of Ey is conj(rho) * Ey[:, C-2]: re' = c*er + s*ei, im' = c*ei - s*er
    the rectangle source    Hz_re = (T)((f64)Hz_re + (ar*wr - ai*wi)), Hz_im = (T)((f64)Hz_im + (ar*wi + ai*wr)) with the
                            complex float64 weight of the cell's column
    the image               Hz[:, C-1] = rho * Hz[:, 0], likewise Hzx; Ex, Ey and the pole state have none
    the monitors            the window DFT and the probes of each part of Hz, the complex result re + 1j * im

Without a phase (``set_hz_bloch_phase(None)``) it is the HzPeriodicOracle.  No device, no library."""
import numpy as np

from oracle_batch_bloch import rotate, unrotate
from oracle_batch_dispersive import pole_coefficients
from oracle_batch_hz import HzPeriodicOracle, hz_e_half
from oracle_batch_lossy import lossy_coefficients


def hz_bloch_h_half(parts, mu, dt, dx, P, c, s):
    """The H half-step of both parts of one member in place; the image columns are not yet refreshed.
    parts = ((Hz, Hzx, Ex, Ey) real, (Hz, Hzx, Ex, Ey) imaginary).  hz_h_half's periodic expressions on each part."""
    inner = (slice(1, -1), slice(0, -1))
    one = np.ones(parts[0][0].shape[1], parts[0][0].dtype)
    aec, bec = one[None, :-1], one[None, :-1]
    ch = dt / (mu[inner] * dx)
    wrap = unrotate(c, s, parts[0][3][1:, -2], parts[1][3][1:, -2])     # conj(rho) * Ey[i, C-2], both parts
    for (Hz, Hzx, Ex, Ey), w in zip(parts, wrap):
        ey = Ey[1:, :-1]
        left = np.roll(ey, 1, axis=1)
        left[:, 0] = w                                    # column 0's left neighbour, across the seam
        dey = ey - left
        dex = Ex[1:-1, :] - Ex[:-2, :]
        layer = np.broadcast_to(P["in_r"][1:-1, None], Hz[inner].shape)
        h, zx = Hz[inner], Hzx[inner]
        plain = h - (dey - dex) * ch
        x = aec * zx - (bec * ch) * dey
        y = P["aer"][1:-1, None] * (h - zx) + (P["ber"][1:-1, None] * ch) * dex
        Hzx[inner] = np.where(layer, x, zx)
        Hz[inner] = np.where(layer, x + y, plain)


class HzBlochOracle(HzPeriodicOracle):
    rho = None            # (c (B,), s (B,)) in the batch dtype while a phase is set

    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="periodic", device=0,
                 polarization="hz"):
        HzPeriodicOracle.__init__(self, count, rows, cols, dt, dx, dtype, boundary)
        self.phi = self.weights = None

    @property
    def hz_bloch(self):
        return self.rho is not None

    bloch = False         # BatchEngine.bloch stays false in the Hz polarisation

    # -- the phase and the source weights --------------------------------------------------------------------------
    def set_hz_bloch_phase(self, phi, rotation=None):
        B, shape = self.count, (self.count, self.rows, self.cols)
        if phi is None and rotation is None:
            self.rho = self.phi = self.weights = None
            self.Ez[:, :, -1], self.Ezx[:, :, -1] = self.Ez[:, :, 0], self.Ezx[:, :, 0]
            return self
        if self.rho is None:
            assert self.points is None and self.held is None, "point sources and the held window exclude a Bloch phase"
            if self.win is not None:
                assert self.win["win"][1] + self.win["win"][3] <= self.cols - 1, "the window touches the image column"
                self.win["re_i"], self.win["im_i"] = np.zeros_like(self.win["re"]), np.zeros_like(self.win["im"])
            if self.probes is not None:
                assert np.all(self.probes["cells"][..., 1] < self.cols - 1), "a probe lies in the image column"
                self.probes["trace_i"] = np.zeros_like(self.probes["trace"])
            self.Ez_i, self.Ezx_i = np.zeros(shape, self.dtype), np.zeros(shape, self.dtype)
            self.Hx_i = np.zeros((B, self.rows, self.cols - 1), self.dtype)
            self.Hy_i = np.zeros((B, self.rows - 1, self.cols), self.dtype)
            self.Jx_i, self.Qx_i, self.Jy_i, self.Qy_i = (np.zeros(shape, self.dtype) for _ in range(4))
            self.weights = np.ones((B, self.cols - 1), np.complex128)
        if rotation is not None:
            c, s = (np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)) for v in rotation)
            self.phi = None
        else:
            self.phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (B,))
            c, s = np.cos(self.phi), np.sin(self.phi)
        self.rho = (c.astype(self.dtype), s.astype(self.dtype))
        self._images()
        return self

    def set_hz_bloch_source(self, weights="ramp"):
        assert self.rho is not None
        Q = self.cols - 1
        if weights is None:
            w = np.ones(Q)
        elif isinstance(weights, str):
            assert weights == "ramp" and self.phi is not None
            w = np.exp(1j * self.phi[:, None] * np.arange(Q)[None, :] / Q)
        else:
            w = np.asarray(weights, dtype=np.complex128)
        self.weights = np.array(np.broadcast_to(w, (self.count, Q)), dtype=np.complex128)
        return self

    def _images(self):
        """Hz[:, C-1] = rho * Hz[:, 0] and likewise Hzx, every member."""
        c, s = (v[:, None] for v in self.rho)
        for re, im in ((self.Ez, self.Ez_i), (self.Ezx, self.Ezx_i)):
            re[:, :, -1], im[:, :, -1] = rotate(c, s, re[:, :, 0], im[:, :, 0])

    # -- what a phase excludes -------------------------------------------------------------------------------------
    def set_dft_window(self, window, omegas, every=1):
        if self.rho is not None:
            assert int(window[1]) + int(window[3]) <= self.cols - 1, "the window touches the image column"
        HzPeriodicOracle.set_dft_window(self, window, omegas, every)
        if self.rho is not None:
            self.win["re_i"], self.win["im_i"] = np.zeros_like(self.win["re"]), np.zeros_like(self.win["im"])
        return self

    def set_probes(self, cells, capacity):
        if self.rho is not None:
            assert np.all(np.asarray(cells)[..., 1] < self.cols - 1), "a probe lies in the image column"
        HzPeriodicOracle.set_probes(self, cells, capacity)
        if self.rho is not None:
            self.probes["trace_i"] = np.zeros_like(self.probes["trace"])
        return self

    def set_point_sources(self, cells, weights=None):
        assert cells is None or self.rho is None, "point sources exclude a Bloch phase"
        return HzPeriodicOracle.set_point_sources(self, cells, weights)

    def set_pml(self, *a, **kw):
        HzPeriodicOracle.set_pml(self, *a, **kw)
        if self.rho is not None:
            self.Ezx_i[...] = 0
        return self

    def clear_pml(self):
        HzPeriodicOracle.clear_pml(self)
        if self.rho is not None:
            self.Ezx_i[...] = 0
        return self

    # -- state ---------------------------------------------------------------------------------------------------
    def reset(self):
        HzPeriodicOracle.reset(self)
        if self.rho is not None:
            for a in (self.Ez_i, self.Ezx_i, self.Hx_i, self.Hy_i, self.Jx_i, self.Qx_i, self.Jy_i, self.Qy_i):
                a[...] = 0
            if self.win is not None:
                self.win["re_i"][...] = 0
                self.win["im_i"][...] = 0
            if self.probes is not None:
                self.probes["trace_i"][...] = 0
        return self

    def upload(self, Ez=None, Hx=None, Hy=None):
        if self.rho is None:
            return HzPeriodicOracle.upload(self, Ez, Hx, Hy)
        for name, a in (("Ez", Ez), ("Hx", Hx), ("Hy", Hy)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).real.astype(self.dtype)
                getattr(self, name + "_i")[...] = np.asarray(a).imag.astype(self.dtype)
        self._images()
        return self

    def upload_ezx(self, Ezx):
        if self.rho is None:
            return HzPeriodicOracle.upload_ezx(self, Ezx)
        self.Ezx[...] = np.asarray(Ezx).real.astype(self.dtype)
        self.Ezx_i[...] = np.asarray(Ezx).imag.astype(self.dtype)
        self._images()
        return self

    def download(self):
        if self.rho is None:
            return HzPeriodicOracle.download(self)
        return self.Ez + 1j * self.Ez_i, self.Hx + 1j * self.Hx_i, self.Hy + 1j * self.Hy_i

    def download_ezx(self):
        return self.Ezx.copy() if self.rho is None else self.Ezx + 1j * self.Ezx_i

    def download_dispersion(self):
        re = HzPeriodicOracle.download_dispersion(self)
        if self.rho is None:
            return re
        return tuple(a + 1j * b for a, b in zip(re, (self.Jx_i, self.Qx_i, self.Jy_i, self.Qy_i)))

    def upload_hz_dispersion(self, Jx=None, Qx=None, Jy=None, Qy=None):
        if self.rho is None:
            return HzPeriodicOracle.upload_hz_dispersion(self, Jx, Qx, Jy, Qy)
        for name, a in (("Jx", Jx), ("Qx", Qx), ("Jy", Jy), ("Qy", Qy)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).real.astype(self.dtype)
                getattr(self, name + "_i")[...] = np.asarray(a).imag.astype(self.dtype)
        return self

    def read_dft_window(self):
        w = self.win
        if self.rho is None:
            return HzPeriodicOracle.read_dft_window(self)
        return (w["re"] + 1j * w["im"]) + 1j * (w["re_i"] + 1j * w["im_i"])

    def read_probes(self, first=0, count=None):
        re = HzPeriodicOracle.read_probes(self, first, count)
        if self.rho is None:
            return re
        tr = self.probes["trace_i"]
        return re + 1j * tr[:, :, first:tr.shape[2] if count is None else first + count]

    # -- the loop ------------------------------------------------------------------------------------------------
    def run(self, nsteps, amps=None, channels=None):
        if self.rho is None:
            return HzPeriodicOracle.run(self, nsteps, amps, channels)
        assert channels is None, "channels exclude a Bloch phase"
        a = None if amps is None else np.asarray(amps, dtype=np.complex128)
        for b in range(self.count):
            self._run_bloch_member(b, nsteps, None if a is None else a[b])
        self.step += nsteps
        return self

    def _run_bloch_member(self, b, nsteps, amps):
        T = self.dtype.type
        parts = ((self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b]), (self.Ez_i[b], self.Ezx_i[b], self.Hx_i[b], self.Hy_i[b]))
        state = ((self.Jx[b], self.Qx[b], self.Jy[b], self.Qy[b]), (self.Jx_i[b], self.Qx_i[b], self.Jy_i[b], self.Qy_i[b]))
        eps, mu, P = self.eps[b], self.mu[b], self.profiles[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        coef = None
        if self.dispersive:
            coef = pole_coefficients(self.wp2[b], self.gamma[b], self.omega0[b], self.dt, self.dx, self.dtype)
        c, s = T(self.rho[0][b]), T(self.rho[1][b])
        r, c0, nr, nc = (int(v) for v in self.rects[b])
        wr, wi = self.weights[b].real[c0:c0 + nc], self.weights[b].imag[c0:c0 + nc]
        win, probes = self.win, self.probes
        for n in range(nsteps):
            for (Hz, _, Ex, Ey), st in zip(parts, state):     # the image column holds rho * column 0
                hz_e_half(Hz, Ex, Ey, eps, self.dt, self.dx, P, ca, cb, True, None if coef is None else st + tuple(coef))
            hz_bloch_h_half(parts, mu, self.dt, self.dx, P, c, s)
            if amps is not None and nr and nc:
                ar, ai = amps[n].real, amps[n].imag
                for (Hz, _, _, _), add in zip(parts, (ar * wr - ai * wi, ar * wi + ai * wr)):
                    Hz[r:r + nr, c0:c0 + nc] = (Hz[r:r + nr, c0:c0 + nc].astype(np.float64) + add[None, :]).astype(T)
            for k in (0, 1):                              # Hz, then Hzx
                parts[0][k][:, -1], parts[1][k][:, -1] = rotate(c, s, parts[0][k][:, 0], parts[1][k][:, 0])
            st = self.step + n + 1
            if win is not None and (st - win["step0"]) % win["every"] == 0:
                r0, w0, wnr, wnc = win["win"]
                t = float(st) * self.dt
                for (Hz, _, _, _), kr, ki in zip(parts, ("re", "re_i"), ("im", "im_i")):
                    e = Hz[r0:r0 + wnr, w0:w0 + wnc].astype(np.float64)
                    win[kr][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                    win[ki][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
            if probes is not None:
                k = st - 1 - probes["step0"]
                if 0 <= k < probes["trace"].shape[2]:
                    cells = probes["cells"][b]
                    probes["trace"][b, :, k] = parts[0][0][cells[:, 0], cells[:, 1]]
                    probes["trace_i"][b, :, k] = parts[1][0][cells[:, 0], cells[:, 1]]
