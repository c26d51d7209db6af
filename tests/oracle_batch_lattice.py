"""The stand-in of a lattice batch, restating in NumPy the definition that include/fdtd2d_batch_lattice.h fixes: the unit
cell of a rectangular 2D lattice.  The member shape is (R, C), the period (R-1) x (C-1); row R-1 is the image of row 0
and column C-1 the image of column 0.  Every field is a real part (the PeriodicOracle's own arrays) and an imaginary part
(the BlochOracle's ``*_i`` arrays) of the batch dtype T; member b has the rotations rho_r = (cr, sr) across the row seam
and rho_c = (cc, sc) across the column seam, float64 cos and sin rounded to T.  One step, operation for operation:

    H      for i <= R-2, j <= C-2, per part: Hx = Hx - ch * (Ez[i+1, j] - Ez[i, j]), Hy = Hy + ch * (Ez[i, j+1] - Ez[i, j]);
           the images are stored rotated here, so the seam cells read rho_r * Ez[0, j] and rho_c * Ez[i, 0]
    E      for i <= R-2, j <= C-2, per part: dhy = Hy[i, j] - Hy[i, j-1], dhx = Hx[i, j] - Hx[i-1, j],
           Ez = ca * Ez + (dhy - dhx) * cb, with Hy[i, -1] = conj(rho_c) * Hy[i, C-2] and Hx[-1, j] = conj(rho_r) * Hx[R-2, j]
    then   the Bloch rectangle source (oracle_batch_bloch), the images Ez[i, C-1] = rho_c * Ez[i, 0] and
           Ez[R-1, :] = rho_r * Ez[0, :] (the corner therefore rho_r * (rho_c * Ez[0, 0])), the monitors of each part.

``rotate`` and ``unrotate`` are oracle_batch_bloch's; the source, the monitors, the weights, upload, download and reset are
the BlochOracle's.  There is no layer, no Ezx and no margin for the conductivity.  No device, no library."""
import numpy as np

from oracle_batch_bloch import rotate, unrotate
from oracle_batch_bloch_adjoint import BlochAdjointOracle
from oracle_batch_lossy import LossyOracle, lossy_coefficients

EPS0, MU0 = 8.85418e-12, 4 * np.pi * 1e-7


def lattice_step(parts, mu, dt, dx, ca, cb, rho_r, rho_c):
    """One H -> E step of one member in place.  parts = ((Ez, Hx, Hy) real, (Ez, Hx, Hy) imaginary); the images hold the
    rotated copies on entry and are not yet refreshed on return."""
    ch = dt / (mu[:-1, :-1] * dx)
    for Ez, Hx, Hy in parts:
        core = Ez[:-1, :-1]
        Hx[:-1, :] = Hx[:-1, :] - ch * (Ez[1:, :-1] - core)
        Hy[:, :-1] = Hy[:, :-1] + ch * (Ez[:-1, 1:] - core)
    left = unrotate(rho_c[0], rho_c[1], parts[0][2][:, -2], parts[1][2][:, -2])      # conj(rho_c) * Hy[i, C-2]
    up = unrotate(rho_r[0], rho_r[1], parts[0][1][-2, :], parts[1][1][-2, :])        # conj(rho_r) * Hx[R-2, j]
    for (Ez, Hx, Hy), lw, uw in zip(parts, left, up):
        hy, hx = Hy[:, :-1], Hx[:-1, :]
        west = np.roll(hy, 1, axis=1)
        west[:, 0] = lw
        north = np.roll(hx, 1, axis=0)
        north[0, :] = uw
        dhy = hy - west
        dhx = hx - north
        Ez[:-1, :-1] = ca[:-1, :-1] * Ez[:-1, :-1] + (dhy - dhx) * cb[:-1, :-1]


class LatticeOracle(BlochAdjointOracle):
    rho_r = None          # (c (B,), s (B,)) across the row seam; BlochOracle.rho holds the column seam's

    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="lattice", device=0):
        assert boundary == "lattice"
        BlochAdjointOracle.__init__(self, count, rows, cols, dt, dx, dtype, "periodic")
        self.boundary = "lattice"
        self.set_materials(EPS0, MU0)     # the engine starts with vacuum materials
        self.set_lattice_phase(0.0, 0.0, rotation=((1.0, 0.0), (1.0, 0.0)))

    lattice = True

    @property
    def bloch(self):
        return False

    # -- the phases ------------------------------------------------------------------------------------------------
    def set_lattice_phase(self, phi_rows, phi_cols, rotation=None):
        B = self.count
        if rotation is not None:
            (cr, sr), (cc, sc) = rotation
            self.phi_r = None
        else:
            self.phi_r = np.broadcast_to(np.asarray(phi_rows, dtype=np.float64), (B,))
            phc = np.broadcast_to(np.asarray(phi_cols, dtype=np.float64), (B,))
            cr, sr, cc, sc = np.cos(self.phi_r), np.sin(self.phi_r), np.cos(phc), np.sin(phc)
        cr, sr = (np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)).astype(self.dtype) for v in (cr, sr))
        self.rho_r = (cr, sr)
        # the column seam's rotation, the imaginary parts, the weights and the monitors: the Bloch phase's
        BlochAdjointOracle.set_bloch_phase(self, None if rotation is not None else phi_cols,
                                           rotation=None if rotation is None else (cc, sc))
        return self

    def set_bloch_phase(self, phi, rotation=None):
        raise AssertionError("set_bloch_phase is refused in the lattice mode")

    def _images(self):
        """Ez[:, C-1] = rho_c * Ez[:, 0], then Ez[R-1, :] = rho_r * Ez[0, :], every member."""
        if self.rho_r is None:
            return
        for re, im in ((self.Ez, self.Ez_i),):
            c, s = (v[:, None] for v in self.rho)
            re[:, :, -1], im[:, :, -1] = rotate(c, s, re[:, :, 0], im[:, :, 0])
            c, s = (v[:, None] for v in self.rho_r)
            re[:, -1, :], im[:, -1, :] = rotate(c, s, re[:, 0, :], im[:, 0, :])

    # -- what the images exclude -----------------------------------------------------------------------------------
    def set_pml(self, *a, **kw):
        raise AssertionError("a layer is refused in the lattice mode")

    def margin(self):
        return 0

    def _check(self, s, r0, c0):
        assert np.all(np.isfinite(s)) and np.all(s >= 0)

    def set_conductivity(self, sigma):
        if sigma is not None and np.isscalar(sigma):
            sigma = np.full((self.count, self.rows, self.cols), float(sigma))
        return LossyOracle.set_conductivity(self, sigma)

    def set_sources(self, rects):
        BlochAdjointOracle.set_sources(self, rects)
        r = self.rects
        assert np.all((r[:, 2] == 0) | (r[:, 0] + r[:, 2] <= self.rows - 1)), "a source reaches the image row"
        return self

    def set_dft_window(self, window, omegas, every=1):
        assert int(window[0]) + int(window[2]) <= self.rows - 1, "the window touches the image row"
        return BlochAdjointOracle.set_dft_window(self, window, omegas, every)

    def set_probes(self, cells, capacity):
        assert np.all(np.asarray(cells)[..., 0] < self.rows - 1), "a probe lies in the image row"
        return BlochAdjointOracle.set_probes(self, cells, capacity)

    def set_bloch_point_sources(self, cells, weights=None):
        raise AssertionError("point sources are refused in the lattice mode")

    def run_bloch_channels(self, *a, **kw):
        raise AssertionError("channels are refused in the lattice mode")

    def hold_bloch_window(self):
        raise AssertionError("the held window is refused in the lattice mode")

    def upload_ezx(self, Ezx):
        raise AssertionError("there is no Ezx in the lattice mode")

    def download_ezx(self):
        raise AssertionError("there is no Ezx in the lattice mode")

    def bloch_field_absmax(self, which="Ez"):
        re, im = {"Ez": (self.Ez, self.Ez_i), "Hx": (self.Hx, self.Hx_i), "Hy": (self.Hy, self.Hy_i)}[which]
        top = lambda f: np.abs(f[:, :self.rows - 1, :self.cols - 1].astype(np.float64)).reshape(self.count, -1).max(axis=1)
        return np.maximum(top(re), top(im))

    # -- the loop ------------------------------------------------------------------------------------------------
    def run(self, nsteps, amps=None, channels=None):
        assert channels is None, "channels are refused in the lattice mode"
        a = None if amps is None else np.asarray(amps, dtype=np.complex128)
        for b in range(self.count):
            self._run_lattice_member(b, nsteps, None if a is None else a[b])
        self.step += nsteps
        return self

    def _run_lattice_member(self, b, nsteps, amps):
        T = self.dtype.type
        parts = ((self.Ez[b], self.Hx[b], self.Hy[b]), (self.Ez_i[b], self.Hx_i[b], self.Hy_i[b]))
        eps, mu = self.eps[b], self.mu[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        rho_c = (T(self.rho[0][b]), T(self.rho[1][b]))
        rho_r = (T(self.rho_r[0][b]), T(self.rho_r[1][b]))
        r, c0, nr, nc = (int(v) for v in self.rects[b])
        wr, wi = self.weights[b].real[c0:c0 + nc], self.weights[b].imag[c0:c0 + nc]
        win, probes = self.win, self.probes
        for n in range(nsteps):
            lattice_step(parts, mu, self.dt, self.dx, ca, cb, rho_r, rho_c)
            if amps is not None and nr and nc:
                ar, ai = amps[n].real, amps[n].imag
                for (Ez, _, _), add in zip(parts, (ar * wr - ai * wi, ar * wi + ai * wr)):
                    Ez[r:r + nr, c0:c0 + nc] = (Ez[r:r + nr, c0:c0 + nc].astype(np.float64) + add[None, :]).astype(T)
            er, ei = parts[0][0], parts[1][0]
            er[:, -1], ei[:, -1] = rotate(rho_c[0], rho_c[1], er[:, 0], ei[:, 0])
            er[-1, :], ei[-1, :] = rotate(rho_r[0], rho_r[1], er[0, :], ei[0, :])
            st = self.step + n + 1
            if win is not None and (st - win["step0"]) % win["every"] == 0:
                r0, w0, wnr, wnc = win["win"]
                t = float(st) * self.dt
                for (Ez, _, _), kr, ki in zip(parts, ("re", "re_i"), ("im", "im_i")):
                    e = Ez[r0:r0 + wnr, w0:w0 + wnc].astype(np.float64)
                    win[kr][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                    win[ki][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
            if probes is not None:
                k = st - 1 - probes["step0"]
                if 0 <= k < probes["trace"].shape[2]:
                    cells = probes["cells"][b]
                    probes["trace"][b, :, k] = er[cells[:, 0], cells[:, 1]]
                    probes["trace_i"][b, :, k] = ei[cells[:, 0], cells[:, 1]]
