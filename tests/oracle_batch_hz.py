"""The stand-ins of tests/oracle_batch_lossy.py (boundary "pml") and tests/oracle_batch_periodic.py in the Hz
polarisation, restating in NumPy, line by line, the arithmetic that include/fdtd2d_batch_hz.h fixes.

Storage is the batch's own: ``Ez`` holds Hz, ``Hx`` (R x C-1) holds Ex, ``Hy`` (R-1 x C) holds Ey, ``Ezx`` holds Hzx.
eps[i,j] serves Ex[i,j] and Ey[i,j], mu[i,j] serves Hz[i,j].  ce = dt/(eps dx), ch = dt/(mu dx) in T; ca, cb from sigma as
oracle_batch_lossy.lossy_coefficients forms them; a, ck, cj as oracle_batch_dispersive.pole_coefficients forms them.

One step, every operation rounded to T:

    E   for i <= R-2, j <= C-2, dxi = Hz[i+1,j] - Hz[i,j], dyj = Hz[i,j+1] - Hz[i,j].  Material cells (L <= i <= R-2-L
        and, on "pml", L <= j <= C-2-L):
            jx = a*Jx + (cj*Ex - ck*Qx);  Qx = Qx + jx;  Ex = ca*Ex + (dxi - jx)*cb;  Jx = jx
            jy = a*Jy + (cj*Ey - ck*Qy);  Qy = Qy + jy;  Ey = ca*Ey - (dyj + jy)*cb;  Jy = jy
        all others: Ex = ahr[i]*Ex + (bhr[i]*ce)*dxi,  Ey = ahc[j]*Ey - (bhc[j]*ce)*dyj  (periodic: column factors one)
    H   for 1 <= i <= R-2 and 1 <= j <= C-2 (periodic: 0 <= j <= C-2, cyclically), dey = Ey[i,j] - Ey[i,j-1],
        dex = Ex[i,j] - Ex[i-1,j].  Outside the layer Hz = Hz - (dey - dex)*ch; in it
            x = aec*Hzx - (bec*ch)*dey;  y = aer*(Hz - Hzx) + (ber*ch)*dex;  Hzx = x;  Hz = x + y
    then the rectangle source and the point sources on Hz, the image column of Hz and Hzx (periodic), the monitors on Hz.

sigma and wp2 may be non-zero on rows g <= i <= R-2-g (g = margin()) and, on "pml", columns g <= j <= C-2-g; column C-1
of a periodic member is accepted and never read.  No device, no library."""
import numpy as np

from oracle_batch_dispersive import pole_coefficients, stability
from oracle_batch_lossy import LossyOracle, lossy_coefficients
from oracle_batch_periodic import PeriodicOracle


def hz_e_half(Hz, Ex, Ey, eps, dt, dx, P, ca, cb, periodic, pole=None):
    """The E half-step of one member in place.  pole: None or (Jx, Qx, Jy, Qy, a, ck, cj)."""
    R, C = Hz.shape
    L = P["L"]
    c = (slice(None, -1), slice(None, -1))
    core = Hz[c]
    dxi = Hz[1:, :-1] - core
    dyj = Hz[:-1, 1:] - core
    ce = dt / (eps[c] * dx)
    ex, ey = Ex[:-1, :], Ey[:, :-1]
    one = np.ones(C, Hz.dtype)
    ahc, bhc = (one, one) if periodic else (P["ahc"], P["bhc"])
    lay_x = P["ahr"][:-1, None] * ex + (P["bhr"][:-1, None] * ce) * dxi
    lay_y = ahc[None, :-1] * ey - (bhc[None, :-1] * ce) * dyj
    i, j = np.arange(R - 1)[:, None], np.arange(C - 1)[None, :]
    mat = (i >= L) & (i <= R - 2 - L) & (np.ones_like(j, bool) if periodic else (j >= L) & (j <= C - 2 - L))
    if pole is None:
        mat_x = ca[c] * ex + dxi * cb[c]
        mat_y = ca[c] * ey - dyj * cb[c]
    else:
        Jx, Qx, Jy, Qy, a, ck, cj = pole
        jx = a * Jx[c] + (cj[c] * ex - ck * Qx[c])
        qx = Qx[c] + jx
        mat_x = ca[c] * ex + (dxi - jx) * cb[c]
        jy = a * Jy[c] + (cj[c] * ey - ck * Qy[c])
        qy = Qy[c] + jy
        mat_y = ca[c] * ey - (dyj + jy) * cb[c]
        Qx[c] = np.where(mat, qx, Qx[c])
        Jx[c] = np.where(mat, jx, Jx[c])
        Qy[c] = np.where(mat, qy, Qy[c])
        Jy[c] = np.where(mat, jy, Jy[c])
    Ex[:-1, :] = np.where(mat, mat_x, lay_x)
    Ey[:, :-1] = np.where(mat, mat_y, lay_y)


def hz_h_half(Hz, Hzx, Ex, Ey, mu, dt, dx, P, periodic):
    """The H half-step of one member in place; the image column is not yet refreshed."""
    if periodic:
        one = np.ones(Hz.shape[1], Hz.dtype)
        inner = (slice(1, -1), slice(0, -1))
        ey = Ey[1:, :-1]
        dey = ey - np.roll(ey, 1, axis=1)                 # column 0's left neighbour is column C-2
        dex = Ex[1:-1, :] - Ex[:-2, :]
        aec, bec = one[None, :-1], one[None, :-1]
        layer = np.broadcast_to(P["in_r"][1:-1, None], Hz[inner].shape)
    else:
        inner = (slice(1, -1), slice(1, -1))
        dey = Ey[1:, 1:-1] - Ey[1:, :-2]
        dex = Ex[1:-1, 1:] - Ex[:-2, 1:]
        aec, bec = P["aec"][None, 1:-1], P["bec"][None, 1:-1]
        layer = P["in_r"][1:-1, None] | P["in_c"][None, 1:-1]
    ch = dt / (mu[inner] * dx)
    h, zx = Hz[inner], Hzx[inner]
    plain = h - (dey - dex) * ch
    x = aec * zx - (bec * ch) * dey
    y = P["aer"][1:-1, None] * (h - zx) + (P["ber"][1:-1, None] * ch) * dex
    Hzx[inner] = np.where(layer, x, zx)
    Hz[inner] = np.where(layer, x + y, plain)


class _Hz:
    """The Hz polarisation's methods, shared by the two stand-ins below."""
    polarization = "hz"
    wp2 = gamma = omega0 = None

    @property
    def dispersive(self):
        return self.wp2 is not None

    def reset(self):
        super().reset()
        z = np.zeros_like(self.Ez)
        self.Jx, self.Qx, self.Jy, self.Qy = z, z.copy(), z.copy(), z.copy()
        return self

    # -- where a cell may conduct or carry a pole ------------------------------------------------------------------
    def allowed(self):
        """(R, C) bool: the cells that may have sigma or wp2 non-zero (column C-1 of a periodic member: never read)."""
        g = self.margin()
        ok = np.zeros((self.rows, self.cols), bool)
        if self.boundary == "periodic":
            ok[g:self.rows - 1 - g, :] = True
        else:
            ok[g:self.rows - 1 - g, g:self.cols - 1 - g] = True
        return ok

    def _check(self, s, r0, c0):
        assert np.all(np.isfinite(s)) and np.all(s >= 0)
        full = np.zeros((self.count, self.rows, self.cols))
        full[:, r0:r0 + s.shape[1], c0:c0 + s.shape[2]] = s
        assert not np.any(full[:, ~self.allowed()]), "non-zero where no material update is taken"

    def _full(self, v):
        shape = (self.count, self.rows, self.cols)
        if np.isscalar(v):
            return np.where(self.allowed()[None], float(v), 0.0) * np.ones(shape)
        a = np.array(v, dtype=np.float64)
        assert a.shape == shape
        return a

    def set_conductivity(self, sigma):
        if sigma is None:
            self.sigma = None
            return self
        s = self._full(sigma)
        self._check(s, 0, 0)
        self.sigma = s
        return self

    def set_dispersion(self, wp2, gamma=0.0, omega0=0.0):
        if wp2 is None:
            self.wp2 = self.gamma = self.omega0 = None
            return self
        w = self._full(wp2)
        gam = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.count,)).copy()
        om0 = np.broadcast_to(np.asarray(omega0, dtype=np.float64), (self.count,)).copy()
        assert np.all(np.isfinite(gam)) and np.all(gam >= 0) and np.all(np.isfinite(om0)) and np.all(om0 >= 0)
        assert np.all(np.isfinite(w)) and np.all(w >= 0), "wp2 must be >= 0 and finite"
        self._check(w, 0, 0)
        mu = self.mu.astype(np.float64).reshape(self.count, -1).min(axis=1)[:, None, None]
        s = stability(w, om0[:, None, None], self.eps.astype(np.float64), mu, self.dt, self.dx)
        bad = np.argwhere((w > 0) & ~(s <= 4))
        assert not len(bad), f"member {bad[0][0] if len(bad) else 0}: the pole is unstable"
        self.wp2, self.gamma, self.omega0 = w, gam, om0
        return self

    def download_dispersion(self):
        return self.Jx.copy(), self.Qx.copy(), self.Jy.copy(), self.Qy.copy()

    def upload_dispersion(self, Jh=None, Q=None):
        """BatchEngine.upload_dispersion in the Hz polarisation: Jh = (Jx, Jy), Q = (Qx, Qy)."""
        jx, jy = (None, None) if Jh is None else Jh
        qx, qy = (None, None) if Q is None else Q
        return self.upload_hz_dispersion(jx, qx, jy, qy)

    def upload_hz_dispersion(self, Jx=None, Qx=None, Jy=None, Qy=None):
        for name, a in (("Jx", Jx), ("Qx", Qx), ("Jy", Jy), ("Qy", Qy)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).astype(self.dtype)
        return self

    def _refuse(self, *a, **k):
        raise AssertionError("not available in the Hz polarisation")

    set_conductivity_window = set_dispersion_window = hold_dft_window = dft_window_product = _refuse

    # -- the loop ------------------------------------------------------------------------------------------------
    def _run_member(self, b, nsteps, amps, sums):
        periodic = self.boundary == "periodic"
        Hz, Hzx, Ex, Ey, eps, mu = self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b], self.eps[b], self.mu[b]
        P = self.profiles[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        pole = None
        if self.dispersive:
            a, ck, cj = pole_coefficients(self.wp2[b], self.gamma[b], self.omega0[b], self.dt, self.dx, self.dtype)
            pole = (self.Jx[b], self.Qx[b], self.Jy[b], self.Qy[b], a, ck, cj)
        r, c, nr, nc = (int(v) for v in self.rects[b])
        win, probes = self.win, self.probes
        if sums is not None:
            pr, pc = self.points[0][b][:, 0], self.points[0][b][:, 1]
        for n in range(nsteps):
            hz_e_half(Hz, Ex, Ey, eps, self.dt, self.dx, P, ca, cb, periodic, pole)
            hz_h_half(Hz, Hzx, Ex, Ey, mu, self.dt, self.dx, P, periodic)
            if amps is not None and nr and nc:
                Hz[r:r + nr, c:c + nc] = (Hz[r:r + nr, c:c + nc].astype(np.float64) + amps[n]).astype(Hz.dtype)
            if sums is not None:
                Hz[pr, pc] = (Hz[pr, pc].astype(np.float64) + sums[:, n]).astype(Hz.dtype)
            if periodic:
                Hz[:, -1] = Hz[:, 0]
                Hzx[:, -1] = Hzx[:, 0]
            s = self.step + n + 1
            if win is not None and (s - win["step0"]) % win["every"] == 0:
                r0, c0, wr, wc = win["win"]
                e = Hz[r0:r0 + wr, c0:c0 + wc].astype(np.float64)
                t = float(s) * self.dt
                win["re"][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                win["im"][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
            if probes is not None:
                k = s - 1 - probes["step0"]
                if 0 <= k < probes["trace"].shape[2]:
                    cells = probes["cells"][b]
                    probes["trace"][b, :, k] = Hz[cells[:, 0], cells[:, 1]]


class HzPmlOracle(_Hz, LossyOracle):
    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="pml", device=0,
                 polarization="hz"):
        assert boundary == "pml" and polarization == "hz", "the Hz polarisation needs the layer or periodic columns"
        LossyOracle.__init__(self, count, rows, cols, dt, dx, dtype, "pml")

    def upload_ezx(self, Ezx):
        self.Ezx[...] = np.asarray(Ezx).astype(self.dtype)
        return self

    def download_ezx(self):
        return self.Ezx.copy()


class HzPeriodicOracle(_Hz, PeriodicOracle):
    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="periodic", device=0,
                 polarization="hz"):
        assert polarization == "hz"
        PeriodicOracle.__init__(self, count, rows, cols, dt, dx, dtype, "periodic")

    def set_conductivity(self, sigma):
        return _Hz.set_conductivity(self, sigma)


def oracle_for(boundary):
    return HzPeriodicOracle if boundary == "periodic" else HzPmlOracle
