"""The stand-in of tests/oracle_batch.py (with the session's three methods, tests/test_batch_session_cpu.py) plus an
electric conductivity per cell, restating the arithmetic that include/fdtd2d_batch_lossy.h fixes in NumPy.  Per cell,
with eps as the engine stores it (in its type T):

    s = sigma * dt / (2 * eps) in float64;  ca = (T)((1 - s)/(1 + s));  inv = (T)(1/(1 + s));  cb = ce * inv in T

and the cells that take the reference's plain update take e = ca * e + (dhy - dhx) * cb.  H, the Mur frame (stages B, C,
D of oracle/fdtd_numpy.update_e), the PML branch (oracle/pml_numpy.step), the sources and the monitors are unchanged.
The coefficients are formed from the current eps and sigma at every run, so they are consistent by construction.
boundary "none" (a closed box: stage A alone) is accepted too.  No device, no library."""
import numpy as np

from oracle import fdtd_numpy as onp
from test_batch_session_cpu import SessionOracle


def lossy_coefficients(eps, sigma, dt, dx):
    """(ca, cb, ce) of one member in eps' type."""
    T = eps.dtype
    s = np.asarray(sigma, dtype=np.float64) * dt / (2 * eps.astype(np.float64))
    ca = ((1 - s) / (1 + s)).astype(T)
    inv = (1 / (1 + s)).astype(T)
    ce = dt / (eps * dx)
    return ca, ce * inv, ce


def update_e_lossy(Ez, Hx, Hy, mu, eps, dt, dx, ca, cb, mur=True):
    """oracle/fdtd_numpy.update_e with the lossy stage A; mur False stops after it (boundary "none")."""
    P = Ez.copy()
    b = onp.BAND
    curl = (Hy[1:, 1:-1] - Hy[1:, :-2]) - (Hx[1:-1, 1:] - Hx[:-2, 1:])
    Ez[1:-1, 1:-1] = ca[1:-1, 1:-1] * Ez[1:-1, 1:-1] + curl * cb[1:-1, 1:-1]
    if not mur:
        return Ez
    k = onp.mur_coefficient(mu[0, 0], eps[0, 0], dt, dx)
    left = P[1:-1, 1:b + 1] + k * (Ez[1:-1, 1:b + 1] - P[1:-1, 0:b])
    right = P[1:-1, -b - 1:-1] + k * (Ez[1:-1, -b - 1:-1] - P[1:-1, -b:])
    Ez[1:-1, 0:b] = left
    Ez[1:-1, -b:] = right
    top = P[1:b + 1, 1:-1] + k * (Ez[1:b + 1, 1:-1] - P[0:b, 1:-1])
    bot = P[-b - 1:-1, 1:-1] + k * (Ez[-b - 1:-1, 1:-1] - P[-b:, 1:-1])
    Ez[0:b, 1:-1] = top
    Ez[-b:, 1:-1] = bot
    tl = (Ez[0:b, 1:b + 1] + Ez[1:b + 1, 0:b]) / 2
    tr = (Ez[0:b, -b - 1:-1] + Ez[1:b + 1, -b:]) / 2
    bl = (Ez[-b - 1:-1, 0:b] + Ez[-b:, 1:b + 1]) / 2
    br = (Ez[-b - 1:-1, -b:] + Ez[-b:, -b - 1:-1]) / 2
    Ez[0:b, 0:b] = tl
    Ez[0:b, -b:] = tr
    Ez[-b:, 0:b] = bl
    Ez[-b:, -b:] = br
    return Ez


def pml_step_lossy(Ez, Ezx, Hx, Hy, eps, mu, dt, dx, P, ca, cb):
    """oracle/pml_numpy.step with the lossy plain update outside the layer."""
    ch = dt / (mu[:-1, :-1] * dx)
    core = Ez[:-1, :-1]
    Hx[:-1, :] = P["ahr"][:-1, None] * Hx[:-1, :] - (P["bhr"][:-1, None] * ch) * (Ez[1:, :-1] - core)
    Hy[:, :-1] = P["ahc"][None, :-1] * Hy[:, :-1] + (P["bhc"][None, :-1] * ch) * (Ez[:-1, 1:] - core)
    ce = dt / (eps[1:-1, 1:-1] * dx)
    dhy = Hy[1:, 1:-1] - Hy[1:, :-2]
    dhx = Hx[1:-1, 1:] - Hx[:-2, 1:]
    plain = ca[1:-1, 1:-1] * Ez[1:-1, 1:-1] + (dhy - dhx) * cb[1:-1, 1:-1]
    ey = Ez[1:-1, 1:-1] - Ezx[1:-1, 1:-1]
    ex = P["aec"][None, 1:-1] * Ezx[1:-1, 1:-1] + (P["bec"][None, 1:-1] * ce) * dhy
    ey = P["aer"][1:-1, None] * ey - (P["ber"][1:-1, None] * ce) * dhx
    layer = P["in_r"][1:-1, None] | P["in_c"][None, 1:-1]
    Ezx[1:-1, 1:-1] = np.where(layer, ex, Ezx[1:-1, 1:-1])
    Ez[1:-1, 1:-1] = np.where(layer, ex + ey, plain)


class LossyOracle(SessionOracle):
    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="mur", device=0):
        self.sigma = None
        SessionOracle.__init__(self, count, rows, cols, dt, dx, dtype, "mur" if boundary == "none" else boundary)
        self.boundary = boundary

    @property
    def lossy(self):
        return self.sigma is not None

    def margin(self):
        if self.boundary == "mur":
            return 6
        return max(6, self.profiles[0]["L"]) if self.boundary == "pml" and self.profiles else 1

    def _check(self, s, r0, c0):
        g = self.margin()
        assert np.all(np.isfinite(s)) and np.all(s >= 0)
        full = np.zeros((self.count, self.rows, self.cols))
        full[:, r0:r0 + s.shape[1], c0:c0 + s.shape[2]] = s
        inner = np.zeros((self.rows, self.cols), bool)
        inner[g:self.rows - g, g:self.cols - g] = True
        assert not np.any(full[:, ~inner]), "sigma is non-zero where no plain update is taken"

    def set_conductivity(self, sigma):
        if sigma is None:
            self.sigma = None
            return self
        shape = (self.count, self.rows, self.cols)
        if np.isscalar(sigma):
            g = self.margin()
            s = np.zeros(shape)
            s[:, g:self.rows - g, g:self.cols - g] = sigma
        else:
            s = np.array(sigma, dtype=np.float64)
        assert s.shape == shape
        self._check(s, 0, 0)
        self.sigma = s
        return self

    def set_conductivity_window(self, window, sigma):
        r0, c0, nr, nc = (int(v) for v in window)
        s = np.asarray(sigma, dtype=np.float64)
        assert s.shape == (self.count, nr, nc)
        self._check(s, r0, c0)
        if self.sigma is None:
            self.sigma = np.zeros((self.count, self.rows, self.cols))
        self.sigma[:, r0:r0 + nr, c0:c0 + nc] = s
        return self

    def _run_member(self, b, nsteps, amps, sums):
        if self.sigma is None and self.boundary != "none":
            return SessionOracle._run_member(self, b, nsteps, amps, sums)
        Ez, Ezx, Hx, Hy, eps, mu = self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b], self.eps[b], self.mu[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        r, c, nr, nc = (int(v) for v in self.rects[b])
        win, probes = self.win, self.probes
        if sums is not None:
            pr, pc = self.points[0][b][:, 0], self.points[0][b][:, 1]
        for n in range(nsteps):
            if self.boundary == "pml":
                pml_step_lossy(Ez, Ezx, Hx, Hy, eps, mu, self.dt, self.dx, self.profiles[b], ca, cb)
            else:
                onp.update_h(Ez, Hx, Hy, mu, eps, self.dt, self.dx)
                update_e_lossy(Ez, Hx, Hy, mu, eps, self.dt, self.dx, ca, cb, mur=self.boundary == "mur")
            if amps is not None and nr and nc:
                Ez[r:r + nr, c:c + nc] = (Ez[r:r + nr, c:c + nc].astype(np.float64) + amps[n]).astype(Ez.dtype)
            if sums is not None:
                Ez[pr, pc] = (Ez[pr, pc].astype(np.float64) + sums[:, n]).astype(Ez.dtype)
            s = self.step + n + 1
            if win is not None and (s - win["step0"]) % win["every"] == 0:
                r0, c0, wr, wc = win["win"]
                e = Ez[r0:r0 + wr, c0:c0 + wc].astype(np.float64)
                t = float(s) * self.dt
                win["re"][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                win["im"][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
            if probes is not None:
                k = s - 1 - probes["step0"]
                if 0 <= k < probes["trace"].shape[2]:
                    cells = probes["cells"][b]
                    probes["trace"][b, :, k] = Ez[cells[:, 0], cells[:, 1]]

    def upload(self, Ez=None, Hx=None, Hy=None):
        for name, a in (("Ez", Ez), ("Hx", Hx), ("Hy", Hy)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).astype(self.dtype)
        return self

    def upload_ezx(self, Ezx):
        self.Ezx[...] = np.asarray(Ezx).astype(self.dtype)
        return self
