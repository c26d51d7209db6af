"""The stand-ins of tests/oracle_batch_lossy.py (boundary "pml") and tests/oracle_batch_periodic.py with one
Drude-Lorentz pole per member, restating in NumPy the arithmetic that include/fdtd2d_batch_dispersive.h fixes.

Member b has a damping gamma_b and a resonance omega0_b (rad/s), every cell a strength wp2 (rad^2/s^2).  Formed in
float64 and rounded once to the batch type T:

    g = gamma_b dt / 2;  a_b = (T)((1 - g)/(1 + g));  bq = dt/(1 + g);  ck_b = (T)(bq omega0_b^2 dt)
    cj[i, j] = (T)(dx bq EPS0 wp2[i, j])

and the cells that take the plain update e = ca*e + (dhy - dhx)*cb take instead, every operation rounded to T,

    jn = a*Jh + (cj*e - ck*Q);  Q = Q + jn;  e = ca*e + ((dhy - dhx) - jn)*cb;  Jh = jn

The layer, the PEC rows and the edge leave Jh and Q untouched.  H, the layer's split update, the sources and the monitors
are those of the stand-ins this one is built on.  On a periodic member the image column of Jh and Q repeats column 0.
wp2 may be non-zero where a conductivity may be, and a cell with wp2 > 0 must keep
dt^2 (omega0^2 + wp2 EPS0 / eps) + 8 dt^2 / (eps mu dx^2) <= 4 (mu: the member's smallest).  No device, no library."""
import numpy as np

from oracle_batch_lossy import LossyOracle, lossy_coefficients
from oracle_batch_periodic import PeriodicOracle

EPS0 = 8.85418e-12


def pole_coefficients(wp2, gamma, omega0, dt, dx, dtype):
    """(a, ck, cj) of one member: two scalars and an array of `dtype`."""
    T = np.dtype(dtype).type
    g = float(gamma) * dt / 2
    bq = dt / (1 + g)
    cj = (dx * bq * EPS0 * np.asarray(wp2, dtype=np.float64)).astype(dtype)
    return T((1 - g) / (1 + g)), T(bq * (float(omega0) * float(omega0)) * dt), cj


def stability(wp2, omega0, eps, mu, dt, dx):
    """The left side of the stability bound (at most 4 where wp2 > 0)."""
    return dt * dt * (omega0 * omega0 + wp2 * EPS0 / eps) + 8 * dt * dt / (eps * mu * dx * dx)


def pole_update(e, curl, ca, cb, jh, q, a, ck, cj):
    """(e, Jh, Q) after the dispersive plain update of the cells given."""
    jn = a * jh + (cj * e - ck * q)
    return ca * e + (curl - jn) * cb, jn, q + jn


def pml_step_dispersive(Ez, Ezx, Hx, Hy, eps, mu, dt, dx, P, ca, cb, Jh, Q, a, ck, cj):
    """oracle_batch_lossy.pml_step_lossy with the pole on the cells outside the layer."""
    ch = dt / (mu[:-1, :-1] * dx)
    core = Ez[:-1, :-1]
    Hx[:-1, :] = P["ahr"][:-1, None] * Hx[:-1, :] - (P["bhr"][:-1, None] * ch) * (Ez[1:, :-1] - core)
    Hy[:, :-1] = P["ahc"][None, :-1] * Hy[:, :-1] + (P["bhc"][None, :-1] * ch) * (Ez[:-1, 1:] - core)
    ce = dt / (eps[1:-1, 1:-1] * dx)
    dhy = Hy[1:, 1:-1] - Hy[1:, :-2]
    dhx = Hx[1:-1, 1:] - Hx[:-2, 1:]
    inner = (slice(1, -1), slice(1, -1))
    plain, jn, qn = pole_update(Ez[inner], dhy - dhx, ca[inner], cb[inner], Jh[inner], Q[inner], a, ck, cj[inner])
    ey = Ez[inner] - Ezx[inner]
    ex = P["aec"][None, 1:-1] * Ezx[inner] + (P["bec"][None, 1:-1] * ce) * dhy
    ey = P["aer"][1:-1, None] * ey - (P["ber"][1:-1, None] * ce) * dhx
    layer = P["in_r"][1:-1, None] | P["in_c"][None, 1:-1]
    Ezx[inner] = np.where(layer, ex, Ezx[inner])
    Ez[inner] = np.where(layer, ex + ey, plain)
    Jh[inner] = np.where(layer, Jh[inner], jn)
    Q[inner] = np.where(layer, Q[inner], qn)


def periodic_step_dispersive(Ez, Ezx, Hx, Hy, eps, mu, dt, dx, P, ca, cb, Jh, Q, a, ck, cj):
    """oracle_batch_periodic.periodic_step with the pole on the rows outside the layer; the image column is not yet
    refreshed."""
    one = np.ones(Ez.shape[1], Ez.dtype)
    ch = dt / (mu[:-1, :-1] * dx)
    core = Ez[:-1, :-1]
    Hx[:-1, :] = P["ahr"][:-1, None] * Hx[:-1, :] - (P["bhr"][:-1, None] * ch) * (Ez[1:, :-1] - core)
    Hy[:, :-1] = one[None, :-1] * Hy[:, :-1] + (one[None, :-1] * ch) * (Ez[:-1, 1:] - core)
    ce = dt / (eps[1:-1, :-1] * dx)
    hy = Hy[1:, :-1]
    dhy = hy - np.roll(hy, 1, axis=1)                 # column 0's left neighbour is column C-2
    dhx = Hx[1:-1, :] - Hx[:-2, :]
    inner = (slice(1, -1), slice(0, -1))
    e, x = Ez[inner], Ezx[inner]
    plain, jn, qn = pole_update(e, dhy - dhx, ca[inner], cb[inner], Jh[inner], Q[inner], a, ck, cj[inner])
    ey = e - x
    ex = one[None, :-1] * x + (one[None, :-1] * ce) * dhy
    ey = P["aer"][1:-1, None] * ey - (P["ber"][1:-1, None] * ce) * dhx
    layer = np.broadcast_to(P["in_r"][1:-1, None], e.shape)
    Ezx[inner] = np.where(layer, ex, x)
    Ez[inner] = np.where(layer, ex + ey, plain)
    Jh[inner] = np.where(layer, Jh[inner], jn)
    Q[inner] = np.where(layer, Q[inner], qn)


class _Pole:
    """The pole's methods, shared by the two stand-ins below."""
    wp2 = gamma = omega0 = None

    @property
    def dispersive(self):
        return self.wp2 is not None

    def reset(self):
        super().reset()
        self.Jh, self.Q = np.zeros_like(self.Ez), np.zeros_like(self.Ez)
        return self

    def _check_pole(self, w, r0, c0, omega0):
        assert np.all(np.isfinite(w)) and np.all(w >= 0), "wp2 must be >= 0 and finite"
        self._check(w, r0, c0)                       # non-zero only where a conductivity may be
        eps = self.eps.astype(np.float64)[:, r0:r0 + w.shape[1], c0:c0 + w.shape[2]]
        mu = self.mu.astype(np.float64).reshape(self.count, -1).min(axis=1)[:, None, None]
        s = stability(w, np.asarray(omega0)[:, None, None], eps, mu, self.dt, self.dx)
        assert not np.any((w > 0) & ~(s <= 4)), "the pole is unstable"

    def set_dispersion(self, wp2, gamma=0.0, omega0=0.0):
        if wp2 is None:
            self.wp2 = self.gamma = self.omega0 = None
            return self
        shape = (self.count, self.rows, self.cols)
        if np.isscalar(wp2):
            g = self.margin()
            w = np.zeros(shape)
            if self.boundary == "periodic":
                w[:, g:self.rows - g, :] = wp2
            else:
                w[:, g:self.rows - g, g:self.cols - g] = wp2
        else:
            w = np.array(wp2, dtype=np.float64)
        assert w.shape == shape
        gam = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.count,)).copy()
        om0 = np.broadcast_to(np.asarray(omega0, dtype=np.float64), (self.count,)).copy()
        assert np.all(np.isfinite(gam)) and np.all(gam >= 0) and np.all(np.isfinite(om0)) and np.all(om0 >= 0)
        self._check_pole(w, 0, 0, om0)
        self.wp2, self.gamma, self.omega0 = w, gam, om0
        return self

    def set_dispersion_window(self, window, wp2):
        assert self.dispersive, "no pole is set"
        r0, c0, nr, nc = (int(v) for v in window)
        w = np.asarray(wp2, dtype=np.float64)
        assert w.shape == (self.count, nr, nc)
        self._check_pole(w, r0, c0, self.omega0)
        self.wp2[:, r0:r0 + nr, c0:c0 + nc] = w
        return self

    def download_dispersion(self):
        return self.Jh.copy(), self.Q.copy()

    def upload_dispersion(self, Jh=None, Q=None):
        for name, a in (("Jh", Jh), ("Q", Q)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).astype(self.dtype)
                if self.boundary == "periodic":
                    getattr(self, name)[:, :, -1] = getattr(self, name)[:, :, 0]
        return self

    def _refuse(self, *a, **k):
        raise AssertionError("not available while a dispersive pole is set")

    def hold_dft_window(self):
        return self._refuse() if self.dispersive else super().hold_dft_window()

    def dft_window_product(self, coef):
        return self._refuse() if self.dispersive else super().dft_window_product(coef)

    def _run_member(self, b, nsteps, amps, sums):
        if not self.dispersive:
            return super()._run_member(b, nsteps, amps, sums)
        periodic = self.boundary == "periodic"
        step = periodic_step_dispersive if periodic else pml_step_dispersive
        Ez, Ezx, Hx, Hy, eps, mu = self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b], self.eps[b], self.mu[b]
        Jh, Q = self.Jh[b], self.Q[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        a, ck, cj = pole_coefficients(self.wp2[b], self.gamma[b], self.omega0[b], self.dt, self.dx, self.dtype)
        r, c, nr, nc = (int(v) for v in self.rects[b])
        win, probes = self.win, self.probes
        if sums is not None:
            pr, pc = self.points[0][b][:, 0], self.points[0][b][:, 1]
        for n in range(nsteps):
            step(Ez, Ezx, Hx, Hy, eps, mu, self.dt, self.dx, self.profiles[b], ca, cb, Jh, Q, a, ck, cj)
            if amps is not None and nr and nc:
                Ez[r:r + nr, c:c + nc] = (Ez[r:r + nr, c:c + nc].astype(np.float64) + amps[n]).astype(Ez.dtype)
            if sums is not None:
                Ez[pr, pc] = (Ez[pr, pc].astype(np.float64) + sums[:, n]).astype(Ez.dtype)
            if periodic:
                Ez[:, -1] = Ez[:, 0]
                Ezx[:, -1] = Ezx[:, 0]
                Jh[:, -1] = Jh[:, 0]
                Q[:, -1] = Q[:, 0]
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


class DispersivePmlOracle(_Pole, LossyOracle):
    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="pml", device=0):
        assert boundary == "pml", "a pole needs the layer or periodic columns"
        LossyOracle.__init__(self, count, rows, cols, dt, dx, dtype, "pml")

    def upload_ezx(self, Ezx):
        self.Ezx[...] = np.asarray(Ezx).astype(self.dtype)
        return self

    def download_ezx(self):
        return self.Ezx.copy()


class DispersivePeriodicOracle(_Pole, PeriodicOracle):
    pass


def oracle_for(boundary):
    return DispersivePeriodicOracle if boundary == "periodic" else DispersivePmlOracle
