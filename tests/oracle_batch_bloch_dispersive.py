"""The stand-ins of tests/oracle_batch_bloch_adjoint.py (a Bloch phase) and tests/oracle_batch_lattice.py (the lattice
mode) with one Drude-Lorentz pole per member, restating in NumPy the definition that
include/fdtd2d_batch_bloch_dispersive.h fixes.

The coefficients are ``pole_coefficients`` of tests/oracle_batch_dispersive.py and the update of a cell is its
``pole_update``, applied to the real part and to the imaginary part separately: in every cell that takes the plain update
e = ca*e + (dhy - dhx)*cb of ``bloch_step`` / ``lattice_step``, each part takes

    jn = a*Jh + (cj*e - ck*Q);  Q = Q + jn;  e = ca*e + ((dhy - dhx) - jn)*cb;  Jh = jn

with dhy and dhx as those steps form them (the neighbours across a seam rotated by conj(rho)).  The state is Jh, Q (real
parts) and Jh_i, Q_i (imaginary parts) in the batch dtype.  Like Ez, their images are stored rotated here: column C-1
holds rho * column 0 (lattice: rho_c), row R-1 holds rho_r * row 0.  H, the layer's split update, the PEC rows, the source
and the monitors are those of the stand-ins this one is built on.  No device, no library."""
import numpy as np

from oracle_batch_bloch import rotate, unrotate
from oracle_batch_bloch_adjoint import BlochAdjointOracle
from oracle_batch_dispersive import pole_coefficients, pole_update, stability
from oracle_batch_lattice import LatticeOracle
from oracle_batch_lossy import lossy_coefficients


def bloch_step_dispersive(parts, eps, mu, dt, dx, P, ca, cb, c, s, pole, a, ck, cj, skip_pole=False):
    """oracle_batch_bloch.bloch_step with the pole on the rows outside the layer.  pole = ((Jh, Q) real, (Jh, Q)
    imaginary).  skip_pole leaves the pole block out (what a test must be able to tell apart)."""
    one = np.ones(parts[0][0].shape[1], parts[0][0].dtype)
    ch = dt / (mu[:-1, :-1] * dx)
    for Ez, _, Hx, Hy in parts:
        core = Ez[:-1, :-1]
        Hx[:-1, :] = P["ahr"][:-1, None] * Hx[:-1, :] - (P["bhr"][:-1, None] * ch) * (Ez[1:, :-1] - core)
        Hy[:, :-1] = one[None, :-1] * Hy[:, :-1] + (one[None, :-1] * ch) * (Ez[:-1, 1:] - core)
    ce = dt / (eps[1:-1, :-1] * dx)
    wrap = unrotate(c, s, parts[0][3][1:, -2], parts[1][3][1:, -2])     # conj(rho) * Hy[i, C-2], both parts
    inner = (slice(1, -1), slice(0, -1))
    for (Ez, Ezx, Hx, Hy), w, (Jh, Q) in zip(parts, wrap, pole):
        hy = Hy[1:, :-1]
        left = np.roll(hy, 1, axis=1)
        left[:, 0] = w                                    # column 0's left neighbour, across the seam
        dhy = hy - left
        dhx = Hx[1:-1, :] - Hx[:-2, :]
        e, x = Ez[inner], Ezx[inner]
        if skip_pole:
            plain, jn, qn = ca[inner] * e + (dhy - dhx) * cb[inner], Jh[inner], Q[inner]
        else:
            plain, jn, qn = pole_update(e, dhy - dhx, ca[inner], cb[inner], Jh[inner], Q[inner], a, ck, cj[inner])
        ey = e - x
        ex = one[None, :-1] * x + (one[None, :-1] * ce) * dhy
        ey = P["aer"][1:-1, None] * ey - (P["ber"][1:-1, None] * ce) * dhx
        layer = np.broadcast_to(P["in_r"][1:-1, None], e.shape)
        Ezx[inner] = np.where(layer, ex, x)
        Ez[inner] = np.where(layer, ex + ey, plain)
        Jh[inner] = np.where(layer, Jh[inner], jn)
        Q[inner] = np.where(layer, Q[inner], qn)


def lattice_step_dispersive(parts, mu, dt, dx, ca, cb, rho_r, rho_c, pole, a, ck, cj, skip_pole=False):
    """oracle_batch_lattice.lattice_step with the pole on every cell of the period."""
    ch = dt / (mu[:-1, :-1] * dx)
    for Ez, Hx, Hy in parts:
        core = Ez[:-1, :-1]
        Hx[:-1, :] = Hx[:-1, :] - ch * (Ez[1:, :-1] - core)
        Hy[:, :-1] = Hy[:, :-1] + ch * (Ez[:-1, 1:] - core)
    left = unrotate(rho_c[0], rho_c[1], parts[0][2][:, -2], parts[1][2][:, -2])      # conj(rho_c) * Hy[i, C-2]
    up = unrotate(rho_r[0], rho_r[1], parts[0][1][-2, :], parts[1][1][-2, :])        # conj(rho_r) * Hx[R-2, j]
    inner = (slice(0, -1), slice(0, -1))
    for (Ez, Hx, Hy), lw, uw, (Jh, Q) in zip(parts, left, up, pole):
        hy, hx = Hy[:, :-1], Hx[:-1, :]
        west = np.roll(hy, 1, axis=1)
        west[:, 0] = lw
        north = np.roll(hx, 1, axis=0)
        north[0, :] = uw
        dhy = hy - west
        dhx = hx - north
        if skip_pole:
            Ez[inner] = ca[inner] * Ez[inner] + (dhy - dhx) * cb[inner]
            continue
        Ez[inner], Jh[inner], Q[inner] = pole_update(Ez[inner], dhy - dhx, ca[inner], cb[inner], Jh[inner], Q[inner],
                                                     a, ck, cj[inner])


class _ComplexPole:
    """The pole's methods, shared by the two stand-ins below."""
    wp2 = gamma = omega0 = None
    Jh = Q = Jh_i = Q_i = None
    skip_pole = False         # tests alone: run the steps without the pole block

    @property
    def dispersive(self):
        return self.wp2 is not None

    def _pole_images(self):
        for re, im in ((self.Jh, self.Jh_i), (self.Q, self.Q_i)):
            c, s = (v[:, None] for v in self.rho)
            re[:, :, -1], im[:, :, -1] = rotate(c, s, re[:, :, 0], im[:, :, 0])
            if self.boundary == "lattice":
                c, s = (v[:, None] for v in self.rho_r)
                re[:, -1, :], im[:, -1, :] = rotate(c, s, re[:, 0, :], im[:, 0, :])

    def _check_pole(self, w, r0, c0, omega0):
        assert np.all(np.isfinite(w)) and np.all(w >= 0), "wp2 must be >= 0 and finite"
        self._check(w, r0, c0)                       # non-zero only where a conductivity may be
        eps = self.eps.astype(np.float64)[:, r0:r0 + w.shape[1], c0:c0 + w.shape[2]]
        mu = self.mu.astype(np.float64).reshape(self.count, -1).min(axis=1)[:, None, None]
        s = stability(w, np.asarray(omega0)[:, None, None], eps, mu, self.dt, self.dx)
        assert not np.any((w > 0) & ~(s <= 4)), "the pole is unstable"

    def set_bloch_dispersion(self, wp2, gamma=0.0, omega0=0.0):
        assert self.rho is not None, "needs a Bloch phase or the lattice mode: use set_dispersion"
        if wp2 is None:
            self.wp2 = self.gamma = self.omega0 = None
            self.Jh = self.Q = self.Jh_i = self.Q_i = None
            return self
        assert self.bpoints is None and self.held_b is None, "point sources and the held window exclude the pole"
        shape = (self.count, self.rows, self.cols)
        if np.isscalar(wp2):
            g = self.margin()
            w = np.zeros(shape)
            w[:, g:self.rows - g, :] = wp2
        else:
            w = np.array(wp2, dtype=np.float64)
        assert w.shape == shape
        gam = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.count,)).copy()
        om0 = np.broadcast_to(np.asarray(omega0, dtype=np.float64), (self.count,)).copy()
        assert np.all(np.isfinite(gam)) and np.all(gam >= 0) and np.all(np.isfinite(om0)) and np.all(om0 >= 0)
        self._check_pole(w, 0, 0, om0)
        if self.Jh is None:
            self.Jh, self.Q, self.Jh_i, self.Q_i = (np.zeros(shape, self.dtype) for _ in range(4))
        self.wp2, self.gamma, self.omega0 = w, gam, om0
        return self

    def set_bloch_dispersion_window(self, window, wp2):
        assert self.dispersive, "no pole is set"
        r0, c0, nr, nc = (int(v) for v in window)
        w = np.asarray(wp2, dtype=np.float64)
        assert w.shape == (self.count, nr, nc)
        self._check_pole(w, r0, c0, self.omega0)
        self.wp2[:, r0:r0 + nr, c0:c0 + nc] = w
        return self

    def download_bloch_dispersion(self):
        assert self.dispersive, "no pole is set"
        return self.Jh + 1j * self.Jh_i, self.Q + 1j * self.Q_i

    def upload_bloch_dispersion(self, Jh=None, Q=None):
        assert self.dispersive, "no pole is set"
        for name, a in (("Jh", Jh), ("Q", Q)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).real.astype(self.dtype)
                getattr(self, name + "_i")[...] = np.asarray(a).imag.astype(self.dtype)
        self._pole_images()
        return self

    def reset(self):
        super().reset()
        if self.dispersive:
            for a in (self.Jh, self.Q, self.Jh_i, self.Q_i):
                a[...] = 0
        return self

    def _new_rotations(self):
        if self.dispersive:
            self._pole_images()

    # -- refused while the pole is set ---------------------------------------------------------------------------------
    def _refuse(self, what):
        assert not self.dispersive, f"{what} is not available while a dispersive pole is set"

    def set_dispersion(self, *a, **k):
        raise AssertionError("a dispersive pole is not available with complex fields: use set_bloch_dispersion")

    def set_bloch_point_sources(self, cells, weights=None):
        if cells is not None:
            self._refuse("a point source")
        return super().set_bloch_point_sources(cells, weights)

    def run_bloch_channels(self, *a, **k):
        self._refuse("a run with channels")
        return super().run_bloch_channels(*a, **k)

    def hold_bloch_window(self):
        self._refuse("the held window")
        return super().hold_bloch_window()

    def bloch_window_product(self, coef):
        self._refuse("the window product")
        return super().bloch_window_product(coef)

    # -- the loop: the families' member loops with the dispersive steps -----------------------------------------------
    def _run_pole_member(self, b, nsteps, amps, lattice):
        T = self.dtype.type
        if lattice:
            parts = ((self.Ez[b], self.Hx[b], self.Hy[b]), (self.Ez_i[b], self.Hx_i[b], self.Hy_i[b]))
        else:
            parts = ((self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b]),
                     (self.Ez_i[b], self.Ezx_i[b], self.Hx_i[b], self.Hy_i[b]))
        pole = ((self.Jh[b], self.Q[b]), (self.Jh_i[b], self.Q_i[b]))
        eps, mu = self.eps[b], self.mu[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        a, ck, cj = pole_coefficients(self.wp2[b], self.gamma[b], self.omega0[b], self.dt, self.dx, self.dtype)
        rho_c = (T(self.rho[0][b]), T(self.rho[1][b]))
        rho_r = (T(self.rho_r[0][b]), T(self.rho_r[1][b])) if lattice else None
        r, c0, nr, nc = (int(v) for v in self.rects[b])
        wr, wi = self.weights[b].real[c0:c0 + nc], self.weights[b].imag[c0:c0 + nc]
        win, probes = self.win, self.probes
        er, ei = parts[0][0], parts[1][0]
        rotated = [(er, ei)] + [tuple(pole[k][q] for k in (0, 1)) for q in (0, 1)]      # Ez, Jh, Q
        if not lattice:
            rotated.append((parts[0][1], parts[1][1]))                                   # Ezx
        for n in range(nsteps):
            if lattice:
                lattice_step_dispersive(parts, mu, self.dt, self.dx, ca, cb, rho_r, rho_c, pole, a, ck, cj, self.skip_pole)
            else:
                bloch_step_dispersive(parts, eps, mu, self.dt, self.dx, self.profiles[b], ca, cb, rho_c[0], rho_c[1],
                                      pole, a, ck, cj, self.skip_pole)
            if amps is not None and nr and nc:
                ar, ai = amps[n].real, amps[n].imag
                for Ez, add in zip((er, ei), (ar * wr - ai * wi, ar * wi + ai * wr)):
                    Ez[r:r + nr, c0:c0 + nc] = (Ez[r:r + nr, c0:c0 + nc].astype(np.float64) + add[None, :]).astype(T)
            for re, im in rotated:
                re[:, -1], im[:, -1] = rotate(rho_c[0], rho_c[1], re[:, 0], im[:, 0])
                if lattice:
                    re[-1, :], im[-1, :] = rotate(rho_r[0], rho_r[1], re[0, :], im[0, :])
            st = self.step + n + 1
            if win is not None and (st - win["step0"]) % win["every"] == 0:
                r0, w0, wnr, wnc = win["win"]
                t = float(st) * self.dt
                for Ez, kr, ki in zip((er, ei), ("re", "re_i"), ("im", "im_i")):
                    e = Ez[r0:r0 + wnr, w0:w0 + wnc].astype(np.float64)
                    win[kr][b] += e[None] * np.cos(win["omega"][b] * t)[:, None, None]
                    win[ki][b] += e[None] * (-np.sin(win["omega"][b] * t))[:, None, None]
            if probes is not None:
                k = st - 1 - probes["step0"]
                if 0 <= k < probes["trace"].shape[2]:
                    cells = probes["cells"][b]
                    probes["trace"][b, :, k] = er[cells[:, 0], cells[:, 1]]
                    probes["trace_i"][b, :, k] = ei[cells[:, 0], cells[:, 1]]


class BlochDispersiveOracle(_ComplexPole, BlochAdjointOracle):
    """A periodic batch with a Bloch phase and the pole."""

    def set_bloch_phase(self, phi, rotation=None):
        if phi is None and rotation is None:
            self._refuse("turning the Bloch phase off")
        BlochAdjointOracle.set_bloch_phase(self, phi, rotation)
        self._new_rotations()
        return self

    def _run_bloch_member(self, b, nsteps, amps):
        if not self.dispersive:
            return BlochAdjointOracle._run_bloch_member(self, b, nsteps, amps)
        return self._run_pole_member(b, nsteps, amps, False)


class LatticeDispersiveOracle(_ComplexPole, LatticeOracle):
    """A lattice batch with the pole."""

    def set_lattice_phase(self, phi_rows, phi_cols, rotation=None):
        LatticeOracle.set_lattice_phase(self, phi_rows, phi_cols, rotation)
        self._new_rotations()
        return self

    def _run_lattice_member(self, b, nsteps, amps):
        if not self.dispersive:
            return LatticeOracle._run_lattice_member(self, b, nsteps, amps)
        return self._run_pole_member(b, nsteps, amps, True)
