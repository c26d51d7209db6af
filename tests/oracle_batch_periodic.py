"""The stand-in of tests/oracle_batch_lossy.py with periodic columns, restating in NumPy the definition that
include/fdtd2d_batch_periodic.h fixes.  The period is Q = C - 1 cells and column C-1 is the image of column 0.  One step:

    H      oracle/pml_numpy.step's H half-step for i <= R-2, j <= C-2, with column factors that are exact ones
           (Hy[i, C-2] reads the image column)
    E      for 1 <= i <= R-2, 0 <= j <= C-2: dhy = Hy[i,j] - Hy[i,(j-1) mod Q], dhx = Hx[i,j] - Hx[i-1,j]; rows in the
           layer (i < L or i > R-1-L) take the split update of pml_numpy.step with column factors that are exact ones,
           the others e = ca*e + (dhy - dhx)*cb; rows 0 and R-1 are never updated
    then   the rectangle source, the point sources, Ez[:, C-1] = Ez[:, 0], Ezx[:, C-1] = Ezx[:, 0], the monitors.

The layer is graded on rows alone (set_pml: s_max from the Courant number of cell [0, 0], as pml_numpy.profiles does for
its rows); clear_pml leaves exact ones and no layer rows (PEC top and bottom).  upload and upload_ezx overwrite the image
column with column 0.  Sources and point sources lie in columns 0..C-2; a conductivity may be non-zero in columns
0..C-2 on rows outside the layer and at least 6 rows from the top and bottom edges (column C-1 is accepted and never
read).  No device, no library."""
import numpy as np

from oracle import pml_numpy as pm
from oracle_batch_lossy import LossyOracle, lossy_coefficients


def row_profiles(rows, courant00, L, m=3, R0=1e-6, dtype=np.float64):
    """The four row factor arrays and the layer mask of an L-cell layer on the top and bottom rows."""
    smax = (m + 1) * np.log(1.0 / R0) * courant00 / (4.0 * L)
    se = smax * (pm.depth(rows, L) / L) ** m
    sh = smax * (pm.depth(rows, L, half=True) / L) ** m
    return {"L": L, "aer": ((1 - se) / (1 + se)).astype(dtype), "ber": (1 / (1 + se)).astype(dtype),
            "ahr": ((1 - sh) / (1 + sh)).astype(dtype), "bhr": (1 / (1 + sh)).astype(dtype),
            "in_r": pm.depth(rows, L) > 0}


def no_layer(rows, dtype):
    one = np.ones(rows, dtype)
    return {"L": 0, "aer": one, "ber": one, "ahr": one, "bhr": one, "in_r": np.zeros(rows, bool)}


def periodic_step(Ez, Ezx, Hx, Hy, eps, mu, dt, dx, P, ca, cb):
    """One H -> E step of one member in place, arithmetic in the arrays' dtype; the image column is not yet refreshed."""
    one = np.ones(Ez.shape[1], Ez.dtype)
    ch = dt / (mu[:-1, :-1] * dx)
    core = Ez[:-1, :-1]
    Hx[:-1, :] = P["ahr"][:-1, None] * Hx[:-1, :] - (P["bhr"][:-1, None] * ch) * (Ez[1:, :-1] - core)
    Hy[:, :-1] = one[None, :-1] * Hy[:, :-1] + (one[None, :-1] * ch) * (Ez[:-1, 1:] - core)
    ce = dt / (eps[1:-1, :-1] * dx)
    hy = Hy[1:, :-1]
    dhy = hy - np.roll(hy, 1, axis=1)                 # column 0's left neighbour is column C-2
    dhx = Hx[1:-1, :] - Hx[:-2, :]
    e, x = Ez[1:-1, :-1], Ezx[1:-1, :-1]
    plain = ca[1:-1, :-1] * e + (dhy - dhx) * cb[1:-1, :-1]
    ey = e - x
    ex = one[None, :-1] * x + (one[None, :-1] * ce) * dhy
    ey = P["aer"][1:-1, None] * ey - (P["ber"][1:-1, None] * ce) * dhx
    layer = np.broadcast_to(P["in_r"][1:-1, None], e.shape)
    Ezx[1:-1, :-1] = np.where(layer, ex, x)
    Ez[1:-1, :-1] = np.where(layer, ex + ey, plain)


class PeriodicOracle(LossyOracle):
    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="periodic", device=0):
        assert boundary == "periodic"
        LossyOracle.__init__(self, count, rows, cols, dt, dx, dtype, "pml")
        self.boundary = "periodic"
        self.clear_pml()

    periodic = True

    # -- the layer: rows alone -------------------------------------------------------------------------------------
    def set_pml(self, L=40, m=3, R0=1e-6, courant00=None):
        assert L >= 1 and 2 * L + 3 <= self.rows and self.cols >= 3, "the layer does not fit the rows"
        c = np.broadcast_to(np.asarray(courant00, dtype=np.float64), (self.count,))
        self.profiles = [row_profiles(self.rows, float(v), L, m, R0, self.dtype) for v in c]
        if self.sigma is not None:
            self._check(self.sigma, 0, 0)
        self.Ezx[...] = 0
        return self

    def clear_pml(self):
        self.profiles = [no_layer(self.rows, self.dtype)] * self.count
        self.Ezx[...] = 0
        return self

    # -- what the image column excludes ----------------------------------------------------------------------------
    def margin(self):
        return max(6, self.profiles[0]["L"])

    def _check(self, s, r0, c0):
        g = self.margin()
        assert np.all(np.isfinite(s)) and np.all(s >= 0)
        full = np.zeros((self.count, self.rows, self.cols))
        full[:, r0:r0 + s.shape[1], c0:c0 + s.shape[2]] = s
        barred = np.ones(self.rows, bool)
        barred[g:self.rows - g] = False
        assert not np.any(full[:, barred, :-1]), "sigma is non-zero in a row that takes no plain update"

    def set_conductivity(self, sigma):
        if sigma is not None and np.isscalar(sigma):
            g = self.margin()
            s = np.zeros((self.count, self.rows, self.cols))
            s[:, g:self.rows - g, :] = sigma
            sigma = s
        return LossyOracle.set_conductivity(self, sigma)

    def set_sources(self, rects):
        LossyOracle.set_sources(self, rects)
        r = self.rects
        assert np.all((r[:, 2] == 0) | (r[:, 1] + r[:, 3] <= self.cols - 1)), "a source reaches the image column"
        return self

    def set_point_sources(self, cells, weights=None):
        if cells is not None:
            assert np.all(np.asarray(cells)[..., 1] < self.cols - 1), "a point source lies in the image column"
        return LossyOracle.set_point_sources(self, cells, weights)

    # -- state ---------------------------------------------------------------------------------------------------
    def upload(self, Ez=None, Hx=None, Hy=None):
        LossyOracle.upload(self, Ez, Hx, Hy)
        if Ez is not None:
            self.Ez[:, :, -1] = self.Ez[:, :, 0]
        return self

    def upload_ezx(self, Ezx):
        self.Ezx[...] = np.asarray(Ezx).astype(self.dtype)
        self.Ezx[:, :, -1] = self.Ezx[:, :, 0]
        return self

    def download_ezx(self):
        return self.Ezx.copy()

    # -- the loop ------------------------------------------------------------------------------------------------
    def _run_member(self, b, nsteps, amps, sums):
        Ez, Ezx, Hx, Hy, eps, mu = self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b], self.eps[b], self.mu[b]
        sigma = np.zeros(eps.shape) if self.sigma is None else self.sigma[b]
        ca, cb, _ = lossy_coefficients(eps, sigma, self.dt, self.dx)
        r, c, nr, nc = (int(v) for v in self.rects[b])
        win, probes = self.win, self.probes
        if sums is not None:
            pr, pc = self.points[0][b][:, 0], self.points[0][b][:, 1]
        for n in range(nsteps):
            periodic_step(Ez, Ezx, Hx, Hy, eps, mu, self.dt, self.dx, self.profiles[b], ca, cb)
            if amps is not None and nr and nc:
                Ez[r:r + nr, c:c + nc] = (Ez[r:r + nr, c:c + nc].astype(np.float64) + amps[n]).astype(Ez.dtype)
            if sums is not None:
                Ez[pr, pc] = (Ez[pr, pc].astype(np.float64) + sums[:, n]).astype(Ez.dtype)
            Ez[:, -1] = Ez[:, 0]
            Ezx[:, -1] = Ezx[:, 0]
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
