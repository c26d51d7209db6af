"""An oracle-backed stand-in for the slice of ``BatchEngine`` that ``batch_eps_gradient`` and the point-source tests
use: members advanced one by one with ``oracle/fdtd_numpy.py`` (Mur) or ``oracle/pml_numpy.py`` (PML), the monitors and
the point sources restated in NumPy with the arithmetic that include/fdtd2d_batch_monitor.h and
include/fdtd2d_batch_adjoint.h fix.  No device, no library."""
import numpy as np

from oracle import fdtd_numpy as onp
from oracle import pml_numpy as pm


def point_sums(weights, channels):
    """(P, n): s = 0.0; s = s + w[c] * a[c][n] for c ascending, one float64 rounding per operation."""
    s = np.zeros((weights.shape[0], channels.shape[1]))
    for c in range(weights.shape[1]):
        s = s + weights[:, c, None] * channels[c][None, :]
    return s


def window_product(coef, held, cur):
    """sum_k Re(coef * held * cur) with the operation order of fdtd2d_batch_dft_window_product; held, cur (F, ...)."""
    out = np.zeros(held.shape[1:])
    for k in range(held.shape[0]):
        hr, hi, cr, ci = held[k].real, held[k].imag, cur[k].real, cur[k].imag
        tr = hr * cr - hi * ci
        ti = hr * ci + hi * cr
        out = out + (coef[k].real * tr - coef[k].imag * ti)
    return out


class OracleBatch:
    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="mur", device=0):
        assert boundary in ("mur", "pml")
        self.count, self.rows, self.cols, self.dt, self.dx = count, rows, cols, dt, dx
        self.dtype, self.boundary = np.dtype(dtype), boundary
        self.rects = np.zeros((count, 4), int)
        self.win = self.probes = self.points = self.held = None
        self.profiles = None
        self.reset()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def set_materials(self, eps, mu):
        shape = (self.count, self.rows, self.cols)
        self.eps = np.ascontiguousarray(np.broadcast_to(np.asarray(eps), shape), dtype=self.dtype)
        self.mu = np.ascontiguousarray(np.broadcast_to(np.asarray(mu), shape), dtype=self.dtype)
        return self

    def set_pml(self, L=40, courant00=None):
        c = np.broadcast_to(np.asarray(courant00, dtype=np.float64), (self.count,))
        self.profiles = [pm.profiles(self.rows, self.cols, float(v), L=L, dtype=self.dtype) for v in c]
        return self

    def set_sources(self, rects):
        r = np.asarray(rects)
        self.rects = np.concatenate([r, np.ones_like(r)], axis=1) if r.shape[1] == 2 else r
        return self

    def reset(self):
        B, R, C = self.count, self.rows, self.cols
        self.Ez, self.Ezx = np.zeros((B, R, C), self.dtype), np.zeros((B, R, C), self.dtype)
        self.Hx, self.Hy = np.zeros((B, R, C - 1), self.dtype), np.zeros((B, R - 1, C), self.dtype)
        self.step = 0
        if self.win is not None:
            self.win["re"][...] = 0
            self.win["im"][...] = 0
            self.win["step0"] = 0
        if self.probes is not None:
            self.probes["trace"][...] = 0
            self.probes["step0"] = 0
        return self

    def set_dft_window(self, window, omegas, every=1):
        w = np.asarray(omegas, dtype=np.float64)
        w = np.broadcast_to(w, (self.count, w.shape[-1]))
        r0, c0, nr, nc = (int(v) for v in window)
        z = np.zeros((self.count, w.shape[1], nr, nc))
        self.win = dict(win=(r0, c0, nr, nc), omega=w, every=every, step0=self.step, re=z, im=z.copy())
        self.held = None
        return self

    def set_probes(self, cells, capacity):
        c = np.asarray(cells)
        c = np.broadcast_to(c, (self.count,) + c.shape[-2:])
        self.probes = dict(cells=c, step0=self.step, trace=np.zeros((self.count, c.shape[1], int(capacity))))
        return self

    def set_point_sources(self, cells, weights=None):
        if cells is None:
            self.points = None
            return self
        c = np.asarray(cells)
        w = np.asarray(weights, dtype=np.float64)
        self.points = (np.broadcast_to(c, (self.count,) + c.shape[-2:]),
                       np.broadcast_to(w, (self.count,) + w.shape[-2:]))
        return self

    def run(self, nsteps, amps=None, channels=None):
        sums = None
        if channels is not None:
            ch = np.asarray(channels, dtype=np.float64)
            sums = [point_sums(self.points[1][b], ch[b] if ch.ndim == 3 else ch) for b in range(self.count)]
        for b in range(self.count):
            self._run_member(b, nsteps, None if amps is None else np.asarray(amps, dtype=np.float64)[b],
                             None if sums is None else sums[b])
        self.step += nsteps
        return self

    def _run_member(self, b, nsteps, amps, sums):
        Ez, Ezx, Hx, Hy, eps, mu = self.Ez[b], self.Ezx[b], self.Hx[b], self.Hy[b], self.eps[b], self.mu[b]
        r, c, nr, nc = (int(v) for v in self.rects[b])
        win, probes = self.win, self.probes
        if sums is not None:
            pr, pc = self.points[0][b][:, 0], self.points[0][b][:, 1]
        for n in range(nsteps):
            if self.boundary == "pml":
                pm.step(Ez, Ezx, Hx, Hy, eps, mu, self.dt, self.dx, self.profiles[b])
            else:
                onp.update_h(Ez, Hx, Hy, mu, eps, self.dt, self.dx)
                onp.update_e(Ez, Hx, Hy, mu, eps, self.dt, self.dx)
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

    def read_dft_window(self):
        return self.win["re"] + 1j * self.win["im"]

    def hold_dft_window(self):
        self.held = self.read_dft_window().copy()
        return self

    def dft_window_product(self, coef):
        k = np.asarray(coef, dtype=np.complex128)
        k = np.broadcast_to(k, (self.count, k.shape[-1]))
        cur = self.read_dft_window()
        return np.stack([window_product(k[b], self.held[b], cur[b]) for b in range(self.count)])

    def read_probes(self, first=0, count=None):
        tr = self.probes["trace"]
        return tr[:, :, first:tr.shape[2] if count is None else first + count].copy()

    def download(self):
        return self.Ez.copy(), self.Hx.copy(), self.Hy.copy()
