"""The stand-ins of tests/oracle_batch_dispersive.py with the two calls of include/fdtd2d_batch_dispersive_adjoint.h:
the held window of a member with a pole, in a buffer of its own, and its product with the current window for up to three
coefficient sets, restated in NumPy with the operation order the header fixes.  The parents keep refusing
hold_dft_window and dft_window_product while a pole is set.  No device, no library."""
import numpy as np

from oracle_batch import window_product
from oracle_batch_dispersive import DispersivePeriodicOracle, DispersivePmlOracle


class _HeldPole:
    held_dispersive = None

    def hold_dispersive_window(self):
        assert self.dispersive, "the held dispersive window needs a dispersive pole"
        assert self.win is not None, "no window DFT is set"
        self.held_dispersive = self.read_dft_window().copy()
        return self

    def dispersive_window_product(self, coefs, scales=None):
        assert self.dispersive, "the dispersive window product needs a dispersive pole"
        assert self.held_dispersive is not None, "no held dispersive window"
        k = np.asarray(coefs, dtype=np.complex128)
        if k.ndim == 2:
            k = np.broadcast_to(k[:, None, :], (k.shape[0], self.count, k.shape[1]))
        n = k.shape[0]
        assert 1 <= n <= 3 and k.shape[1:] == (self.count, self.win["omega"].shape[1])
        s = np.ones((self.count, n)) if scales is None else np.asarray(scales, dtype=np.float64)
        s = np.broadcast_to(s, (self.count, n))
        cur = self.read_dft_window()
        return np.stack([np.stack([s[b, c] * window_product(k[c, b], self.held_dispersive[b], cur[b])
                                   for b in range(self.count)]) for c in range(n)])

    # the held window goes with the window and with the pole
    def set_dft_window(self, window, omegas, every=1):
        self.held_dispersive = None
        return super().set_dft_window(window, omegas, every)

    def set_dispersion(self, wp2, gamma=0.0, omega0=0.0):
        if wp2 is None:
            self.held_dispersive = None
        return super().set_dispersion(wp2, gamma, omega0)


class DispersiveAdjointPmlOracle(_HeldPole, DispersivePmlOracle):
    pass


class DispersiveAdjointPeriodicOracle(_HeldPole, DispersivePeriodicOracle):
    pass


def oracle_for(boundary):
    return DispersiveAdjointPeriodicOracle if boundary == "periodic" else DispersiveAdjointPmlOracle
