"""Batched engine: many independent grids of one shape advanced together on one MI355X.

``BatchEngine`` owns one ``fdtd2d_batch`` handle: B members of rows x cols, each with its own materials,
source rectangle, amplitudes and DFT frequency.  Members small enough for one workgroup's LDS run a whole
``run(n)`` in one resident launch; larger ones run one launch per half-step for the whole batch.  Every
member is value-identical to an ``Engine`` run on it.  A thin wrapper over the C ABI, like ``Engine``.
``boundary="pml"`` gives every member the split-field layer of ``Engine(boundary="pml")`` (``set_pml``).
Monitors (``set_dft_window``, ``set_probes``) record a window DFT at up to 16 frequencies and up to 64 point probes
per member inside the step kernels.  Point sources with channels (``set_point_sources``, ``run(channels=...)``) and the
held window (``hold_dft_window``, ``dft_window_product``) are what an adjoint run needs (``adjoint.py``).
``probe_spectra``, ``field_absmax`` and ``set_eps_window`` keep a design loop's traffic on the device
(``AdjointSession``).  ``set_conductivity`` gives every member an electric conductivity per cell (lossy dielectrics,
absorbers, resistive sheets); the batch then runs on the lossy step kernels.
``boundary="periodic"`` makes every member one period of a structure that repeats along its columns (gratings,
metasurface unit cells, photonic-crystal slabs): column C-1 is the image of column 0, rows end in the PML of ``set_pml``
or in PEC (fdtd2d_batch_periodic.h).  ``set_bloch_phase`` gives a periodic batch one Bloch phase per member: the fields
become complex and repeat as F(x + period) = F(x) e^{i phi} (oblique incidence, angle sweeps, band diagrams;
fdtd2d_batch_bloch.h).  ``set_dispersion`` gives a PML or periodic batch one Drude-Lorentz pole per member with a strength
per cell (metals, absorption lines; fdtd2d_batch_dispersive.h); the batch then runs on the dispersive step kernels, and
``hold_dispersive_window`` / ``dispersive_window_product`` are what its adjoint gradients need
(fdtd2d_batch_dispersive_adjoint.h).
``set_bloch_dispersion`` is that pole for a batch with complex fields (a Bloch phase or the lattice mode;
fdtd2d_batch_bloch_dispersive.h): a metal unit cell with one angle of incidence or one k-point per member.
``set_polarization("hz")`` turns a "pml" or "periodic" batch to the other polarisation: Hz with Ex and Ey, the electric field
in the plane, with ``set_conductivity`` and ``set_dispersion`` acting on Ex and Ey (metal strips, wire grids, plasmonic
gratings seen by in-plane E; fdtd2d_batch_hz.h).  ``set_hz_flux_lines`` gives such a batch flux lines: the transforms of Hz
and of the tangential E, and through ``flux()`` the power that crosses each line (fdtd2d_batch_hz_flux.h).
``set_hz_bloch_flux_lines`` gives the batch of ``set_hz_bloch_phase`` (below) those lines under the phase: the power per
k-point, with ``flux_orders`` a metal grating's diffraction efficiencies (fdtd2d_batch_hz_bloch_flux.h).
``set_hz_bloch_phase`` gives a periodic batch in the Hz polarisation one Bloch phase per member: complex Hz, Ex, Ey, Hzx and
pole state, with the conductivity and the pole acting under the phase (Brewster incidence, grating-coupled surface plasmons,
angle sweeps of wire grids; fdtd2d_batch_hz_bloch.h).
``boundary="lattice"`` makes every member the unit cell of a rectangular 2D lattice: row R-1 is the image of row 0 and
column C-1 the image of column 0, the fields are complex, and ``set_lattice_phase`` gives every member one Bloch phase
across each pair of edges (band diagrams of 2D photonic crystals: a k-path is one batch; fdtd2d_batch_lattice.h).
``set_hz_lattice_phase`` gives a periodic batch in the Hz polarisation that lattice mode: the band structure with E in the
plane, with the conductivity and the pole anywhere in the period (metallic crystals; fdtd2d_batch_hz_lattice.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .engine import _BOUNDARY, _code, _host

_KIND = {"none": _abi.SRC_NONE, "ricker": _abi.SRC_RICKER, "sinusoidal": _abi.SRC_SINUSOIDAL}
_ROW_KEYS, _COL_KEYS = ("ahr", "bhr", "aer", "ber"), ("ahc", "bhc", "aec", "bec")


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _window_omegas(omegas, count):
    """(B, F) float64 from (F,) for every member or (B, F)."""
    w = np.asarray(omegas, dtype=np.float64)
    if w.ndim == 1:
        w = np.broadcast_to(w, (count, w.size))
    elif w.ndim != 2 or w.shape[0] != count:
        raise ValueError(f"omegas must have shape (F,) or ({count}, F), got {w.shape}")
    return np.ascontiguousarray(w)


def _probe_cells(cells, count):
    """(B, P, 2) int32 from (P, 2) for every member or (B, P, 2)."""
    c = np.asarray(cells)
    if c.ndim == 2 and c.shape[1] == 2:
        c = np.broadcast_to(c, (count,) + c.shape)
    elif c.ndim != 3 or c.shape[0] != count or c.shape[2] != 2:
        raise ValueError(f"probe cells must have shape (P, 2) or ({count}, P, 2), got {c.shape}")
    if c.size and not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"probe cells must be integers, got {c.dtype}")
    return np.ascontiguousarray(c, dtype=np.int32)


def _flux_lines(lines, omegas, every, count, rows, cols, periodic):
    """The arguments of set_flux_lines, checked on the host as the library would refuse them: ((N, 4) int32 lines as
    {orientation, index, first, count}, (B, F) float64 omegas, every)."""
    lines = list(lines)
    if not 1 <= len(lines) <= _abi.BATCH_MAX_FLUX_LINES:
        raise ValueError(f"flux lines: 1..{_abi.BATCH_MAX_FLUX_LINES} lines, got {len(lines)}")
    out = np.empty((len(lines), 4), np.int32)
    for k, line in enumerate(lines):
        if len(line) != 4 or line[0] not in ("row", "col"):
            raise ValueError(f'flux line {k}: ("row", i, c0, nc) or ("col", j, r0, nr), got {line!r}')
        col = line[0] == "col"
        at, first, n = (int(v) for v in line[1:])
        if not col and not 1 <= at <= rows - 2:
            raise ValueError(f"flux line {k}: row {at} outside 1..{rows - 2}")
        lo = 0 if periodic else 1
        if col and not lo <= at <= cols - 2:
            raise ValueError(f"flux line {k}: column {at} outside {lo}..{cols - 2}"
                             + (f" (column {cols - 1} is the image of column 0)" if periodic else ""))
        extent = rows if col else cols - 1 if periodic else cols
        if n < 1 or first < 0 or first + n > extent:
            raise ValueError(f"flux line {k}: cells [{first}, {first} + {n}) are empty or run past {extent}")
        out[k] = (int(col), at, first, n)
    w = _window_omegas(omegas, count)
    if not 1 <= w.shape[1] <= _abi.BATCH_MAX_FLUX_FREQS:
        raise ValueError(f"flux omegas must hold 1..{_abi.BATCH_MAX_FLUX_FREQS} frequencies, got {w.shape[1]}")
    if not np.all(np.isfinite(w)):
        raise ValueError("flux omegas must be finite")
    if int(every) < 1:
        raise ValueError(f"every must be >= 1, got {every}")
    return out, w, int(every)


def pml_fits(rows, cols, L, periodic=False):
    """Whether an L-cell layer fits a rows x cols member (the rule of fdtd2d_set_pml / fdtd2d_batch_set_pml).
    periodic: the layer of a batch with periodic columns, which lies on rows alone."""
    if periodic:
        return L >= 1 and 2 * L + 3 <= rows and cols >= 3
    return L >= 1 and 2 * L + 3 <= min(rows, cols)


def batch_pml_profiles(count, rows, cols, courant00, L=40, m=3, R0=1e-6, dtype=np.float64):
    """Per-member PML factors as fdtd2d_batch_set_pml takes them: (row_factors (B, 4R) = {ahr, bhr, aer, ber},
    col_factors (B, 4C) = {ahc, bhc, aec, bec}), member b's from pml_profiles(rows, cols, courant00[b], ...).
    courant00: scalar or (B,); members with equal values share one pml_profiles call.  Host only."""
    from .api import pml_profiles
    c = np.broadcast_to(np.asarray(courant00, dtype=np.float64), (count,))
    rowf = np.empty((count, 4 * rows), dtype)
    colf = np.empty((count, 4 * cols), dtype)
    done = {}
    for b, v in enumerate(c):
        v = float(v)
        if v not in done:
            P = pml_profiles(rows, cols, v, L, m, R0, dtype)
            done[v] = (np.concatenate([P[k] for k in _ROW_KEYS]), np.concatenate([P[k] for k in _COL_KEYS]))
        rowf[b], colf[b] = done[v]
    return rowf, colf


class BatchEngine:
    """``count`` grids of rows x cols resident on one MI355X.

    Host arrays are member-major: Ez (B, R, C), Hx (B, R, C-1), Hy (B, R-1, C), eps / mu (B, R, C).
    boundary: "mur" (reference, main.py:29-61), "none", or "pml": the split-field layer of Engine(boundary="pml")
    on every member, set with set_pml() before the first run (the handle is a NONE batch: the layer's outer
    edge is PEC).  "periodic": the columns wrap around with the period C - 1 (column C-1 is the image of column 0 and
    is output only: no source there, materials there are never read, upload() overwrites it with column 0); set_pml()
    lays the layer on the top and bottom rows alone, clear_pml() leaves PEC there.  set_bloch_phase() makes the fields
    complex with one Bloch phase per member.  "lattice": rows and columns both wrap around, with the periods R - 1 and
    C - 1 (row R-1 and column C-1 are images and output only); the fields are complex, set_lattice_phase() sets the two
    Bloch phases of every member (zero until then), there is no layer, and the engine starts with vacuum materials.
    """
    _lattice = None               # ((cr, sr), (cc, sc)): the (B,) rotations of a lattice engine (None: not one)
    _hz = False                   # set_polarization("hz"): Hz with Ex, Ey (fdtd2d_batch_hz.h)
    _hzbflux = False              # set_hz_bloch_flux_lines: the flux lines are those under set_hz_bloch_phase
    _hzb = False                  # set_hz_bloch_phase: _bloch holds the rotations of fdtd2d_batch_hz_bloch.h's phase
    _hzlat = False                # set_hz_lattice_phase: _lattice holds the rotations of fdtd2d_batch_hz_lattice.h's mode

    def __init__(self, count, rows, cols, dt=5e-14, dx=1e-4, dtype=np.float32, boundary="mur", device=0):
        self._lib = _abi.load()
        self._h = C.c_void_p()
        self.count, self.rows, self.cols = int(count), int(rows), int(cols)
        self.dt, self.dx = float(dt), float(dx)
        self.dtype = np.dtype(dtype)
        self.boundary = boundary
        if boundary not in _BOUNDARY and boundary not in ("periodic", "lattice"):
            raise ValueError(f"unknown boundary {boundary!r}")
        self._pml_on = False          # a layer is set
        self._pml_chosen = False      # set_pml (or clear_pml) has been called: a "pml" batch may run
        self._pml_L = 0               # the layer's depth
        self._win = None              # (F, nrows, ncols) of the window DFT
        self._nprobe = 0
        self._flux = None             # ((N, 4) lines, (B, F) omegas) of the flux lines
        self._bflux = False           # they are Bloch lines (set_bloch_flux_lines): complex fields, two parts
        self._hzflux = False          # they are lines of the Hz polarisation (set_hz_flux_lines): Hz and the tangential E
        self._hzbflux = False         # they are lines under set_hz_bloch_phase (set_hz_bloch_flux_lines): two parts of those
        self._npoint = (0, 0)         # (P, K) of the point sources
        self._bloch = None            # (c, s): the (B,) rotations of a Bloch phase
        self._phi = None              # the phases as given (None with rotation=)
        code = _abi.BOUNDARY_NONE if boundary in ("pml", "periodic", "lattice") else _BOUNDARY[boundary]
        rc = self._lib.fdtd2d_batch_create(C.byref(self._h), self.count, self.rows, self.cols, self.dt, self.dx,
                                           _code(dtype), code, int(device))
        if rc != 0:
            msg = self._lib.fdtd2d_batch_last_error(None).decode()
            self._h = C.c_void_p()
            raise _abi.Fdtd2dError(rc, msg)
        if boundary == "periodic":
            try:
                self._ck(self._lib.fdtd2d_batch_set_periodic(self._h, 1))
            except BaseException:
                self.close()
                raise
            self._pml_chosen = True   # without set_pml() the rows end in PEC
        if boundary == "lattice":
            try:
                self.set_materials()  # the lattice mode needs materials: vacuum until set_materials()
                self._ck(self._lib.fdtd2d_batch_set_periodic(self._h, 1))
                self.set_lattice_phase(0.0, 0.0, rotation=((1.0, 0.0), (1.0, 0.0)))
            except BaseException:
                self.close()
                raise
            self._pml_chosen = True

    # -- lifetime -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.fdtd2d_batch_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        return _abi.check_batch(self._h, rc)

    def info(self, what: int) -> int:
        return int(self._lib.fdtd2d_batch_info(self._h, what))

    @property
    def periodic(self) -> bool:
        """Whether the columns are periodic (the batch runs on the periodic kernels)."""
        return bool(self.info(_abi.BATCH_INFO_PERIODIC))

    @property
    def bloch(self) -> bool:
        """Whether a Bloch phase is set (complex fields, the batch runs on the Bloch kernels)."""
        return bool(self.info(_abi.BATCH_INFO_BLOCH))

    @property
    def hz_bloch(self) -> bool:
        """Whether the Bloch phase of the Hz polarisation is set (set_hz_bloch_phase; `bloch` stays False there)."""
        return bool(self.info(_abi.BATCH_HZ_BLOCH_INFO))

    def _bloch_fn(self, name):
        """The entry point `name` of fdtd2d_batch_bloch.h, or on an Hz engine its counterpart of fdtd2d_batch_hz_bloch.h."""
        hz = {"set_bloch_source": "set_hz_bloch_source", "run_bloch": "run_hz_bloch", "transfer_bloch": "transfer_hz_bloch",
              "read_dft_window_bloch": "read_dft_window_hz_bloch", "read_probes_bloch": "read_probes_hz_bloch"}
        return getattr(self._lib, "fdtd2d_batch_" + (hz[name] if self._hzb else name))

    @property
    def lattice(self) -> bool:
        """Whether the lattice mode is on (complex fields, Bloch conditions on both pairs of edges)."""
        return bool(self._lib.fdtd2d_batch_is_lattice(self._h))

    @property
    def hz_lattice(self) -> bool:
        """Whether the lattice mode of the Hz polarisation is on (set_hz_lattice_phase; `lattice`, `bloch` and `hz_bloch`
        stay False there)."""
        return bool(self._lib.fdtd2d_batch_is_hz_lattice(self._h))

    def _no_lattice(self, what):
        """The library's refusal of `what` in the lattice mode, before the call."""
        if self._lattice is not None:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} is not available in the lattice mode (complex fields)")

    def set_lattice_phase(self, phi_rows, phi_cols, rotation=None):
        """The two Bloch phases of every member of a boundary="lattice" engine: F(r + a_rows) = F(r) * exp(1j * phi_rows)
        across the row seam and F(r + a_cols) = F(r) * exp(1j * phi_cols) across the column seam.  Scalars or (B,) in
        radians; the library takes their cos and sin, rounded to the batch dtype.  rotation=((cr, sr), (cc, sc)), scalars
        or (B,), gives those pairs directly, so that exact ones such as (-1, 0) and (0, 1) can be set (the phases are
        then not read).  Fields, monitors and sources are not touched: a k-point sweep is B members that differ in
        their phases alone."""
        if self.boundary != "lattice":
            raise _abi.Fdtd2dError(_abi.E_STATE, f'set_lattice_phase needs boundary="lattice", not {self.boundary!r}')
        self._no_hz("the lattice mode")
        if rotation is not None:
            if len(rotation) != 2 or any(not isinstance(r, (tuple, list)) or len(r) != 2 for r in rotation):
                raise ValueError(f"rotation must be two pairs ((cr, sr), (cc, sc)), got {rotation!r}")
            vals = [np.asarray(v, dtype=np.float64) for r in rotation for v in r]
            names = ("cr", "sr", "cc", "sc")
            ph = None
        else:
            ph = [np.asarray(phi_rows, dtype=np.float64), np.asarray(phi_cols, dtype=np.float64)]
            vals = [np.cos(ph[0]), np.sin(ph[0]), np.cos(ph[1]), np.sin(ph[1])]
            names = ("phi_rows", "phi_rows", "phi_cols", "phi_cols")
        for v, nm in zip(vals if ph is None else (ph[0], ph[0], ph[1], ph[1]), names):
            if v.shape not in ((), (self.count,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({self.count},), got {v.shape}")
        cr, sr, cc, sc = (np.ascontiguousarray(np.broadcast_to(v, (self.count,))) for v in vals)
        self._ck(self._lib.fdtd2d_batch_set_lattice(self._h, _dptr(cr), _dptr(sr), _dptr(cc), _dptr(sc)))
        self._lattice = ((cr, sr), (cc, sc))
        self._bloch = (cc, sc)        # upload, download, run and the monitors then behave as on a Bloch engine
        self._phi = None if ph is None else np.ascontiguousarray(np.broadcast_to(ph[1], (self.count,)))
        return self

    # -- the polarisation (fdtd2d_batch_hz.h) ---------------------------------------------------------------------------
    @property
    def polarization(self) -> str:
        """"ez" (Ez with Hx, Hy: the electric field along the invariant axis) or "hz" (Hz with Ex, Ey)."""
        return "hz" if self._hz else "ez"

    def set_polarization(self, polarization):
        """"hz" turns a boundary="pml" or "periodic" batch to the Hz polarisation, "ez" back; call it right after
        creation (``BatchEngine(..., boundary="periodic").set_polarization("hz")``).  The batch's storage serves both:
        upload / download then carry (Hz, Ex, Ey) of the shapes of (Ez, Hx, Hy), upload_ezx / download_ezx carry Hzx,
        sources, the DFTs and the probes act on Hz, eps[i, j] is the permittivity of Ex[i, j] and Ey[i, j] and mu[i, j]
        the permeability of Hz[i, j].  set_conductivity and set_dispersion then act on Ex and Ey (fdtd2d_batch_hz.h).
        A change zeroes the fields as reset() does.  The library refuses (E_STATE) a change beside a conductivity or a
        pole of the polarisation being left, flux lines or a held window; "mur" and "lattice" batches and a Bloch
        phase of the Ez polarisation have no Hz kernels (the Hz polarisation's own phase is set_hz_bloch_phase, and
        "ez" is refused while it is set).  Not available in the Hz polarisation: the adjoint helpers and sessions,
        set_flux_lines, set_bloch_flux_lines and the line sources (its flux lines are set_hz_flux_lines'), the Ez Bloch
        API, the held window and the window patchers."""
        if polarization not in ("ez", "hz"):
            raise ValueError(f'polarization must be "ez" or "hz", got {polarization!r}')
        if polarization == "hz" and self.boundary not in ("pml", "periodic"):
            raise _abi.Fdtd2dError(_abi.E_STATE, f'the Hz polarisation needs boundary="pml" or "periodic", not '
                                   f'{self.boundary!r}: the Mur frame, a plain box and the lattice mode have no Hz kernels')
        if self._hzb and polarization == "ez":
            self._no_bloch("a change of polarisation (turn the phase of set_hz_bloch_phase off first)")
        if polarization == "hz" and not self._hzb:
            self._no_bloch("the Hz polarisation")
        self._ck(self._lib.fdtd2d_batch_set_polarization(self._h, _abi.POL_HZ if polarization == "hz" else _abi.POL_EZ))
        self._hz = bool(self._lib.fdtd2d_batch_polarization(self._h) == _abi.POL_HZ)
        return self

    def _no_hz(self, what):
        """The library's refusal of `what` in the Hz polarisation, before the call."""
        if self._hz:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} is not available in the Hz polarisation")

    def _no_dispersion(self, what):
        """The library's refusal of `what` while a dispersive pole is set, before the call."""
        if self.dispersive:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} is not available while a dispersive pole is set")

    def _no_bloch(self, what):
        """The library's refusal of `what` while a Bloch phase is set, before the call."""
        self._no_lattice(what)
        if self._bloch is not None:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} is not available while a Bloch phase is set (complex fields)")

    # -- a Bloch phase (fdtd2d_batch_bloch.h) -------------------------------------------------------------------------
    def set_bloch_phase(self, phi, rotation=None):
        """One Bloch phase per member of a periodic batch: F(x + period) = F(x) * exp(1j * phi).  phi: a scalar or (B,)
        in radians; the library takes cos(phi) and sin(phi), rounded to the batch dtype.  rotation=(c, s), scalars or
        (B,), gives those pairs directly, so that exact ones such as (-1, 0) and (0, 1) can be set (phi is then not
        read).  None (and no rotation) turns the phase off: a plain periodic batch again, real parts as they are.
        While a phase is set the fields, the window DFT and the probes are complex (upload, download, download_ezx,
        read_dft_window, read_probes), run() takes complex amps, and set_dft, point sources and channels, the held
        window, probe_spectra, field_absmax and the real adjoint helpers are refused, as are windows and probes touching
        column C-1.  Their complex counterparts are set_bloch_point_sources, run_bloch_channels, hold_bloch_window,
        bloch_window_product, bloch_probe_spectra and bloch_field_absmax (batch_bloch_gradient, BlochAdjointSession)."""
        self._no_lattice("set_bloch_phase (use set_lattice_phase)")
        if phi is None and rotation is None:
            self._ck(self._lib.fdtd2d_batch_set_bloch(self._h, None, None))
            if self._bloch is not None:
                self._npoint = (0, 0)         # the point sources of a Bloch batch go with the phase
            self._bloch = self._phi = None
            return self
        self._no_hz("a Bloch phase")
        if rotation is not None:
            if len(rotation) != 2:
                raise ValueError(f"rotation must be a pair (c, s), got {rotation!r}")
            c, s = (np.asarray(v, dtype=np.float64) for v in rotation)
            ph = None
        else:
            ph = np.asarray(phi, dtype=np.float64)
            c, s = np.cos(ph), np.sin(ph)
        for v, nm in ((c, "c"), (s, "s")) if ph is None else ((ph, "phi"),):
            if v.shape not in ((), (self.count,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({self.count},), got {v.shape}")
        if self.boundary != "periodic":
            raise _abi.Fdtd2dError(_abi.E_STATE, "a Bloch phase needs periodic columns: call fdtd2d_batch_set_periodic "
                                   "first")
        c = np.ascontiguousarray(np.broadcast_to(c, (self.count,)))
        s = np.ascontiguousarray(np.broadcast_to(s, (self.count,)))
        self._ck(self._lib.fdtd2d_batch_set_bloch(self._h, _dptr(c), _dptr(s)))
        self._bloch = (c, s)
        self._phi = None if ph is None else np.ascontiguousarray(np.broadcast_to(ph, (self.count,)))
        return self

    def set_bloch_source(self, weights="ramp"):
        """The complex weight of the rectangle source per column 0..C-2: "ramp" = exp(1j * phi * j / (C - 1)) (a line
        source across the period then launches the obliquely travelling wave; needs set_bloch_phase(phi), not
        rotation=), None = ones, or a complex array (C-1,) for every member or (B, C-1)."""
        Q = self.cols - 1
        if self._bloch is None:
            raise _abi.Fdtd2dError(_abi.E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first")
        if weights is None:
            self._ck(self._bloch_fn("set_bloch_source")(self._h, None, None))
            return self
        if isinstance(weights, str):
            if weights != "ramp":
                raise ValueError(f'weights must be "ramp", None or an array, not {weights!r}')
            if self._phi is None:
                raise ValueError('weights="ramp" needs the phases: call set_bloch_phase(phi) without rotation=')
            w = np.exp(1j * self._phi[:, None] * np.arange(Q)[None, :] / Q)
        else:
            w = np.asarray(weights, dtype=np.complex128)
            if w.shape not in ((Q,), (self.count, Q)):
                raise ValueError(f"weights must have shape ({Q},) or ({self.count}, {Q}), got {w.shape}")
            w = np.broadcast_to(w, (self.count, Q))
        wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
        self._ck(self._bloch_fn("set_bloch_source")(self._h, _dptr(wr), _dptr(wi)))
        return self

    # -- a Bloch phase in the Hz polarisation (fdtd2d_batch_hz_bloch.h) ---------------------------------------------------
    def set_hz_bloch_phase(self, phi, rotation=None):
        """set_bloch_phase for a periodic engine in the Hz polarisation (set_polarization("hz")): one Bloch phase per
        member, the arguments of set_bloch_phase; None (and no rotation) turns it off, real parts as they are.  While it
        is set Hz, Ex, Ey, Hzx, the pole state, the window DFT and the probes are complex (upload, download, upload_ezx,
        download_ezx, download_dispersion, upload_hz_dispersion, read_dft_window, read_probes), run() takes complex
        amps, and set_conductivity, set_dispersion, set_pml, set_materials, set_eps_window and reset keep working.
        Refused while it is set: set_dft, point sources and channels, set_hz_flux_lines (and this call while such lines
        are set; flux lines under the phase are set_hz_bloch_flux_lines', and turning the phase off is refused while
        those are set), set_polarization("ez"), windows and probes touching column C-1, and everything the Hz
        polarisation refuses without it (the Ez Bloch API, the adjoint helpers and sessions)."""
        if not self._hz:
            raise _abi.Fdtd2dError(_abi.E_STATE, 'set_hz_bloch_phase needs the Hz polarisation (set_polarization("hz")): '
                                                 "the Ez polarisation takes set_bloch_phase")
        self._no_lattice("set_hz_bloch_phase (use set_hz_lattice_phase)")
        if phi is None and rotation is None:
            if self._hzbflux:
                raise _abi.Fdtd2dError(_abi.E_STATE, "turning the Bloch phase off is not available while flux lines of the "
                                       "Hz Bloch phase are set: remove them first (set_hz_bloch_flux_lines(None, None))")
            self._ck(self._lib.fdtd2d_batch_set_hz_bloch(self._h, None, None))
            self._bloch = self._phi = None
            self._hzb = False
            return self
        if rotation is not None:
            if len(rotation) != 2:
                raise ValueError(f"rotation must be a pair (c, s), got {rotation!r}")
            c, s = (np.asarray(v, dtype=np.float64) for v in rotation)
            ph = None
        else:
            ph = np.asarray(phi, dtype=np.float64)
            c, s = np.cos(ph), np.sin(ph)
        for v, nm in ((c, "c"), (s, "s")) if ph is None else ((ph, "phi"),):
            if v.shape not in ((), (self.count,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({self.count},), got {v.shape}")
            if not np.all(np.isfinite(v)):
                raise ValueError(f"{nm} must be finite")
        if self.boundary != "periodic":
            raise _abi.Fdtd2dError(_abi.E_STATE, "a Bloch phase needs periodic columns: call fdtd2d_batch_set_periodic "
                                   "first")
        if self._hzflux:
            raise _abi.Fdtd2dError(_abi.E_STATE, "a Bloch phase is not available while flux lines of the Hz polarisation "
                                   "are set: remove them first")
        c = np.ascontiguousarray(np.broadcast_to(c, (self.count,)))
        s = np.ascontiguousarray(np.broadcast_to(s, (self.count,)))
        self._ck(self._lib.fdtd2d_batch_set_hz_bloch(self._h, _dptr(c), _dptr(s)))
        self._bloch = (c, s)
        self._hzb = True
        self._phi = None if ph is None else np.ascontiguousarray(np.broadcast_to(ph, (self.count,)))
        return self

    # -- the lattice mode in the Hz polarisation (fdtd2d_batch_hz_lattice.h) ----------------------------------------------
    def set_hz_lattice_phase(self, phi_rows, phi_cols, rotation=None):
        """The lattice mode of a boundary="periodic" engine in the Hz polarisation (set_polarization("hz")): row R-1
        becomes the image of row 0 as column C-1 is of column 0, the fields are complex and every member takes one Bloch
        phase across each pair of edges, the arguments of set_lattice_phase (scalars or (B,) in radians, or
        rotation=((cr, sr), (cc, sc)) for exact rotations).  None, None turns the mode off: a plain periodic Hz batch
        again, real parts as they are (refused while a conductivity or a pole sits in rows that batch forbids).  A later
        call changes the phases alone.  While the mode is on Hz, Ex, Ey, the pole state, the window DFT and the probes
        are complex (upload, download, download_dispersion, upload_hz_dispersion, read_dft_window, read_probes), run()
        takes complex amps, set_hz_bloch_source("ramp") uses the column phase, and set_conductivity and set_dispersion may
        be non-zero in every cell of the period.  Refused while it is on: a layer, set_hz_bloch_phase, the flux lines of
        either Hz call, set_dft, point sources and channels, set_polarization("ez"), and windows, probes and sources
        touching row R-1 or column C-1."""
        if not self._hz:
            raise _abi.Fdtd2dError(_abi.E_STATE, 'set_hz_lattice_phase needs the Hz polarisation (set_polarization("hz")): '
                                                 'the Ez polarisation takes boundary="lattice" and set_lattice_phase')
        if phi_rows is None and phi_cols is None and rotation is None:
            self._ck(self._lib.fdtd2d_batch_set_hz_lattice(self._h, None, None, None, None))
            if self._hzlat:
                self._lattice = self._bloch = self._phi = None
                self._hzb = self._hzlat = False
            return self
        if rotation is not None:
            if len(rotation) != 2 or any(not isinstance(r, (tuple, list)) or len(r) != 2 for r in rotation):
                raise ValueError(f"rotation must be two pairs ((cr, sr), (cc, sc)), got {rotation!r}")
            vals = [np.asarray(v, dtype=np.float64) for r in rotation for v in r]
            names = ("cr", "sr", "cc", "sc")
            ph = None
        else:
            if phi_rows is None or phi_cols is None:
                raise ValueError("phi_rows and phi_cols must both be given (or both None)")
            ph = [np.asarray(phi_rows, dtype=np.float64), np.asarray(phi_cols, dtype=np.float64)]
            vals = [np.cos(ph[0]), np.sin(ph[0]), np.cos(ph[1]), np.sin(ph[1])]
            names = ("phi_rows", "phi_rows", "phi_cols", "phi_cols")
        for v, nm in zip(vals if ph is None else (ph[0], ph[0], ph[1], ph[1]), names):
            if v.shape not in ((), (self.count,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({self.count},), got {v.shape}")
            if not np.all(np.isfinite(v)):
                raise ValueError(f"{nm} must be finite")
        if self.boundary != "periodic":
            raise _abi.Fdtd2dError(_abi.E_STATE, "the lattice mode of the Hz polarisation needs periodic columns "
                                   f'(boundary="periodic"), not {self.boundary!r}')
        if not self._hzlat:
            if self._pml_on:
                raise _abi.Fdtd2dError(_abi.E_STATE, "the lattice mode of the Hz polarisation has no layer: remove it "
                                       "(clear_pml) first")
            if self._hzb:
                raise _abi.Fdtd2dError(_abi.E_STATE, "the lattice mode of the Hz polarisation is not available while a "
                                       "Bloch phase is set: turn it off first (set_hz_bloch_phase(None))")
            if self._flux is not None:
                raise _abi.Fdtd2dError(_abi.E_STATE, "the lattice mode of the Hz polarisation is not available while flux "
                                       "lines are set: remove them first")
            if self._npoint[0]:
                raise _abi.Fdtd2dError(_abi.E_STATE, "a point source is not available in the lattice mode of the Hz "
                                       "polarisation (remove them)")
        cr, sr, cc, sc = (np.ascontiguousarray(np.broadcast_to(v, (self.count,))) for v in vals)
        self._ck(self._lib.fdtd2d_batch_set_hz_lattice(self._h, _dptr(cr), _dptr(sr), _dptr(cc), _dptr(sc)))
        self._lattice = ((cr, sr), (cc, sc))
        self._bloch = (cc, sc)        # upload, download, run and the monitors then behave as under set_hz_bloch_phase
        self._hzb = self._hzlat = True
        self._phi = None if ph is None else np.ascontiguousarray(np.broadcast_to(ph[1], (self.count,)))
        return self

    def set_hz_bloch_source(self, weights="ramp"):
        """set_bloch_source for the phase of set_hz_bloch_phase: the complex weight of the rectangle source (which adds
        to Hz) per column 0..C-2: "ramp", None = ones, or a complex array (C-1,) or (B, C-1)."""
        if not self._hzb:
            raise _abi.Fdtd2dError(_abi.E_STATE, "no Bloch phase of the Hz polarisation is set: call set_hz_bloch_phase "
                                   "first")
        return self.set_bloch_source(weights)

    def _touches_image(self, what, cols):
        """The library's refusal of a monitor in column C-1 while a Bloch phase is set."""
        if self._lattice is not None:
            return
        if self._bloch is not None and np.any(np.asarray(cols) >= self.cols - 1):
            raise _abi.Fdtd2dError(_abi.E_ARG, f"{what} touches column {self.cols - 1}, the image of column 0: not "
                                   "while a Bloch phase is set")

    def _touches_lattice_image(self, what, rows, cols):
        """The library's refusal of a monitor in row R-1 or column C-1 in the lattice mode."""
        if self._lattice is not None and (np.any(np.asarray(rows) >= self.rows - 1) or
                                          np.any(np.asarray(cols) >= self.cols - 1)):
            raise _abi.Fdtd2dError(_abi.E_ARG, f"{what} touches row {self.rows - 1} or column {self.cols - 1}, the images "
                                   "of row 0 and column 0: not in the lattice mode")

    @property
    def resident(self) -> bool:
        """Whether run() takes the resident path (one launch per run) with the current settings."""
        return bool(self.info(_abi.BATCH_INFO_RESIDENT))

    @property
    def step_count(self) -> int:
        return self.info(_abi.BATCH_INFO_STEP)

    @property
    def launches(self) -> int:
        return self.info(_abi.BATCH_INFO_LAUNCHES)

    @property
    def resident_max_cells(self) -> int:
        return self.info(_abi.BATCH_INFO_RESIDENT_MAX_CELLS)

    @property
    def lds_bytes(self) -> int:
        return self.info(_abi.BATCH_INFO_LDS_BYTES)

    def _shape(self, a, shape, name):
        if a.shape != shape:
            raise ValueError(f"{name} must have shape {shape}, got {a.shape}")

    # -- options --------------------------------------------------------------------
    def set_option(self, resident=None, steps_per_launch=None):
        """resident: -1 / None = by the capacity rule, 0 / False = never.  steps_per_launch: steps per
        resident launch, 0 = the whole run.  Results never depend on them."""
        if resident is not None:
            v = 0 if resident is False or resident == 0 else -1
            self._ck(self._lib.fdtd2d_batch_set_option(self._h, _abi.BATCH_OPT_RESIDENT, v))
        if steps_per_launch is not None:
            self._ck(self._lib.fdtd2d_batch_set_option(self._h, _abi.BATCH_OPT_STEPS_PER_LAUNCH,
                                                       int(steps_per_launch)))
        return self

    def set_stream(self, hip_stream: int | None):
        self._ck(self._lib.fdtd2d_batch_set_stream(self._h, hip_stream))

    # -- materials ------------------------------------------------------------------
    def set_materials(self, eps=None, mu=None):
        """eps, mu: (B, R, C) arrays, scalars, or None for vacuum (material_init(None, ...))."""
        from .api import EPS0, MU0
        eps = EPS0 if eps is None else eps
        mu = MU0 if mu is None else mu
        if np.isscalar(eps) and np.isscalar(mu):
            self._ck(self._lib.fdtd2d_batch_set_materials_uniform(self._h, float(eps), float(mu)))
            return self
        shape = (self.count, self.rows, self.cols)
        e = _host(np.broadcast_to(eps, shape) if np.isscalar(eps) else eps, "eps")
        m = _host(np.broadcast_to(mu, shape) if np.isscalar(mu) else mu, "mu")
        self._shape(e, shape, "eps")
        self._shape(m, shape, "mu")
        if e.dtype != m.dtype:
            m = m.astype(e.dtype)
        self._ck(self._lib.fdtd2d_batch_set_materials(self._h, e.ctypes.data, m.ctypes.data, _code(e.dtype)))
        return self

    # -- the PML (boundary="pml") ------------------------------------------------------
    def set_pml(self, L=40, m=3, R0=1e-6, courant00=None, profiles=None):
        """Give every member the split-field PML (Engine.set_pml per member).  courant00: the Courant number of
        each member's [0,0] material cell, scalar or (B,) (default: vacuum).  profiles: the eight factor arrays
        themselves (ahr bhr aer ber of length rows, ahc bhc aec bec of length cols), each (n,) for every member
        or (B, n), instead of the graded ones.  Ezx starts at zero.  boundary="periodic": the layer lies on the top and
        bottom rows alone (2 L + 3 <= rows), the column factors are exactly 1 (the library refuses others)."""
        self._no_lattice("a PML layer (every edge is periodic)")
        periodic = self.boundary == "periodic"
        if self.boundary != "pml" and not periodic:
            raise _abi.Fdtd2dError(_abi.E_STATE, f'set_pml needs boundary="pml" or "periodic", not {self.boundary!r}')
        if not pml_fits(self.rows, self.cols, int(L), periodic):    # as the library refuses it, before grading anything
            raise _abi.Fdtd2dError(_abi.E_ARG, f"a {int(L)}-cell layer does not fit a {self.rows}x{self.cols} member")
        if profiles is None:
            if courant00 is None:
                from .api import EPS0, MU0
                courant00 = (1 / np.sqrt(EPS0 * MU0) * self.dt) / self.dx
            # periodic: only the rows are graded (columns wide enough for any L give the same row factors)
            rowf, colf = batch_pml_profiles(self.count, self.rows, 2 * int(L) + 3 if periodic else self.cols, courant00,
                                            L, m, R0, self.dtype)
            if periodic:
                colf = np.ones((self.count, 4 * self.cols), self.dtype)
        else:
            def stack(keys, n):
                out = []
                for k in keys:
                    a = np.asarray(profiles[k], dtype=self.dtype)
                    if a.shape not in ((n,), (self.count, n)):
                        raise ValueError(f"PML factor {k} must have shape ({n},) or ({self.count}, {n}), got {a.shape}")
                    out.append(np.broadcast_to(a, (self.count, n)))
                return np.concatenate(out, axis=1)
            rowf, colf = stack(_ROW_KEYS, self.rows), stack(_COL_KEYS, self.cols)
        rowf, colf = np.ascontiguousarray(rowf), np.ascontiguousarray(colf)
        self._ck(self._lib.fdtd2d_batch_set_pml(self._h, rowf.ctypes.data, colf.ctypes.data, _code(self.dtype),
                                                int(L)))
        self._pml_on = self._pml_chosen = True
        self._pml_L = int(L)
        return self

    def clear_pml(self):
        """Remove the layer (and Ezx): the batch then runs as boundary="none"; a periodic batch keeps its periodic
        columns and ends in PEC at the top and bottom rows."""
        if self.boundary not in ("pml", "periodic"):
            raise _abi.Fdtd2dError(_abi.E_STATE, f'clear_pml needs boundary="pml" or "periodic", not {self.boundary!r}')
        self._ck(self._lib.fdtd2d_batch_set_pml(self._h, None, None, _code(self.dtype), 0))
        self._pml_on, self._pml_chosen, self._pml_L = False, True, 0
        return self

    @property
    def pml(self) -> bool:
        """Whether a layer is set."""
        return self._pml_on

    def upload_ezx(self, Ezx):
        """(B, R, C) split field, host -> device (needs a layer)."""
        self._no_lattice("upload_ezx (there is no Ezx)")
        z = np.asarray(Ezx)
        if np.iscomplexobj(z) and self._bloch is None:
            raise ValueError("complex fields need a Bloch phase (set_bloch_phase)")
        a = np.ascontiguousarray(z.real, dtype=self.dtype)
        self._shape(a, (self.count, self.rows, self.cols), "Ezx")
        self._ck(self._lib.fdtd2d_batch_transfer_ezx(self._h, a.ctypes.data, _code(a.dtype), 1))
        if self._bloch is not None:
            i = np.ascontiguousarray(z.imag, dtype=self.dtype)
            self._ck(self._bloch_fn("transfer_bloch")(self._h, None, None, None, i.ctypes.data, _code(i.dtype), 1))
        return self

    def download_ezx(self):
        """(B, R, C) split field, device -> host (needs a layer)."""
        self._no_lattice("download_ezx (there is no Ezx)")
        a = np.empty((self.count, self.rows, self.cols), self.dtype)
        self._ck(self._lib.fdtd2d_batch_transfer_ezx(self._h, a.ctypes.data, _code(a.dtype), 0))
        if self._bloch is not None:
            i = np.empty_like(a)
            self._ck(self._bloch_fn("transfer_bloch")(self._h, None, None, None, i.ctypes.data, _code(i.dtype), 0))
            return a + 1j * i
        return a

    def _need_pml(self):
        if self.boundary == "pml" and not self._pml_chosen:
            raise _abi.Fdtd2dError(_abi.E_STATE, 'boundary="pml": call set_pml() before running')

    def courant(self) -> np.ndarray:
        out = np.empty(self.count, np.float64)
        self._ck(self._lib.fdtd2d_batch_courant(self._h, _dptr(out)))
        return out

    # -- field transfer -------------------------------------------------------------
    def _field_shapes(self):
        B, R, Cc = self.count, self.rows, self.cols
        return (B, R, Cc), (B, R, Cc - 1), (B, R - 1, Cc)

    def upload(self, Ez=None, Hx=None, Hy=None):
        """Host -> device, any float dtype; a field given as None is left as is.  With a Bloch phase the fields may be
        complex (a real array has a zero imaginary part).  In the Hz polarisation the three slots are (Hz, Ex, Ey):
        Hz (B, R, C), Ex (B, R, C-1), Ey (B, R-1, C), the physical fields with no hidden sign."""
        if any(a is not None and np.iscomplexobj(a) for a in (Ez, Hx, Hy)) and self._bloch is None:
            raise ValueError("complex fields need a Bloch phase (set_bloch_phase)")
        if self._bloch is not None:
            given = [None if a is None else np.asarray(a) for a in (Ez, Hx, Hy)]
            for a, shp, nm in zip(given, self._field_shapes(), ("Ez", "Hx", "Hy")):
                if a is not None:
                    self._shape(a, shp, nm)
            im = [None if a is None else np.ascontiguousarray(a.imag, dtype=np.float64) for a in given]
            Ez, Hx, Hy = (None if a is None else np.ascontiguousarray(a.real) for a in given)
            if any(a is not None for a in im):
                ptr = [None if a is None else a.ctypes.data for a in im]
                self._ck(self._bloch_fn("transfer_bloch")(self._h, ptr[0], ptr[1], ptr[2], None, _abi.F64, 1))
        arrs, code = [], None
        for a, shp, nm in zip((Ez, Hx, Hy), self._field_shapes(), ("Ez", "Hx", "Hy")):
            if a is None:
                arrs.append(None)
                continue
            a = _host(a, nm)
            self._shape(a, shp, nm)
            if code is None:
                code = _code(a.dtype)
            elif _code(a.dtype) != code:
                a = a.astype(np.float64 if code == _abi.F64 else np.float32)
            arrs.append(a)
        if code is None:
            return self
        ptr = [None if a is None else a.ctypes.data for a in arrs]
        self._ck(self._lib.fdtd2d_batch_upload(self._h, ptr[0], ptr[1], ptr[2], code))
        return self

    def download(self, dtype=None):
        """Device -> host: new arrays (Ez, Hx, Hy) of the engine dtype (or `dtype`); complex ones with a Bloch phase,
        the image column of Ez then rotated by the member's phase.  In the Hz polarisation the three are (Hz, Ex, Ey)."""
        dt = self.dtype if dtype is None else np.dtype(dtype)
        out = [np.empty(s, dt) for s in self._field_shapes()]
        self._ck(self._lib.fdtd2d_batch_download(self._h, *(a.ctypes.data for a in out), _code(dt)))
        if self._bloch is not None:
            im = [np.empty(s, dt) for s in self._field_shapes()]
            self._ck(self._bloch_fn("transfer_bloch")(self._h, *(a.ctypes.data for a in im), None, _code(dt), 0))
            return tuple(a + 1j * b for a, b in zip(out, im))
        return tuple(out)

    def reset(self):
        self._ck(self._lib.fdtd2d_batch_reset(self._h))
        return self

    # -- sources and the loop ---------------------------------------------------------
    def set_sources(self, rects):
        """rects: (B, 2) {row, col} one-cell sources or (B, 4) {row, col, nrows, ncols} rectangles
        (0 x 0 = no source for that member)."""
        r = np.asarray(rects)
        if r.ndim != 2 or r.shape[0] != self.count or r.shape[1] not in (2, 4):
            raise ValueError(f"rects must have shape ({self.count}, 2) or ({self.count}, 4), got {r.shape}")
        if r.shape[1] == 2:
            r = np.concatenate([r, np.ones_like(r)], axis=1)
        r = np.ascontiguousarray(r, dtype=np.int32)
        self._ck(self._lib.fdtd2d_batch_set_sources(self._h, r.ctypes.data_as(C.POINTER(C.c_int))))
        return self

    def run(self, nsteps, amps=None, channels=None):
        """nsteps of H -> E -> source for every member.  amps: (B, nsteps) float64 (None = no source).
        channels: (K, nsteps) for every member or (B, K, nsteps) float64, the time series of set_point_sources;
        without them the point sources stay silent."""
        nsteps = int(nsteps)
        self._need_pml()
        a = ai = None
        if amps is not None and np.iscomplexobj(amps):
            if self._bloch is None:
                raise ValueError("complex amps need a Bloch phase (set_bloch_phase)")
            ai = np.asarray(amps).imag
            amps = np.asarray(amps).real
        if amps is not None:
            a = np.asarray(amps, dtype=np.float64)
            if a.ndim != 2 or a.shape[0] != self.count or a.shape[1] < nsteps:
                raise ValueError(f"amps must have shape ({self.count}, {nsteps}), got {a.shape}")
            a = np.ascontiguousarray(a[:, :nsteps])
        if channels is not None:
            self._no_bloch("a run with channels")
        if ai is not None:
            ai = np.ascontiguousarray(ai[:, :nsteps], dtype=np.float64)
            self._ck(self._bloch_fn("run_bloch")(self._h, nsteps, _dptr(a), _dptr(ai)))
            return self
        if channels is None:
            self._ck(self._lib.fdtd2d_batch_run(self._h, nsteps, None if a is None else _dptr(a)))
            return self
        ch = np.asarray(channels, dtype=np.float64)
        K = self._npoint[1] or self.info(_abi.BATCH_FLUX_LINE_SOURCES_INFO)   # line sources take the same channels
        if ch.shape[-1:] != () and ch.shape[-1] >= nsteps:
            ch = ch[..., :nsteps]
        if ch.shape not in ((K, nsteps), (self.count, K, nsteps)):
            raise ValueError(f"channels must have shape ({K}, {nsteps}) or ({self.count}, {K}, {nsteps}), "
                             f"got {ch.shape}")
        ch = np.ascontiguousarray(ch)
        self._ck(self._lib.fdtd2d_batch_run_channels(self._h, nsteps, None if a is None else _dptr(a), _dptr(ch),
                                                     int(ch.ndim == 3)))
        return self

    # -- point sources and the held window (fdtd2d_batch_adjoint.h) ---------------------------------
    def set_point_sources(self, cells, weights=None):
        """Up to 64 point cells per member, each adding sum_c weights[p, c] * channels[c, n] to Ez after the
        rectangle source of step n of a run(channels=...): cells (P, 2) {row, col} for every member or (B, P, 2),
        weights (P, K) or (B, P, K) float64, K <= 32.  cells None removes them."""
        if cells is None:
            self._ck(self._lib.fdtd2d_batch_set_point_sources(self._h, 0, None, 0, None))
            self._npoint = (0, 0)
            return self
        self._no_bloch("a point source")
        c = _probe_cells(cells, self.count)
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim == 2:
            w = np.broadcast_to(w, (self.count,) + w.shape)
        if w.ndim != 3 or w.shape[:2] != c.shape[:2]:
            raise ValueError(f"weights must have shape ({c.shape[1]}, K) or ({self.count}, {c.shape[1]}, K), "
                             f"got {np.shape(weights)}")
        w = np.ascontiguousarray(w)
        self._ck(self._lib.fdtd2d_batch_set_point_sources(self._h, int(c.shape[1]), c.ctypes.data_as(C.POINTER(C.c_int)),
                                                          int(w.shape[2]), _dptr(w)))
        self._npoint = (int(c.shape[1]), int(w.shape[2]))
        return self

    def hold_dft_window(self):
        """Keep a device copy of the window DFT as it is now; it survives reset() and further runs."""
        self._no_hz("the held window (the adjoint)")
        self._no_bloch("the held window")
        self._no_dispersion("the held window (the adjoint of a dispersive medium)")
        self._ck(self._lib.fdtd2d_batch_hold_dft_window(self._h))
        return self

    def dft_window_product(self, coef) -> np.ndarray:
        """float64 (B, nrows, ncols): sum_k Re(coef[b, k] * held[b, k] * current[b, k]) over the window, on the device.
        coef: complex (F,) for every member or (B, F)."""
        self._no_hz("the window product (the adjoint)")
        self._no_bloch("the window product")
        self._no_dispersion("the window product (the adjoint of a dispersive medium)")
        f, nr, nc = self._win or (0, 1, 1)
        k = np.asarray(coef, dtype=np.complex128)
        if k.ndim == 1:
            k = np.broadcast_to(k, (self.count, k.size))
        if self._win is not None and k.shape != (self.count, f):
            raise ValueError(f"coef must have shape ({f},) or ({self.count}, {f}), got {np.shape(coef)}")
        re, im = np.ascontiguousarray(k.real), np.ascontiguousarray(k.imag)
        out = np.empty((self.count, nr, nc))
        self._ck(self._lib.fdtd2d_batch_dft_window_product(self._h, _dptr(re), _dptr(im), _dptr(out)))
        return out

    # -- the same for a batch with a dispersive pole (fdtd2d_batch_dispersive_adjoint.h) ----------------------------
    def _need_dispersion(self, what, plain):
        """The library's refusals of a dispersive adjoint call, before the call."""
        if getattr(self, "_hz", False):
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} is not available in the Hz polarisation")
        self._no_bloch(what)
        if not self.dispersive:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} needs a dispersive pole (fdtd2d_batch_set_dispersion): a batch "
                                   f"without one takes {plain}")

    def hold_dispersive_window(self):
        """hold_dft_window for a batch with a dispersive pole: a device copy of the window DFT in a buffer of its own
        (hold_dft_window keeps refusing such a batch).  It survives reset(), set_point_sources and further runs, and
        goes with the window or the pole."""
        self._need_dispersion("the held dispersive window", "fdtd2d_batch_hold_dft_window")
        self._ck(self._lib.fdtd2d_batch_hold_dispersive_window(self._h))
        return self

    def dispersive_window_product(self, coefs, scales=None) -> np.ndarray:
        """float64 (ncoef, B, nrows, ncols): scales[b, c] * sum_k Re(coefs[c, b, k] * held[b, k] * current[b, k]) over the
        window for ncoef = 1..3 coefficient sets, in one pass over the two windows, one launch and one read-back.
        coefs: complex (ncoef, F) for every member or (ncoef, B, F); scales: None (ones), (ncoef,) or (B, ncoef).  With
        one set and no scales it is dft_window_product's arithmetic bit for bit."""
        self._need_dispersion("the dispersive window product", "fdtd2d_batch_dft_window_product")
        f, nr, nc = self._win or (0, 1, 1)
        k = np.asarray(coefs, dtype=np.complex128)
        if k.ndim == 2:
            k = np.broadcast_to(k[:, None, :], (k.shape[0], self.count, k.shape[1]))
        if k.ndim != 3 or not 1 <= k.shape[0] <= _abi.BATCH_MAX_PRODUCT_SETS or \
                (self._win is not None and k.shape[1:] != (self.count, f)):
            raise ValueError(f"coefs must have shape (ncoef, {f}) or (ncoef, {self.count}, {f}) with ncoef in 1.."
                             f"{_abi.BATCH_MAX_PRODUCT_SETS}, got {np.shape(coefs)}")
        n = int(k.shape[0])
        s = np.ones((self.count, n)) if scales is None else np.asarray(scales, dtype=np.float64)
        if s.shape == (n,):
            s = np.broadcast_to(s, (self.count, n))
        if s.shape != (self.count, n):
            raise ValueError(f"scales must have shape ({n},) or ({self.count}, {n}), got {np.shape(scales)}")
        re, im, s = np.ascontiguousarray(k.real), np.ascontiguousarray(k.imag), np.ascontiguousarray(s)
        out = np.empty((n, self.count, nr, nc))
        self._ck(self._lib.fdtd2d_batch_dispersive_window_product(self._h, n, _dptr(re), _dptr(im), _dptr(s), _dptr(out)))
        return out

    # -- the same for a Bloch batch (fdtd2d_batch_bloch_adjoint.h) -----------------------------------------------------
    def _need_bloch(self):
        """The library's refusal of a Bloch call without a phase, before the call."""
        self._no_hz("the Bloch API")
        if self._bloch is None:
            raise _abi.Fdtd2dError(_abi.E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first")

    def set_bloch_point_sources(self, cells, weights=None):
        """set_point_sources for a Bloch batch: each cell adds the real sum_c weights[p, c] * channels[c, n] to the real
        part of Ez after the rectangle source of step n of a run_bloch_channels (the imaginary part takes nothing; the
        seam carries the series into it).  Cells lie in columns 0..C-2; cells None removes them, and so does turning
        the phase off."""
        self._no_lattice("a point source")
        self._need_bloch()
        if cells is None:
            self._ck(self._lib.fdtd2d_batch_set_bloch_point_sources(self._h, 0, None, 0, None))
            self._npoint = (0, 0)
            return self
        c = _probe_cells(cells, self.count)
        if np.any(c[..., 1] >= self.cols - 1):
            b = int(np.nonzero((c[..., 1] >= self.cols - 1).any(axis=1))[0][0])
            raise _abi.Fdtd2dError(_abi.E_ARG, f"member {b}: a point source lies in column {self.cols - 1}, the image "
                                   "of column 0 of a periodic batch")
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim == 2:
            w = np.broadcast_to(w, (self.count,) + w.shape)
        if w.ndim != 3 or w.shape[:2] != c.shape[:2]:
            raise ValueError(f"weights must have shape ({c.shape[1]}, K) or ({self.count}, {c.shape[1]}, K), "
                             f"got {np.shape(weights)}")
        w = np.ascontiguousarray(w)
        self._ck(self._lib.fdtd2d_batch_set_bloch_point_sources(self._h, int(c.shape[1]),
                                                                c.ctypes.data_as(C.POINTER(C.c_int)), int(w.shape[2]),
                                                                _dptr(w)))
        self._npoint = (int(c.shape[1]), int(w.shape[2]))
        return self

    def run_bloch_channels(self, nsteps, amps=None, channels=None, conjugate=False):
        """run() of a Bloch batch with the point sources of set_bloch_point_sources: amps (B, nsteps) real or complex
        (None = no rectangle source), channels (K, nsteps) for every member or (B, K, nsteps) float64.  conjugate True
        steps with the rotation conj(rho) = (c, -s): the transpose of the one-step operator, what an adjoint run needs;
        downloads after it rotate the image column by that rotation."""
        nsteps = int(nsteps)
        self._no_lattice("a run with channels")
        self._need_bloch()
        self._need_pml()
        a = ai = None
        if amps is not None:
            z = np.asarray(amps)
            if z.ndim != 2 or z.shape[0] != self.count or z.shape[1] < nsteps:
                raise ValueError(f"amps must have shape ({self.count}, {nsteps}), got {z.shape}")
            a = np.ascontiguousarray(z.real[:, :nsteps], dtype=np.float64)
            if np.iscomplexobj(z):
                ai = np.ascontiguousarray(z.imag[:, :nsteps], dtype=np.float64)
        ch = np.asarray(channels, dtype=np.float64)
        # the line sources of set_bloch_flux_line_sources take the channels where Bloch lines exclude point sources
        K = self._npoint[1] or (self.info(_abi.BATCH_FLUX_LINE_SOURCES_INFO) if self._bflux else 0)
        if ch.shape[-1:] != () and ch.shape[-1] >= nsteps:
            ch = ch[..., :nsteps]
        if ch.shape not in ((K, nsteps), (self.count, K, nsteps)):
            raise ValueError(f"channels must have shape ({K}, {nsteps}) or ({self.count}, {K}, {nsteps}), "
                             f"got {ch.shape}")
        ch = np.ascontiguousarray(ch)
        self._ck(self._lib.fdtd2d_batch_run_bloch_channels(self._h, nsteps, None if a is None else _dptr(a),
                                                           None if ai is None else _dptr(ai), _dptr(ch),
                                                           int(ch.ndim == 3), int(bool(conjugate))))
        return self

    def hold_bloch_window(self):
        """hold_dft_window for a Bloch batch: a device copy of both parts of the window DFT."""
        self._no_lattice("the held window")
        self._need_bloch()
        self._ck(self._lib.fdtd2d_batch_hold_bloch_window(self._h))
        return self

    def bloch_window_product(self, coef) -> np.ndarray:
        """float64 (B, nrows, ncols): sum_k Re(coef[b, k] * held[b, k] * current[b, k]) of the complex windows
        W(re) + 1j * W(im), on the device; the plain product, nothing conjugated.  coef: complex (F,) or (B, F)."""
        self._no_lattice("the window product")
        self._need_bloch()
        f, nr, nc = self._win or (0, 1, 1)
        k = np.asarray(coef, dtype=np.complex128)
        if k.ndim == 1:
            k = np.broadcast_to(k, (self.count, k.size))
        if self._win is not None and k.shape != (self.count, f):
            raise ValueError(f"coef must have shape ({f},) or ({self.count}, {f}), got {np.shape(coef)}")
        re, im = np.ascontiguousarray(k.real), np.ascontiguousarray(k.imag)
        out = np.empty((self.count, nr, nc))
        self._ck(self._lib.fdtd2d_batch_bloch_window_product(self._h, _dptr(re), _dptr(im), _dptr(out)))
        return out

    def bloch_probe_spectra(self, omegas, first=0, count=None, peak=False):
        """probe_spectra of the complex traces of a Bloch batch: complex128 (B, P, F).  peak True: also float64 (B,), the
        larger of the largest |real sample| and the largest |imaginary sample| of each member in the range."""
        self._need_bloch()
        w = _window_omegas(omegas, self.count)
        if count is None:
            count = max(0, self.probe_samples - int(first))
        F = int(w.shape[1])
        re, im = np.empty((self.count, self._nprobe, F)), np.empty((self.count, self._nprobe, F))
        pk = np.empty(self.count) if peak else None
        buf = (re, im) if re.size else (np.empty(1), np.empty(1))    # a refused call still passes valid pointers
        self._ck(self._lib.fdtd2d_batch_bloch_probe_spectra(self._h, F, _dptr(w) if F else None, int(first), int(count),
                                                            _dptr(buf[0]) if F else None, _dptr(buf[1]) if F else None,
                                                            None if pk is None else _dptr(pk)))
        out = re + 1j * im
        return (out, pk) if peak else out

    def bloch_field_absmax(self, which="Ez"):
        """float64 (B,): max(max |Re field|, max |Im field|) over each member's cells, reduced on the device; of Ez over
        columns 0..C-2 (the image column repeats column 0, rotated).  which "Ez", "Hx" or "Hy"."""
        codes = {"Ez": _abi.FIELD_EZ, "Hx": _abi.FIELD_HX, "Hy": _abi.FIELD_HY}
        if which not in codes:
            raise ValueError(f'which must be "Ez", "Hx" or "Hy", not {which!r}')
        self._need_bloch()
        out = np.empty(self.count)
        self._ck(self._lib.fdtd2d_batch_bloch_field_absmax(self._h, codes[which], _dptr(out)))
        return out

    def run_waveform(self, nsteps, kind="ricker", fc=30e9, step0=0):
        """run() with the waveform evaluated by the library at t = (step0 + n) * dt; fc scalar or (B,)."""
        self._need_pml()
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(fc, dtype=np.float64), (self.count,)))
        self._ck(self._lib.fdtd2d_batch_run_waveform(self._h, int(nsteps), _KIND[kind], _dptr(f), int(step0)))
        return self

    def set_dft(self, omega, every=1):
        """Running Fourier transform of the whole grid at one angular frequency per member (scalar or (B,));
        None removes it."""
        if omega is None:
            self._ck(self._lib.fdtd2d_batch_set_dft(self._h, None, 0))
            return self
        self._no_bloch("the whole-grid transform (use fdtd2d_batch_set_dft_window)")
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(omega, dtype=np.float64), (self.count,)))
        self._ck(self._lib.fdtd2d_batch_set_dft(self._h, _dptr(w), int(every)))
        return self

    def read_dft(self) -> np.ndarray:
        """complex128 (B, R, C): sum of Ez * exp(-i omega n dt) over the sampled steps."""
        shape = (self.count, self.rows, self.cols)
        re, im = np.empty(shape), np.empty(shape)
        self._ck(self._lib.fdtd2d_batch_read_dft(self._h, _dptr(re), _dptr(im)))
        return re + 1j * im

    # -- monitors (fdtd2d_batch_monitor.h) ----------------------------------------------------------
    def set_dft_window(self, window, omegas, every=1):
        """Running Fourier transform of Ez over window = (row0, col0, nrows, ncols), shared by all members, at up to
        16 angular frequencies per member: omegas (F,) for every member or (B, F).  After every `every`-th step n
        (counted from this call) adds Ez * exp(-1j * omega * n * dt) in float64, as set_dft does.  omegas None or
        empty removes the window.  Beside set_dft, not instead of it."""
        if omegas is None or np.size(omegas) == 0:
            self._ck(self._lib.fdtd2d_batch_set_dft_window(self._h, 0, 0, 0, 0, 0, None, 1))
            self._win = None
            return self
        w = _window_omegas(omegas, self.count)
        r0, c0, nr, nc = (int(v) for v in window)
        self._touches_image(f"window ({r0},{c0})+{nr}x{nc}", c0 + nc - 1)
        self._touches_lattice_image(f"window ({r0},{c0})+{nr}x{nc}", r0 + nr - 1, c0 + nc - 1)
        self._ck(self._lib.fdtd2d_batch_set_dft_window(self._h, r0, c0, nr, nc, int(w.shape[1]), _dptr(w), int(every)))
        self._win = (int(w.shape[1]), nr, nc)
        return self

    def read_dft_window(self) -> np.ndarray:
        """complex128 (B, F, nrows, ncols) of the window DFT.  With a Bloch phase: of the complex Ez, W(re) + 1j * W(im)."""
        f, nr, nc = self._win or (0, 0, 0)
        shape = (self.count, f, nr, nc)
        re, im = np.empty(shape), np.empty(shape)
        if self._win is None:     # the library refuses (no window): keep the buffers valid
            re = im = np.empty(1)
        self._ck(self._lib.fdtd2d_batch_read_dft_window(self._h, _dptr(re), _dptr(im)))
        if self._bloch is not None:
            re2, im2 = np.empty_like(re), np.empty_like(im)
            self._ck(self._bloch_fn("read_dft_window_bloch")(self._h, _dptr(re2), _dptr(im2)))
            return (re + 1j * im) + 1j * (re2 + 1j * im2)
        return re + 1j * im

    @property
    def window_in_lds(self) -> bool:
        """Whether the window accumulators live in LDS on the resident path now."""
        return bool(self.info(_abi.BATCH_INFO_DFT_WINDOW_LDS))

    def set_window_lds(self, allow=True):
        """allow False keeps the window accumulators in global memory (results never depend on it)."""
        self._ck(self._lib.fdtd2d_batch_set_option(self._h, _abi.BATCH_OPT_DFT_WINDOW_LDS, -1 if allow else 0))
        return self

    # -- flux lines (fdtd2d_batch_flux.h) --------------------------------------------------------------
    def set_flux_lines(self, lines, omegas, every=1):
        """Flux monitors on a "pml" or "periodic" engine: up to 4 lines, ("row", i, c0, nc) counting power towards
        increasing row or ("col", j, r0, nr) towards increasing column, the same for all members, at up to 16 angular
        frequencies per member: omegas (F,) for every member or (B, F).  After every `every`-th step n (counted from
        this call) the engine adds Ez * exp(-1j * omega * n * dt) and Ht * exp(-1j * omega * n * dt) on the line cells in
        float64, Ht being the tangential H of the step's H half-step centred on the cell (fdtd2d_batch_flux.h).  lines
        None or empty removes them.  A lossless "pml" engine runs the lossy kernels with a zero conductivity while
        lines are set (bit-identical fields, a smaller resident capacity: see resident_max_cells)."""
        if lines is None or len(lines) == 0:
            self._ck(self._lib.fdtd2d_batch_set_flux_lines(self._h, 0, None, 0, None, 1))
            if not self._hzflux and not self._hzbflux:
                self._flux, self._bflux = None, False
            return self
        self._no_hz("flux lines (the sign and the averaged component differ)")
        ln, w, every = _flux_lines(lines, omegas, every, self.count, self.rows, self.cols, self.boundary == "periodic")
        self._ck(self._lib.fdtd2d_batch_set_flux_lines(self._h, len(ln), ln.ctypes.data_as(C.POINTER(C.c_int)),
                                                       int(w.shape[1]), _dptr(w), every))
        self._flux, self._bflux = (ln, w), False
        return self

    def set_bloch_flux_lines(self, lines, omegas, every=1):
        """The flux lines of set_flux_lines on a "periodic" engine with a Bloch phase (set_bloch_phase), with or without
        the pole of set_bloch_dispersion: the same lines, limits and sampling, on complex fields
        (fdtd2d_batch_bloch_flux.h).  The frequencies may have either sign: omega and -omega are different spectra of
        a complex field.  At column 0 a column line reads its left neighbour across the seam, rotated back by the
        phase.  lines None or empty removes them.  While they are set, turning the phase off, Bloch point sources,
        run_bloch_channels and hold_bloch_window are refused (the last two until set_bloch_flux_line_sources installs sources
        on the lines); a new phase keeps the lines and their sums."""
        if lines is None or len(lines) == 0:
            self._ck(self._lib.fdtd2d_batch_set_bloch_flux_lines(self._h, 0, None, 0, None, 1))
            if self._bflux:
                self._flux, self._bflux = None, False
            return self
        self._no_hz("Bloch flux lines")
        ln, w, every = _flux_lines(lines, omegas, every, self.count, self.rows, self.cols, True)
        self._ck(self._lib.fdtd2d_batch_set_bloch_flux_lines(self._h, len(ln), ln.ctypes.data_as(C.POINTER(C.c_int)),
                                                             int(w.shape[1]), _dptr(w), every))
        self._flux, self._bflux = (ln, w), True
        return self

    def set_hz_flux_lines(self, lines, omegas, every=1):
        """The flux lines of set_flux_lines on an engine in the Hz polarisation (set_polarization("hz")), with or without
        set_conductivity and set_dispersion: the same lines, limits and sampling (fdtd2d_batch_hz_flux.h).  After every
        `every`-th step n the engine adds Hz * exp(-1j * omega * n * dt) and Et * exp(-1j * omega * n * dt) on the line
        cells in float64, Et being the tangential E of the step's E half-step centred on the cell: 0.5 * (Ex[i-1, j] +
        Ex[i, j]) on a row line, 0.5 * (Ey[i, j-1] + Ey[i, j]) on a column line.  lines None or empty removes them.
        read_flux_lines, flux, flux_lines_in_lds and set_flux_lds serve them; set_polarization("ez") is refused while
        they are set."""
        if lines is None or len(lines) == 0:
            self._ck(self._lib.fdtd2d_batch_set_hz_flux_lines(self._h, 0, None, 0, None, 1))
            if self._hzflux:
                self._flux, self._hzflux = None, False
            return self
        if self._hzb:
            self._no_bloch("set_hz_flux_lines")
        if not self._hz:
            raise _abi.Fdtd2dError(_abi.E_STATE, 'set_hz_flux_lines needs the Hz polarisation (set_polarization("hz")): '
                                                 "the lines of the Ez polarisation are set_flux_lines'")
        ln, w, every = _flux_lines(lines, omegas, every, self.count, self.rows, self.cols, self.boundary == "periodic")
        self._ck(self._lib.fdtd2d_batch_set_hz_flux_lines(self._h, len(ln), ln.ctypes.data_as(C.POINTER(C.c_int)),
                                                          int(w.shape[1]), _dptr(w), every))
        self._flux, self._bflux, self._hzflux = (ln, w), False, True
        return self

    def set_hz_bloch_flux_lines(self, lines, omegas, every=1):
        """The flux lines of set_hz_flux_lines on a "periodic" engine in the Hz polarisation with the phase of
        set_hz_bloch_phase, with or without set_conductivity and set_dispersion: the same lines, limits and sampling, the
        sums taken on the real and on the imaginary part of Hz and of the tangential E (fdtd2d_batch_hz_bloch_flux.h).  On
        a column line at column 0 the left neighbour of Ey is the one the step itself uses, rotated back across the seam.
        The frequencies may have either sign.  lines None or empty removes them.  read_flux_lines,
        read_hz_bloch_flux_parts, flux, flux_orders, flux_lines_in_lds and set_flux_lds serve them; a new phase,
        set_conductivity, set_dispersion and reset() keep them, set_hz_bloch_phase(None) is refused while they are set."""
        if lines is None or len(lines) == 0:
            self._ck(self._lib.fdtd2d_batch_set_hz_bloch_flux_lines(self._h, 0, None, 0, None, 1))
            if self._hzbflux:
                self._flux, self._hzbflux = None, False
            return self
        self._no_lattice("set_hz_bloch_flux_lines")
        if not self._hzb:
            raise _abi.Fdtd2dError(_abi.E_STATE, "set_hz_bloch_flux_lines needs the phase of the Hz polarisation: call "
                                   "set_hz_bloch_phase first (without a phase use set_hz_flux_lines, in the Ez "
                                   "polarisation set_bloch_flux_lines)")
        ln, w, every = _flux_lines(lines, omegas, every, self.count, self.rows, self.cols, True)
        self._ck(self._lib.fdtd2d_batch_set_hz_bloch_flux_lines(self._h, len(ln), ln.ctypes.data_as(C.POINTER(C.c_int)),
                                                                int(w.shape[1]), _dptr(w), every))
        self._flux, self._bflux, self._hzflux, self._hzbflux = (ln, w), False, False, True
        return self

    def read_flux_lines(self, raw=False):
        """(Ez_hat, Ht_hat), each complex128 (B, F, cells): the transforms on the line cells, lines concatenated in the
        order given.  Ht_hat carries the half-step factor exp(+1j * omega * dt / 2) (the H of a step lives half a step
        before its Ez) unless raw, which returns the sums as accumulated.  Serves the lines of set_flux_lines and of
        set_bloch_flux_lines (the transforms of the complex fields: those of the real part plus 1j times those of the
        imaginary part).  With the lines of set_hz_flux_lines it returns (Et_hat, Hz_hat), the electric transform first
        as in the other polarisation, and the factor goes on Et_hat (the E of a step lives half a step before its Hz);
        with those of set_hz_bloch_flux_lines likewise, each the sum of the two parts as on the Ez Bloch lines."""
        ln, w = self._flux or (np.zeros((0, 4), np.int32), np.zeros((self.count, 0)))
        shape = (self.count, w.shape[1], int(ln[:, 3].sum()))
        if self._hzbflux:
            (hr, er), (hi, ei) = self.read_hz_bloch_flux_parts()
            e, h = er + 1j * ei, hr + 1j * hi
            return (e, h) if raw else (e * np.exp(0.5j * w * self.dt)[:, :, None], h)
        if self._hzflux:
            a = [np.empty(shape) for _ in range(4)]
            self._ck(self._lib.fdtd2d_batch_read_hz_flux_lines(self._h, *(_dptr(x) for x in a)))
            h, e = a[0] + 1j * a[1], a[2] + 1j * a[3]
            return (e, h) if raw else (e * np.exp(0.5j * w * self.dt)[:, :, None], h)
        if self._bflux:
            (er, hr), (ei, hi) = self.read_bloch_flux_parts()
            e, h = er + 1j * ei, hr + 1j * hi
            return (e, h) if raw else (e, h * np.exp(0.5j * w * self.dt)[:, :, None])
        a = [np.empty(shape) if self._flux is not None else np.empty(1) for _ in range(4)]
        self._ck(self._lib.fdtd2d_batch_read_flux_lines(self._h, *(_dptr(x) for x in a)))
        e, h = a[0] + 1j * a[1], a[2] + 1j * a[3]
        return (e, h) if raw else (e, h * np.exp(0.5j * w * self.dt)[:, :, None])

    def read_bloch_flux_parts(self):
        """The raw sums of set_bloch_flux_lines as the engine holds them: ((Ez_hat, Ht_hat) of the real part of the
        fields, (Ez_hat, Ht_hat) of the imaginary part), each complex128 (B, F, cells), without the half-step factor."""
        ln, w = self._flux if self._bflux else (np.zeros((0, 4), np.int32), np.zeros((self.count, 0)))
        shape = (self.count, w.shape[1], int(ln[:, 3].sum()))
        out = []
        for part in (0, 1):
            a = [np.empty(shape) if self._bflux else np.empty(1) for _ in range(4)]
            self._ck(self._lib.fdtd2d_batch_read_bloch_flux_lines(self._h, part, *(_dptr(x) for x in a)))
            out.append((a[0] + 1j * a[1], a[2] + 1j * a[3]))
        return tuple(out)

    def read_hz_bloch_flux_parts(self):
        """The raw sums of set_hz_bloch_flux_lines as the engine holds them: ((Hz_hat, Et_hat) of the real part of the
        fields, (Hz_hat, Et_hat) of the imaginary part), each complex128 (B, F, cells), without the half-step factor."""
        ln, w = self._flux if self._hzbflux else (np.zeros((0, 4), np.int32), np.zeros((self.count, 0)))
        shape = (self.count, w.shape[1], int(ln[:, 3].sum()))
        out = []
        for part in (0, 1):
            a = [np.empty(shape) if self._hzbflux else np.empty(1) for _ in range(4)]
            self._ck(self._lib.fdtd2d_batch_read_hz_bloch_flux_lines(self._h, part, *(_dptr(x) for x in a)))
            out.append((a[0] + 1j * a[1], a[2] + 1j * a[3]))
        return tuple(out)

    def flux_orders(self, line=0):
        """float64 (B, F, Q), Q = C - 1: the power through a whole-period row line of set_bloch_flux_lines split over the
        diffraction orders, P_m = dx * Q * Re(E_m * conj(H_m)) with E_m = (1/Q) * sum_j Ez_hat[j] * exp(-1j * (phi + 2 pi
        m) * j / Q) and H_m likewise (Ht_hat with the half-step factor), m in np.fft.fftfreq(Q, 1/Q) order.  By Parseval
        the orders sum to flux()[:, line, :]: these are a grating's diffraction efficiencies before normalisation.
        Host NumPy over read_flux_lines().  On the lines of set_hz_bloch_flux_lines, with the phase of
        set_hz_bloch_phase: P_m = -dx * Q * Re(H_m * conj(E_m)) from Hz_hat and Et_hat (the half-step factor on Et_hat)."""
        if not self._bflux and not self._hzbflux:
            raise _abi.Fdtd2dError(_abi.E_STATE, "no Bloch flux lines are set")
        ln, _ = self._flux
        Q = self.cols - 1
        if not 0 <= int(line) < len(ln):
            raise ValueError(f"line {line} outside 0..{len(ln) - 1}")
        col, _, first, n = (int(x) for x in ln[int(line)])
        if col or first != 0 or n != Q:
            raise ValueError(f"flux_orders needs a row line over the whole period (columns 0..{Q - 1}), not line {line}")
        c, s = self._bloch
        phi = self._phi if self._phi is not None else np.arctan2(s, c)
        o = int(ln[:int(line), 3].sum())
        E, H = (a[:, :, o:o + Q] for a in self.read_flux_lines())
        envelope = np.exp(-1j * phi[:, None, None] * np.arange(Q)[None, None, :] / Q)
        Em, Hm = np.fft.fft(E * envelope, axis=2) / Q, np.fft.fft(H * envelope, axis=2) / Q
        if not self._bflux:           # the Hz polarisation: S_y = -Ex Hz
            return -self.dx * Q * np.real(Hm * np.conj(Em))
        return self.dx * Q * np.real(Em * np.conj(Hm))

    def flux(self) -> np.ndarray:
        """float64 (B, N, F): the power that crosses each line per frequency, P = s * dx * sum over the line's cells of
        Re(Ez_hat * conj(Ht_hat)), s = +1 for a row line and -1 for a column line, formed on the device.  No factor 1/2
        and no normalisation: take ratios.  With the lines of set_hz_flux_lines the sum is of Re(Hz_hat * conj(Et_hat)) and
        s = -1 for a row line, +1 for a column line (S_y = -Ex Hz, S_x = Ey Hz): a line counts power towards increasing
        row or column in either polarisation.  The lines of set_hz_bloch_flux_lines: the same on the complex spectra."""
        ln, w = self._flux or (np.zeros((0, 4), np.int32), np.zeros((self.count, 0)))
        out = np.empty((self.count, len(ln), w.shape[1]))
        buf = out if out.size else np.empty(1)     # a refused read still passes a valid pointer
        fn = (self._lib.fdtd2d_batch_bloch_flux if self._bflux else
              self._lib.fdtd2d_batch_hz_flux if self._hzflux else
              self._lib.fdtd2d_batch_hz_bloch_flux if self._hzbflux else self._lib.fdtd2d_batch_flux)
        self._ck(fn(self._h, _dptr(buf)))
        return out

    # -- line sources on the flux lines (fdtd2d_batch_flux_adjoint.h) --------------------------------------
    def _flux_entries(self, what):
        self._no_hz(what)
        if self._flux is None or self._bflux:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} live on flux lines: call set_flux_lines first (not with "
                                                 f"set_bloch_flux_lines)")
        return int(self._flux[0][:, 3].sum())

    def set_flux_line_sources(self, we, wh):
        """Sources on the cells of set_flux_lines, the transpose of the monitor: we drives Ez and wh the tangential H
        with the monitor's centring.  we, wh: float64 (cells, K) for every member or (B, cells, K), K <= 32, cells being
        the lines' cells concatenated in the order of read_flux_lines (a cell on two lines has two entries); either may
        be None, both None removes the sources.  In step n of run(nsteps, amps, channels=...) entry w forms
        s_e = sum_c we[w, c] * channels[c, n] and s_h likewise; 0.5 * s_h is added to each of the two H values the
        monitor averages for the cell before the H update of the step, and s_e to Ez where the point sources add theirs
        (fdtd2d_batch_flux_adjoint.h has the order of every addition).  An electric and a magnetic sheet on one line form
        a one-way source.  K must equal the channel count of point sources that are set too; set_flux_lines removes the
        line sources, reset() keeps them."""
        if we is None and wh is None:
            self._ck(self._lib.fdtd2d_batch_set_flux_line_sources(self._h, 0, None, None))
            return self
        cells = self._flux_entries("line sources")
        parts = []
        for name, w in (("we", we), ("wh", wh)):
            if w is None:
                parts.append(None)
                continue
            w = np.asarray(w, dtype=np.float64)
            if w.ndim == 2:
                w = np.broadcast_to(w, (self.count,) + w.shape)
            if w.ndim != 3 or w.shape[:2] != (self.count, cells):
                raise ValueError(f"{name} must have shape ({cells}, K) or ({self.count}, {cells}, K), got {w.shape}")
            parts.append(np.ascontiguousarray(w))
        K = {int(w.shape[2]) for w in parts if w is not None}
        if len(K) != 1:
            raise ValueError(f"we and wh must have the same number of channels, got {sorted(K)}")
        K = K.pop()
        if not 1 <= K <= _abi.BATCH_MAX_CHANNELS:
            raise ValueError(f"line sources take 1..{_abi.BATCH_MAX_CHANNELS} channels, got {K}")
        self._ck(self._lib.fdtd2d_batch_set_flux_line_sources(self._h, K, *(None if w is None else _dptr(w)
                                                                            for w in parts)))
        return self

    def read_flux_line_sources(self):
        """(we, wh), each float64 (B, cells, K): the weights as the engine holds them (an absent part reads as zeros)."""
        cells, K = self._flux_entries("line sources"), self.info(_abi.BATCH_FLUX_LINE_SOURCES_INFO)
        out = [np.zeros((self.count, cells, K)) if K else np.zeros(1) for _ in range(2)]
        self._ck(self._lib.fdtd2d_batch_read_flux_line_sources(self._h, *(_dptr(a) for a in out)))
        return tuple(out)

    def flux_adjoint_sources(self, dJdP, solve, scale_e=None, scale_h=None):
        """Forms the line sources of the adjoint of a flux objective on the device, from the lines' current sums, and
        installs them with K = 2F channels (one launch; nothing is read back).  dJdP: (B, N, F), the derivative of the
        objective by flux().  solve: (2F, 2F) for every member or (B, 2F, 2F), the inverse of the channel system
        (adjoint.channel_system).  scale_e, scale_h: (B, cells) real factors per entry (None: ones): the adjoint takes
        dt / (eps dx) and -dt / (mu dx) of the cells.  With E, H the raw sums, g = exp(1j * omega * dt / 2) and
        c = dJdP * s * dx per line, the targets are scale_e * c * conj(H g) for we and scale_h * c * conj(E g) for wh,
        and the weights are solve @ [Re target; Im target].  flux_adjoint_weights is the same arithmetic on the host."""
        cells = self._flux_entries("the adjoint sources")
        ln, w = self._flux
        N, F = len(ln), w.shape[1]
        g = np.ascontiguousarray(dJdP, dtype=np.float64)
        if g.shape != (self.count, N, F):
            raise ValueError(f"dJdP must have shape ({self.count}, {N}, {F}), got {g.shape}")
        s = np.ascontiguousarray(solve, dtype=np.float64)
        if s.shape not in ((2 * F, 2 * F), (self.count, 2 * F, 2 * F)):
            raise ValueError(f"solve must have shape ({2 * F}, {2 * F}) or ({self.count}, {2 * F}, {2 * F}), got {s.shape}")
        scales = []
        for name, a in (("scale_e", scale_e), ("scale_h", scale_h)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (self.count, cells):
                    raise ValueError(f"{name} must have shape ({self.count}, {cells}), got {a.shape}")
            scales.append(a)
        self._ck(self._lib.fdtd2d_batch_flux_line_weights(self._h, _dptr(g), _dptr(s), int(s.ndim == 3),
                                                          *(None if a is None else _dptr(a) for a in scales)))
        return self

    # -- line sources on Bloch flux lines (fdtd2d_batch_bloch_flux_adjoint.h) ---------------------------------
    def _bloch_flux_entries(self, what):
        if self._flux is None or not self._bflux:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} live on Bloch flux lines: call set_bloch_flux_lines first")
        return int(self._flux[0][:, 3].sum())

    def set_bloch_flux_line_sources(self, we, wh):
        """set_flux_line_sources on the lines of set_bloch_flux_lines, with complex weights: we, wh complex (cells, K)
        for every member or (B, cells, K), K <= 32; either may be None, both None removes the sources.  A real array is
        accepted and its imaginary part is absent (it takes nothing).  In step n of run_bloch_channels(nsteps, amps,
        channels) entry w forms the complex s_e = sum_c we[w, c] * channels[c, n] and s_h likewise (the channels are
        real); s_e is added to the complex Ez where Bloch point sources would add theirs, and 0.5 * s_h to each of the
        two H values the monitor averages for the cell, before the H update of the step.  For a column-line cell at
        column 0 the left H value lies across the seam and takes rho * 0.5 * s_h, with the rotation the run steps with
        (conj(rho) in a conjugated run: the transpose of the monitor's read).  With ramp weights exp(1j * phi * j / Q)
        an electric and a magnetic sheet on a row line form a one-way source at oblique incidence.  Once sources are
        installed (zeros included) run_bloch_channels and hold_bloch_window are accepted on a batch with Bloch lines;
        set_bloch_flux_lines removes them, reset(), a new phase and set_bloch_dispersion keep them."""
        if we is None and wh is None:
            self._ck(self._lib.fdtd2d_batch_set_bloch_flux_line_sources(self._h, 0, None, None, None, None))
            return self
        cells = self._bloch_flux_entries("Bloch line sources")
        parts = []
        for name, w in (("we", we), ("wh", wh)):
            if w is None:
                parts += [None, None]
                continue
            w = np.asarray(w)
            cplx = np.iscomplexobj(w)
            if w.ndim == 2:
                w = np.broadcast_to(w, (self.count,) + w.shape)
            if w.ndim != 3 or w.shape[:2] != (self.count, cells):
                raise ValueError(f"{name} must have shape ({cells}, K) or ({self.count}, {cells}, K), got {w.shape}")
            parts.append(np.ascontiguousarray(w.real, dtype=np.float64))
            parts.append(np.ascontiguousarray(w.imag, dtype=np.float64) if cplx else None)
        K = {int(w.shape[2]) for w in parts if w is not None}
        if len(K) != 1:
            raise ValueError(f"we and wh must have the same number of channels, got {sorted(K)}")
        K = K.pop()
        if not 1 <= K <= _abi.BATCH_MAX_CHANNELS:
            raise ValueError(f"line sources take 1..{_abi.BATCH_MAX_CHANNELS} channels, got {K}")
        self._ck(self._lib.fdtd2d_batch_set_bloch_flux_line_sources(self._h, K, *(None if w is None else _dptr(w)
                                                                                  for w in parts)))
        return self

    def read_bloch_flux_line_sources(self):
        """(we, wh), each complex128 (B, cells, K): the weights as the engine holds them (an absent part reads as
        zeros)."""
        cells = self._bloch_flux_entries("Bloch line sources")
        K = self.info(_abi.BATCH_FLUX_LINE_SOURCES_INFO)
        out = [np.zeros((self.count, cells, K)) if K else np.zeros(1) for _ in range(4)]
        self._ck(self._lib.fdtd2d_batch_read_bloch_flux_line_sources(self._h, *(_dptr(a) for a in out)))
        return out[0] + 1j * out[1], out[2] + 1j * out[3]

    def bloch_flux_adjoint_sources(self, dJdP, solve, scale_e=None, scale_h=None):
        """flux_adjoint_sources on the lines of set_bloch_flux_lines: forms the line sources of the adjoint of an
        objective on flux() on the device, from both parts' current sums, and installs them as real weights with
        K = 2F channels (one launch; nothing is read back).  The arguments are those of flux_adjoint_sources; E and H
        are the raw sums of the complex fields.  bloch_flux_adjoint_weights is the same arithmetic on the host."""
        cells = self._bloch_flux_entries("the adjoint sources")
        ln, w = self._flux
        N, F = len(ln), w.shape[1]
        g = np.ascontiguousarray(dJdP, dtype=np.float64)
        if g.shape != (self.count, N, F):
            raise ValueError(f"dJdP must have shape ({self.count}, {N}, {F}), got {g.shape}")
        s = np.ascontiguousarray(solve, dtype=np.float64)
        if s.shape not in ((2 * F, 2 * F), (self.count, 2 * F, 2 * F)):
            raise ValueError(f"solve must have shape ({2 * F}, {2 * F}) or ({self.count}, {2 * F}, {2 * F}), got {s.shape}")
        scales = []
        for name, a in (("scale_e", scale_e), ("scale_h", scale_h)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (self.count, cells):
                    raise ValueError(f"{name} must have shape ({self.count}, {cells}), got {a.shape}")
            scales.append(a)
        self._ck(self._lib.fdtd2d_batch_bloch_flux_line_weights(self._h, _dptr(g), _dptr(s), int(s.ndim == 3),
                                                                *(None if a is None else _dptr(a) for a in scales)))
        return self

    @property
    def flux_lines_in_lds(self) -> bool:
        """Whether the flux lines' sums live in LDS on the resident path now."""
        return bool(self.info(_abi.BATCH_INFO_FLUX_LDS))

    def set_flux_lds(self, allow=True):
        """allow False keeps the flux lines' sums in global memory (results never depend on it)."""
        self._ck(self._lib.fdtd2d_batch_set_option(self._h, _abi.BATCH_OPT_FLUX_LDS, -1 if allow else 0))
        return self

    def set_probes(self, cells, capacity):
        """Record Ez after the source of every following step at up to 64 cells per member: cells (P, 2) {row, col}
        for every member or (B, P, 2); `capacity` float64 samples per probe, sample 0 = the next step.  None (or no
        cells) removes the probes."""
        if cells is None:
            self._ck(self._lib.fdtd2d_batch_set_probes(self._h, 0, None, 0))
            self._nprobe = 0
            return self
        c = _probe_cells(cells, self.count)
        self._touches_image("a probe", c[..., 1])
        self._touches_lattice_image("a probe", c[..., 0], c[..., 1])
        self._ck(self._lib.fdtd2d_batch_set_probes(self._h, int(c.shape[1]), c.ctypes.data_as(C.POINTER(C.c_int)),
                                                   int(capacity)))
        self._nprobe = int(c.shape[1])
        return self

    @property
    def probe_samples(self) -> int:
        """Samples recorded so far per probe."""
        return self.info(_abi.BATCH_INFO_PROBE_SAMPLES)

    def read_probes(self, first=0, count=None) -> np.ndarray:
        """float64 (B, P, count): samples [first, first + count) of every probe; count None = up to the samples
        recorded so far.  complex128 with a Bloch phase."""
        if count is None:
            count = max(0, self.probe_samples - int(first))
        out = np.empty((self.count, self._nprobe, max(0, int(count))))
        buf = out if out.size else np.empty(1)     # a refused or empty read still passes a valid pointer
        self._ck(self._lib.fdtd2d_batch_read_probes(self._h, _dptr(buf), int(first), int(count)))
        if self._bloch is not None:
            im = np.empty_like(out)
            buf = im if im.size else np.empty(1)
            self._ck(self._bloch_fn("read_probes_bloch")(self._h, _dptr(buf), int(first), int(count)))
            return out + 1j * im
        return out

    # -- the design loop (fdtd2d_batch_design.h) ---------------------------------------------------------------
    def probe_spectra(self, omegas, first=0, count=None, peak=False):
        """complex128 (B, P, F): sum over the samples n in [first, first + count) of trace[b, p, n] *
        exp(-1j * omegas[b, k] * s * dt), s the step after which sample n was recorded, formed on the device with the
        window DFT's arithmetic in ascending n.  omegas (F,) for every member or (B, F), F <= 16; count None = up to
        the samples recorded so far.  peak True: also float64 (B,), the largest |sample| of each member in the range."""
        self._no_bloch("fdtd2d_batch_probe_spectra")
        w = _window_omegas(omegas, self.count)
        if count is None:
            count = max(0, self.probe_samples - int(first))
        F = int(w.shape[1])
        re, im = np.empty((self.count, self._nprobe, F)), np.empty((self.count, self._nprobe, F))
        pk = np.empty(self.count) if peak else None
        buf = (re, im) if re.size else (np.empty(1), np.empty(1))    # a refused call still passes valid pointers
        self._ck(self._lib.fdtd2d_batch_probe_spectra(self._h, F, _dptr(w) if F else None, int(first), int(count),
                                                      _dptr(buf[0]) if F else None, _dptr(buf[1]) if F else None,
                                                      None if pk is None else _dptr(pk)))
        out = re + 1j * im
        return (out, pk) if peak else out

    def field_absmax(self, field="Ez"):
        """float64 (B,): max |field| over each member's cells, reduced on the device.  field "Ez", "Hx" or "Hy"."""
        codes = {"Ez": _abi.FIELD_EZ, "Hx": _abi.FIELD_HX, "Hy": _abi.FIELD_HY}
        if field not in codes:
            raise ValueError(f'field must be "Ez", "Hx" or "Hy", not {field!r}')
        self._no_bloch("fdtd2d_batch_field_absmax")
        out = np.empty(self.count)
        self._ck(self._lib.fdtd2d_batch_field_absmax(self._h, codes[field], _dptr(out)))
        return out

    def set_eps_window(self, window, eps):
        """New permittivity for window = (row0, col0, nrows, ncols) of every member: eps (B, nrows, ncols).  The
        engine is then as set_materials with the full updated arrays would leave it; fields, monitors, sources and the
        PML stay.  Needs material arrays (not a uniform batch); the window must not hold cell [0, 0]."""
        r0, c0, nr, nc = (int(v) for v in window)
        e = _host(eps, "eps")
        self._shape(e, (self.count, nr, nc), "eps")
        self._ck(self._lib.fdtd2d_batch_set_eps_window(self._h, r0, c0, nr, nc, e.ctypes.data, _code(e.dtype)))
        return self

    # -- lossy materials (fdtd2d_batch_lossy.h) ------------------------------------------------------------------
    @property
    def conductivity_margin(self) -> int:
        """Cells next to every edge that may not conduct with the current boundary: the 5-cell Mur frame and cell
        [0, 0] (6), the PML layer (its depth, at least 6), or the edge cells of a closed box (1).  With periodic columns
        it counts rows alone (the layer's depth, at least 6): every column of the period may conduct."""
        if self.boundary == "mur":
            return 6
        if self.boundary == "lattice" or self._hzlat:
            return 0                  # no edge: every cell of the period may conduct
        if self.boundary == "periodic":
            return max(6, self._pml_L)
        return max(6, self._pml_L) if self._pml_on else 1

    def set_conductivity(self, sigma):
        """Electric conductivity in S/m, >= 0: (B, R, C), or a scalar for every cell that may conduct (zero in the
        margin of conductivity_margin), or None to remove it.  The cells that take the plain E update then take
        e = ca * e + (dhy - dhx) * cb with s = sigma dt / (2 eps), ca = (1 - s) / (1 + s), cb = ce / (1 + s); it
        persists across set_materials and set_eps_window.  Needs materials (a uniform batch gets coefficient arrays).
        The library refuses (E_ARG) a value that is negative, not finite, or non-zero inside the margin."""
        setter = self._lib.fdtd2d_batch_set_hz_conductivity if self._hz else self._lib.fdtd2d_batch_set_conductivity
        if sigma is None:
            self._ck(setter(self._h, None, _code(self.dtype)))
            return self
        shape = (self.count, self.rows, self.cols)
        if np.isscalar(sigma):
            g = self.conductivity_margin
            s = np.zeros(shape, np.float64)
            if self._hz:
                s[self._hz_allowed()] = float(sigma)
            elif self.boundary in ("periodic", "lattice"):
                s[:, g:self.rows - g, :] = float(sigma)
            else:
                s[:, g:self.rows - g, g:self.cols - g] = float(sigma)
            if not float(sigma) >= 0:             # negative or NaN: let the library name it even where s is empty
                s[...] = float(sigma)
        else:
            s = _host(sigma, "sigma")
        self._shape(s, shape, "sigma")
        self._ck(setter(self._h, s.ctypes.data, _code(s.dtype)))
        return self

    def _hz_allowed(self):
        """(B, R, C) bool: the cells that may conduct or carry a pole in the Hz polarisation: rows g..R-2-g and, on a
        "pml" batch, columns g..C-2-g (Ex[i, j] lives at i + 1/2; column C-1 of a periodic batch is never read)."""
        g = self.conductivity_margin
        ok = np.zeros((self.count, self.rows, self.cols), bool)
        if self._hzlat:               # every cell of the period: rows 0..R-2 and columns 0..C-2
            ok[:, :self.rows - 1, :self.cols - 1] = True
        elif self.boundary == "periodic":
            ok[:, g:self.rows - 1 - g, :] = True
        else:
            ok[:, g:self.rows - 1 - g, g:self.cols - 1 - g] = True
        return ok

    def set_conductivity_window(self, window, sigma):
        """New conductivity for window = (row0, col0, nrows, ncols) of every member: sigma (B, nrows, ncols).  The
        engine is then as set_conductivity with the full updated array would leave it (a batch without conductivity
        starts from zero)."""
        self._no_hz("set_conductivity_window")
        w = np.ascontiguousarray([int(v) for v in window], dtype=np.int32)
        if w.shape != (4,):
            raise ValueError(f"window must be 4 integers (row0, col0, nrows, ncols), got {window!r}")
        s = _host(sigma, "sigma")
        self._shape(s, (self.count, int(w[2]), int(w[3])), "sigma")
        self._ck(self._lib.fdtd2d_batch_set_conductivity_window(self._h, w.ctypes.data_as(C.POINTER(C.c_int)),
                                                                s.ctypes.data, _code(s.dtype)))
        return self

    @property
    def lossy(self) -> bool:
        """Whether a conductivity is set (the batch runs on the lossy kernels)."""
        return bool(self.info(_abi.BATCH_INFO_LOSSY))

    # -- dispersive materials (fdtd2d_batch_dispersive.h) --------------------------------------------------------
    def set_dispersion(self, wp2, gamma=0.0, omega0=0.0):
        """One Drude-Lorentz pole per member: chi(w) = wp2 / (omega0**2 - w**2 - 1j * gamma * w) for a field
        ~ exp(-1j * w * t), so eps(w) = eps + EPS0 * chi(w).  wp2 in rad^2/s^2, >= 0: (B, R, C), or a scalar for every
        cell that may carry it (zero in the margin of conductivity_margin), or None to remove the pole.  gamma and
        omega0 in rad/s, >= 0: a scalar or (B,); omega0 = 0 is a Drude pole, a Lorentz pole of strength d_eps has
        wp2 = d_eps * omega0**2.  Needs boundary="pml" with its layer set, or boundary="periodic", and materials.  The
        state (download_dispersion) starts at zero and survives later calls; reset() zeroes it.  The library refuses
        (E_ARG) a value that is negative or not finite, wp2 non-zero inside the margin, and a cell whose pole breaks
        dt^2 (omega0^2 + wp2 EPS0 / eps) + 8 dt^2 / (eps mu dx^2) <= 4; while a pole is set it refuses (E_STATE) a Bloch
        phase, removing the layer of a "pml" batch and the held window with its product."""
        if not self._hzlat:           # the lattice mode of the Hz polarisation takes the pole of set_polarization("hz")
            self._no_lattice("a dispersive pole")
        setter = self._lib.fdtd2d_batch_set_hz_dispersion if self._hz else self._lib.fdtd2d_batch_set_dispersion
        if wp2 is None:
            self._ck(setter(self._h, None, _code(self.dtype), None, None))
            return self
        shape = (self.count, self.rows, self.cols)
        if np.isscalar(wp2):
            g = self.conductivity_margin
            w = np.zeros(shape, np.float64)
            if self._hz:
                w[self._hz_allowed()] = float(wp2)
            elif self.boundary == "periodic":
                w[:, g:self.rows - g, :] = float(wp2)
            else:
                w[:, g:self.rows - g, g:self.cols - g] = float(wp2)
            if not float(wp2) >= 0:               # negative or NaN: let the library name it even where w is empty
                w[...] = float(wp2)
        else:
            w = _host(wp2, "wp2")
        self._shape(w, shape, "wp2")
        per = []
        for v, nm in ((gamma, "gamma"), (omega0, "omega0")):
            a = np.asarray(v, dtype=np.float64)
            if a.shape not in ((), (self.count,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({self.count},), got {a.shape}")
            per.append(np.ascontiguousarray(np.broadcast_to(a, (self.count,))))
        self._ck(setter(self._h, w.ctypes.data, _code(w.dtype), _dptr(per[0]), _dptr(per[1])))
        return self

    def set_dispersion_window(self, window, wp2):
        """New strengths for window = (row0, col0, nrows, ncols) of every member: wp2 (B, nrows, ncols).  The engine
        is then as set_dispersion with the full updated array would leave it.  Needs a pole (E_STATE)."""
        self._no_lattice("a dispersive pole")
        self._no_hz("set_dispersion_window")
        w = np.ascontiguousarray([int(v) for v in window], dtype=np.int32)
        if w.shape != (4,):
            raise ValueError(f"window must be 4 integers (row0, col0, nrows, ncols), got {window!r}")
        s = _host(wp2, "wp2")
        self._shape(s, (self.count, int(w[2]), int(w[3])), "wp2")
        self._ck(self._lib.fdtd2d_batch_set_dispersion_window(self._h, w.ctypes.data_as(C.POINTER(C.c_int)),
                                                              s.ctypes.data, _code(s.dtype)))
        return self

    @property
    def dispersive(self) -> bool:
        """Whether a dispersive pole is set (the batch runs on the dispersive kernels)."""
        return bool(self.info(_abi.BATCH_INFO_DISPERSIVE))

    def download_dispersion(self):
        """(Jh, Q), each (B, R, C) of the engine dtype: dx times the polarisation current at the last half step, and
        dx * P / dt (needs a pole).  In the Hz polarisation four arrays: (Jx, Qx, Jy, Qy), the state of Ex and of Ey."""
        jh = np.empty((self.count, self.rows, self.cols), self.dtype)
        q = np.empty_like(jh)
        if self._hz:
            jy, qy = np.empty_like(jh), np.empty_like(jh)
            self._ck(self._lib.fdtd2d_batch_transfer_hz_dispersion(self._h, jh.ctypes.data, q.ctypes.data, jy.ctypes.data,
                                                                   qy.ctypes.data, _code(jh.dtype), 0))
            if self._hzb:             # complex under the phase of set_hz_bloch_phase
                im = [np.empty_like(jh) for _ in range(4)]
                self._ck(self._lib.fdtd2d_batch_transfer_hz_bloch_dispersion(self._h, *(a.ctypes.data for a in im),
                                                                             _code(jh.dtype), 0))
                return tuple(a + 1j * b for a, b in zip((jh, q, jy, qy), im))
            return jh, q, jy, qy
        self._ck(self._lib.fdtd2d_batch_transfer_dispersion(self._h, jh.ctypes.data, q.ctypes.data, _code(jh.dtype), 0))
        return jh, q

    def upload_dispersion(self, Jh=None, Q=None):
        """(B, R, C) each, host -> device; one given as None is left as is.  On a periodic batch column C-1 is
        overwritten with column 0 (needs a pole).  In the Hz polarisation Jh is the pair (Jx, Jy) and Q the pair
        (Qx, Qy), stored as given (the state has no image column): upload_hz_dispersion with the four arrays named."""
        if self._hz:
            jx, jy = (None, None) if Jh is None else Jh
            qx, qy = (None, None) if Q is None else Q
            return self.upload_hz_dispersion(jx, qx, jy, qy)
        arrs = []
        for a, nm in ((Jh, "Jh"), (Q, "Q")):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=self.dtype)
                self._shape(a, (self.count, self.rows, self.cols), nm)
            arrs.append(a)
        ptr = [None if a is None else a.ctypes.data for a in arrs]
        self._ck(self._lib.fdtd2d_batch_transfer_dispersion(self._h, ptr[0], ptr[1], _code(self.dtype), 1))
        return self

    def upload_hz_dispersion(self, Jx=None, Qx=None, Jy=None, Qy=None):
        """The pole state of the Hz polarisation, (B, R, C) each in the order download_dispersion returns them, host ->
        device; one given as None is left as is (needs the Hz polarisation and a pole)."""
        given = [None if a is None else np.asarray(a) for a in (Jx, Qx, Jy, Qy)]
        if any(a is not None and np.iscomplexobj(a) for a in given) and not self._hzb:
            raise ValueError("a complex pole state needs the phase of set_hz_bloch_phase")
        arrs, ims = [], []
        for a, nm in zip(given, ("Jx", "Qx", "Jy", "Qy")):
            i = None
            if a is not None:
                if self._hzb:
                    i = np.ascontiguousarray(a.imag, dtype=self.dtype)
                a = np.ascontiguousarray(a.real, dtype=self.dtype)
                self._shape(a, (self.count, self.rows, self.cols), nm)
            arrs.append(a)
            ims.append(i)
        ptr = [None if a is None else a.ctypes.data for a in arrs]
        self._ck(self._lib.fdtd2d_batch_transfer_hz_dispersion(self._h, *ptr, _code(self.dtype), 1))
        if self._hzb and any(i is not None for i in ims):
            ptr = [None if i is None else i.ctypes.data for i in ims]
            self._ck(self._lib.fdtd2d_batch_transfer_hz_bloch_dispersion(self._h, *ptr, _code(self.dtype), 1))
        return self

    # -- the pole of a Bloch or lattice batch (fdtd2d_batch_bloch_dispersive.h) ----------------------------------
    def _need_complex(self, what):
        """The library's refusal of a complex pole's call on a batch with real fields, before the call."""
        if self._bloch is None:
            raise _abi.Fdtd2dError(_abi.E_STATE, f"{what} needs a Bloch phase or the lattice mode: a batch with real "
                                   "fields takes set_dispersion")

    def set_bloch_dispersion(self, wp2, gamma=0.0, omega0=0.0):
        """set_dispersion for an engine with complex fields (set_bloch_phase, or boundary="lattice"): one Drude-Lorentz
        pole per member, acting on the real and on the imaginary part alike (every coefficient is real).  wp2: (B, R, C),
        or a scalar for every cell that may carry it (with a Bloch phase: zero in the margin of conductivity_margin on
        the rows; on a lattice: every cell), or None to remove the pole.  gamma and omega0: a scalar or (B,).  The state
        (download_bloch_dispersion) is complex, starts at zero and survives later calls; reset() zeroes it.  The library
        refuses what set_dispersion refuses for these values (E_ARG), and (E_STATE) an engine without complex fields, one
        with Bloch point sources or a held Bloch window; while this pole is set it refuses (E_STATE) turning the phase
        off, set_bloch_point_sources, run_bloch_channels, hold_bloch_window and bloch_window_product, so
        batch_bloch_gradient and BlochAdjointSession refuse too.  New phases (a k-point or angle sweep with the metal in
        place) keep working."""
        self._need_complex("set_bloch_dispersion")
        if wp2 is None:
            self._ck(self._lib.fdtd2d_batch_set_bloch_dispersion(self._h, None, _code(self.dtype), None, None))
            return self
        shape = (self.count, self.rows, self.cols)
        if np.isscalar(wp2):
            g = self.conductivity_margin
            w = np.zeros(shape, np.float64)
            w[:, g:self.rows - g, :] = float(wp2)
            if not float(wp2) >= 0:               # negative or NaN: let the library name it even where w is empty
                w[...] = float(wp2)
        else:
            w = _host(wp2, "wp2")
        self._shape(w, shape, "wp2")
        per = []
        for v, nm in ((gamma, "gamma"), (omega0, "omega0")):
            a = np.asarray(v, dtype=np.float64)
            if a.shape not in ((), (self.count,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({self.count},), got {a.shape}")
            per.append(np.ascontiguousarray(np.broadcast_to(a, (self.count,))))
        self._ck(self._lib.fdtd2d_batch_set_bloch_dispersion(self._h, w.ctypes.data, _code(w.dtype), _dptr(per[0]),
                                                             _dptr(per[1])))
        return self

    def set_bloch_dispersion_window(self, window, wp2):
        """set_dispersion_window for the pole of set_bloch_dispersion (E_STATE without it)."""
        self._need_complex("set_bloch_dispersion_window")
        w = np.ascontiguousarray([int(v) for v in window], dtype=np.int32)
        if w.shape != (4,):
            raise ValueError(f"window must be 4 integers (row0, col0, nrows, ncols), got {window!r}")
        s = _host(wp2, "wp2")
        self._shape(s, (self.count, int(w[2]), int(w[3])), "wp2")
        self._ck(self._lib.fdtd2d_batch_set_bloch_dispersion_window(self._h, w.ctypes.data_as(C.POINTER(C.c_int)),
                                                                    s.ctypes.data, _code(s.dtype)))
        return self

    def download_bloch_dispersion(self):
        """Complex (Jh, Q), each (B, R, C): the state of the pole of set_bloch_dispersion, the image column (on a lattice
        also the image row) rotated by the member's phases, as download() delivers Ez."""
        self._need_complex("download_bloch_dispersion")
        out = [np.empty((self.count, self.rows, self.cols), self.dtype) for _ in range(4)]
        self._ck(self._lib.fdtd2d_batch_transfer_bloch_dispersion(self._h, *(a.ctypes.data for a in out),
                                                                  _code(self.dtype), 0))
        return out[0] + 1j * out[1], out[2] + 1j * out[3]

    def upload_bloch_dispersion(self, Jh=None, Q=None):
        """(B, R, C) each, real or complex, host -> device; one given as None is left as is.  The image column (on a
        lattice also the image row) is overwritten from column 0 (row 0)."""
        self._need_complex("upload_bloch_dispersion")
        ptr, keep = [], []
        for a, nm in ((Jh, "Jh"), (Q, "Q")):
            if a is None:
                ptr += [None, None]
                continue
            a = np.asarray(a)
            self._shape(a, (self.count, self.rows, self.cols), nm)
            keep += [np.ascontiguousarray(a.real, dtype=self.dtype), np.ascontiguousarray(a.imag, dtype=self.dtype)]
            ptr += [keep[-2].ctypes.data, keep[-1].ctypes.data]
        self._ck(self._lib.fdtd2d_batch_transfer_bloch_dispersion(self._h, *ptr, _code(self.dtype), 1))
        return self

    def sync(self):
        self._ck(self._lib.fdtd2d_batch_sync(self._h))
        return self


def _waveform_amps(kind, fc, nsteps, dt):
    """(B, nsteps) amplitudes evaluated step by step as run_fdtd does (one row per distinct fc)."""
    from .api import ricker_amplitude, sinusoidal_amplitude
    f = {"ricker": ricker_amplitude, "sinusoidal": sinusoidal_amplitude}[kind]
    rows = {}
    out = np.empty((len(fc), nsteps), np.float64)
    for b, v in enumerate(fc):
        v = float(v)
        if v not in rows:
            rows[v] = np.array([f(i * dt, v) for i in range(nsteps)], dtype=np.float64)
        out[b] = rows[v]
    return out


def run_fdtd_batch(eps, mu=None, *, nsteps, sources, fc=30e9, waveform="ricker", dt=5e-14, dx=1e-4,
                   dtype=np.float64, boundary="mur", omega=None, dft_every=1, device=0, pml_cells=40,
                   dft_window=None, window_omegas=None, probes=None, bloch_phase=None, source_weights=None,
                   dispersion=None, bloch_dispersion=None, polarization="ez", conductivity=None,
                   hz_bloch_phase=None, hz_lattice_phase=None, hz_flux_lines=None, hz_flux_omegas=None, hz_bloch_flux_lines=None,
                   hz_bloch_flux_omegas=None, bloch_flux_lines=None, bloch_flux_omegas=None, flux_lines=None,
                   flux_omegas=None):
    """run_fdtd for B members of one shape at once: zero fields, Courant check per member, nsteps of
    H -> E -> source with t = i*dt.

    eps: (B, R, C); mu: None (vacuum), a scalar or (B, R, C).  sources: (B, 2) or (B, 4) rectangles
    (BatchEngine.set_sources); fc: scalar or (B,); waveform "ricker", "sinusoidal" or None.  omega: None,
    or the angular frequency per member (scalar or (B,)) of a running DFT of Ez sampled every `dft_every`
    steps.  boundary "mur", "none" or "pml": a pml_cells-deep layer on every member, graded with the Courant number
    of the member's own eps[0,0], mu[0,0] (as run_fdtd does); "periodic": periodic columns (period C - 1) with that
    layer on the top and bottom rows (pml_cells 0 or None: PEC there).  dft_window = (row0, col0, nrows, ncols) with
    window_omegas (F,) or (B, F), F <= 16: a window DFT sampled every `dft_every` steps (set_dft_window).  probes:
    (P, 2) or (B, P, 2) cells, P <= 64, recorded at every step (set_probes).  Returns (Ez, Hx, Hy), plus the complex
    (B, R, C) DFT when omega is given, then the complex (B, F, nrows, ncols) window DFT when dft_window is given, then
    the float64 (B, P, nsteps) probe traces when probes are given.  bloch_phase (boundary "periodic" alone): a scalar or
    (B,) in radians, the Bloch phase of set_bloch_phase; every returned array is then complex.  source_weights: "ramp",
    None or an array as set_bloch_source takes them (needs bloch_phase).  dispersion = (wp2, gamma, omega0) as
    set_dispersion takes them: one Drude-Lorentz pole per member (boundary "pml" or "periodic", not with bloch_phase).
    boundary "lattice": every member is the unit cell of a rectangular lattice (periods R - 1 and C - 1, no layer:
    pml_cells is not read) and bloch_phase = (phi_rows, phi_cols), each a scalar or (B,), gives its two Bloch phases
    (set_lattice_phase; default zero); every returned array is complex.  A band-path sweep is one call: B copies of the
    unit cell with the phases of the k-points along the path.  bloch_dispersion = (wp2, gamma, omega0) as
    set_bloch_dispersion takes them: the pole of a run with complex fields (boundary "periodic" with bloch_phase, or
    "lattice"): a metal unit cell swept over the angle of incidence or along a band path.  flux_lines with flux_omegas
    (boundary "pml" or "periodic", not with bloch_phase): flux monitors as set_flux_lines takes them, sampled every
    `dft_every` steps; the float64 (B, N, F) flux array of BatchEngine.flux() is then appended to the returned tuple.
    bloch_flux_lines with bloch_flux_omegas (boundary "periodic" with bloch_phase): the same on the complex fields of a
    Bloch run, as set_bloch_flux_lines takes them; the flux array is appended likewise.
    polarization "hz" (boundary "pml" or "periodic" alone, not with bloch_phase, flux_lines or bloch_flux_lines): the run
    advances Hz with Ex and Ey (set_polarization); the source, the DFTs and the probes act on Hz, dispersion acts on Ex
    and Ey, and the first three returned arrays are (Hz, Ex, Ey).  conductivity: None, or a scalar or (B, R, C) as
    set_conductivity takes it, in either polarisation.  hz_flux_lines with hz_flux_omegas (polarization "hz" alone): flux
    monitors as set_hz_flux_lines takes them, sampled every `dft_every` steps; the flux array is appended as with
    flux_lines.  hz_bloch_phase (polarization "hz" with boundary "periodic" alone): a scalar or (B,) in radians, the
    Bloch phase of set_hz_bloch_phase; every returned array is then complex, dispersion and conductivity act under the
    phase, source_weights goes to set_hz_bloch_source, and omega and hz_flux_lines are not available.
    hz_bloch_flux_lines with hz_bloch_flux_omegas (with hz_bloch_phase alone): flux monitors as set_hz_bloch_flux_lines
    takes them, sampled every `dft_every` steps; the flux array is appended as with flux_lines.
    hz_lattice_phase = (phi_rows, phi_cols), each a scalar or (B,) (polarization "hz" with boundary "periodic" alone,
    without a layer: pml_cells must be 0 or None): the lattice mode of set_hz_lattice_phase, every member the unit cell of a
    rectangular lattice with E in the plane; every returned array is complex, conductivity and dispersion may fill the
    period, source_weights goes to set_hz_bloch_source; not with hz_bloch_phase, omega or flux lines of any kind.
    """
    from .api import MU0
    eps = np.asarray(eps)
    if eps.ndim != 3:
        raise ValueError(f"eps must have shape (B, R, C), got {eps.shape}")
    B, R, Cc = eps.shape
    mu = MU0 if mu is None else mu
    mu_arr = np.asarray(mu)
    if mu_arr.ndim not in (0, 3) or (mu_arr.ndim == 3 and mu_arr.shape != eps.shape):
        raise ValueError(f"mu must be a scalar or have shape {eps.shape}, got {mu_arr.shape}")
    mu_min = mu_arr.reshape(B, -1).min(axis=1) if mu_arr.ndim == 3 else np.full(B, float(mu_arr))
    courant = (1 / np.sqrt(eps.reshape(B, -1).min(axis=1) * mu_min) * dt) / dx
    assert np.all(courant <= 1.0), \
        f"Courant stability condition not met: members {np.nonzero(~(courant <= 1.0))[0].tolist()} > 1.0"
    fcs = np.broadcast_to(np.asarray(fc, dtype=np.float64), (B,))
    if hz_lattice_phase is not None:
        if polarization != "hz":
            raise ValueError('hz_lattice_phase needs polarization="hz": in the Ez polarisation use boundary="lattice"')
        if boundary != "periodic":
            raise ValueError(f'hz_lattice_phase needs boundary="periodic", not {boundary!r}')
        if hz_bloch_phase is not None:
            raise ValueError("hz_lattice_phase and hz_bloch_phase exclude each other")
        if not isinstance(hz_lattice_phase, (tuple, list)) or len(hz_lattice_phase) != 2:
            raise ValueError(f"hz_lattice_phase must be (phi_rows, phi_cols), got {hz_lattice_phase!r}")
        for v, nm in zip(hz_lattice_phase, ("phi_rows", "phi_cols")):
            if np.shape(v) not in ((), (B,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({B},), got {np.shape(v)}")
            if not np.all(np.isfinite(np.asarray(v, dtype=np.float64))):
                raise ValueError(f"{nm} must be finite")
        if omega is not None:
            raise ValueError("omega (the whole-grid transform) is not available with hz_lattice_phase: use dft_window")
        for given, nm in ((flux_lines, "flux_lines"), (bloch_flux_lines, "bloch_flux_lines"),
                          (hz_flux_lines, "hz_flux_lines"), (hz_bloch_flux_lines, "hz_bloch_flux_lines")):
            if given is not None:
                raise ValueError(f"{nm} is not available with hz_lattice_phase: the lattice mode has no flux lines")
        if pml_cells:
            raise ValueError(f"hz_lattice_phase is not available with a layer (pml_cells={pml_cells!r}): the lattice mode "
                             "has none, pass pml_cells=0")
    layered = boundary == "pml" or (boundary == "periodic" and pml_cells)
    if boundary == "periodic" and layered and not pml_fits(R, Cc, int(pml_cells), True):
        raise ValueError(f"a {int(pml_cells)}-cell PML does not fit {R}x{Cc} periodic members (2L + 3 <= rows): the "
                         f"largest that does is {(R - 3) // 2}")
    if boundary == "pml":
        L = int(pml_cells)
        if not pml_fits(R, Cc, L):
            raise ValueError(f"a {L}-cell PML does not fit {R}x{Cc} members (2L + 3 <= min(rows, cols)): the largest "
                             f"that does is {(min(R, Cc) - 3) // 2}")
    if layered:
        L = int(pml_cells)
        m00 = mu_arr[:, 0, 0] if mu_arr.ndim == 3 else np.full(B, float(mu_arr))
        courant00 = np.array([(1 / np.sqrt(float(e) * float(u)) * dt) / dx for e, u in zip(eps[:, 0, 0], m00)])
    lattice = boundary == "lattice"
    if lattice:
        if bloch_phase is None:
            bloch_phase = (0.0, 0.0)
        if not isinstance(bloch_phase, (tuple, list)) or len(bloch_phase) != 2:
            raise ValueError(f'boundary="lattice" takes bloch_phase=(phi_rows, phi_cols), got {bloch_phase!r}')
        for v, nm in zip(bloch_phase, ("phi_rows", "phi_cols")):
            if np.shape(v) not in ((), (B,)):
                raise ValueError(f"{nm} must be a scalar or have shape ({B},), got {np.shape(v)}")
        if dispersion is not None:
            raise ValueError('dispersion is not available with boundary="lattice"')
    if bloch_phase is not None and boundary not in ("periodic", "lattice"):
        raise ValueError(f'bloch_phase needs boundary="periodic" or "lattice", not {boundary!r}')
    if source_weights is not None and bloch_phase is None and hz_bloch_phase is None and hz_lattice_phase is None:
        raise ValueError("source_weights needs bloch_phase")
    if bloch_phase is not None and omega is not None:
        raise ValueError("omega (the whole-grid transform) is not available with bloch_phase: use dft_window")
    if polarization not in ("ez", "hz"):
        raise ValueError(f'polarization must be "ez" or "hz", got {polarization!r}')
    if polarization == "hz":
        if boundary not in ("pml", "periodic"):
            raise ValueError(f'polarization="hz" needs boundary="pml" or "periodic", not {boundary!r}')
        for given, nm in ((bloch_phase, "bloch_phase"), (flux_lines, "flux_lines"), (bloch_flux_lines, "bloch_flux_lines"),
                          (bloch_dispersion, "bloch_dispersion")):
            if given is not None:
                raise ValueError(f'{nm} is not available with polarization="hz"')
    if hz_bloch_phase is not None:
        if polarization != "hz":
            raise ValueError('hz_bloch_phase needs polarization="hz": in the Ez polarisation use bloch_phase')
        if boundary != "periodic":
            raise ValueError(f'hz_bloch_phase needs boundary="periodic", not {boundary!r}')
        if np.shape(hz_bloch_phase) not in ((), (B,)):
            raise ValueError(f"hz_bloch_phase must be a scalar or have shape ({B},), got {np.shape(hz_bloch_phase)}")
        if not np.all(np.isfinite(np.asarray(hz_bloch_phase, dtype=np.float64))):
            raise ValueError("hz_bloch_phase must be finite")
        if omega is not None:
            raise ValueError("omega (the whole-grid transform) is not available with hz_bloch_phase: use dft_window")
        if hz_flux_lines is not None:
            raise ValueError("hz_flux_lines is not available with hz_bloch_phase")
    if (hz_bloch_flux_lines is None) != (hz_bloch_flux_omegas is None):
        raise ValueError("hz_bloch_flux_lines and hz_bloch_flux_omegas must be given together")
    if hz_bloch_flux_lines is not None:
        if hz_bloch_phase is None:
            raise ValueError("hz_bloch_flux_lines needs hz_bloch_phase: without a phase use hz_flux_lines")
        _flux_lines(hz_bloch_flux_lines, hz_bloch_flux_omegas, dft_every, B, R, Cc, True)
    if (hz_flux_lines is None) != (hz_flux_omegas is None):
        raise ValueError("hz_flux_lines and hz_flux_omegas must be given together")
    if hz_flux_lines is not None:
        if polarization != "hz":
            raise ValueError('hz_flux_lines needs polarization="hz": in the Ez polarisation use flux_lines')
        _flux_lines(hz_flux_lines, hz_flux_omegas, dft_every, B, R, Cc, boundary == "periodic")
    if dispersion is not None:
        if len(dispersion) != 3:
            raise ValueError("dispersion must be (wp2, gamma, omega0)")
        if boundary not in ("pml", "periodic"):
            raise ValueError(f'dispersion needs boundary="pml" or "periodic", not {boundary!r}')
        if bloch_phase is not None:
            raise ValueError("dispersion is not available with bloch_phase")
    if bloch_dispersion is not None:
        if len(bloch_dispersion) != 3:
            raise ValueError("bloch_dispersion must be (wp2, gamma, omega0)")
        if bloch_phase is None:
            raise ValueError('bloch_dispersion needs bloch_phase (boundary="periodic") or boundary="lattice": without a '
                             "phase use dispersion")
        if dispersion is not None:
            raise ValueError("bloch_dispersion and dispersion exclude each other")
    win, wom, cells = _check_monitors(B, R, Cc, dft_window, window_omegas, probes, dft_every)
    if (flux_lines is None) != (flux_omegas is None):
        raise ValueError("flux_lines and flux_omegas must be given together")
    if flux_lines is not None:
        if boundary not in ("pml", "periodic"):
            raise ValueError(f'flux_lines needs boundary="pml" or "periodic", not {boundary!r}')
        if bloch_phase is not None:
            raise ValueError("flux_lines is not available with bloch_phase")
        _flux_lines(flux_lines, flux_omegas, dft_every, B, R, Cc, boundary == "periodic")
    if (bloch_flux_lines is None) != (bloch_flux_omegas is None):
        raise ValueError("bloch_flux_lines and bloch_flux_omegas must be given together")
    if bloch_flux_lines is not None:
        if boundary != "periodic" or bloch_phase is None:
            raise ValueError(f'bloch_flux_lines needs boundary="periodic" and bloch_phase (boundary {boundary!r}'
                             f'{"" if bloch_phase is not None else ", no bloch_phase"}): without a phase use flux_lines')
        if flux_lines is not None:
            raise ValueError("bloch_flux_lines and flux_lines exclude each other")
        _flux_lines(bloch_flux_lines, bloch_flux_omegas, dft_every, B, R, Cc, True)
    if bloch_phase is not None:
        if win is not None and win[1] + win[3] > Cc - 1:
            raise ValueError(f"dft_window {win} touches column {Cc - 1}, the image of column 0: not with bloch_phase")
        if cells is not None and np.any(cells[..., 1] >= Cc - 1):
            raise ValueError(f"a probe lies in column {Cc - 1}, the image of column 0: not with bloch_phase")
    if hz_bloch_phase is not None:
        if win is not None and win[1] + win[3] > Cc - 1:
            raise ValueError(f"dft_window {win} touches column {Cc - 1}, the image of column 0: not with hz_bloch_phase")
        if cells is not None and np.any(cells[..., 1] >= Cc - 1):
            raise ValueError(f"a probe lies in column {Cc - 1}, the image of column 0: not with hz_bloch_phase")
    if hz_lattice_phase is not None:
        if win is not None and (win[0] + win[2] > R - 1 or win[1] + win[3] > Cc - 1):
            raise ValueError(f"dft_window {win} touches row {R - 1} or column {Cc - 1}, the images of row 0 and column 0: "
                             "not with hz_lattice_phase")
        if cells is not None and (np.any(cells[..., 0] >= R - 1) or np.any(cells[..., 1] >= Cc - 1)):
            raise ValueError(f"a probe lies in row {R - 1} or column {Cc - 1}, the images of row 0 and column 0: not with "
                             "hz_lattice_phase")
    if lattice:
        if win is not None and win[0] + win[2] > R - 1:
            raise ValueError(f'dft_window {win} touches row {R - 1}, the image of row 0: not with boundary="lattice"')
        if cells is not None and np.any(cells[..., 0] >= R - 1):
            raise ValueError(f'a probe lies in row {R - 1}, the image of row 0: not with boundary="lattice"')
    with BatchEngine(B, R, Cc, dt, dx, dtype=dtype, boundary=boundary, device=device) as eng:
        if polarization == "hz":
            eng.set_polarization("hz")
        eng.set_materials(eps, mu)
        if layered:
            eng.set_pml(L, courant00=courant00)
        if hz_lattice_phase is not None:      # first: the mode lifts the row margin of the conductivity and the pole
            eng.set_hz_lattice_phase(*hz_lattice_phase)
            if source_weights is not None:
                eng.set_hz_bloch_source(source_weights)
        eng.set_sources(sources)
        if conductivity is not None:
            eng.set_conductivity(conductivity)
        if dispersion is not None:
            eng.set_dispersion(*dispersion)
        if lattice:
            eng.set_lattice_phase(*bloch_phase)
        elif bloch_phase is not None:
            eng.set_bloch_phase(bloch_phase)
        if bloch_phase is not None:
            if source_weights is not None:
                eng.set_bloch_source(source_weights)
        if bloch_dispersion is not None:
            eng.set_bloch_dispersion(*bloch_dispersion)
        if hz_bloch_phase is not None:
            eng.set_hz_bloch_phase(hz_bloch_phase)
            if source_weights is not None:
                eng.set_hz_bloch_source(source_weights)
        if omega is not None:
            eng.set_dft(omega, dft_every)
        if win is not None:
            eng.set_dft_window(win, wom, dft_every)
        if cells is not None:
            eng.set_probes(cells, max(1, int(nsteps)))
        if flux_lines is not None:
            eng.set_flux_lines(flux_lines, flux_omegas, dft_every)
        if bloch_flux_lines is not None:
            eng.set_bloch_flux_lines(bloch_flux_lines, bloch_flux_omegas, dft_every)
        if hz_flux_lines is not None:
            eng.set_hz_flux_lines(hz_flux_lines, hz_flux_omegas, dft_every)
        if hz_bloch_flux_lines is not None:
            eng.set_hz_bloch_flux_lines(hz_bloch_flux_lines, hz_bloch_flux_omegas, dft_every)
        eng.run(nsteps, None if waveform is None else _waveform_amps(waveform, fcs, nsteps, dt))
        out = eng.download()
        if omega is not None:
            out += (eng.read_dft(),)
        if win is not None:
            out += (eng.read_dft_window(),)
        if cells is not None:
            out += (eng.read_probes(0, int(nsteps)),)
        if (flux_lines is not None or bloch_flux_lines is not None or hz_flux_lines is not None or
                hz_bloch_flux_lines is not None):
            out += (eng.flux(),)
        return out


def _check_monitors(B, R, Cc, dft_window, window_omegas, probes, every):
    """run_fdtd_batch's monitor arguments, checked on the host as the library would refuse them: (window, (B, F)
    omegas, (B, P, 2) cells), None where not given."""
    win = wom = cells = None
    if (dft_window is None) != (window_omegas is None):
        raise ValueError("dft_window and window_omegas must be given together")
    if dft_window is not None:
        w = np.asarray(dft_window)
        if w.shape != (4,) or not np.issubdtype(w.dtype, np.integer):
            raise ValueError(f"dft_window must be 4 integers (row0, col0, nrows, ncols), got {dft_window!r}")
        r0, c0, nr, nc = (int(v) for v in w)
        if nr < 1 or nc < 1 or r0 < 0 or c0 < 0 or r0 + nr > R or c0 + nc > Cc:
            raise ValueError(f"dft_window {(r0, c0, nr, nc)} is empty or leaves the {R}x{Cc} grid")
        wom = _window_omegas(window_omegas, B)
        if not 1 <= wom.shape[1] <= _abi.BATCH_MAX_DFT_FREQS:
            raise ValueError(f"window_omegas must hold 1..{_abi.BATCH_MAX_DFT_FREQS} frequencies, got {wom.shape[1]}")
        if not np.all(np.isfinite(wom)):
            raise ValueError("window_omegas must be finite")
        if int(every) < 1:
            raise ValueError(f"dft_every must be >= 1, got {every}")
        win = (r0, c0, nr, nc)
    if probes is not None:
        cells = _probe_cells(probes, B)
        if not 1 <= cells.shape[1] <= _abi.BATCH_MAX_PROBES:
            raise ValueError(f"probes must hold 1..{_abi.BATCH_MAX_PROBES} cells per member, got {cells.shape[1]}")
        r, c = cells[..., 0], cells[..., 1]
        if np.any(r < 0) or np.any(r >= R) or np.any(c < 0) or np.any(c >= Cc):
            raise ValueError(f"probe cells must lie in the {R}x{Cc} grid")
    return win, wom, cells
