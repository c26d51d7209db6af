"""ctypes binding of libfdtd2d.so (include/fdtd2d.h).

This is the whole FFI: plain pointers and sizes, no torch types.  The library is
built in-tree by ``__graft_entry__.build()`` / ``fdtd-2d_amd/csrc/Makefile`` and is
required: there is no CPU fallback, a missing library or device raises.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# FDTD2D_ARITHMETIC=fused selects the tolerance build (libfdtd2d_fused.so: multiply-add pairs contracted into FMA,
# results within rounding of the reference's); default "exact" = value-identical to the reference.
# FDTD2D_LIB: alternative build of the same library (kernel A/B experiments only)
ARITHMETIC = os.environ.get("FDTD2D_ARITHMETIC", "exact")
if ARITHMETIC not in ("exact", "fused"):
    raise ImportError(f"FDTD2D_ARITHMETIC must be 'exact' or 'fused', not {ARITHMETIC!r}")
LIB_PATH = os.environ.get("FDTD2D_LIB") or os.path.join(
    HERE, "libfdtd2d.so" if ARITHMETIC == "exact" else "libfdtd2d_fused.so")

F32, F64 = 0, 1
BOUNDARY_NONE, BOUNDARY_MUR5, BOUNDARY_PML = 0, 1, 2
SRC_NONE, SRC_RICKER, SRC_SINUSOIDAL = 0, 1, 2
FIELD_EZ, FIELD_HX, FIELD_HY = 0, 1, 2

OPT_MAX_PASS_STEPS, OPT_BAND_ROWS, OPT_ZONE_SPLIT, OPT_LEVEL_SPLIT, OPT_SPLIT_WAVES, OPT_AUTOTUNE, OPT_XCD_MAP, OPT_SIDE_WAVES = 0, 1, 2, 3, 4, 5, 7, 8
OPT_ACTIVE_WINDOW = 9
OPT_WINDOW_OCTAGON = 10

E_ARG, E_NODEVICE, E_NOMEM, E_STATE, E_COURANT = -1, -2, -3, -4, -5

(INFO_ROWS, INFO_COLS, INFO_ROW0, INFO_NROWS, INFO_HALO, INFO_PITCH, INFO_DTYPE,
 INFO_BOUNDARY, INFO_DEVICE, INFO_EPS_UNIFORM, INFO_MU_UNIFORM, INFO_E_VALID_LO,
 INFO_E_VALID_HI, INFO_H_VALID_LO, INFO_H_VALID_HI, INFO_STEP, INFO_PASS_LAUNCHES,
 INFO_STEP_LAUNCHES, INFO_CYCLE_STEPS, INFO_LAST_BAND_ROWS, INFO_LAST_WAVES, INFO_LAST_EDGE_ROWS,
 INFO_LAST_PASS_STEPS, INFO_LAST_SIDE_WAVES, INFO_LAST_XCD_MAP) = range(25)
(INFO_WINDOW_ROW_LO, INFO_WINDOW_ROW_HI, INFO_WINDOW_COL_LO, INFO_WINDOW_COL_HI, INFO_WINDOWED_LAUNCHES,
 INFO_WINDOW_ENABLED) = range(25, 31)
# what the last windowed pass launched (read-only; fdtd2d.h)
(INFO_WIN_BAND_ROWS, INFO_WIN_WAVES, INFO_WIN_STRIP_FIRST, INFO_WIN_INNER, INFO_WIN_N_SRC, INFO_WIN_EDGES, INFO_WIN_ZTOP,
 INFO_WIN_ZBOT, INFO_WIN_XCD_MAP, INFO_WIN_XCD_PAD, INFO_WIN_EDGE_ROWS) = range(31, 42)
# its diagonal bounds (closed ranges of i + j and of i - j) and the bulk tasks skipped for them
(OCT_INFO_SUM_LO, OCT_INFO_SUM_HI, OCT_INFO_DIFF_LO, OCT_INFO_DIFF_HI, OCT_INFO_SKIPPED) = range(42, 47)
OCT_UNBOUNDED = 1 << 29

(BATCH_INFO_COUNT, BATCH_INFO_ROWS, BATCH_INFO_COLS, BATCH_INFO_DTYPE, BATCH_INFO_STEP, BATCH_INFO_RESIDENT,
 BATCH_INFO_LAUNCHES, BATCH_INFO_RESIDENT_MAX_CELLS, BATCH_INFO_LDS_BYTES, BATCH_INFO_PITCH) = range(10)
BATCH_OPT_RESIDENT, BATCH_OPT_STEPS_PER_LAUNCH = 0, 1
# include/fdtd2d_batch_monitor.h
BATCH_INFO_DFT_WINDOW_LDS, BATCH_INFO_PROBE_SAMPLES = 10, 11
BATCH_OPT_DFT_WINDOW_LDS = 2
BATCH_MAX_DFT_FREQS, BATCH_MAX_PROBES = 16, 64
# include/fdtd2d_batch_adjoint.h
BATCH_INFO_POINT_SOURCES, BATCH_INFO_HELD_WINDOW = 12, 13
BATCH_MAX_POINT_SOURCES, BATCH_MAX_CHANNELS = 64, 32
# include/fdtd2d_batch_lossy.h
BATCH_INFO_LOSSY = 14
# include/fdtd2d_batch_periodic.h
BATCH_INFO_PERIODIC = 15
# include/fdtd2d_batch_bloch.h
BATCH_INFO_BLOCH = 16
# include/fdtd2d_batch_bloch_adjoint.h
BATCH_INFO_BLOCH_POINT_SOURCES, BATCH_INFO_HELD_BLOCH_WINDOW = 17, 18
# include/fdtd2d_batch_dispersive.h
BATCH_INFO_DISPERSIVE = 19
# include/fdtd2d_batch_dispersive_adjoint.h
BATCH_INFO_HELD_DISPERSIVE_WINDOW = 20
BATCH_MAX_PRODUCT_SETS = 3
# include/fdtd2d_batch_flux.h
BATCH_INFO_FLUX_LINES, BATCH_INFO_FLUX_LDS = 21, 22
BATCH_OPT_FLUX_LDS = 3
BATCH_MAX_FLUX_LINES, BATCH_MAX_FLUX_FREQS = 4, 16
# include/fdtd2d_batch_flux_adjoint.h: FDTD2D_BATCH_INFO_FLUX_LINE_SOURCES.  Named apart from the BATCH_INFO_* above:
# fdtd2d_batch_bloch_flux.h's check that it added no id pins the largest of those names at 22
BATCH_FLUX_LINE_SOURCES_INFO = 23

_vp, _i, _d, _ll = C.c_void_p, C.c_int, C.c_double, C.c_longlong

# name -> (restype, argtypes); every symbol include/fdtd2d.h declares
SIGNATURES = {
    "fdtd2d_create": (_i, [C.POINTER(_vp), _i, _i, _d, _d, _i, _i, _i]),
    "fdtd2d_create_slab": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _d, _d, _i, _i, _i]),
    "fdtd2d_destroy": (None, [_vp]),
    "fdtd2d_last_error": (C.c_char_p, [_vp]),
    "fdtd2d_info": (_ll, [_vp, _i]),
    "fdtd2d_set_stream": (_i, [_vp, _vp]),
    "fdtd2d_set_materials": (_i, [_vp, _vp, _vp, _i, C.POINTER(_d), _i]),
    "fdtd2d_set_materials_uniform": (_i, [_vp, _d, _d]),
    "fdtd2d_set_pml": (_i, [_vp, _vp, _vp, _i, _i]),
    "fdtd2d_transfer_ezx": (_i, [_vp, _vp, _i, _i]),
    "fdtd2d_courant": (_d, [_vp]),
    "fdtd2d_upload": (_i, [_vp, _vp, _vp, _vp, _i]),
    "fdtd2d_download": (_i, [_vp, _vp, _vp, _vp, _i]),
    "fdtd2d_reset": (_i, [_vp]),
    "fdtd2d_update_h": (_i, [_vp]),
    "fdtd2d_update_e": (_i, [_vp]),
    "fdtd2d_add_point": (_i, [_vp, _i, _i, _d]),
    "fdtd2d_set_source_extent": (_i, [_vp, _i, _i]),
    "fdtd2d_prepare": (_i, [_vp, _i]),
    "fdtd2d_prepare_run": (_i, [_vp, _i, _i, _i, _i]),
    "fdtd2d_set_probe": (_i, [_vp, _i, _i, C.c_longlong]),
    "fdtd2d_read_probe": (_i, [_vp, _vp, C.c_longlong, C.c_longlong]),
    "fdtd2d_run": (_i, [_vp, _i, _i, _i, C.POINTER(_d)]),
    "fdtd2d_pass_rows": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(_d)]),
    "fdtd2d_pass_commit": (_i, [_vp]),
    "fdtd2d_run_waveform": (_i, [_vp, _i, _i, _i, _i, _d, _ll]),
    "fdtd2d_source_amplitude": (_d, [_i, _d, _d]),
    "fdtd2d_set_option": (_i, [_vp, _i, _ll]),
    "fdtd2d_set_shape": (_i, [_vp, _i, C.POINTER(_i), _i]),
    "fdtd2d_last_shape": (_i, [_vp, C.POINTER(_i), _i]),
    "fdtd2d_sync": (_i, [_vp]),
    "fdtd2d_halo_bytes": (_ll, [_vp]),
    "fdtd2d_halo_pack": (_i, [_vp, _i, _vp]),
    "fdtd2d_halo_unpack": (_i, [_vp, _i, _vp]),
    "fdtd2d_slab_attach": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fdtd2d_rccl_unique_id": (_i, [_vp]),
    "fdtd2d_rccl_selftest": (_i, [_i, _ll]),
    "fdtd2d_slab_attach_rccl": (_i, [_vp, _vp, _i, _i]),
    "fdtd2d_slab_detach": (_i, [_vp]),
    "fdtd2d_slab_ranks": (_ll, [_vp]),
    "fdtd2d_run_slab": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(_d)]),
    "fdtd2d_set_dft": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(_d), _i]),
    "fdtd2d_read_dft": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_snapshot_index": (_i, [_vp, _d, _d, _i, _vp]),
    "fdtd2d_reduce": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_timer_start": (_i, [_vp]),
    "fdtd2d_timer_stop": (_i, [_vp, C.POINTER(C.c_float)]),
    "fdtd2d_time_launches": (_i, [_vp, _i, _i, C.POINTER(C.c_float)]),
    "fdtd2d_clock_probe_start": (_i, [_vp, _i]),
    "fdtd2d_measure_copy": (_i, [_vp, _i, C.POINTER(_d)]),
    "fdtd2d_clock_probe_read": (_i, [_vp, C.POINTER(_d)]),
    "fdtd2d_bytes_per_cell_step": (_i, [_vp]),
    "fdtd2d_device_ptr": (_vp, [_vp, _i]),
    "fdtd2d_version": (C.c_char_p, []),
    # batched grids
    "fdtd2d_batch_create": (_i, [C.POINTER(_vp), _i, _i, _i, _d, _d, _i, _i, _i]),
    "fdtd2d_batch_destroy": (None, [_vp]),
    "fdtd2d_batch_last_error": (C.c_char_p, [_vp]),
    "fdtd2d_batch_info": (_ll, [_vp, _i]),
    "fdtd2d_batch_set_option": (_i, [_vp, _i, _ll]),
    "fdtd2d_batch_set_stream": (_i, [_vp, _vp]),
    "fdtd2d_batch_set_materials": (_i, [_vp, _vp, _vp, _i]),
    "fdtd2d_batch_set_materials_uniform": (_i, [_vp, _d, _d]),
    "fdtd2d_batch_courant": (_i, [_vp, C.POINTER(_d)]),
    "fdtd2d_batch_upload": (_i, [_vp, _vp, _vp, _vp, _i]),
    "fdtd2d_batch_download": (_i, [_vp, _vp, _vp, _vp, _i]),
    "fdtd2d_batch_reset": (_i, [_vp]),
    "fdtd2d_batch_set_sources": (_i, [_vp, C.POINTER(_i)]),
    "fdtd2d_batch_run": (_i, [_vp, _i, C.POINTER(_d)]),
    "fdtd2d_batch_run_waveform": (_i, [_vp, _i, _i, C.POINTER(_d), _ll]),
    "fdtd2d_batch_set_dft": (_i, [_vp, C.POINTER(_d), _i]),
    "fdtd2d_batch_read_dft": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_sync": (_i, [_vp]),
}

# every symbol include/fdtd2d_batch_pml.h declares (the batch's PML, a companion of fdtd2d.h)
BATCH_PML_SIGNATURES = {
    "fdtd2d_batch_set_pml": (_i, [_vp, _vp, _vp, _i, _i]),
    "fdtd2d_batch_transfer_ezx": (_i, [_vp, _vp, _i, _i]),
}

# every symbol include/fdtd2d_batch_monitor.h declares (window DFT and probes of a batch, a companion of fdtd2d.h)
BATCH_MONITOR_SIGNATURES = {
    "fdtd2d_batch_set_dft_window": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(_d), _i]),
    "fdtd2d_batch_read_dft_window": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_set_probes": (_i, [_vp, _i, C.POINTER(_i), _ll]),
    "fdtd2d_batch_read_probes": (_i, [_vp, C.POINTER(_d), _ll, _ll]),
}

# every symbol include/fdtd2d_batch_adjoint.h declares (point sources with channels, the held window and its product)
BATCH_ADJOINT_SIGNATURES = {
    "fdtd2d_batch_set_point_sources": (_i, [_vp, _i, C.POINTER(_i), _i, C.POINTER(_d)]),
    "fdtd2d_batch_run_channels": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d), _i]),
    "fdtd2d_batch_hold_dft_window": (_i, [_vp]),
    "fdtd2d_batch_dft_window_product": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
}

# every symbol include/fdtd2d_batch_design.h declares (probe spectra, field maxima and a permittivity window on the device)
BATCH_DESIGN_SIGNATURES = {
    "fdtd2d_batch_probe_spectra": (_i, [_vp, _i, C.POINTER(_d), _ll, _ll, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_field_absmax": (_i, [_vp, _i, C.POINTER(_d)]),
    "fdtd2d_batch_set_eps_window": (_i, [_vp, _i, _i, _i, _i, _vp, _i]),
}

# every symbol include/fdtd2d_batch_lossy.h declares (an electric conductivity per cell of a batch)
BATCH_LOSSY_SIGNATURES = {
    "fdtd2d_batch_set_conductivity": (_i, [_vp, _vp, _i]),
    "fdtd2d_batch_set_conductivity_window": (_i, [_vp, C.POINTER(_i), _vp, _i]),
}

# every symbol include/fdtd2d_batch_periodic.h declares (periodic columns of a batch)
BATCH_PERIODIC_SIGNATURES = {
    "fdtd2d_batch_set_periodic": (_i, [_vp, _i]),
}

# every symbol include/fdtd2d_batch_bloch.h declares (a Bloch phase for a periodic batch: complex fields)
BATCH_BLOCH_SIGNATURES = {
    "fdtd2d_batch_set_bloch": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_set_bloch_source": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_run_bloch": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_transfer_bloch": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "fdtd2d_batch_read_dft_window_bloch": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_read_probes_bloch": (_i, [_vp, C.POINTER(_d), _ll, _ll]),
}

# every symbol include/fdtd2d_batch_bloch_adjoint.h declares (point sources, the held window, its product, probe spectra and
# field maxima of a Bloch batch: what an adjoint run of complex fields needs)
BATCH_BLOCH_ADJOINT_SIGNATURES = {
    "fdtd2d_batch_set_bloch_point_sources": (_i, [_vp, _i, C.POINTER(_i), _i, C.POINTER(_d)]),
    "fdtd2d_batch_run_bloch_channels": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), _i, _i]),
    "fdtd2d_batch_hold_bloch_window": (_i, [_vp]),
    "fdtd2d_batch_bloch_window_product": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_bloch_probe_spectra": (_i, [_vp, _i, C.POINTER(_d), _ll, _ll, C.POINTER(_d), C.POINTER(_d),
                                              C.POINTER(_d)]),
    "fdtd2d_batch_bloch_field_absmax": (_i, [_vp, _i, C.POINTER(_d)]),
}

# every symbol include/fdtd2d_batch_dispersive.h declares (a Drude-Lorentz pole per member of a batch)
BATCH_DISPERSIVE_SIGNATURES = {
    "fdtd2d_batch_set_dispersion": (_i, [_vp, _vp, _i, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_set_dispersion_window": (_i, [_vp, C.POINTER(_i), _vp, _i]),
    "fdtd2d_batch_transfer_dispersion": (_i, [_vp, _vp, _vp, _i, _i]),
}

# every symbol include/fdtd2d_batch_lattice.h declares (doubly periodic Bloch batches: the unit cell of a 2D lattice)
BATCH_LATTICE_SIGNATURES = {
    "fdtd2d_batch_set_lattice": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_is_lattice": (_i, [_vp]),
}

# every symbol include/fdtd2d_batch_bloch_dispersive.h declares (the pole of a Bloch or lattice batch: complex Jh and Q)
BATCH_BLOCH_DISPERSIVE_SIGNATURES = {
    "fdtd2d_batch_set_bloch_dispersion": (_i, [_vp, _vp, _i, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_set_bloch_dispersion_window": (_i, [_vp, C.POINTER(_i), _vp, _i]),
    "fdtd2d_batch_transfer_bloch_dispersion": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
}

# every symbol include/fdtd2d_batch_dispersive_adjoint.h declares (the held window of a batch with a pole and its product
# for up to three coefficient sets: what the adjoint of a dispersive batch needs)
BATCH_DISPERSIVE_ADJOINT_SIGNATURES = {
    "fdtd2d_batch_hold_dispersive_window": (_i, [_vp]),
    "fdtd2d_batch_dispersive_window_product": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d),
                                                    C.POINTER(_d)]),
}

# every symbol include/fdtd2d_batch_flux.h declares (flux lines of a PML or periodic batch: the transforms of Ez and of
# the tangential H on up to 4 lines, and the power that crosses them per frequency)
BATCH_FLUX_SIGNATURES = {
    "fdtd2d_batch_set_flux_lines": (_i, [_vp, _i, C.POINTER(_i), _i, C.POINTER(_d), _i]),
    "fdtd2d_batch_read_flux_lines": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_flux": (_i, [_vp, C.POINTER(_d)]),
}
# every symbol include/fdtd2d_batch_bloch_flux.h declares (the flux lines of a batch with a Bloch phase: the sums of the
# real and of the imaginary part of the fields, and the power per member, line and frequency)
BATCH_BLOCH_FLUX_SIGNATURES = {
    "fdtd2d_batch_set_bloch_flux_lines": (_i, [_vp, _i, C.POINTER(_i), _i, C.POINTER(_d), _i]),
    "fdtd2d_batch_read_bloch_flux_lines": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_bloch_flux": (_i, [_vp, C.POINTER(_d)]),
}
# every symbol include/fdtd2d_batch_flux_adjoint.h declares (line sources on the flux lines, the transpose of the monitor,
# and the weights of the adjoint of a flux objective formed on the device)
BATCH_FLUX_ADJOINT_SIGNATURES = {
    "fdtd2d_batch_set_flux_line_sources": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_read_flux_line_sources": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_flux_line_weights": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), _i, C.POINTER(_d), C.POINTER(_d)]),
}
# every symbol include/fdtd2d_batch_bloch_flux_adjoint.h declares (complex line sources on Bloch flux lines and the
# adjoint weights formed from both parts' sums)
BATCH_BLOCH_FLUX_ADJOINT_SIGNATURES = {
    "fdtd2d_batch_set_bloch_flux_line_sources": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d),
                                                      C.POINTER(_d)]),
    "fdtd2d_batch_read_bloch_flux_line_sources": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_bloch_flux_line_weights": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), _i, C.POINTER(_d), C.POINTER(_d)]),
}
# every symbol include/fdtd2d_batch_hz.h declares (the Hz polarisation of PML and periodic batches, with a conductivity and
# a Drude-Lorentz pole on Ex and Ey); the polarisation has a query of its own, no numbered info id
POL_EZ, POL_HZ = 0, 1
BATCH_HZ_SIGNATURES = {
    "fdtd2d_batch_set_polarization": (_i, [_vp, _i]),
    "fdtd2d_batch_polarization": (_i, [_vp]),
    "fdtd2d_batch_set_hz_conductivity": (_i, [_vp, _vp, _i]),
    "fdtd2d_batch_set_hz_dispersion": (_i, [_vp, _vp, _i, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_transfer_hz_dispersion": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
}
# every symbol include/fdtd2d_batch_hz_flux.h declares (flux lines in the Hz polarisation: the transforms of Hz and of the
# tangential E on up to 4 lines, and the power through each); the ids and the option are fdtd2d_batch_flux.h's
BATCH_HZ_FLUX_SIGNATURES = {
    "fdtd2d_batch_set_hz_flux_lines": (_i, [_vp, _i, C.POINTER(_i), _i, C.POINTER(_d), _i]),
    "fdtd2d_batch_read_hz_flux_lines": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_hz_flux": (_i, [_vp, C.POINTER(_d)]),
}
# every symbol include/fdtd2d_batch_hz_bloch.h declares (a Bloch phase in the Hz polarisation: complex Hz, Ex, Ey, Hzx
# and pole state).  FDTD2D_BATCH_INFO_HZ_BLOCH is named apart from the BATCH_INFO_* above, like the line sources' id
BATCH_HZ_BLOCH_INFO = 24
BATCH_HZ_BLOCH_SIGNATURES = {
    "fdtd2d_batch_set_hz_bloch": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_set_hz_bloch_source": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_run_hz_bloch": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_transfer_hz_bloch": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "fdtd2d_batch_transfer_hz_bloch_dispersion": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "fdtd2d_batch_read_dft_window_hz_bloch": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_read_probes_hz_bloch": (_i, [_vp, C.POINTER(_d), _ll, _ll]),
}
# every symbol include/fdtd2d_batch_hz_bloch_flux.h declares (flux lines under that phase: the sums of Hz and of the
# tangential E of the real and of the imaginary part of the fields, and the power per member, line and frequency); the
# ids and the option are fdtd2d_batch_flux.h's
BATCH_HZ_BLOCH_FLUX_SIGNATURES = {
    "fdtd2d_batch_set_hz_bloch_flux_lines": (_i, [_vp, _i, C.POINTER(_i), _i, C.POINTER(_d), _i]),
    "fdtd2d_batch_read_hz_bloch_flux_lines": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_hz_bloch_flux": (_i, [_vp, C.POINTER(_d)]),
}
# every symbol include/fdtd2d_batch_hz_lattice.h declares (the lattice mode in the Hz polarisation: both seams, complex
# Hz, Ex, Ey and pole state).  FDTD2D_BATCH_INFO_HZ_LATTICE is 25, written relative to the Hz Bloch phase's id
BATCH_HZ_LATTICE_INFO_ID = BATCH_HZ_BLOCH_INFO + 1
BATCH_HZ_LATTICE_SIGNATURES = {
    "fdtd2d_batch_set_hz_lattice": (_i, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "fdtd2d_batch_is_hz_lattice": (_i, [_vp]),
}

# transport callback of fdtd2d_slab_attach
EXCHANGE_FN = C.CFUNCTYPE(_i, _vp, _vp, _vp, _vp, _vp, _ll, _vp)

_lib = None


class Fdtd2dError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libfdtd2d error {code}: {msg}")
        self.code = code


def _share_torch_hip_runtime():
    """One HIP runtime per process.  ROCm wheels of torch bundle their own libamdhip64.so / libhsa-runtime64.so (same
    SONAMEs as /opt/rocm's, other files).  Imported first, torch's copies satisfy libfdtd2d.so's dependency and the process
    holds one runtime; imported AFTER libfdtd2d.so, torch maps its copies beside the system's, and the runtime that
    initialises second can find the GPU taken (round 3: "No HIP GPUs are available" in a test process after 440 tests).
    SlabRunner and bench.py need torch in the same process (streams, RCCL), so where torch is installed its copy is
    mapped first, whatever the import order.  FDTD2D_SYSTEM_HIP=1 keeps the system's runtime."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("FDTD2D_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    for d in (spec.submodule_search_locations or []) if spec else []:
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(d, "lib", name)
            if os.path.exists(path):
                try:
                    C.CDLL(path, mode=C.RTLD_GLOBAL)
                except OSError:
                    return


def load():
    """Load libfdtd2d.so and declare every prototype.  Raises if it is not built."""
    global _lib
    if _lib is None:
        _share_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C fdtd-2d_amd/csrc`). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **BATCH_PML_SIGNATURES, **BATCH_MONITOR_SIGNATURES,
                                   **BATCH_ADJOINT_SIGNATURES, **BATCH_DESIGN_SIGNATURES,
                                   **BATCH_LOSSY_SIGNATURES, **BATCH_PERIODIC_SIGNATURES,
                                   **BATCH_BLOCH_SIGNATURES, **BATCH_BLOCH_ADJOINT_SIGNATURES,
                                   **BATCH_DISPERSIVE_SIGNATURES, **BATCH_LATTICE_SIGNATURES,
                                   **BATCH_BLOCH_DISPERSIVE_SIGNATURES,
                                   **BATCH_DISPERSIVE_ADJOINT_SIGNATURES, **BATCH_FLUX_SIGNATURES,
                                   **BATCH_BLOCH_FLUX_SIGNATURES, **BATCH_FLUX_ADJOINT_SIGNATURES,
                                   **BATCH_BLOCH_FLUX_ADJOINT_SIGNATURES, **BATCH_HZ_SIGNATURES,
                                   **BATCH_HZ_FLUX_SIGNATURES, **BATCH_HZ_BLOCH_SIGNATURES,
                                   **BATCH_HZ_BLOCH_FLUX_SIGNATURES, **BATCH_HZ_LATTICE_SIGNATURES}.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(handle, rc: int):
    if rc != 0:
        msg = load().fdtd2d_last_error(handle)
        raise Fdtd2dError(rc, msg.decode() if msg else "")
    return rc


def check_batch(handle, rc: int):
    if rc != 0:
        msg = load().fdtd2d_batch_last_error(handle)
        raise Fdtd2dError(rc, msg.decode() if msg else "")
    return rc
