// fdtd2d_batch_* -- host side of the batched engine (include/fdtd2d.h, "batched grids").
// B independent members of one shape, advanced together: members whose fields fit in one workgroup's
// LDS run a whole fdtd2d_batch_run in one resident launch (k_batch_resident), the others one launch per
// half-step for the whole batch (k_batch_h / k_batch_e).  Results never depend on the path.
// fdtd2d_batch_set_pml gives a NONE batch the split-field PML: the same two paths with k_batch_resident_pml and
// k_batch_h_pml / k_batch_e_pml (kernels_batch_pml.hpp).
// With a window DFT or probes set (fdtd2d_batch_monitor.h) every path takes the monitored instance of its kernels
// (kernels_batch_monitor.hpp, instantiated in batch_monitor.hip).
// fdtd2d_batch_run_channels (fdtd2d_batch_adjoint.h) takes the point-source instances of those kernels
// (batch_adjoint.hip), which also holds the window product kernel.
// The design-loop entry points (fdtd2d_batch_design.h) launch the post-run kernels of batch_design.hip.
// With a conductivity set (fdtd2d_batch_lossy.h) every run takes the lossy kernels of batch_lossy.hip.
// With periodic columns (fdtd2d_batch_periodic.h) every run takes the periodic kernels of batch_periodic.hip.
// With a Bloch phase (fdtd2d_batch_bloch.h) every run takes the complex-field kernels of batch_bloch.hip.
// fdtd2d_batch_run_bloch_channels (fdtd2d_batch_bloch_adjoint.h) takes their point-source instances
// (batch_bloch_adjoint.hip), which also holds the product kernel of two complex windows.
// With a Drude-Lorentz pole (fdtd2d_batch_dispersive.h) every run takes the dispersive kernels of batch_dispersive.hip.
// In the lattice mode (fdtd2d_batch_lattice.h: Bloch conditions on both pairs of edges) every run takes the kernels of
// batch_lattice.hip; the mode shares the Bloch phase's host state (`bloch` is set too) and adds the row rotation.
// With the pole of fdtd2d_batch_bloch_dispersive.h a Bloch or lattice batch takes the kernels of
// batch_bloch_dispersive.hip; the pole shares the host state of fdtd2d_batch_dispersive.h's (`dcj` is set too) and adds
// the imaginary parts of Jh and Q.
// With flux lines (fdtd2d_batch_flux.h) a PML or periodic batch takes the kernels of batch_flux.hip, with or without a
// pole; a lossless PML batch then holds an all-zero conductivity of its own (sigma_implicit), like a batch with a pole.
// With the lines of fdtd2d_batch_bloch_flux.h a Bloch batch takes the kernels of batch_bloch_flux.hip, with or without
// the complex pole; the lines share the host state of fdtd2d_batch_flux.h's (`flux_nl` is set too) and add the sums of
// the imaginary part.
// With the lines of fdtd2d_batch_hz_flux.h a batch in the Hz polarisation takes the kernels of batch_hz_flux.hip, with or
// without a conductivity and a pole; the lines share that host state too (`hzflux` beside `flux_nl`).
// With the lines of fdtd2d_batch_hz_bloch_flux.h an Hz Bloch batch takes the kernels of batch_hz_bloch_flux.hip; the lines
// share the host state of the Ez Bloch lines (`hzbflux` beside `flux_nl`, the imaginary part's sums in flux_acc_im).
// In the lattice mode of the Hz polarisation (fdtd2d_batch_hz_lattice.h) a batch holds `hz`, `bloch` and `lattice`
// together: the host state of the Hz Bloch phase with the row rotation of the lattice mode and no Hzx; every run takes the
// kernels of batch_hz_lattice.hip.
// With the phase of fdtd2d_batch_hz_bloch.h a periodic batch in the Hz polarisation holds `hz` and `bloch` together: the
// imaginary parts, the rotations, the weights and the monitors are the Bloch phase's, a pole adds the imaginary parts of
// Jx, Qx (djh_im, dq_im) and Jy, Qy (djy_im, dqy_im), and every run takes the kernels of batch_hz_bloch.hip.
#include "../../include/fdtd2d.h"
#include "../../include/fdtd2d_batch_adjoint.h"
#include "../../include/fdtd2d_batch_bloch.h"
#include "../../include/fdtd2d_batch_bloch_adjoint.h"
#include "../../include/fdtd2d_batch_bloch_dispersive.h"
#include "../../include/fdtd2d_batch_bloch_flux.h"
#include "../../include/fdtd2d_batch_bloch_flux_adjoint.h"
#include "../../include/fdtd2d_batch_design.h"
#include "../../include/fdtd2d_batch_dispersive.h"
#include "../../include/fdtd2d_batch_dispersive_adjoint.h"
#include "../../include/fdtd2d_batch_flux.h"
#include "../../include/fdtd2d_batch_flux_adjoint.h"
#include "../../include/fdtd2d_batch_hz.h"
#include "../../include/fdtd2d_batch_hz_bloch.h"
#include "../../include/fdtd2d_batch_hz_bloch_flux.h"
#include "../../include/fdtd2d_batch_hz_lattice.h"
#include "../../include/fdtd2d_batch_hz_flux.h"
#include "../../include/fdtd2d_batch_lattice.h"
#include "../../include/fdtd2d_batch_lossy.h"
#include "../../include/fdtd2d_batch_monitor.h"
#include "../../include/fdtd2d_batch_periodic.h"
#include "../../include/fdtd2d_batch_pml.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "kernels_batch.hpp"
#include "kernels_batch_adjoint.hpp"
#include "kernels_batch_bloch.hpp"
#include "kernels_batch_bloch_adjoint.hpp"
#include "kernels_batch_bloch_dispersive.hpp"
#include "kernels_batch_bloch_flux.hpp"
#include "kernels_batch_bloch_flux_adjoint.hpp"
#include "kernels_batch_design.hpp"
#include "kernels_batch_dispersive.hpp"
#include "kernels_batch_flux.hpp"
#include "kernels_batch_flux_adjoint.hpp"
#include "kernels_batch_hz.hpp"
#include "kernels_batch_hz_bloch.hpp"
#include "kernels_batch_hz_bloch_flux.hpp"
#include "kernels_batch_hz_lattice.hpp"
#include "kernels_batch_hz_flux.hpp"
#include "kernels_batch_lattice.hpp"
#include "kernels_batch_lossy.hpp"
#include "kernels_batch_monitor.hpp"
#include "kernels_batch_periodic.hpp"
#include "kernels_batch_pml.hpp"

struct fdtd2d_batch {
    int count = 0, rows = 0, cols = 0, dtype = FDTD2D_F32, boundary = FDTD2D_BOUNDARY_MUR5, device = 0;
    double dt = 0, dx = 0;
    long long pitch = 0;          // elements per stored row
    size_t esz = 4;               // element size
    size_t mstride = 0;           // elements per member (rows * pitch)
    size_t field_bytes = 0;       // bytes of one field of the whole batch

    void *ez[2] = {nullptr, nullptr};
    int cur = 0;                  // ez[cur] is the current Ez (the streamed path ping-pongs)
    void *hx = nullptr, *hy = nullptr;
    void *ce = nullptr, *ch = nullptr;    // coefficient arrays (nullptr with uniform materials)
    void *kmur = nullptr;                 // Mur factor per member, in T
    bool have_mat = false, uniform = true;
    double ce_u = 0, ch_u = 0;            // uniform coefficients, already rounded to T
    std::vector<double> courant;          // per member (fdtd.py:25-26)
    // fdtd2d_batch_set_eps_window: eps as the engine stores it (count x rows x cols) and mu's minimum per member,
    // kept from fdtd2d_batch_set_materials on; eps' minimum outside the last window, while that window stays
    std::vector<double> eps_host, mu_min, eps_out_min;
    int out_win[4] = {0, 0, 0, 0};
    // fdtd2d_batch_set_conductivity: ca and cb = ce / (1 + s) beside ce (nullptr = lossless), sigma as given
    void *ca = nullptr, *cb = nullptr;
    std::vector<double> sigma_host;
    double eps_u = 0, mu_u = 0;           // uniform materials as given (a conductivity materialises them)
    // fdtd2d_batch_set_dispersion: Jh, Q and cj beside the fields (nullptr = no pole), a and ck per member in T; the
    // strengths (count x rows x cols), the dampings and the resonances as given
    void *djh = nullptr, *dq = nullptr, *dcj = nullptr, *da = nullptr, *dck = nullptr;
    std::vector<double> wp2_host, disp_gamma, disp_omega0;
    // fdtd2d_batch_set_bloch_dispersion: the pole of a Bloch or lattice batch.  Everything above is set too (Jh and Q
    // hold the real parts) and these hold the imaginary parts
    bool bdisp = false;
    void *djh_im = nullptr, *dq_im = nullptr;
    // fdtd2d_batch_set_polarization: the Hz polarisation.  The Ez slot holds Hz, hx Ex, hy Ey, ezx Hzx; the batch then
    // always holds ca / cb (sigma_implicit without a conductivity), and a pole's djh, dq are Jx, Qx and these Jy, Qy
    bool hz = false;
    void *djy = nullptr, *dqy = nullptr;
    // fdtd2d_batch_set_hz_bloch: `hz` and `bloch` together; with a pole djh_im, dq_im hold the imaginary Jx, Qx and these
    // the imaginary Jy, Qy.  hz_bloch_call: an entry point of fdtd2d_batch_hz_bloch.h is using one of the Bloch phase's
    bool hz_bloch_call = false;
    void *djy_im = nullptr, *dqy_im = nullptr;
    void *dsg = nullptr;                  // device scratch of the design-loop entry points
    size_t dsg_cap = 0;
    // fdtd2d_batch_set_periodic: column C-1 is the image of column 0.  The batch then always holds Ezx and the factors
    // (all exactly 1 and pml_L = 0 without a layer) and ca / cb (sigma_implicit: made by the batch itself, all zero)
    bool periodic = false, sigma_implicit = false;
    std::vector<int> rect_host;           // the source rectangles as given (4 per member)
    // fdtd2d_batch_set_bloch: the imaginary parts of Ez, Hx, Hy, Ezx (the periodic kernels never flip `cur`, so one Ez),
    // rho = count x {c, s} in T, the source weights count x {wr[C-1], wi[C-1]}, the imaginary amplitudes of a run and
    // the imaginary parts of the monitors (allocated while the monitor is set)
    bool bloch = false;
    void *ez_im = nullptr, *hx_im = nullptr, *hy_im = nullptr, *ezx_im = nullptr, *rho = nullptr;
    std::vector<double> rho_host;         // count x {c, s} as the engine stores them
    double *bloch_w = nullptr, *amps_im = nullptr, *win_acc_im = nullptr, *probe_trace_im = nullptr;
    size_t amps_im_cap = 0;
    const double *run_amps_im = nullptr;  // device imaginary amplitudes of the run in progress (nullptr = zero)
    std::vector<int> probe_host;          // the probes' cells as the device holds them (row * C + col)
    // fdtd2d_batch_bloch_adjoint.h: count x {c, -s} beside rho, whether the last run took it (downloads rotate the image
    // by the rotation the run used), and the held copy of the imaginary part's window (win_held holds the real part's)
    void *rho_conj = nullptr;
    bool run_conj = false;
    double *win_held_im = nullptr;
    // fdtd2d_batch_set_lattice: row R-1 is the image of row 0 too.  `bloch` is set as well (the imaginary parts, the
    // weights and the monitors are the Bloch phase's, without Ezx's imaginary part), rho / rho_host hold the column
    // rotation and these the row rotation.  fdtd2d_batch_set_hz_lattice sets it beside `hz` and `bloch`: the same state
    // with Hz, Ex, Ey in the slots and the pole state of the Hz Bloch phase
    bool lattice = false;
    void *rho_r = nullptr;
    std::vector<double> rho_r_host;       // count x {c, s} as the engine stores them

    int *rect = nullptr;                  // device copy of the source rectangles (4 per member)
    bool have_src = false;                // some member has a non-empty rectangle
    double *amps = nullptr;               // device amplitudes of the current run
    size_t amps_cap = 0;

    void *ezx = nullptr;                  // PML: x-part of Ez (nullptr = no layer)
    void *pml_row = nullptr, *pml_col = nullptr;   // PML: per member 4R / 4C factors, in T
    int pml_L = 0;

    double *dft = nullptr;                // per member re[R*C], im[R*C]
    double *omega = nullptr;
    int dft_every = 0;
    long long dft_step0 = 0;

    // window DFT (fdtd2d_batch_set_dft_window): per member re[nf][W], im[nf][W], W = win_nr * win_nc
    int win_r0 = 0, win_c0 = 0, win_nr = 0, win_nc = 0, win_nf = 0, win_every = 1;
    long long win_step0 = 0;
    double *win_acc = nullptr, *win_omega = nullptr;
    double *win_ph = nullptr;             // streamed path: count x nf phasors of the step being completed
    int win_lds_opt = -1;                 // -1: accumulators in LDS when they fit, 0: never
    // probes (fdtd2d_batch_set_probes): [member][probe][probe_cap]
    int nprobe = 0;
    int *probe_cells = nullptr;           // count x nprobe, row * C + col
    double *probe_trace = nullptr;
    long long probe_cap = 0, probe_step0 = 0;
    // flux lines (fdtd2d_batch_set_flux_lines): per member Ez re[nff][cells], Ez im, Ht re, Ht im, cells = the lines'
    // counts together; flux_line holds {orientation, index, first, count} per line
    int flux_nl = 0, flux_nff = 0, flux_every = 1, flux_cells = 0;
    int flux_line[4 * FDTD2D_BATCH_MAX_FLUX_LINES] = {};
    long long flux_step0 = 0;
    double *flux_acc = nullptr, *flux_omega = nullptr;
    double *flux_ph = nullptr;            // streamed path: count x nff phasors of the step being completed
    int flux_lds_opt = -1;                // -1: sums in LDS when they fit, 0: never
    // fdtd2d_batch_set_bloch_flux_lines: the lines above on a Bloch batch.  flux_acc holds the sums of the real part and
    // flux_acc_im, of the same layout, those of the imaginary part
    bool bflux = false;
    double *flux_acc_im = nullptr;
    // fdtd2d_batch_set_hz_flux_lines: the lines above on a batch in the Hz polarisation.  flux_acc holds the sums of Hz
    // where the Ez lines hold those of Ez, and those of the tangential E where they hold those of the tangential H
    bool hzflux = false;
    // fdtd2d_batch_set_hz_bloch_flux_lines: the lines above on an Hz Bloch batch.  flux_acc holds the sums of Hz and of the
    // tangential E of the real part of the fields and flux_acc_im, of the same layout, those of the imaginary part
    bool hzbflux = false;
    // line sources on the flux lines (fdtd2d_batch_flux_adjoint.h): count x flux_cells x fsrc_nchan weights each
    // (nullptr: no such part); fsrc_nchan = 0 without them
    int fsrc_nchan = 0;
    double *fsrc_we = nullptr, *fsrc_wh = nullptr;
    // on Bloch lines (fdtd2d_batch_bloch_flux_adjoint.h) fsrc_we, fsrc_wh are the real parts and these the imaginary ones
    double *fsrc_we_im = nullptr, *fsrc_wh_im = nullptr;
    int *fsrc_geom = nullptr;             // the lines as batch_fluxsrc_gather reads them (BatchFluxSrc::geom)
    double *win_held = nullptr;           // fdtd2d_batch_hold_dft_window: a copy of win_acc
    double *win_held_disp = nullptr;      // fdtd2d_batch_hold_dispersive_window: a copy of win_acc while a pole is set
    // point sources (fdtd2d_batch_set_point_sources), every table in the resident owners' order
    int npts = 0, pts_nchan = 0;
    int npts_user = 0;                    // npts without the image entries of a periodic batch
    int *pts_cells = nullptr, *pts_own = nullptr;   // count x npts: row * C + col; owner thread * 16 + slot
    double *pts_w = nullptr;              // count x nchan x npts
    double *pts_tab = nullptr;            // streamed path: count x npts sums of a step
    double *chan = nullptr;               // device channels of the current run
    size_t chan_cap = 0;

    long long step = 0, launches = 0;
    int resident_opt = -1;                // -1: by the capacity rule, 0: never
    int steps_per_launch = 0;             // resident path: 0 = the whole run in one launch

    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
};

// the body of fdtd2d_batch_set_point_sources, shared with fdtd2d_batch_set_bloch_point_sources
static int batch_set_points(fdtd2d_batch *b, int ncell, const int *cells, int nchan, const double *weights);

namespace {

thread_local std::string g_batch_create_error = "";

int bfail(fdtd2d_batch *b, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (b) b->err = buf;
    else g_batch_create_error = buf;
    return code;
}

#define BCHK(b, expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return bfail((b), -(1000 + (int)e_), "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

int use_device(fdtd2d_batch *b)
{
    hipError_t e = hipSetDevice(b->device);
    if (e != hipSuccess)
        return bfail(b, FDTD2D_E_NODEVICE, "hipSetDevice(%d): %s", b->device, hipGetErrorString(e));
    return 0;
}

// dt/(x*dx) in T, as main.py:27,70,74 evaluate it for arrays of type T (same rounding as k_coef)
template <class T> double coef_of(double x, double dt, double dx)
{
    const T xt = (T)x, dtt = (T)dt, dxt = (T)dx;
    volatile T prod = xt * dxt;
    volatile T q = dtt / prod;
    return (double)q;
}

// (c*dt - dx)/(c*dt + dx), c = 1/sqrt(mu00*eps00), every operation in T (main.py:30-31)
template <class T> double mur_of(double eps00, double mu00, double dt, double dx)
{
    const T e = (T)eps00, m = (T)mu00, dtt = (T)dt, dxt = (T)dx;
    volatile T prod = m * e;
    volatile T s = std::sqrt((T)prod);
    volatile T c = (T)1 / s;
    volatile T cdt = c * dtt;
    volatile T num = cdt - dxt, den = cdt + dxt;
    volatile T k = num / den;
    return (double)k;
}

double courant_of(double eps_min, double mu_min, double dt, double dx)
{
    const double c = 1 / std::sqrt(eps_min * mu_min);
    return (c * dt) / dx;
}

double get_elem(const void *p, int dt, size_t i)
{
    return dt == FDTD2D_F64 ? ((const double *)p)[i] : (double)((const float *)p)[i];
}

// a host value as the engine's type T stores it (NumPy astype: round to nearest)
double as_engine(const fdtd2d_batch *b, double x) { return b->dtype == FDTD2D_F32 ? (double)(float)x : x; }

// Host arrays (count x nrows x ncols of host_dtype) <-> the padded device layout of one field.
// The element type changes on the host, one rounding per element like a NumPy astype.
int copy_in(fdtd2d_batch *b, void *dev, const void *host, int host_dtype, int nrows, int ncols)
{
    std::vector<unsigned char> stage(b->field_bytes, 0);
    for (int m = 0; m < b->count; ++m)
        for (int i = 0; i < nrows; ++i) {
            const size_t src = ((size_t)m * nrows + i) * ncols, dst = (size_t)m * b->mstride + (size_t)i * b->pitch;
            if (b->dtype == FDTD2D_F32) {
                float *d = (float *)stage.data() + dst;
                for (int j = 0; j < ncols; ++j) d[j] = (float)get_elem(host, host_dtype, src + j);
            } else {
                double *d = (double *)stage.data() + dst;
                for (int j = 0; j < ncols; ++j) d[j] = get_elem(host, host_dtype, src + j);
            }
        }
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(dev, stage.data(), b->field_bytes, hipMemcpyHostToDevice));
    return 0;
}

int copy_out(fdtd2d_batch *b, const void *dev, void *host, int host_dtype, int nrows, int ncols)
{
    std::vector<unsigned char> stage(b->field_bytes);
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(stage.data(), dev, b->field_bytes, hipMemcpyDeviceToHost));
    for (int m = 0; m < b->count; ++m)
        for (int i = 0; i < nrows; ++i) {
            const size_t dst = ((size_t)m * nrows + i) * ncols, src = (size_t)m * b->mstride + (size_t)i * b->pitch;
            for (int j = 0; j < ncols; ++j) {
                const double v = b->dtype == FDTD2D_F32 ? (double)((const float *)stage.data())[src + j]
                                                        : ((const double *)stage.data())[src + j];
                if (host_dtype == FDTD2D_F32) ((float *)host)[dst + j] = (float)v;
                else ((double *)host)[dst + j] = v;
            }
        }
    return 0;
}

int zero_fields(fdtd2d_batch *b)
{
    for (void *p : {b->ez[0], b->ez[1], b->hx, b->hy}) BCHK(b, hipMemsetAsync(p, 0, b->field_bytes, b->stream));
    if (b->ezx) BCHK(b, hipMemsetAsync(b->ezx, 0, b->field_bytes, b->stream));
    if (b->dcj)
        for (void *p : {b->djh, b->dq, b->djh_im, b->dq_im, b->djy, b->dqy, b->djy_im, b->dqy_im})
            if (p) BCHK(b, hipMemsetAsync(p, 0, b->field_bytes, b->stream));     // the imaginary parts: a complex pole's
    if (b->bloch)
        for (void *p : {b->ez_im, b->hx_im, b->hy_im, b->ezx_im})
            if (p) BCHK(b, hipMemsetAsync(p, 0, b->field_bytes, b->stream));     // a lattice batch has no Ezx
    b->cur = 0;
    b->step = 0;
    b->run_conj = false;
    return 0;
}

// ---- the capacity rule of the resident path ------------------------------------------------------------
// Mur / none: Ez, Hx, Hy (+ ce, ch); PML: Ez, Hx, Hy, Ezx (+ ce, ch) and the 4R + 4C factors; with a conductivity
// cb stands in ce's place and ca is one more array; a Bloch phase: the four fields twice and cb, ch, ca, the row
// factors alone, the source weights with the tables and the accumulators twice; a pole: the lossy PML arrays and Jh,
// Q, cj; the lattice mode: Ez, Hx, Hy twice and cb, ch, ca, no factors; a Bloch or lattice batch with a pole: Jh and Q
// twice and cj more
int lds_arrays(const fdtd2d_batch *b)
{
    if (b->hz && b->lattice) return b->dcj ? 18 : 9;  // Hz, Ex, Ey twice, ch, cb, ca and cj, Jx, Qx, Jy, Qy twice
    if (b->hz && b->bloch) return b->dcj ? 20 : 11;   // Hz, Ex, Ey, Hzx twice, ch, cb, ca and cj, Jx, Qx, Jy, Qy twice
    if (b->hz) return b->dcj ? 12 : 7;       // Hz, Ex, Ey, Hzx, ch, cb, ca and cj, Jx, Qx, Jy, Qy
    if (b->lattice) return b->bdisp ? 14 : 9;
    if (b->bloch) return b->bdisp ? 16 : 11;
    if (b->dcj) return 10;
    if (b->periodic) return 7;
    if (b->ca) return b->ezx ? 7 : 6;
    return (b->have_mat && b->uniform) ? (b->ezx ? 4 : 3) : (b->ezx ? 6 : 5);
}

// bytes of the PML factors in LDS (0 without a layer)
size_t lds_factor_bytes(const fdtd2d_batch *b)
{
    if ((!b->ezx && !b->periodic) || b->lattice) return 0;
    if (b->bloch)                           // the row factors alone
        return b->dtype == FDTD2D_F32 ? fdtd::batch_lds_seg<float>(4 * b->rows) * 4
                                      : fdtd::batch_lds_seg<double>(4 * b->rows) * 8;
    return b->dtype == FDTD2D_F32 ? fdtd::batch_pml_lds_elems<float>(0, b->rows, b->cols) * 4
                                  : fdtd::batch_pml_lds_elems<double>(0, b->rows, b->cols) * 8;
}

// the member's arrays (and PML factors): the offset of the monitors' LDS in the resident kernels
size_t lds_field_bytes(const fdtd2d_batch *b)
{
    const int cells = b->rows * b->cols;
    return (size_t)lds_arrays(b) * (b->dtype == FDTD2D_F32 ? fdtd::batch_lds_seg<float>(cells) * 4
                                                           : fdtd::batch_lds_seg<double>(cells) * 8) +
           lds_factor_bytes(b);
}

// window DFT: the phasor table (part of the capacity rule) and the accumulators (in LDS only when they fit too);
// flux lines: their phasor table behind the window's; point sources: the sums of a step, behind the phasor tables
size_t lds_table_bytes(const fdtd2d_batch *b)
{
    return 16 * (size_t)b->win_nf + 16 * (size_t)(b->flux_nl ? b->flux_nff : 0) + 8 * (size_t)b->npts +
           (b->bloch ? 16 * (size_t)(b->cols - 1) : 0);
}
size_t win_acc_bytes(const fdtd2d_batch *b) { return 16 * (size_t)b->win_nf * b->win_nr * b->win_nc; }
size_t lds_acc_bytes(const fdtd2d_batch *b) { return (b->bloch ? 2 : 1) * win_acc_bytes(b); }   // both parts
bool win_acc_in_lds(const fdtd2d_batch *b)
{
    return b->win_nf && b->win_lds_opt != 0 &&
           lds_field_bytes(b) + lds_table_bytes(b) + lds_acc_bytes(b) <= fdtd::BATCH_LDS_LIMIT;
}

// flux lines: the sums of one member (of both parts on a Bloch batch); in LDS behind the window's accumulators (wherever
// those live) when they fit too
size_t flux_part_bytes(const fdtd2d_batch *b) { return b->flux_nl ? 32 * (size_t)b->flux_nff * b->flux_cells : 0; }
size_t flux_acc_bytes(const fdtd2d_batch *b) { return (b->bflux || b->hzbflux ? 2 : 1) * flux_part_bytes(b); }
bool flux_acc_in_lds(const fdtd2d_batch *b)
{
    return b->flux_nl && b->flux_lds_opt != 0 &&
           lds_field_bytes(b) + lds_table_bytes(b) + (win_acc_in_lds(b) ? lds_acc_bytes(b) : 0) + flux_acc_bytes(b) <=
               fdtd::BATCH_LDS_LIMIT;
}

size_t lds_bytes(const fdtd2d_batch *b)
{
    return lds_field_bytes(b) + lds_table_bytes(b) + (win_acc_in_lds(b) ? lds_acc_bytes(b) : 0) +
           (flux_acc_in_lds(b) ? flux_acc_bytes(b) : 0);
}

// largest R*C whose arrays fit in one workgroup's LDS (materials as currently set; arrays before any call;
// with a layer, beside this batch's own 4R + 4C factors; with a window, beside its phasor table; with point sources,
// beside their sums):
// R*C <= this  <=>  lds_field_bytes + lds_table_bytes <= BATCH_LDS_LIMIT
long long resident_max_cells(const fdtd2d_batch *b)
{
    const size_t fac = lds_factor_bytes(b) + lds_table_bytes(b);
    if (fac >= fdtd::BATCH_LDS_LIMIT) return 0;
    const size_t per_array = (fdtd::BATCH_LDS_LIMIT - fac) / (size_t)lds_arrays(b) / 16 * 16;
    return (long long)(per_array / b->esz);
}

bool use_resident(const fdtd2d_batch *b)
{
    return b->resident_opt != 0 && (long long)b->rows * b->cols <= resident_max_cells(b);
}

// threads of a resident workgroup: a wave multiple, at least a quarter of the cells, at most 1024
int resident_threads(int cells)
{
    const int want = ((cells + 3) / 4 + 63) / 64 * 64;
    return want < fdtd::BATCH_RES_THREADS ? want : fdtd::BATCH_RES_THREADS;
}

template <class T> fdtd::BatchView<T> view(fdtd2d_batch *b, const double *amps, long long amp_stride)
{
    fdtd::BatchView<T> v;
    v.ez = (T *)b->ez[b->cur];
    v.hx = (T *)b->hx;
    v.hy = (T *)b->hy;
    v.ce = (const T *)b->ce;
    v.ch = (const T *)b->ch;
    v.ce_u = (T)b->ce_u;
    v.ch_u = (T)b->ch_u;
    v.kmur = (const T *)b->kmur;
    v.B = b->count;
    v.R = b->rows;
    v.C = b->cols;
    v.mur = b->boundary == FDTD2D_BOUNDARY_MUR5;
    v.pitch = b->pitch;
    v.mstride = b->mstride;
    v.rect = b->rect;
    v.amps = (b->have_src && amps) ? amps : nullptr;
    v.amp_stride = amp_stride;
    v.dft = b->dft;
    v.omega = b->omega;
    v.every = b->dft_every > 0 ? b->dft_every : 1;
    v.dft_step0 = b->dft_step0;
    v.dt = b->dt;
    return v;
}

template <class T, bool ARR, int MAXC>
int launch_resident(fdtd2d_batch *b, const fdtd::BatchView<T> &v, int n0, int nt, int threads)
{
    auto kern = &fdtd::k_batch_resident<T, ARR, MAXC>;
    const size_t lds = lds_bytes(b);
    BCHK(b, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    int per_cu = 0, cus = 0;
    BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
    BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
    if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "resident kernel does not fit a CU (%zu B of LDS)", lds);
    const long long round = (long long)per_cu * cus;
    const int blocks = (int)(b->count < round ? b->count : round);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, b->stream, v, n0, nt, b->step);
    BCHK(b, hipGetLastError());
    b->launches++;
    return 0;
}

template <class T, bool ARR> int run_resident(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    const int cells = b->rows * b->cols, threads = resident_threads(cells);
    const int per_thread = (cells + threads - 1) / threads;
    const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
    for (int n = 0; n < nsteps; n += chunk) {
        const int nt = nsteps - n < chunk ? nsteps - n : chunk;
        const fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        int rc;
        if (per_thread <= 4) rc = launch_resident<T, ARR, 4>(b, v, n, nt, threads);
        else if (per_thread <= 8) rc = launch_resident<T, ARR, 8>(b, v, n, nt, threads);
        else if (per_thread <= 16) rc = launch_resident<T, ARR, 16>(b, v, n, nt, threads);
        else rc = bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the resident kernel's 16", per_thread);
        if (rc) return rc;
        b->step += nt;
    }
    return 0;
}

template <class T, bool ARR> int run_streamed(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        const fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        hipLaunchKernelGGL((fdtd::k_batch_h<T, ARR>), grid, dim3(256), 0, b->stream, v);
        BCHK(b, hipGetLastError());
        hipLaunchKernelGGL((fdtd::k_batch_e<T, ARR>), grid, dim3(256), 0, b->stream, v, (T *)b->ez[b->cur ^ 1], n,
                           b->step + 1);
        BCHK(b, hipGetLastError());
        b->launches += 2;
        b->cur ^= 1;
        b->step++;
    }
    return 0;
}

// ---- the PML mode (kernels_batch_pml.hpp) ---------------------------------------------------------------
template <class T> fdtd::BatchPml<T> pml_view(const fdtd2d_batch *b)
{
    return fdtd::BatchPml<T>{(T *)b->ezx, (const T *)b->pml_row, (const T *)b->pml_col, b->pml_L};
}

template <class T, bool ARR, int MAXC>
int launch_resident_pml(fdtd2d_batch *b, const fdtd::BatchView<T> &v, int n0, int nt, int threads)
{
    auto kern = &fdtd::k_batch_resident_pml<T, ARR, MAXC>;
    const size_t lds = lds_bytes(b);
    BCHK(b, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    int per_cu = 0, cus = 0;
    BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
    BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
    if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "resident PML kernel does not fit a CU (%zu B of LDS)", lds);
    const long long round = (long long)per_cu * cus;
    const int blocks = (int)(b->count < round ? b->count : round);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, b->stream, v, pml_view<T>(b), n0, nt, b->step);
    BCHK(b, hipGetLastError());
    b->launches++;
    return 0;
}

template <class T, bool ARR>
int run_resident_pml(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    const int cells = b->rows * b->cols, threads = resident_threads(cells);
    const int per_thread = (cells + threads - 1) / threads;
    const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
    for (int n = 0; n < nsteps; n += chunk) {
        const int nt = nsteps - n < chunk ? nsteps - n : chunk;
        const fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        int rc;
        if (per_thread <= 4) rc = launch_resident_pml<T, ARR, 4>(b, v, n, nt, threads);
        else if (per_thread <= 8) rc = launch_resident_pml<T, ARR, 8>(b, v, n, nt, threads);
        else if (per_thread <= 16) rc = launch_resident_pml<T, ARR, 16>(b, v, n, nt, threads);
        else rc = bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the resident kernel's 16", per_thread);
        if (rc) return rc;
        b->step += nt;
    }
    return 0;
}

// Ez and Ezx are updated in place (a new Ez reads no neighbour's Ez), so there is no ping-pong
template <class T, bool ARR>
int run_streamed_pml(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    const fdtd::BatchPml<T> p = pml_view<T>(b);
    for (int n = 0; n < nsteps; ++n) {
        const fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        hipLaunchKernelGGL((fdtd::k_batch_h_pml<T, ARR>), grid, dim3(256), 0, b->stream, v, p);
        BCHK(b, hipGetLastError());
        hipLaunchKernelGGL((fdtd::k_batch_e_pml<T, ARR>), grid, dim3(256), 0, b->stream, v, p, n, b->step + 1);
        BCHK(b, hipGetLastError());
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- monitored runs (fdtd2d_batch_monitor.h): the same paths with the kernels of batch_monitor.hip ----------------
fdtd::BatchMon mon_view(const fdtd2d_batch *b)
{
    fdtd::BatchMon m;
    m.acc = b->win_acc;
    m.omega = b->win_omega;
    m.ph = b->win_ph;
    m.r0 = b->win_r0; m.c0 = b->win_c0; m.nr = b->win_nr; m.nc = b->win_nc;
    m.nf = b->win_nf;
    m.every = b->win_every;
    m.step0 = b->win_step0;
    m.lds_acc = win_acc_in_lds(b) ? 1 : 0;
    m.cells = b->probe_cells;
    m.trace = b->probe_trace;
    m.np = b->nprobe;
    m.cap = b->probe_cap;
    m.pstep0 = b->probe_step0;
    return m;
}

int launch_ptr(fdtd2d_batch *b, const void *kern, dim3 grid, dim3 block, void **args, size_t lds)
{
    BCHK(b, hipLaunchKernel(kern, grid, block, args, lds, b->stream));
    BCHK(b, hipGetLastError());
    return 0;
}

// pts: the point sources of fdtd2d_batch_run_channels (nullptr: none); the *_pts kernels take them behind the monitors
template <class T>
int run_monitored(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts)
{
    const fdtd::BatchMonKernels &K = pts ? fdtd::batch_pts_kernels<T>() : fdtd::batch_mon_kernels<T>();
    const int arr = b->uniform ? 0 : 1;
    const bool pml = b->ezx != nullptr;
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        const int mi = per_thread <= 4 ? 0 : per_thread <= 8 ? 1 : per_thread <= 16 ? 2 : -1;
        if (mi < 0) return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the resident kernel's 16", per_thread);
        const void *kern = pml ? K.resident_pml[arr][mi] : K.resident[arr][mi];
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "monitored resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            void *mur_args[] = {&v, &m, &n0, &nt, &step_base};
            void *pml_args[] = {&v, &p, &m, &n0, &nt, &step_base};
            void *mur_pts[] = {&v, &m, pts, &n0, &nt, &step_base};
            void *pml_pts[] = {&v, &p, &m, pts, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads),
                                pts ? (pml ? pml_pts : mur_pts) : (pml ? pml_args : mur_args), lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        long long step = b->step + 1;
        T *ez_new = (T *)b->ez[b->cur ^ 1];
        int rc;
        if (pml) {
            void *h_args[] = {&v, &p, &m, &step};
            void *e_args[] = {&v, &p, &m, &n, &step};
            void *h_pts[] = {&v, &p, &m, pts, &n, &step};
            void *e_pts[] = {&v, &p, &m, pts, &n, &step};
            if ((rc = launch_ptr(b, K.h_pml[arr], grid, dim3(256), pts ? h_pts : h_args, 0))) return rc;
            if ((rc = launch_ptr(b, K.e_pml[arr], grid, dim3(256), pts ? e_pts : e_args, 0))) return rc;
        } else {
            void *h_args[] = {&v, &m, &step};
            void *e_args[] = {&v, &m, &ez_new, &n, &step};
            void *h_pts[] = {&v, &m, pts, &n, &step};
            void *e_pts[] = {&v, &m, pts, &ez_new, &n, &step};
            if ((rc = launch_ptr(b, K.h[arr], grid, dim3(256), pts ? h_pts : h_args, 0))) return rc;
            if ((rc = launch_ptr(b, K.e[arr], grid, dim3(256), pts ? e_pts : e_args, 0))) return rc;
            b->cur ^= 1;
        }
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- lossy runs (fdtd2d_batch_lossy.h): the point-source paths with the kernels of batch_lossy.hip -----------------
// v.ce carries cb; without point sources the table is empty and the kernels' point-source code stays silent
template <class T>
int run_lossy(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts)
{
    const fdtd::BatchLossyKernels &K = fdtd::batch_lossy_kernels<T>();
    const fdtd::BatchMonKernels &H = fdtd::batch_pts_kernels<T>();   // the streamed H launches: H sees no conductivity
    const bool pml = b->ezx != nullptr;
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchPts silent{};
    if (!pts) pts = &silent;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        const int mi = per_thread <= 4 ? 0 : per_thread <= 8 ? 1 : per_thread <= 16 ? 2 : -1;
        if (mi < 0) return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the resident kernel's 16", per_thread);
        const void *kern = pml ? K.resident_pml[mi] : K.resident[mi];
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "lossy resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *mur_args[] = {&v, &m, pts, &ca, &n0, &nt, &step_base};
            void *pml_args[] = {&v, &p, &m, pts, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), pml ? pml_args : mur_args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        T *ez_new = (T *)b->ez[b->cur ^ 1];
        int rc;
        if (pml) {
            void *h_args[] = {&v, &p, &m, pts, &n, &step};
            void *e_args[] = {&v, &p, &m, pts, &ca, &n, &step};
            if ((rc = launch_ptr(b, H.h_pml[1], grid, dim3(256), h_args, 0))) return rc;
            if ((rc = launch_ptr(b, K.e_pml, grid, dim3(256), e_args, 0))) return rc;
        } else {
            void *h_args[] = {&v, &m, pts, &n, &step};
            void *e_args[] = {&v, &m, pts, &ca, &ez_new, &n, &step};
            if ((rc = launch_ptr(b, H.h[1], grid, dim3(256), h_args, 0))) return rc;
            if ((rc = launch_ptr(b, K.e, grid, dim3(256), e_args, 0))) return rc;
            b->cur ^= 1;
        }
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- periodic runs (fdtd2d_batch_periodic.h): the lossy PML paths with the kernels of batch_periodic.hip ---------------
// H needs no wrap of its own: Hy[i, C-2] reads the image column.
template <class T>
int run_periodic(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts)
{
    if (!b->ca || !b->ezx) return bfail(b, FDTD2D_E_STATE, "periodic batch without its coefficient arrays");
    const fdtd::BatchPeriodicKernels &K = fdtd::batch_periodic_kernels<T>();
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchPts silent{};
    if (!pts) pts = &silent;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        const int mi = per_thread <= 4 ? 0 : per_thread <= 8 ? 1 : per_thread <= 16 ? 2 : -1;
        if (mi < 0) return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the resident kernel's 16", per_thread);
        const void *kern = K.resident[mi];
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "periodic resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, pts, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *h_args[] = {&v, &p, &m, pts, &n, &step};
        void *e_args[] = {&v, &p, &m, pts, &ca, &n, &step};
        if ((rc = launch_ptr(b, K.h, grid, dim3(256), h_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.e, grid, dim3(256), e_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- dispersive runs (fdtd2d_batch_dispersive.h): the lossy PML or the periodic paths with the kernels of
// batch_dispersive.hip.  The streamed H launches are those paths' own: H does not see the pole.
template <class T>
int run_dispersive(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts)
{
    if (!b->ca || !b->ezx || !b->djh || !b->dq || !b->da || !b->dck)
        return bfail(b, FDTD2D_E_STATE, "dispersive batch without its arrays");
    const fdtd::BatchDispersiveKernels &K = fdtd::batch_dispersive_kernels<T>();
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchPts silent{};
    if (!pts) pts = &silent;
    fdtd::BatchDisp<T> d{(T *)b->djh, (T *)b->dq, (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        if (per_thread > 4)
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the dispersive resident kernel's 4", per_thread);
        const void *kern = b->periodic ? K.resident_periodic : K.resident_pml;
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "dispersive resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, pts, &d, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const void *kh = b->periodic ? fdtd::batch_periodic_kernels<T>().h : fdtd::batch_pts_kernels<T>().h_pml[1];
    const void *ke = b->periodic ? K.e_periodic : K.e_pml;
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *h_args[] = {&v, &p, &m, pts, &n, &step};
        void *e_args[] = {&v, &p, &m, pts, &d, &ca, &n, &step};
        if ((rc = launch_ptr(b, kh, grid, dim3(256), h_args, 0))) return rc;
        if ((rc = launch_ptr(b, ke, grid, dim3(256), e_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- runs in the Hz polarisation (fdtd2d_batch_hz.h): the paths of run_dispersive with the kernels of batch_hz.hip.
// v.ce carries cb; the first streamed launch of a step is the E half-step, the second the H half-step with the sources
// and the monitors.
fdtd::BatchFlux flux_view(const fdtd2d_batch *b);

template <class T>
int run_hz(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts)
{
    if (!b->ezx)
        return bfail(b, FDTD2D_E_STATE, "the Hz polarisation needs a PML layer (fdtd2d_batch_set_pml) or periodic columns: "
                     "a plain box has no Hz kernels");
    const int disp = b->dcj ? 1 : 0, per = b->periodic ? 1 : 0;
    if (!b->ca || !b->cb || !b->ch || (disp && (!b->djh || !b->dq || !b->djy || !b->dqy || !b->da || !b->dck)))
        return bfail(b, FDTD2D_E_STATE, "Hz batch without its arrays");
    // with the lines of fdtd2d_batch_hz_flux.h: the kernels of batch_hz_flux.hip, which take the lines behind the pole
    const bool lines = b->hzflux;
    if (lines && !b->flux_acc) return bfail(b, FDTD2D_E_STATE, "Hz batch with flux lines without its arrays");
    const fdtd::BatchHzKernels &K = fdtd::batch_hz_kernels<T>();
    const fdtd::BatchHzFluxKernels &KF = fdtd::batch_hz_flux_kernels<T>();
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchFlux f = flux_view(b);
    fdtd::BatchPts silent{};
    if (!pts) pts = &silent;
    fdtd::BatchHzDisp<T> d{(T *)b->djh, (T *)b->dq, (T *)b->djy, (T *)b->dqy,
                           (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        const int mi = per_thread <= 4 ? 0 : per_thread <= 8 ? 1 : -1;
        const void *kern = mi < 0 ? nullptr : lines ? KF.resident[per][disp][mi] : K.resident[per][disp][mi];
        if (!kern)
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the Hz resident kernel's %d", per_thread,
                         disp ? 4 : 8);
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "Hz resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, pts, &d, &ca, &n0, &nt, &step_base};
            void *line_args[] = {&v, &p, &m, pts, &d, &f, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), lines ? line_args : args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *e_args[] = {&v, &p, &m, pts, &d, &ca, &n, &step};
        void *h_args[] = {&v, &p, &m, pts, &n, &step};
        void *e_line_args[] = {&v, &p, &m, pts, &d, &f, &ca, &n, &step};
        void *h_line_args[] = {&v, &p, &m, pts, &f, &n, &step};
        if ((rc = launch_ptr(b, lines ? KF.e[per][disp] : K.e[per][disp], grid, dim3(256), lines ? e_line_args : e_args, 0)))
            return rc;
        if ((rc = launch_ptr(b, lines ? KF.h[per] : K.h[per], grid, dim3(256), lines ? h_line_args : h_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- runs with flux lines (fdtd2d_batch_flux.h): the lossy PML, the periodic or the dispersive paths with the kernels
// of batch_flux.hip, whose streamed H launches also write the lines' phasors
fdtd::BatchFlux flux_view(const fdtd2d_batch *b)
{
    fdtd::BatchFlux f{};
    f.acc = b->flux_acc;
    f.omega = b->flux_omega;
    f.ph = b->flux_ph;
    f.step0 = b->flux_step0;
    f.nl = b->flux_nl;
    f.nff = b->flux_nff;
    f.every = b->flux_every;
    f.cells = b->flux_cells;
    f.lds_acc = flux_acc_in_lds(b) ? 1 : 0;
    int off = 0;
    for (int k = 0; k < b->flux_nl; ++k) {
        f.orient[k] = b->flux_line[4 * k];
        f.index[k] = b->flux_line[4 * k + 1];
        f.first[k] = b->flux_line[4 * k + 2];
        f.count[k] = b->flux_line[4 * k + 3];
        f.offset[k] = off;
        off += f.count[k];
    }
    return f;
}

// fs: the line sources of a run with channels (nullptr: none, the kernels of batch_flux.hip; otherwise those of
// batch_flux_adjoint.hip, which take fs behind the lines)
template <class T>
int run_flux(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts,
             fdtd::BatchFluxSrc *fs = nullptr)
{
    if (!b->ca || !b->ezx || !b->flux_acc || (b->dcj && (!b->djh || !b->dq || !b->da || !b->dck)))
        return bfail(b, FDTD2D_E_STATE, "batch with flux lines without its arrays");
    const fdtd::BatchFluxKernels &K = fs ? fdtd::batch_flux_src_kernels<T>() : fdtd::batch_flux_kernels<T>();
    const int per = b->periodic ? 1 : 0, disp = b->dcj ? 1 : 0;
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchFlux f = flux_view(b);
    fdtd::BatchPts silent{};
    if (!pts) pts = &silent;
    fdtd::BatchDisp<T> d{(T *)b->djh, (T *)b->dq, (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        const int mi = per_thread <= 4 ? 0 : per_thread <= 8 ? 1 : per_thread <= 16 ? 2 : -1;
        if (mi < 0 || (disp && mi > 0))
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the resident kernel's %d", per_thread, disp ? 4 : 16);
        const void *kern = disp ? K.resident_disp[per] : K.resident[per][mi];
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "flux resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, pts, &d, &f, &ca, &n0, &nt, &step_base};
            void *src_args[] = {&v, &p, &m, pts, &d, &f, fs, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), fs ? src_args : args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *h_args[] = {&v, &p, &m, pts, &f, &n, &step};
        void *e_args[] = {&v, &p, &m, pts, &d, &f, &ca, &n, &step};
        void *h_src_args[] = {&v, &p, &m, pts, &f, fs, &n, &step};
        void *e_src_args[] = {&v, &p, &m, pts, &d, &f, fs, &ca, &n, &step};
        if ((rc = launch_ptr(b, K.h[per], grid, dim3(256), fs ? h_src_args : h_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.e[per][disp], grid, dim3(256), fs ? e_src_args : e_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- Bloch runs (fdtd2d_batch_bloch.h): the periodic paths with the complex-field kernels of batch_bloch.hip ----------
template <class T> fdtd::BatchBloch<T> bloch_view(const fdtd2d_batch *b, bool conj)
{
    return fdtd::BatchBloch<T>{(T *)b->ez_im, (T *)b->hx_im, (T *)b->hy_im, (T *)b->ezx_im,
                               (const T *)(conj ? b->rho_conj : b->rho),
                               b->bloch_w, b->have_src ? b->run_amps_im : nullptr, b->win_acc_im, b->probe_trace_im};
}

// pts: the point sources of fdtd2d_batch_run_bloch_channels (nullptr: none, the kernels of batch_bloch.hip); conj: step
// with (c, -s)
template <class T>
int run_bloch(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts = nullptr,
              bool conj = false)
{
    if (!b->ca || !b->ezx || !b->ez_im || !b->rho_conj) return bfail(b, FDTD2D_E_STATE, "Bloch batch without its arrays");
    const fdtd::BatchBlochKernels &K = pts ? fdtd::batch_bloch_pts_kernels<T>() : fdtd::batch_bloch_kernels<T>();
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchBloch<T> bl = bloch_view<T>(b, conj);
    b->run_conj = conj;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        if (per_thread > 4) return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the Bloch resident kernel's 4", per_thread);
        const void *kern = K.resident;
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "Bloch resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, &bl, &ca, &n0, &nt, &step_base};
            void *args_pts[] = {&v, &p, &m, &bl, pts, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), pts ? args_pts : args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *h_args[] = {&v, &p, &m, &bl, &step};
        void *e_args[] = {&v, &p, &m, &bl, &ca, &n, &step};
        void *h_pts[] = {&v, &p, &m, &bl, pts, &n, &step};
        void *e_pts[] = {&v, &p, &m, &bl, pts, &ca, &n, &step};
        if ((rc = launch_ptr(b, K.h, grid, dim3(256), pts ? h_pts : h_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.e, grid, dim3(256), pts ? e_pts : e_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- lattice runs (fdtd2d_batch_lattice.h): the Bloch paths with the kernels of batch_lattice.hip --------------------
template <class T> int run_lattice(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    if (!b->ca || !b->ez_im || !b->rho || !b->rho_r) return bfail(b, FDTD2D_E_STATE, "lattice batch without its arrays");
    const fdtd::BatchLatticeKernels &K = fdtd::batch_lattice_kernels<T>();
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchLattice<T> la{(T *)b->ez_im, (T *)b->hx_im, (T *)b->hy_im, (const T *)b->rho_r, (const T *)b->rho,
                             b->bloch_w, b->have_src ? b->run_amps_im : nullptr, b->win_acc_im, b->probe_trace_im};
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        const void *kern = per_thread <= 4 ? K.resident[0] : per_thread <= 5 ? K.resident[1] : nullptr;
        if (!kern) return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the lattice resident kernels", per_thread);
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "lattice resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &m, &la, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *h_args[] = {&v, &m, &la, &step};
        void *e_args[] = {&v, &m, &la, &ca, &n, &step};
        if ((rc = launch_ptr(b, K.h, grid, dim3(256), h_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.e, grid, dim3(256), e_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- Bloch and lattice runs with a pole (fdtd2d_batch_bloch_dispersive.h): the paths of run_bloch and run_lattice with
// the kernels of batch_bloch_dispersive.hip.  The streamed H launches are those families' own: H does not see the pole.
template <class T> int run_bloch_dispersive(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    if (!b->ca || !b->ez_im || !b->rho || (b->lattice ? !b->rho_r : !b->ezx) || !b->djh || !b->dq || !b->djh_im ||
        !b->dq_im || !b->dcj || !b->da || !b->dck)
        return bfail(b, FDTD2D_E_STATE, "dispersive Bloch batch without its arrays");
    const fdtd::BatchBlochDispersiveKernels &K = fdtd::batch_bloch_dispersive_kernels<T>();
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchBloch<T> bl = bloch_view<T>(b, false);
    fdtd::BatchLattice<T> la{(T *)b->ez_im, (T *)b->hx_im, (T *)b->hy_im, (const T *)b->rho_r, (const T *)b->rho,
                             b->bloch_w, b->have_src ? b->run_amps_im : nullptr, b->win_acc_im, b->probe_trace_im};
    fdtd::BatchBlochDisp<T> d{(T *)b->djh, (T *)b->dq, (T *)b->djh_im, (T *)b->dq_im,
                              (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    b->run_conj = false;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        if (per_thread > 4)
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the dispersive Bloch resident kernels' 4", per_thread);
        const void *kern = b->lattice ? K.resident_lattice : K.resident_bloch;
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1)
            return bfail(b, FDTD2D_E_STATE, "dispersive Bloch resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args_bloch[] = {&v, &p, &m, &bl, &d, &ca, &n0, &nt, &step_base};
            void *args_lattice[] = {&v, &m, &la, &d, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), b->lattice ? args_lattice : args_bloch, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const void *kh = b->lattice ? fdtd::batch_lattice_kernels<T>().h : fdtd::batch_bloch_kernels<T>().h;
    const void *ke = b->lattice ? K.e_lattice : K.e_bloch;
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *h_bloch[] = {&v, &p, &m, &bl, &step};
        void *e_bloch[] = {&v, &p, &m, &bl, &d, &ca, &n, &step};
        void *h_lattice[] = {&v, &m, &la, &step};
        void *e_lattice[] = {&v, &m, &la, &d, &ca, &n, &step};
        if ((rc = launch_ptr(b, kh, grid, dim3(256), b->lattice ? h_lattice : h_bloch, 0))) return rc;
        if ((rc = launch_ptr(b, ke, grid, dim3(256), b->lattice ? e_lattice : e_bloch, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- Bloch runs with flux lines (fdtd2d_batch_bloch_flux.h): the paths of run_bloch and of run_bloch_dispersive with the
// kernels of batch_bloch_flux.hip, whose streamed H launch also writes the lines' phasors
// fs: the line sources of a run with channels (nullptr: none, the kernels of batch_bloch_flux.hip; otherwise those of
// batch_bloch_flux_adjoint.hip, which take fs behind facc_im); conj: step with (c, -s)
template <class T>
int run_bloch_flux(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride,
                   fdtd::BatchBlochFluxSrc *fs = nullptr, bool conj = false)
{
    if (!b->ca || !b->ezx || !b->ez_im || !b->rho || b->lattice || !b->flux_acc || !b->flux_acc_im ||
        (b->bdisp && (!b->djh || !b->dq || !b->djh_im || !b->dq_im || !b->dcj || !b->da || !b->dck)))
        return bfail(b, FDTD2D_E_STATE, "Bloch batch with flux lines without its arrays");
    if (conj && !b->rho_conj) return bfail(b, FDTD2D_E_STATE, "Bloch batch without its conjugated rotations");
    const fdtd::BatchBlochFluxKernels &K = fs ? fdtd::batch_bloch_flux_src_kernels<T>() : fdtd::batch_bloch_flux_kernels<T>();
    const int disp = b->bdisp ? 1 : 0;
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchBloch<T> bl = bloch_view<T>(b, conj);
    fdtd::BatchBlochDisp<T> d{(T *)b->djh, (T *)b->dq, (T *)b->djh_im, (T *)b->dq_im,
                              (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    fdtd::BatchFlux f = flux_view(b);
    double *facc_im = b->flux_acc_im;
    b->run_conj = conj;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        if (per_thread > 4)
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the Bloch resident kernels' 4", per_thread);
        const void *kern = K.resident[disp];
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1)
            return bfail(b, FDTD2D_E_STATE, "Bloch flux resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, &bl, &d, &f, &facc_im, &ca, &n0, &nt, &step_base};
            void *src_args[] = {&v, &p, &m, &bl, &d, &f, &facc_im, fs, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), fs ? src_args : args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *h_args[] = {&v, &p, &m, &bl, &f, &step};
        void *e_args[] = {&v, &p, &m, &bl, &d, &f, &facc_im, &ca, &n, &step};
        void *h_src_args[] = {&v, &p, &m, &bl, &f, fs, &n, &step};
        void *e_src_args[] = {&v, &p, &m, &bl, &d, &f, &facc_im, fs, &ca, &n, &step};
        if ((rc = launch_ptr(b, K.h, grid, dim3(256), fs ? h_src_args : h_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.e[disp], grid, dim3(256), fs ? e_src_args : e_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- Hz Bloch runs (fdtd2d_batch_hz_bloch.h): the periodic paths of run_hz with the complex-field kernels of
// batch_hz_bloch.hip.  v.ce carries cb; the first streamed launch of a step is the E half-step.
template <class T> int run_hz_bloch(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    const int disp = b->dcj ? 1 : 0;
    if (!b->periodic || !b->ezx || !b->ca || !b->cb || !b->ch || !b->ez_im || !b->hx_im || !b->hy_im || !b->ezx_im ||
        !b->rho || !b->bloch_w ||
        (disp && (!b->djh || !b->dq || !b->djy || !b->dqy || !b->djh_im || !b->dq_im || !b->djy_im || !b->dqy_im ||
                  !b->da || !b->dck)))
        return bfail(b, FDTD2D_E_STATE, "Hz Bloch batch without its arrays");
    const fdtd::BatchHzBlochKernels &K = fdtd::batch_hz_bloch_kernels<T>();
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchBloch<T> bl = bloch_view<T>(b, false);
    fdtd::BatchHzBlochDisp<T> d{(T *)b->djh,    (T *)b->dq,    (T *)b->djy,    (T *)b->dqy,
                                (T *)b->djh_im, (T *)b->dq_im, (T *)b->djy_im, (T *)b->dqy_im,
                                (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    b->run_conj = false;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        if (per_thread > 4)
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the Hz Bloch resident kernel's 4", per_thread);
        const void *kern = K.resident[disp];
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "Hz Bloch resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, &bl, &d, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *e_args[] = {&v, &p, &m, &bl, &d, &ca, &step};
        void *h_args[] = {&v, &p, &m, &bl, &n, &step};
        if ((rc = launch_ptr(b, K.e[disp], grid, dim3(256), e_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.h, grid, dim3(256), h_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- Hz lattice runs (fdtd2d_batch_hz_lattice.h): the paths of run_lattice with the kernels of batch_hz_lattice.hip.
// v.ce carries cb; the first streamed launch of a step is the E half-step.
template <class T> int run_hz_lattice(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    const int disp = b->dcj ? 1 : 0;
    if (!b->periodic || !b->ca || !b->cb || !b->ch || !b->ez_im || !b->hx_im || !b->hy_im || !b->rho || !b->rho_r ||
        !b->bloch_w ||
        (disp && (!b->djh || !b->dq || !b->djy || !b->dqy || !b->djh_im || !b->dq_im || !b->djy_im || !b->dqy_im ||
                  !b->da || !b->dck)))
        return bfail(b, FDTD2D_E_STATE, "Hz lattice batch without its arrays");
    const fdtd::BatchHzLatticeKernels &K = fdtd::batch_hz_lattice_kernels<T>();
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchLattice<T> la{(T *)b->ez_im, (T *)b->hx_im, (T *)b->hy_im, (const T *)b->rho_r, (const T *)b->rho,
                             b->bloch_w, b->have_src ? b->run_amps_im : nullptr, b->win_acc_im, b->probe_trace_im};
    fdtd::BatchHzBlochDisp<T> d{(T *)b->djh,    (T *)b->dq,    (T *)b->djy,    (T *)b->dqy,
                                (T *)b->djh_im, (T *)b->dq_im, (T *)b->djy_im, (T *)b->dqy_im,
                                (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    b->run_conj = false;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        const void *kern = per_thread <= 4 ? K.resident[disp][0] : per_thread <= 5 ? K.resident[disp][1] : nullptr;
        if (!kern)
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the Hz lattice resident kernels", per_thread);
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1) return bfail(b, FDTD2D_E_STATE, "Hz lattice resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &m, &la, &d, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *e_args[] = {&v, &m, &la, &d, &ca, &step};
        void *h_args[] = {&v, &m, &la, &n, &step};
        if ((rc = launch_ptr(b, K.e[disp], grid, dim3(256), e_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.h, grid, dim3(256), h_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

// ---- Hz Bloch runs with flux lines (fdtd2d_batch_hz_bloch_flux.h): the paths of run_hz_bloch with the kernels of
// batch_hz_bloch_flux.hip, whose streamed E launch also writes the lines' phasors
template <class T> int run_hz_bloch_flux(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride)
{
    const int disp = b->dcj ? 1 : 0;
    if (!b->periodic || !b->ezx || !b->ca || !b->cb || !b->ch || !b->ez_im || !b->hx_im || !b->hy_im || !b->ezx_im ||
        !b->rho || !b->bloch_w || !b->flux_acc || !b->flux_acc_im || !b->flux_omega || !b->flux_ph ||
        (disp && (!b->djh || !b->dq || !b->djy || !b->dqy || !b->djh_im || !b->dq_im || !b->djy_im || !b->dqy_im ||
                  !b->da || !b->dck)))
        return bfail(b, FDTD2D_E_STATE, "Hz Bloch batch with flux lines without its arrays");
    const fdtd::BatchHzBlochFluxKernels &K = fdtd::batch_hz_bloch_flux_kernels<T>();
    fdtd::BatchPml<T> p = pml_view<T>(b);
    fdtd::BatchMon m = mon_view(b);
    fdtd::BatchBloch<T> bl = bloch_view<T>(b, false);
    fdtd::BatchHzBlochDisp<T> d{(T *)b->djh,    (T *)b->dq,    (T *)b->djy,    (T *)b->dqy,
                                (T *)b->djh_im, (T *)b->dq_im, (T *)b->djy_im, (T *)b->dqy_im,
                                (const T *)b->dcj, (const T *)b->da, (const T *)b->dck};
    fdtd::BatchFlux f = flux_view(b);
    double *facc_im = b->flux_acc_im;
    b->run_conj = false;
    const T *ca = (const T *)b->ca;
    if (use_resident(b)) {
        const int cells = b->rows * b->cols, threads = resident_threads(cells);
        const int per_thread = (cells + threads - 1) / threads;
        if (per_thread > 4)
            return bfail(b, FDTD2D_E_STATE, "%d cells per thread exceed the Hz Bloch resident kernel's 4", per_thread);
        const void *kern = K.resident[disp];
        const size_t lds = lds_bytes(b);
        BCHK(b, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
        if (per_cu < 1)
            return bfail(b, FDTD2D_E_STATE, "Hz Bloch flux resident kernel does not fit a CU (%zu B of LDS)", lds);
        const long long round = (long long)per_cu * cus;
        const int blocks = (int)(b->count < round ? b->count : round);
        const int chunk = b->steps_per_launch > 0 ? b->steps_per_launch : nsteps;
        for (int n = 0; n < nsteps; n += chunk) {
            int n0 = n, nt = nsteps - n < chunk ? nsteps - n : chunk;
            long long step_base = b->step;
            fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
            v.ce = (const T *)b->cb;
            void *args[] = {&v, &p, &m, &bl, &d, &f, &facc_im, &ca, &n0, &nt, &step_base};
            int rc = launch_ptr(b, kern, dim3(blocks), dim3(threads), args, lds);
            if (rc) return rc;
            b->launches++;
            b->step += nt;
        }
        return 0;
    }
    const int cells = b->rows * b->cols;
    const dim3 grid((cells + 255) / 256, b->count < 65535 ? b->count : 65535);
    for (int n = 0; n < nsteps; ++n) {
        fdtd::BatchView<T> v = view<T>(b, amps, amp_stride);
        v.ce = (const T *)b->cb;
        long long step = b->step + 1;
        int rc;
        void *e_args[] = {&v, &p, &m, &bl, &d, &f, &ca, &step};
        void *h_args[] = {&v, &p, &m, &bl, &f, &facc_im, &n, &step};
        if ((rc = launch_ptr(b, K.e[disp], grid, dim3(256), e_args, 0))) return rc;
        if ((rc = launch_ptr(b, K.h, grid, dim3(256), h_args, 0))) return rc;
        b->launches += 2;
        b->step++;
    }
    return 0;
}

template <class T>
int run_impl(fdtd2d_batch *b, int nsteps, const double *amps, long long amp_stride, fdtd::BatchPts *pts = nullptr,
             fdtd::BatchFluxSrc *fs = nullptr)
{
    if (b->hzbflux) return run_hz_bloch_flux<T>(b, nsteps, amps, amp_stride);
    if (b->hz && b->lattice) return run_hz_lattice<T>(b, nsteps, amps, amp_stride);
    if (b->hz && b->bloch) return run_hz_bloch<T>(b, nsteps, amps, amp_stride);
    if (b->hz) return run_hz<T>(b, nsteps, amps, amp_stride, pts);
    if (b->bflux) return run_bloch_flux<T>(b, nsteps, amps, amp_stride);
    if (b->bdisp) return run_bloch_dispersive<T>(b, nsteps, amps, amp_stride);
    if (b->lattice) return run_lattice<T>(b, nsteps, amps, amp_stride);
    if (b->bloch) return run_bloch<T>(b, nsteps, amps, amp_stride);
    if (b->flux_nl) return run_flux<T>(b, nsteps, amps, amp_stride, pts, fs);
    if (b->dcj) return run_dispersive<T>(b, nsteps, amps, amp_stride, pts);
    if (b->periodic) return run_periodic<T>(b, nsteps, amps, amp_stride, pts);
    if (b->ca) return run_lossy<T>(b, nsteps, amps, amp_stride, pts);
    if (b->win_nf || b->nprobe || pts) return run_monitored<T>(b, nsteps, amps, amp_stride, pts);
    const bool arr = !b->uniform;
    if (b->ezx) {
        if (use_resident(b))
            return arr ? run_resident_pml<T, true>(b, nsteps, amps, amp_stride)
                       : run_resident_pml<T, false>(b, nsteps, amps, amp_stride);
        return arr ? run_streamed_pml<T, true>(b, nsteps, amps, amp_stride)
                   : run_streamed_pml<T, false>(b, nsteps, amps, amp_stride);
    }
    if (use_resident(b))
        return arr ? run_resident<T, true>(b, nsteps, amps, amp_stride) : run_resident<T, false>(b, nsteps, amps, amp_stride);
    return arr ? run_streamed<T, true>(b, nsteps, amps, amp_stride) : run_streamed<T, false>(b, nsteps, amps, amp_stride);
}

int need_ready(fdtd2d_batch *b)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    return use_device(b);
}

int alloc(fdtd2d_batch *b, void **p, size_t bytes)
{
    if (hipMalloc(p, bytes) != hipSuccess) {
        *p = nullptr;
        return bfail(b, FDTD2D_E_NOMEM, "hipMalloc of %zu bytes failed", bytes);
    }
    return 0;
}

void release(void **p)
{
    if (*p) (void)hipFree(*p);
    *p = nullptr;
}

// host values of a run (amplitudes, channels) into a device buffer that grows as needed
int stage(fdtd2d_batch *b, double **dev, size_t *cap, const double *host, size_t bytes)
{
    BCHK(b, hipStreamSynchronize(b->stream));   // earlier launches may still read the buffer
    if (bytes > *cap) {
        release((void **)dev);
        *cap = 0;
        int rc = alloc(b, (void **)dev, bytes);
        if (rc) return rc;
        *cap = bytes;
    }
    BCHK(b, hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

// the device scratch of the design-loop entry points, at least `bytes` large; waits for the stream first
int scratch(fdtd2d_batch *b, size_t bytes)
{
    BCHK(b, hipStreamSynchronize(b->stream));
    if (bytes > b->dsg_cap) {
        release(&b->dsg);
        b->dsg_cap = 0;
        int rc = alloc(b, &b->dsg, bytes);
        if (rc) return rc;
        b->dsg_cap = bytes;
    }
    return 0;
}

// ---- fdtd2d_batch_lossy.h --------------------------------------------------------------------------------------
// cells nearer than this to an edge take no plain update (or, like [0, 0], set the Mur factor and the PML grading)
int sigma_margin(const fdtd2d_batch *b, int layer)
{
    if (b->lattice) return 0;                           // no edge: every cell of the period takes the plain update
    if (b->periodic) return layer > 6 ? layer : 6;      // rows alone (sigma_barred)
    return b->boundary == FDTD2D_BOUNDARY_MUR5 ? 6 : layer > 0 ? (layer > 6 ? layer : 6) : 1;
}

// whether cell (i, j) may not conduct with the margin mg; a periodic batch has no column margin (its image column is
// never read)
bool sigma_barred(const fdtd2d_batch *b, int i, int j, int mg)
{
    if (b->lattice) return false;
    const int hi = b->hz ? 2 : 1;       // Hz polarisation: Ex[i,j] and Ey[i,j] live at i + 1/2 and j + 1/2
    if (b->periodic) return j < b->cols - 1 && (i < mg || i > b->rows - hi - mg);
    return i < mg || i > b->rows - hi - mg || j < mg || j > b->cols - hi - mg;
}

// the first cell of sigma_host that is non-zero within `margin` cells of an edge: member * cells + cell, or -1
long long sigma_outside(const fdtd2d_batch *b, int margin)
{
    const size_t per = (size_t)b->rows * b->cols;
    for (size_t t = 0; t < b->sigma_host.size(); ++t) {
        const int i = (int)(t % per / b->cols), j = (int)(t % per % b->cols);
        if (b->sigma_host[t] != 0 && sigma_barred(b, i, j, margin))
            return (long long)t;
    }
    return -1;
}

// ca and cb of a window from sigma_host and eps_host: one upload, one launch (k_batch_sigma_window)
int lossy_reform(fdtd2d_batch *b, int r0, int c0, int nr, int nc)
{
    const size_t W = (size_t)nr * nc, n = (size_t)b->count * W, per = (size_t)b->rows * b->cols;
    std::vector<double> w(2 * n);
    for (int m = 0; m < b->count; ++m)
        for (int i = 0; i < nr; ++i)
            for (int j = 0; j < nc; ++j) {
                const size_t src = m * per + (size_t)(r0 + i) * b->cols + (c0 + j), dst = m * W + (size_t)i * nc + j;
                w[dst] = b->sigma_host[src];
                w[n + dst] = b->eps_host[src];
            }
    int rc = scratch(b, w.size() * sizeof(double));      // waits for launches that still read the coefficients
    if (rc) return rc;
    BCHK(b, hipMemcpyAsync(b->dsg, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    fdtd::batch_sigma_window_launch(b->ca, b->cb, b->ce, (const double *)b->dsg, b->dtype == FDTD2D_F64, b->count, r0, c0,
                                    nr, nc, b->pitch, b->mstride, b->dt, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

// the coefficient arrays of a uniform batch (there is no uniform lossy kernel)
int materialise_uniform(fdtd2d_batch *b)
{
    const std::vector<double> e((size_t)b->count * b->rows * b->cols, b->eps_u), u(e.size(), b->mu_u);
    return fdtd2d_batch_set_materials(b, e.data(), u.data(), FDTD2D_F64);
}

// sets (or patches, window != nullptr) the conductivity after the checks that need no device
int set_sigma(fdtd2d_batch *b, const int *window, const void *sigma, int dtype)
{
    if (!sigma) return bfail(b, FDTD2D_E_ARG, "sigma must not be NULL");
    if (dtype != FDTD2D_F32 && dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad dtype");
    if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    const int r0 = window ? window[0] : 0, c0 = window ? window[1] : 0;
    const int nr = window ? window[2] : b->rows, nc = window ? window[3] : b->cols;
    if (nr < 1 || nc < 1 || r0 < 0 || c0 < 0 || (long long)r0 + nr > b->rows || (long long)c0 + nc > b->cols)
        return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d is empty or outside the %dx%d grid", r0, c0, nr, nc, b->rows,
                     b->cols);
    const int mg = sigma_margin(b, b->ezx ? b->pml_L : 0);
    const size_t W = (size_t)nr * nc, per = (size_t)b->rows * b->cols;
    for (int m = 0; m < b->count; ++m)
        for (size_t t = 0; t < W; ++t) {
            const double s = get_elem(sigma, dtype, m * W + t);
            const int i = r0 + (int)(t / nc), j = c0 + (int)(t % nc);
            if (!(s >= 0) || !std::isfinite(s))
                return bfail(b, FDTD2D_E_ARG, "member %d: sigma must be >= 0 and finite (cell (%d,%d))", m, i, j);
            if (s != 0 && sigma_barred(b, i, j, mg))
                return bfail(b, FDTD2D_E_ARG, "member %d: sigma is non-zero at cell (%d,%d), within %d cells of an edge "
                             "(%s): only cells that take the plain update may conduct", m, i, j, mg,
                             b->periodic ? "the PML rows, the PEC rows and cell [0, 0] of a periodic batch"
                             : b->ezx ? "the PML layer, the frame and cell [0, 0]"
                                    : b->boundary == FDTD2D_BOUNDARY_MUR5 ? "the Mur frame and cell [0, 0]" : "the edge cells");
        }
    int rc = use_device(b);
    if (rc) return rc;
    if (b->uniform && (rc = materialise_uniform(b))) return rc;
    const bool fresh = !b->ca;
    if (fresh) {
        if ((rc = alloc(b, &b->ca, b->field_bytes))) return rc;
        if ((rc = alloc(b, &b->cb, b->field_bytes))) {
            release(&b->ca);
            return rc;
        }
        b->sigma_host.assign((size_t)b->count * per, 0.0);
        hipError_t e = hipMemsetAsync(b->ca, 0, b->field_bytes, b->stream);
        if (e == hipSuccess) e = hipMemsetAsync(b->cb, 0, b->field_bytes, b->stream);
        if (e != hipSuccess) {
            release(&b->ca);
            release(&b->cb);
            b->sigma_host.clear();
            return bfail(b, -(1000 + (int)e), "hipMemset of the lossy coefficients failed: %s", hipGetErrorString(e));
        }
    }
    for (int m = 0; m < b->count; ++m)
        for (size_t t = 0; t < W; ++t)
            b->sigma_host[m * per + (size_t)(r0 + t / nc) * b->cols + (c0 + t % nc)] = get_elem(sigma, dtype, m * W + t);
    rc = fresh ? lossy_reform(b, 0, 0, b->rows, b->cols) : lossy_reform(b, r0, c0, nr, nc);
    if (rc && fresh) {
        release(&b->ca);
        release(&b->cb);
        b->sigma_host.clear();
    }
    return rc;
}

// ---- fdtd2d_batch_periodic.h -----------------------------------------------------------------------------------
// column 0 of a field over its image column C-1, every row of every member (one strided device copy)
int copy_image(fdtd2d_batch *b, void *field)
{
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy2D((char *)field + (size_t)(b->cols - 1) * b->esz, (size_t)b->pitch * b->esz, field,
                        (size_t)b->pitch * b->esz, b->esz, (size_t)b->count * b->rows, hipMemcpyDeviceToDevice));
    return 0;
}

// row 0 of a field over its image row R-1, every member (one strided device copy); after copy_image the corner slot
// holds cell (0, 0)
int copy_row_image(fdtd2d_batch *b, void *field)
{
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy2D((char *)field + (size_t)(b->rows - 1) * b->pitch * b->esz, b->mstride * b->esz, field,
                        b->mstride * b->esz, (size_t)b->cols * b->esz, (size_t)b->count, hipMemcpyDeviceToDevice));
    return 0;
}

// no layer on a periodic batch: Ezx and the factor arrays stay (the periodic kernels always take them), every factor
// exactly 1 and pml_L = 0, so that every row takes the plain update (PEC top and bottom)
int unit_layer(fdtd2d_batch *b)
{
    const size_t rn = (size_t)b->count * 4 * b->rows, cn = (size_t)b->count * 4 * b->cols;
    BCHK(b, hipStreamSynchronize(b->stream));
    int rc;
    if (!b->ezx) {
        for (void **p : {&b->ezx, &b->pml_row, &b->pml_col}) {
            const size_t bytes = p == &b->ezx ? b->field_bytes : (p == &b->pml_row ? rn : cn) * b->esz;
            if ((rc = alloc(b, p, bytes))) {
                for (void **q : {&b->ezx, &b->pml_row, &b->pml_col}) release(q);
                return rc;
            }
        }
    }
    std::vector<unsigned char> ones((rn > cn ? rn : cn) * b->esz);
    for (size_t k = 0; k < (rn > cn ? rn : cn); ++k) {
        if (b->dtype == FDTD2D_F32) ((float *)ones.data())[k] = 1.0f;
        else ((double *)ones.data())[k] = 1.0;
    }
    BCHK(b, hipMemcpy(b->pml_row, ones.data(), rn * b->esz, hipMemcpyHostToDevice));
    BCHK(b, hipMemcpy(b->pml_col, ones.data(), cn * b->esz, hipMemcpyHostToDevice));
    BCHK(b, hipMemsetAsync(b->ezx, 0, b->field_bytes, b->stream));
    if (b->ezx_im) BCHK(b, hipMemsetAsync(b->ezx_im, 0, b->field_bytes, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    b->pml_L = 0;
    return 0;
}

// the first column factor of count x 4C that is not exactly 1: its index, or -1
long long colf_not_one(const fdtd2d_batch *b, const void *col_factors)
{
    for (size_t k = 0; k < (size_t)b->count * 4 * b->cols; ++k)
        if (get_elem(col_factors, b->dtype, k) != 1.0) return (long long)k;
    return -1;
}

// ca and cb of a periodic batch that has materials and no conductivity: all-zero sigma (ca = 1, cb = ce)
int periodic_coefficients(fdtd2d_batch *b)
{
    if (b->uniform) return materialise_uniform(b);      // fdtd2d_batch_set_materials comes back here
    const std::vector<double> zero((size_t)b->count * b->rows * b->cols, 0.0);
    int rc = set_sigma(b, nullptr, zero.data(), FDTD2D_F64);
    if (!rc) b->sigma_implicit = true;
    return rc;
}

// ---- fdtd2d_batch_dispersive.h ---------------------------------------------------------------------------------
int refuse_bloch(fdtd2d_batch *b, const char *what);

constexpr double DISP_EPS0 = 8.85418e-12;     // the library's vacuum constant (the reference's literal)

// what a batch with flux lines cannot do (fdtd2d_batch_flux.h and fdtd2d_batch_bloch_flux.h, "Scope")
int refuse_flux(fdtd2d_batch *b, const char *what)
{
    if (b->bflux)
        return bfail(b, FDTD2D_E_STATE, "%s is not available while Bloch flux lines are set: remove them first "
                     "(fdtd2d_batch_set_bloch_flux_lines with nlines = 0)", what);
    if (b->hzflux)
        return bfail(b, FDTD2D_E_STATE, "%s is not available while flux lines of the Hz polarisation are set: remove them "
                     "first (fdtd2d_batch_set_hz_flux_lines with nlines = 0)", what);
    if (b->hzbflux)
        return bfail(b, FDTD2D_E_STATE, "%s is not available while flux lines of the Hz Bloch phase are set: remove them "
                     "first (fdtd2d_batch_set_hz_bloch_flux_lines with nlines = 0)", what);
    return bfail(b, FDTD2D_E_STATE, "%s is not available while flux lines are set: remove them first "
                 "(fdtd2d_batch_set_flux_lines with nlines = 0)", what);
}

// removes the line sources of fdtd2d_batch_flux_adjoint.h (the stream is idle)
void fsrc_drop(fdtd2d_batch *b)
{
    for (void **p : {(void **)&b->fsrc_we, (void **)&b->fsrc_wh, (void **)&b->fsrc_geom, (void **)&b->fsrc_we_im,
                     (void **)&b->fsrc_wh_im})
        release(p);
    b->fsrc_nchan = 0;
}

// what a batch in the Hz polarisation cannot do (fdtd2d_batch_hz.h)
int refuse_hz(fdtd2d_batch *b, const char *what)
{
    return bfail(b, FDTD2D_E_STATE, "%s is not available in the Hz polarisation (fdtd2d_batch_set_polarization)", what);
}

int refuse_dispersive(fdtd2d_batch *b, const char *what)
{
    return bfail(b, FDTD2D_E_STATE, "%s is not available while a dispersive pole is set", what);
}

// the first cell of wp2_host that is non-zero where sigma_barred bars it with the margin: member * cells + cell, or -1
long long wp2_outside(const fdtd2d_batch *b, int margin)
{
    const size_t per = (size_t)b->rows * b->cols;
    for (size_t t = 0; t < b->wp2_host.size(); ++t) {
        const int i = (int)(t % per / b->cols), j = (int)(t % per % b->cols);
        if (b->wp2_host[t] != 0 && sigma_barred(b, i, j, margin)) return (long long)t;
    }
    return -1;
}

// dt^2 (omega0^2 + wp2 EPS0 / eps) + 8 dt^2 / (eps mu dx^2): at most 4 for a cell with a pole
double disp_stability(const fdtd2d_batch *b, double omega0, double wp2, double eps, double mu)
{
    const double dt2 = b->dt * b->dt;
    return dt2 * (omega0 * omega0 + wp2 * DISP_EPS0 / eps) + 8.0 * dt2 / (eps * mu * b->dx * b->dx);
}

// The stability check over a window of every member: eps(m, i, j) and wp2(m, i, j) give the values to judge, mu_min the
// members' smallest permeabilities.  FDTD2D_E_ARG naming the first offending member, or 0.
template <class Eps, class Wp2>
int disp_check_stability(fdtd2d_batch *b, const std::vector<double> &omega0, const std::vector<double> &mu_min, int r0,
                         int c0, int nr, int nc, Eps eps, Wp2 wp2)
{
    for (int m = 0; m < b->count; ++m)
        for (int i = r0; i < r0 + nr; ++i)
            for (int j = c0; j < c0 + nc; ++j) {
                const double w = wp2(m, i, j);
                if (!(w > 0)) continue;
                const double s = disp_stability(b, omega0[m], w, eps(m, i, j), mu_min[m]);
                if (!(s <= 4.0))
                    return bfail(b, FDTD2D_E_ARG, "member %d: the pole at cell (%d,%d) is unstable: dt^2 (omega0^2 + wp2 EPS0 / "
                                 "eps) + 8 dt^2 / (eps mu dx^2) = %.6g > 4", m, i, j, s);
            }
    return 0;
}

// eps and the smallest mu as the engine stores them, whether the batch holds arrays or uniform materials
double disp_eps_at(const fdtd2d_batch *b, int m, int i, int j)
{
    if (b->uniform) return as_engine(b, b->eps_u);
    return b->eps_host[(size_t)m * b->rows * b->cols + (size_t)i * b->cols + j];
}
std::vector<double> disp_mu_min(const fdtd2d_batch *b)
{
    return b->uniform ? std::vector<double>((size_t)b->count, as_engine(b, b->mu_u)) : b->mu_min;
}

// cj of a window from wp2_host and the dampings: one upload, one launch (k_batch_wp2_window)
int disp_reform(fdtd2d_batch *b, int r0, int c0, int nr, int nc)
{
    const size_t W = (size_t)nr * nc, n = (size_t)b->count * W, per = (size_t)b->rows * b->cols;
    std::vector<double> w(n + (size_t)b->count);
    for (int m = 0; m < b->count; ++m) {
        for (int i = 0; i < nr; ++i)
            for (int j = 0; j < nc; ++j)
                w[m * W + (size_t)i * nc + j] = b->wp2_host[m * per + (size_t)(r0 + i) * b->cols + (c0 + j)];
        w[n + m] = b->dt / (1.0 + b->disp_gamma[m] * b->dt / 2.0);
    }
    int rc = scratch(b, w.size() * sizeof(double));      // waits for launches that still read the coefficients
    if (rc) return rc;
    BCHK(b, hipMemcpyAsync(b->dsg, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    fdtd::batch_wp2_window_launch(b->dcj, (const double *)b->dsg, (const double *)b->dsg + n, b->dtype == FDTD2D_F64,
                                  b->count, r0, c0, nr, nc, b->pitch, b->mstride, b->dx, DISP_EPS0, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

void disp_release(fdtd2d_batch *b)
{
    for (void **p : {&b->djh, &b->dq, &b->dcj, &b->da, &b->dck, &b->djh_im, &b->dq_im, &b->djy, &b->dqy, &b->djy_im,
                     &b->dqy_im})
        release(p);
    release((void **)&b->win_held_disp);     // the held dispersive window goes with the pole
    b->bdisp = false;
    b->wp2_host.clear();
    b->disp_gamma.clear();
    b->disp_omega0.clear();
}

// the refusal of a call of fdtd2d_batch_dispersive.h while the pole of fdtd2d_batch_bloch_dispersive.h is set
int refuse_bloch_pole(fdtd2d_batch *b, const char *what, const char *use)
{
    return bfail(b, FDTD2D_E_STATE, "%s is not available on a batch with complex fields (a Bloch phase or the lattice "
                 "mode): use %s", what, use);
}

// sets the pole (window == nullptr: wp2 whole with gamma and omega0) or patches its strengths; complex: the pole of
// fdtd2d_batch_bloch_dispersive.h, whose entry point has made its own refusals
int set_disp(fdtd2d_batch *b, const int *window, const void *wp2, int dtype, const double *gamma, const double *omega0,
             bool complex = false)
{
    if (b->bdisp && !complex)
        return refuse_bloch_pole(b, window ? "fdtd2d_batch_set_dispersion_window" : "fdtd2d_batch_set_dispersion",
                                 window ? "fdtd2d_batch_set_bloch_dispersion_window" : "fdtd2d_batch_set_bloch_dispersion");
    if (window && !b->dcj)
        return bfail(b, FDTD2D_E_STATE, "no pole is set: call %s first",
                     complex ? "fdtd2d_batch_set_bloch_dispersion" : "fdtd2d_batch_set_dispersion");
    if (b->boundary != FDTD2D_BOUNDARY_NONE)
        return bfail(b, FDTD2D_E_STATE, "a dispersive pole needs a FDTD2D_BOUNDARY_NONE batch with a PML layer or periodic "
                     "columns, not the Mur frame");
    if (!b->ezx && !b->periodic)
        return bfail(b, FDTD2D_E_STATE, "a dispersive pole needs a PML layer (fdtd2d_batch_set_pml) or periodic columns: a "
                     "plain box has no dispersive kernels");
    if (b->bloch && !complex && !b->hz) return refuse_bloch(b, "a dispersive pole");
    if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    if (!wp2) return bfail(b, FDTD2D_E_ARG, "wp2 must not be NULL");
    if (dtype != FDTD2D_F32 && dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad dtype");
    const int r0 = window ? window[0] : 0, c0 = window ? window[1] : 0;
    const int nr = window ? window[2] : b->rows, nc = window ? window[3] : b->cols;
    if (nr < 1 || nc < 1 || r0 < 0 || c0 < 0 || (long long)r0 + nr > b->rows || (long long)c0 + nc > b->cols)
        return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d is empty or outside the %dx%d grid", r0, c0, nr, nc, b->rows,
                     b->cols);
    std::vector<double> gam = b->disp_gamma, om0 = b->disp_omega0;
    if (!window) {
        gam.assign(gamma, gamma + b->count);
        om0.assign(omega0, omega0 + b->count);
        for (int m = 0; m < b->count; ++m) {
            if (!(gam[m] >= 0) || !std::isfinite(gam[m]))
                return bfail(b, FDTD2D_E_ARG, "member %d: gamma must be >= 0 and finite", m);
            if (!(om0[m] >= 0) || !std::isfinite(om0[m]))
                return bfail(b, FDTD2D_E_ARG, "member %d: omega0 must be >= 0 and finite", m);
        }
    }
    const int mg = sigma_margin(b, b->ezx ? b->pml_L : 0);
    const size_t W = (size_t)nr * nc, per = (size_t)b->rows * b->cols;
    for (int m = 0; m < b->count; ++m)
        for (size_t t = 0; t < W; ++t) {
            const double s = get_elem(wp2, dtype, m * W + t);
            const int i = r0 + (int)(t / nc), j = c0 + (int)(t % nc);
            if (!(s >= 0) || !std::isfinite(s))
                return bfail(b, FDTD2D_E_ARG, "member %d: wp2 must be >= 0 and finite (cell (%d,%d))", m, i, j);
            if (s != 0 && sigma_barred(b, i, j, mg))
                return bfail(b, FDTD2D_E_ARG, "member %d: wp2 is non-zero at cell (%d,%d), within %d cells of an edge "
                             "(%s): only cells that take the plain update may carry a pole", m, i, j, mg,
                             b->periodic ? "the PML rows, the PEC rows and cell [0, 0] of a periodic batch"
                                         : "the PML layer, the frame and cell [0, 0]");
        }
    int rc = disp_check_stability(
        b, om0, disp_mu_min(b), r0, c0, nr, nc, [&](int m, int i, int j) { return disp_eps_at(b, m, i, j); },
        [&](int m, int i, int j) { return get_elem(wp2, dtype, m * W + (size_t)(i - r0) * nc + (j - c0)); });
    if (rc) return rc;
    if ((rc = use_device(b))) return rc;
    if (b->uniform && (rc = materialise_uniform(b))) return rc;
    if (!b->ca) {                           // no conductivity: ca = 1, cb = ce
        const std::vector<double> zero((size_t)b->count * per, 0.0);
        if ((rc = set_sigma(b, nullptr, zero.data(), FDTD2D_F64))) return rc;
        b->sigma_implicit = true;
    }
    const bool fresh = !b->dcj;
    if (fresh) {
        const size_t mb = (size_t)b->count * b->esz;
        const bool hzb = b->hz && b->bloch;      // fdtd2d_batch_hz_bloch.h: both parts of Jx, Qx, Jy, Qy
        for (void **p : {&b->djh, &b->dq, &b->dcj, &b->da, &b->dck, &b->djh_im, &b->dq_im, &b->djy, &b->dqy, &b->djy_im,
                         &b->dqy_im}) {
            if (!complex && !hzb && (p == &b->djh_im || p == &b->dq_im)) continue;
            if (!b->hz && (p == &b->djy || p == &b->dqy)) continue;
            if (!hzb && (p == &b->djy_im || p == &b->dqy_im)) continue;
            const size_t bytes = (p == &b->da || p == &b->dck) ? mb : b->field_bytes;
            hipError_t e = hipSuccess;
            if ((rc = alloc(b, p, bytes)) || (e = hipMemsetAsync(*p, 0, bytes, b->stream)) != hipSuccess) {
                if (!rc) rc = bfail(b, -(1000 + (int)e), "hipMemset of the pole's arrays failed: %s", hipGetErrorString(e));
                disp_release(b);
                return rc;
            }
        }
        b->wp2_host.assign((size_t)b->count * per, 0.0);
        b->bdisp = complex;
    }
    for (int m = 0; m < b->count; ++m)
        for (size_t t = 0; t < W; ++t)
            b->wp2_host[m * per + (size_t)(r0 + t / nc) * b->cols + (c0 + t % nc)] = get_elem(wp2, dtype, m * W + t);
    if (!window) {
        b->disp_gamma = gam;
        b->disp_omega0 = om0;
        std::vector<unsigned char> at((size_t)b->count * b->esz), ckt(at.size());
        for (int m = 0; m < b->count; ++m) {
            const double g = gam[m] * b->dt / 2.0, bq = b->dt / (1.0 + g);
            const double a = (1.0 - g) / (1.0 + g), ck = bq * (om0[m] * om0[m]) * b->dt;
            if (b->dtype == FDTD2D_F32) {
                ((float *)at.data())[m] = (float)a;
                ((float *)ckt.data())[m] = (float)ck;
            } else {
                ((double *)at.data())[m] = a;
                ((double *)ckt.data())[m] = ck;
            }
        }
        hipError_t e = hipStreamSynchronize(b->stream);      // a running launch may still read the old scalars
        if (e == hipSuccess) e = hipMemcpy(b->da, at.data(), at.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(b->dck, ckt.data(), ckt.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (fresh) disp_release(b);
            return bfail(b, -(1000 + (int)e), "upload of the pole's scalars failed: %s", hipGetErrorString(e));
        }
    }
    rc = window ? disp_reform(b, r0, c0, nr, nc) : disp_reform(b, 0, 0, b->rows, b->cols);
    if (rc && fresh) disp_release(b);
    return rc;
}

// ---- fdtd2d_batch_bloch.h ----------------------------------------------------------------------------------------
// rho * (re, im) as the kernels form it (batch_bloch_rot), in the engine's type: part 0 = real, 1 = imaginary
template <class T> double bloch_rot_host(double c, double s, double re, double im, int part)
{
    const T ct = (T)c, st = (T)s, rt = (T)re, it = (T)im;
#ifdef FDTD2D_FUSED
    return part ? (double)std::fma(st, rt, (T)(ct * it)) : (double)std::fma(ct, rt, (T)-(st * it));
#else
    const T x = part ? st * rt : ct * rt, y = part ? ct * it : st * it;
    return part ? (double)(T)(x + y) : (double)(T)(x - y);
#endif
}

// Ez or Ezx of a Bloch batch, device -> host (count x rows x cols): one part, the image column delivered as
// rho * the image slot (which holds the unrotated copy of column 0)
int copy_out_bloch(fdtd2d_batch *b, const void *re, const void *im, void *host, int host_dtype, int part)
{
    // the wanted part whole; of the other part only the image slots, which the rotation needs: the stored rows of the
    // batch are count * rows lines of one pitch (mstride = rows * pitch), so that column is one strided copy
    const int C = b->cols;
    const size_t lines = (size_t)b->count * b->rows;
    std::vector<unsigned char> own(b->field_bytes), other(lines * b->esz);
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(own.data(), part ? im : re, b->field_bytes, hipMemcpyDeviceToHost));
    BCHK(b, hipMemcpy2D(other.data(), b->esz, (const unsigned char *)(part ? re : im) + (size_t)(C - 1) * b->esz,
                        (size_t)b->pitch * b->esz, b->esz, lines, hipMemcpyDeviceToHost));
    for (int m = 0; m < b->count; ++m)
        for (int i = 0; i < b->rows; ++i) {
            const size_t line = (size_t)m * b->rows + i, dst = line * C, src = (size_t)m * b->mstride + (size_t)i * b->pitch;
            for (int j = 0; j < C; ++j) {
                double v = get_elem(own.data(), b->dtype, src + j);
                if (j == C - 1) {
                    const double o = get_elem(other.data(), b->dtype, line);
                    const double zr = part ? o : v, zi = part ? v : o;
                    const double c = b->rho_host[2 * m], s = b->run_conj ? -b->rho_host[2 * m + 1] : b->rho_host[2 * m + 1];
                    v = b->dtype == FDTD2D_F32 ? bloch_rot_host<float>(c, s, zr, zi, part)
                                               : bloch_rot_host<double>(c, s, zr, zi, part);
                }
                if (host_dtype == FDTD2D_F32) ((float *)host)[dst + j] = (float)v;
                else ((double *)host)[dst + j] = v;
            }
        }
    return 0;
}

// Ez of a lattice batch, device -> host (count x rows x cols): one part, the images delivered rotated: column C-1 as
// rho_c * its slot, row R-1 as rho_r * its slot, the corner as rho_r * (rho_c * its slot), each rotation rounded to T
// (the slots hold the unrotated copies of column 0, of row 0 and of cell (0, 0))
int copy_out_lattice(fdtd2d_batch *b, const void *re, const void *im, void *host, int host_dtype, int part)
{
    const int R = b->rows, C = b->cols;
    std::vector<unsigned char> sr(b->field_bytes), si(b->field_bytes);
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(sr.data(), re, b->field_bytes, hipMemcpyDeviceToHost));
    BCHK(b, hipMemcpy(si.data(), im, b->field_bytes, hipMemcpyDeviceToHost));
    const bool f32 = b->dtype == FDTD2D_F32;
    auto rot = [&](double c, double s, double &zr, double &zi) {
        const double nr = f32 ? bloch_rot_host<float>(c, s, zr, zi, 0) : bloch_rot_host<double>(c, s, zr, zi, 0);
        const double ni = f32 ? bloch_rot_host<float>(c, s, zr, zi, 1) : bloch_rot_host<double>(c, s, zr, zi, 1);
        zr = nr;
        zi = ni;
    };
    for (int m = 0; m < b->count; ++m)
        for (int i = 0; i < R; ++i) {
            const size_t dst = ((size_t)m * R + i) * C, src = (size_t)m * b->mstride + (size_t)i * b->pitch;
            for (int j = 0; j < C; ++j) {
                double zr = get_elem(sr.data(), b->dtype, src + j), zi = get_elem(si.data(), b->dtype, src + j);
                if (j == C - 1) rot(b->rho_host[2 * m], b->rho_host[2 * m + 1], zr, zi);
                if (i == R - 1) rot(b->rho_r_host[2 * m], b->rho_r_host[2 * m + 1], zr, zi);
                const double v = part ? zi : zr;
                if (host_dtype == FDTD2D_F32) ((float *)host)[dst + j] = (float)v;
                else ((double *)host)[dst + j] = v;
            }
        }
    return 0;
}

// the imaginary part of the window DFT / of the probe traces: there (zeroed) exactly while a Bloch phase and the
// monitor are both set.  The caller has waited for the stream.
int bloch_window(fdtd2d_batch *b)
{
    release((void **)&b->win_acc_im);
    release((void **)&b->win_held_im);     // the held Bloch window goes with the window (win_held: the caller's)
    if (!b->bloch || !b->win_nf) return 0;
    const size_t bytes = (size_t)b->count * win_acc_bytes(b);
    int rc = alloc(b, (void **)&b->win_acc_im, bytes);
    if (rc) return rc;
    BCHK(b, hipMemsetAsync(b->win_acc_im, 0, bytes, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int bloch_probes(fdtd2d_batch *b)
{
    release((void **)&b->probe_trace_im);
    if (!b->bloch || !b->nprobe) return 0;
    const size_t bytes = (size_t)b->count * b->nprobe * (size_t)b->probe_cap * sizeof(double);
    int rc = alloc(b, (void **)&b->probe_trace_im, bytes);
    if (rc) return rc;
    BCHK(b, hipMemsetAsync(b->probe_trace_im, 0, bytes, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

// the first probe in column C-1 (member * nprobe + probe), or -1
long long probe_in_image(const fdtd2d_batch *b, const std::vector<int> &lin)
{
    for (size_t k = 0; k < lin.size(); ++k)
        if (lin[k] % b->cols == b->cols - 1) return (long long)k;
    return -1;
}

int bloch_off(fdtd2d_batch *b)
{
    BCHK(b, hipStreamSynchronize(b->stream));
    for (void **p : {&b->ez_im, &b->hx_im, &b->hy_im, &b->ezx_im, &b->rho, &b->rho_conj, &b->rho_r, (void **)&b->bloch_w,
                     (void **)&b->amps_im, (void **)&b->win_acc_im, (void **)&b->probe_trace_im,
                     (void **)&b->win_held, (void **)&b->win_held_im})     // a held window here is a Bloch one
        release(p);
    b->amps_im_cap = 0;
    b->rho_host.clear();
    b->rho_r_host.clear();
    b->bloch = b->run_conj = b->lattice = false;
    if (b->hz)                              // fdtd2d_batch_hz_bloch.h: the imaginary parts of the pole state go too
        for (void **p : {&b->djh_im, &b->dq_im, &b->djy_im, &b->dqy_im}) release(p);
    return batch_set_points(b, 0, nullptr, 0, nullptr);      // the point sources of a Bloch batch go with the phase
}

// leaving the lattice mode makes a plain periodic batch: the first cell of sigma_host that is non-zero where that batch
// allows none (member * cells + cell), or -1
long long lattice_sigma_outside(fdtd2d_batch *b)
{
    if (!b->lattice || !b->ca) return -1;
    b->lattice = false;
    const long long t = sigma_outside(b, sigma_margin(b, 0));
    b->lattice = true;
    return t;
}

int refuse_lattice_off(fdtd2d_batch *b, long long t)
{
    return bfail(b, FDTD2D_E_ARG, "member %d: sigma is non-zero within 6 rows of the top or bottom edge, where a periodic "
                 "batch without the lattice mode allows none: remove it first", (int)(t / ((long long)b->rows * b->cols)));
}

int refuse_bloch(fdtd2d_batch *b, const char *what)
{
    if (b->lattice) return bfail(b, FDTD2D_E_STATE, "%s is not available in the lattice mode (complex fields)", what);
    return bfail(b, FDTD2D_E_STATE, "%s is not available while a Bloch phase is set (complex fields)", what);
}

// the first probe in row R-1 or column C-1 (member * nprobe + probe), or -1
long long probe_in_lattice_image(const fdtd2d_batch *b, const std::vector<int> &lin)
{
    for (size_t k = 0; k < lin.size(); ++k)
        if (lin[k] % b->cols == b->cols - 1 || lin[k] / b->cols == b->rows - 1) return (long long)k;
    return -1;
}

}  // namespace

// ===================================== C ABI ============================================

extern "C" {

int fdtd2d_batch_create(fdtd2d_batch_t **out, int count, int rows, int cols, double dt, double dx, int dtype,
                        int boundary, int device)
{
    if (!out) return bfail(nullptr, FDTD2D_E_ARG, "out is NULL");
    *out = nullptr;
    if (count < 1) return bfail(nullptr, FDTD2D_E_ARG, "count must be >= 1, not %d", count);
    if (rows < 11 || cols < 11)
        return bfail(nullptr, FDTD2D_E_ARG, "grid %dx%d is below the 11x11 minimum of the 5-px Mur band", rows, cols);
    if (dtype != FDTD2D_F32 && dtype != FDTD2D_F64)
        return bfail(nullptr, FDTD2D_E_ARG, "dtype must be FDTD2D_F32 or FDTD2D_F64");
    if (boundary != FDTD2D_BOUNDARY_NONE && boundary != FDTD2D_BOUNDARY_MUR5)
        return bfail(nullptr, FDTD2D_E_ARG, "boundary %d: a batch takes FDTD2D_BOUNDARY_NONE or _MUR5", boundary);
    if (!(dt > 0) || !(dx > 0)) return bfail(nullptr, FDTD2D_E_ARG, "dt and dx must be positive");
    if (device < 0) return bfail(nullptr, FDTD2D_E_ARG, "device %d out of range", device);
    if (rows > (1 << 20) || cols > (1 << 20) || (long long)rows * cols > (1LL << 30))
        return bfail(nullptr, FDTD2D_E_ARG, "member %dx%d is too large", rows, cols);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return bfail(nullptr, FDTD2D_E_NODEVICE, "no HIP device available (%s); libfdtd2d has no CPU path",
                     e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device >= ndev) return bfail(nullptr, FDTD2D_E_ARG, "device %d out of range (%d visible)", device, ndev);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess)
        return bfail(nullptr, FDTD2D_E_NODEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return bfail(nullptr, FDTD2D_E_NODEVICE, "device %d is %s; this library is built for gfx950", device,
                     prop.gcnArchName);

    fdtd2d_batch *b = new fdtd2d_batch();
    b->count = count; b->rows = rows; b->cols = cols;
    b->dt = dt; b->dx = dx; b->dtype = dtype; b->boundary = boundary; b->device = device;
    b->esz = dtype == FDTD2D_F32 ? 4 : 8;
    b->pitch = ((long long)cols + 63) / 64 * 64;
    b->mstride = (size_t)rows * (size_t)b->pitch;
    b->field_bytes = (size_t)count * b->mstride * b->esz;
    b->courant.assign((size_t)count, 0.0);
    auto bail = [&](int code) {
        g_batch_create_error = b->err;
        fdtd2d_batch_destroy(b);
        return code;
    };
    int rc = use_device(b);
    if (rc) return bail(rc);
    if (hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking) != hipSuccess)
        return bail(bfail(b, FDTD2D_E_NODEVICE, "hipStreamCreate failed"));
    b->stream = b->own_stream;
    for (void **p : {&b->ez[0], &b->ez[1], &b->hx, &b->hy})
        if ((rc = alloc(b, p, b->field_bytes))) return bail(rc);
    if ((rc = alloc(b, &b->kmur, (size_t)count * b->esz))) return bail(rc);
    if ((rc = alloc(b, (void **)&b->rect, (size_t)count * 4 * sizeof(int)))) return bail(rc);
    if (hipMemsetAsync(b->rect, 0, (size_t)count * 4 * sizeof(int), b->stream) != hipSuccess)
        return bail(bfail(b, FDTD2D_E_NODEVICE, "hipMemset of the source rectangles failed"));
    if ((rc = zero_fields(b))) return bail(rc);
    if (hipStreamSynchronize(b->stream) != hipSuccess)
        return bail(bfail(b, FDTD2D_E_NODEVICE, "device sync failed after allocation"));
    *out = b;
    return 0;
}

void fdtd2d_batch_destroy(fdtd2d_batch_t *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (void **p : {&b->ez[0], &b->ez[1], &b->hx, &b->hy, &b->ce, &b->ch, &b->kmur, (void **)&b->rect,
                     (void **)&b->amps, &b->ezx, &b->pml_row, &b->pml_col, (void **)&b->dft, (void **)&b->omega,
                     (void **)&b->win_acc, (void **)&b->win_omega, (void **)&b->win_ph, (void **)&b->probe_cells,
                     (void **)&b->probe_trace, (void **)&b->win_held, (void **)&b->pts_cells, (void **)&b->pts_own,
                     (void **)&b->pts_w, (void **)&b->pts_tab, (void **)&b->chan, &b->dsg, &b->ca, &b->cb,
                     &b->ez_im, &b->hx_im, &b->hy_im, &b->ezx_im, &b->rho, (void **)&b->bloch_w, (void **)&b->amps_im,
                     (void **)&b->win_acc_im, (void **)&b->probe_trace_im, &b->rho_conj, &b->rho_r,
                     (void **)&b->win_held_im, (void **)&b->win_held_disp,
                     &b->djh, &b->dq, &b->dcj, &b->da, &b->dck, &b->djh_im, &b->dq_im, &b->djy, &b->dqy,
                     &b->djy_im, &b->dqy_im, (void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph,
                     (void **)&b->flux_acc_im, (void **)&b->fsrc_we, (void **)&b->fsrc_wh,
                     (void **)&b->fsrc_geom, (void **)&b->fsrc_we_im, (void **)&b->fsrc_wh_im})
        release(p);
    if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
    delete b;
}

const char *fdtd2d_batch_last_error(const fdtd2d_batch_t *b)
{
    return b ? b->err.c_str() : g_batch_create_error.c_str();
}

long long fdtd2d_batch_info(const fdtd2d_batch_t *b, int what)
{
    if (!b) return FDTD2D_E_ARG;
    switch (what) {
    case FDTD2D_BATCH_INFO_COUNT: return b->count;
    case FDTD2D_BATCH_INFO_ROWS: return b->rows;
    case FDTD2D_BATCH_INFO_COLS: return b->cols;
    case FDTD2D_BATCH_INFO_DTYPE: return b->dtype;
    case FDTD2D_BATCH_INFO_STEP: return b->step;
    case FDTD2D_BATCH_INFO_RESIDENT: return use_resident(b) ? 1 : 0;
    case FDTD2D_BATCH_INFO_LAUNCHES: return b->launches;
    case FDTD2D_BATCH_INFO_RESIDENT_MAX_CELLS: return resident_max_cells(b);
    case FDTD2D_BATCH_INFO_LDS_BYTES: return (long long)lds_bytes(b);
    case FDTD2D_BATCH_INFO_PITCH: return b->pitch;
    case FDTD2D_BATCH_INFO_DFT_WINDOW_LDS: return use_resident(b) && win_acc_in_lds(b) ? 1 : 0;
    case FDTD2D_BATCH_INFO_PROBE_SAMPLES: {
        if (!b->nprobe) return 0;
        const long long n = b->step - b->probe_step0;
        return n < b->probe_cap ? n : b->probe_cap;
    }
    case FDTD2D_BATCH_INFO_POINT_SOURCES: return b->bloch ? 0 : b->npts_user;
    case FDTD2D_BATCH_INFO_HELD_WINDOW: return b->win_held && !b->bloch ? 1 : 0;
    case FDTD2D_BATCH_INFO_BLOCH_POINT_SOURCES: return b->bloch ? b->npts_user : 0;
    case FDTD2D_BATCH_INFO_HELD_BLOCH_WINDOW: return b->win_held && b->win_held_im && b->bloch ? 1 : 0;
    case FDTD2D_BATCH_INFO_LOSSY: return b->ca && !b->sigma_implicit ? 1 : 0;
    case FDTD2D_BATCH_INFO_PERIODIC: return b->periodic ? 1 : 0;
    case FDTD2D_BATCH_INFO_BLOCH: return b->bloch && !b->lattice && !b->hz ? 1 : 0;
    case FDTD2D_BATCH_INFO_HZ_BLOCH: return b->bloch && b->hz && !b->lattice ? 1 : 0;
    case FDTD2D_BATCH_INFO_HZ_LATTICE: return b->lattice && b->hz ? 1 : 0;
    case FDTD2D_BATCH_INFO_DISPERSIVE: return b->dcj ? 1 : 0;
    case FDTD2D_BATCH_INFO_HELD_DISPERSIVE_WINDOW: return b->win_held_disp ? 1 : 0;
    case FDTD2D_BATCH_INFO_FLUX_LINES: return b->flux_nl;
    case FDTD2D_BATCH_INFO_FLUX_LDS: return use_resident(b) && flux_acc_in_lds(b) ? 1 : 0;
    case FDTD2D_BATCH_INFO_FLUX_LINE_SOURCES: return b->fsrc_nchan;
    default: return FDTD2D_E_ARG;
    }
}

int fdtd2d_batch_set_option(fdtd2d_batch_t *b, int option, long long value)
{
    if (!b) return FDTD2D_E_ARG;
    switch (option) {
    case FDTD2D_BATCH_OPT_RESIDENT:
        if (value != -1 && value != 0) return bfail(b, FDTD2D_E_ARG, "resident must be -1 (auto) or 0 (never)");
        b->resident_opt = (int)value;
        return 0;
    case FDTD2D_BATCH_OPT_STEPS_PER_LAUNCH:
        if (value < 0 || value > (1 << 30)) return bfail(b, FDTD2D_E_ARG, "steps per launch must be >= 0");
        b->steps_per_launch = (int)value;
        return 0;
    case FDTD2D_BATCH_OPT_DFT_WINDOW_LDS:
        if (value != -1 && value != 0) return bfail(b, FDTD2D_E_ARG, "window LDS must be -1 (auto) or 0 (never)");
        b->win_lds_opt = (int)value;
        return 0;
    case FDTD2D_BATCH_OPT_FLUX_LDS:
        if (value != -1 && value != 0) return bfail(b, FDTD2D_E_ARG, "flux LDS must be -1 (auto) or 0 (never)");
        b->flux_lds_opt = (int)value;
        return 0;
    default: return bfail(b, FDTD2D_E_ARG, "unknown option %d", option);
    }
}

int fdtd2d_batch_set_stream(fdtd2d_batch_t *b, void *hip_stream)
{
    if (!b) return FDTD2D_E_ARG;
    b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
    return 0;
}

int fdtd2d_batch_set_materials(fdtd2d_batch_t *b, const void *eps, const void *mu, int host_dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (!eps || !mu) return bfail(b, FDTD2D_E_ARG, "eps and mu must not be NULL");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    const size_t per = (size_t)b->rows * b->cols;
    std::vector<double> emin((size_t)b->count, 1e300), mmin((size_t)b->count, 1e300), kmur((size_t)b->count);
    std::vector<double> eps_host((size_t)b->count * per);
    for (int m = 0; m < b->count; ++m) {
        for (size_t t = 0; t < per; ++t) {
            const double e = eps_host[m * per + t] = as_engine(b, get_elem(eps, host_dtype, m * per + t));
            const double u = as_engine(b, get_elem(mu, host_dtype, m * per + t));
            if (!(e > 0) || !(u > 0))
                return bfail(b, FDTD2D_E_ARG, "eps and mu must be positive (member %d, cell %zu)", m, t);
            emin[m] = e < emin[m] ? e : emin[m];
            mmin[m] = u < mmin[m] ? u : mmin[m];
        }
        const double e00 = get_elem(eps, host_dtype, m * per), u00 = get_elem(mu, host_dtype, m * per);
        kmur[m] = b->dtype == FDTD2D_F32 ? mur_of<float>(e00, u00, b->dt, b->dx) : mur_of<double>(e00, u00, b->dt, b->dx);
    }
    int rc;
    if (b->dcj &&           // the pole's stability with the new materials, before anything changes
        (rc = disp_check_stability(
             b, b->disp_omega0, mmin, 0, 0, b->rows, b->cols,
             [&](int m, int i, int j) { return eps_host[m * per + (size_t)i * b->cols + j]; },
             [&](int m, int i, int j) { return b->wp2_host[m * per + (size_t)i * b->cols + j]; })))
        return rc;
    if ((rc = use_device(b))) return rc;
    b->have_mat = false;
    for (void **p : {&b->ce, &b->ch})
        if (!*p && (rc = alloc(b, p, b->field_bytes))) return rc;
    // the arrays are uploaded as eps / mu in T, then turned into dt/(x*dx) in place (padding stays 0)
    if ((rc = copy_in(b, b->ce, eps, host_dtype, b->rows, b->cols))) return rc;
    if ((rc = copy_in(b, b->ch, mu, host_dtype, b->rows, b->cols))) return rc;
    const size_t n = (size_t)b->count * b->mstride;
    for (void *p : {b->ce, b->ch}) {
        if (b->dtype == FDTD2D_F32)
            hipLaunchKernelGGL((fdtd::k_coef<float>), dim3(2048), dim3(256), 0, b->stream, (float *)p, n, (float)b->dt,
                               (float)b->dx);
        else
            hipLaunchKernelGGL((fdtd::k_coef<double>), dim3(2048), dim3(256), 0, b->stream, (double *)p, n, b->dt, b->dx);
        BCHK(b, hipGetLastError());
    }
    std::vector<unsigned char> kt((size_t)b->count * b->esz);
    for (int m = 0; m < b->count; ++m) {
        if (b->dtype == FDTD2D_F32) ((float *)kt.data())[m] = (float)kmur[m];
        else ((double *)kt.data())[m] = kmur[m];
        b->courant[m] = courant_of(emin[m], mmin[m], b->dt, b->dx);
    }
    BCHK(b, hipMemcpyAsync(b->kmur, kt.data(), kt.size(), hipMemcpyHostToDevice, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    b->eps_host.swap(eps_host);
    b->mu_min.swap(mmin);
    b->eps_out_min.clear();
    b->uniform = false;
    b->have_mat = true;
    if ((b->periodic || b->hz) && !b->ca) return periodic_coefficients(b);
    return b->ca ? lossy_reform(b, 0, 0, b->rows, b->cols) : 0;
}

int fdtd2d_batch_set_materials_uniform(fdtd2d_batch_t *b, double eps, double mu)
{
    if (!b) return FDTD2D_E_ARG;
    if (!(eps > 0) || !(mu > 0)) return bfail(b, FDTD2D_E_ARG, "eps and mu must be positive");
    const double eps_was = b->eps_u, mu_was = b->mu_u;
    b->eps_u = eps;
    b->mu_u = mu;
    if (b->ca) {                                   // a lossy batch keeps coefficient arrays
        const int rc = materialise_uniform(b);
        if (rc && b->dcj) {                        // refused (the pole's stability): as it was
            b->eps_u = eps_was;
            b->mu_u = mu_was;
        }
        return rc;
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    release(&b->ce);
    release(&b->ch);
    double k;
    if (b->dtype == FDTD2D_F32) {
        b->ce_u = coef_of<float>(eps, b->dt, b->dx);
        b->ch_u = coef_of<float>(mu, b->dt, b->dx);
        k = mur_of<float>(eps, mu, b->dt, b->dx);
    } else {
        b->ce_u = coef_of<double>(eps, b->dt, b->dx);
        b->ch_u = coef_of<double>(mu, b->dt, b->dx);
        k = mur_of<double>(eps, mu, b->dt, b->dx);
    }
    std::vector<unsigned char> kt((size_t)b->count * b->esz);
    for (int m = 0; m < b->count; ++m) {
        if (b->dtype == FDTD2D_F32) ((float *)kt.data())[m] = (float)k;
        else ((double *)kt.data())[m] = k;
    }
    BCHK(b, hipMemcpy(b->kmur, kt.data(), kt.size(), hipMemcpyHostToDevice));
    b->courant.assign((size_t)b->count, courant_of(eps, mu, b->dt, b->dx));
    b->uniform = true;
    b->have_mat = true;
    return b->periodic || b->hz ? periodic_coefficients(b) : 0;   // a periodic or Hz batch keeps coefficient arrays
}

int fdtd2d_batch_set_pml(fdtd2d_batch_t *b, const void *row_factors, const void *col_factors, int host_dtype,
                         int layer_cells)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->boundary != FDTD2D_BOUNDARY_NONE)
        return bfail(b, FDTD2D_E_STATE, "the PML needs a batch created with FDTD2D_BOUNDARY_NONE (its outer edge is PEC)");
    int rc = use_device(b);
    if (rc) return rc;
    if (!row_factors && !col_factors && b->lattice) return 0;                // there is no layer to remove
    if (!row_factors && !col_factors && b->periodic) return unit_layer(b);   // PEC top and bottom
    if (!row_factors && !col_factors && b->dcj)
        return refuse_dispersive(b, "removing the layer of a batch without periodic columns (a plain box has no "
                                    "dispersive kernels)");
    if (!row_factors && !col_factors && b->flux_nl) return refuse_flux(b, "removing the layer of a batch without periodic columns");
    if (!row_factors && !col_factors) {     // remove the layer: a plain NONE batch again
        BCHK(b, hipStreamSynchronize(b->stream));
        for (void **p : {&b->ezx, &b->pml_row, &b->pml_col}) release(p);
        b->pml_L = 0;
        return 0;
    }
    if (b->lattice) return refuse_bloch(b, "a PML layer (every edge is periodic)");
    if (!row_factors || !col_factors) return bfail(b, FDTD2D_E_ARG, "factor arrays must both be given (or both NULL)");
    if (host_dtype != b->dtype) return bfail(b, FDTD2D_E_ARG, "PML factors must have the batch's dtype");
    if (layer_cells < 1 || 2 * layer_cells + 3 > (b->periodic || b->rows < b->cols ? b->rows : b->cols) || b->cols < 3)
        return bfail(b, FDTD2D_E_ARG, "a %d-cell layer does not fit a %dx%d member", layer_cells, b->rows, b->cols);
    if (b->periodic) {
        const long long k = colf_not_one(b, col_factors);
        if (k >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d: column factor %d is not exactly 1: a periodic batch has its layer on "
                         "rows alone", (int)(k / (4 * b->cols)), (int)(k % (4 * b->cols)));
    }
    if (b->ca) {
        const int mg = sigma_margin(b, layer_cells);
        const long long t = sigma_outside(b, mg);
        if (t >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d: sigma is non-zero within %d cells of an edge (the PML layer, the "
                         "frame and cell [0, 0])", (int)(t / ((long long)b->rows * b->cols)), mg);
    }
    if (b->dcj) {
        const int mg = sigma_margin(b, layer_cells);
        const long long t = wp2_outside(b, mg);
        if (t >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d: wp2 is non-zero within %d cells of an edge (the PML layer, the "
                         "frame and cell [0, 0])", (int)(t / ((long long)b->rows * b->cols)), mg);
    }
    const size_t rbytes = (size_t)b->count * 4 * b->rows * b->esz, cbytes = (size_t)b->count * 4 * b->cols * b->esz;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still read the old factors
    if (!b->ezx) {
        for (void **p : {&b->ezx, &b->pml_row, &b->pml_col}) {
            const size_t bytes = p == &b->ezx ? b->field_bytes : p == &b->pml_row ? rbytes : cbytes;
            if ((rc = alloc(b, p, bytes))) {
                for (void **q : {&b->ezx, &b->pml_row, &b->pml_col}) release(q);
                return rc;
            }
        }
    }
    BCHK(b, hipMemcpy(b->pml_row, row_factors, rbytes, hipMemcpyHostToDevice));
    BCHK(b, hipMemcpy(b->pml_col, col_factors, cbytes, hipMemcpyHostToDevice));
    BCHK(b, hipMemsetAsync(b->ezx, 0, b->field_bytes, b->stream));
    if (b->ezx_im) BCHK(b, hipMemsetAsync(b->ezx_im, 0, b->field_bytes, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    b->pml_L = layer_cells;
    return 0;
}

int fdtd2d_batch_transfer_ezx(fdtd2d_batch_t *b, void *host, int host_dtype, int to_device)
{
    if (!b || !host) return FDTD2D_E_ARG;
    if (b->lattice) return refuse_bloch(b, "fdtd2d_batch_transfer_ezx (there is no Ezx)");
    if (!b->ezx) return bfail(b, FDTD2D_E_STATE, "no PML layer is set: call fdtd2d_batch_set_pml first");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    int rc = use_device(b);
    if (rc) return rc;
    if (!to_device && b->bloch) return copy_out_bloch(b, b->ezx, b->ezx_im, host, host_dtype, 0);
    if (!to_device) return copy_out(b, b->ezx, host, host_dtype, b->rows, b->cols);
    if ((rc = copy_in(b, b->ezx, host, host_dtype, b->rows, b->cols))) return rc;
    return b->periodic ? copy_image(b, b->ezx) : 0;
}

int fdtd2d_batch_courant(const fdtd2d_batch_t *b, double *out)
{
    if (!b || !out) return FDTD2D_E_ARG;
    if (!b->have_mat) return FDTD2D_E_STATE;
    for (int m = 0; m < b->count; ++m) out[m] = b->courant[m];
    return 0;
}

int fdtd2d_batch_upload(fdtd2d_batch_t *b, const void *Ez, const void *Hx, const void *Hy, int host_dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    int rc = use_device(b);
    if (rc) return rc;
    if (Ez && (rc = copy_in(b, b->ez[b->cur], Ez, host_dtype, b->rows, b->cols))) return rc;
    if (Ez && b->periodic && (rc = copy_image(b, b->ez[b->cur]))) return rc;
    if (Ez && b->lattice && (rc = copy_row_image(b, b->ez[b->cur]))) return rc;
    if (Hx && (rc = copy_in(b, b->hx, Hx, host_dtype, b->rows, b->cols - 1))) return rc;
    if (Hy && (rc = copy_in(b, b->hy, Hy, host_dtype, b->rows - 1, b->cols))) return rc;
    return 0;
}

int fdtd2d_batch_download(fdtd2d_batch_t *b, void *Ez, void *Hx, void *Hy, int host_dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    int rc = use_device(b);
    if (rc) return rc;
    if (Ez && b->lattice) {
        if ((rc = copy_out_lattice(b, b->ez[b->cur], b->ez_im, Ez, host_dtype, 0))) return rc;
    } else if (Ez && b->bloch) {
        if ((rc = copy_out_bloch(b, b->ez[b->cur], b->ez_im, Ez, host_dtype, 0))) return rc;
    }
    if (Ez && !b->bloch && (rc = copy_out(b, b->ez[b->cur], Ez, host_dtype, b->rows, b->cols))) return rc;
    if (Hx && (rc = copy_out(b, b->hx, Hx, host_dtype, b->rows, b->cols - 1))) return rc;
    if (Hy && (rc = copy_out(b, b->hy, Hy, host_dtype, b->rows - 1, b->cols))) return rc;
    return 0;
}

int fdtd2d_batch_reset(fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    int rc = use_device(b);
    if (rc) return rc;
    if ((rc = zero_fields(b))) return rc;
    // the monitors restart at step 0 (the whole-grid DFT keeps its accumulators and its step0)
    if (b->win_nf) BCHK(b, hipMemsetAsync(b->win_acc, 0, (size_t)b->count * win_acc_bytes(b), b->stream));
    if (b->nprobe)
        BCHK(b, hipMemsetAsync(b->probe_trace, 0, (size_t)b->count * b->nprobe * b->probe_cap * sizeof(double),
                               b->stream));
    if (b->win_acc_im) BCHK(b, hipMemsetAsync(b->win_acc_im, 0, (size_t)b->count * win_acc_bytes(b), b->stream));
    if (b->probe_trace_im)
        BCHK(b, hipMemsetAsync(b->probe_trace_im, 0, (size_t)b->count * b->nprobe * b->probe_cap * sizeof(double),
                               b->stream));
    if (b->flux_nl)
        BCHK(b, hipMemsetAsync(b->flux_acc, 0, (size_t)b->count * flux_part_bytes(b), b->stream));
    if (b->bflux || b->hzbflux)
        BCHK(b, hipMemsetAsync(b->flux_acc_im, 0, (size_t)b->count * flux_part_bytes(b), b->stream));
    b->win_step0 = 0;
    b->probe_step0 = 0;
    b->flux_step0 = 0;
    return 0;
}

int fdtd2d_batch_set_sources(fdtd2d_batch_t *b, const int *rect)
{
    if (!b || !rect) return FDTD2D_E_ARG;
    bool any = false;
    for (int m = 0; m < b->count; ++m) {
        const int r = rect[4 * m], c = rect[4 * m + 1], nr = rect[4 * m + 2], nc = rect[4 * m + 3];
        if (nr < 0 || nc < 0 || ((nr == 0) != (nc == 0)))
            return bfail(b, FDTD2D_E_ARG, "member %d: source extent %dx%d (0 x 0 means none)", m, nr, nc);
        if (nr == 0) continue;
        if (r < 0 || c < 0 || r + nr > b->rows || c + nc > b->cols)
            return bfail(b, FDTD2D_E_ARG, "member %d: source (%d,%d)+%dx%d outside the %dx%d grid", m, r, c, nr, nc,
                         b->rows, b->cols);
        if (b->periodic && c + nc > b->cols - 1)
            return bfail(b, FDTD2D_E_ARG, "member %d: source (%d,%d)+%dx%d reaches column %d, the image of column 0 of a "
                         "periodic batch", m, r, c, nr, nc, b->cols - 1);
        if (b->lattice && r + nr > b->rows - 1)
            return bfail(b, FDTD2D_E_ARG, "member %d: source (%d,%d)+%dx%d reaches row %d, the image of row 0 of a lattice "
                         "batch", m, r, c, nr, nc, b->rows - 1);
        any = true;
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still read the old rectangles
    BCHK(b, hipMemcpy(b->rect, rect, (size_t)b->count * 4 * sizeof(int), hipMemcpyHostToDevice));
    b->have_src = any;
    b->rect_host.assign(rect, rect + (size_t)b->count * 4);
    return 0;
}

int fdtd2d_batch_run(fdtd2d_batch_t *b, int nsteps, const double *amps)
{
    if (b && b->bloch && b->hz) return fdtd2d_batch_run_hz_bloch(b, nsteps, amps, nullptr);
    if (b && b->bloch) return fdtd2d_batch_run_bloch(b, nsteps, amps, nullptr);
    int rc = need_ready(b);
    if (rc) return rc;
    if (nsteps < 0) return bfail(b, FDTD2D_E_ARG, "nsteps < 0");
    for (int m = 0; m < b->count; ++m)
        if (b->courant[m] > 1.0)
            return bfail(b, FDTD2D_E_COURANT, "Courant stability condition not met for member %d: %.17g > 1.0", m,
                         b->courant[m]);
    if (nsteps == 0) return 0;
    const double *dev_amps = nullptr;
    if (amps && b->have_src) {
        if ((rc = stage(b, &b->amps, &b->amps_cap, amps, (size_t)b->count * nsteps * sizeof(double)))) return rc;
        dev_amps = b->amps;
    }
    return b->dtype == FDTD2D_F32 ? run_impl<float>(b, nsteps, dev_amps, nsteps)
                                  : run_impl<double>(b, nsteps, dev_amps, nsteps);
}

int fdtd2d_batch_run_waveform(fdtd2d_batch_t *b, int nsteps, int src_kind, const double *fc, long long step0)
{
    if (!b) return FDTD2D_E_ARG;
    if (nsteps < 0) return bfail(b, FDTD2D_E_ARG, "nsteps < 0");
    if (src_kind == FDTD2D_SRC_NONE) return fdtd2d_batch_run(b, nsteps, nullptr);
    if (src_kind != FDTD2D_SRC_RICKER && src_kind != FDTD2D_SRC_SINUSOIDAL)
        return bfail(b, FDTD2D_E_ARG, "unknown source kind %d", src_kind);
    if (!fc) return bfail(b, FDTD2D_E_ARG, "fc must not be NULL");
    std::vector<double> amps((size_t)b->count * nsteps);
    for (int m = 0; m < b->count; ++m)
        for (int n = 0; n < nsteps; ++n)
            amps[(size_t)m * nsteps + n] = fdtd2d_source_amplitude(src_kind, (double)(step0 + n) * b->dt, fc[m]);
    return fdtd2d_batch_run(b, nsteps, amps.data());
}

int fdtd2d_batch_set_dft(fdtd2d_batch_t *b, const double *omega, int every)
{
    if (!b) return FDTD2D_E_ARG;
    if (omega && b->bloch) return refuse_bloch(b, "the whole-grid transform (use fdtd2d_batch_set_dft_window)");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    release((void **)&b->dft);
    release((void **)&b->omega);
    b->dft_every = 0;
    if (!omega) return 0;
    if (every < 1) return bfail(b, FDTD2D_E_ARG, "every must be >= 1");
    const size_t bytes = (size_t)b->count * 2 * b->rows * b->cols * sizeof(double);
    if ((rc = alloc(b, (void **)&b->dft, bytes))) return rc;
    if ((rc = alloc(b, (void **)&b->omega, (size_t)b->count * sizeof(double)))) return rc;
    BCHK(b, hipMemsetAsync(b->dft, 0, bytes, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(b->omega, omega, (size_t)b->count * sizeof(double), hipMemcpyHostToDevice));
    b->dft_every = every;
    b->dft_step0 = b->step;
    return 0;
}

int fdtd2d_batch_read_dft(fdtd2d_batch_t *b, double *re, double *im)
{
    if (!b || !re || !im) return FDTD2D_E_ARG;
    if (!b->dft) return bfail(b, FDTD2D_E_STATE, "no transform is set");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t per = (size_t)b->rows * b->cols;
    std::vector<double> acc((size_t)b->count * 2 * per);
    BCHK(b, hipMemcpy(acc.data(), b->dft, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int m = 0; m < b->count; ++m) {
        std::memcpy(re + m * per, acc.data() + 2 * m * per, per * sizeof(double));
        std::memcpy(im + m * per, acc.data() + (2 * m + 1) * per, per * sizeof(double));
    }
    return 0;
}

int fdtd2d_batch_set_dft_window(fdtd2d_batch_t *b, int row0, int col0, int nrows, int ncols, int nfreq,
                                const double *omega, int every)
{
    if (!b) return FDTD2D_E_ARG;
    if (nfreq < 0 || nfreq > FDTD2D_BATCH_MAX_DFT_FREQS)
        return bfail(b, FDTD2D_E_ARG, "nfreq %d outside 0..%d", nfreq, FDTD2D_BATCH_MAX_DFT_FREQS);
    if (nfreq > 0) {
        if (!omega) return bfail(b, FDTD2D_E_ARG, "omega must not be NULL");
        if (every < 1) return bfail(b, FDTD2D_E_ARG, "every must be >= 1");
        if (nrows < 1 || ncols < 1 || row0 < 0 || col0 < 0 || (long long)row0 + nrows > b->rows ||
            (long long)col0 + ncols > b->cols)
            return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d is empty or outside the %dx%d grid", row0, col0, nrows,
                         ncols, b->rows, b->cols);
        if (b->bloch && col0 + ncols > b->cols - 1)
            return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d touches column %d, the image of column 0: not while a "
                         "Bloch phase is set", row0, col0, nrows, ncols, b->cols - 1);
        if (b->lattice && row0 + nrows > b->rows - 1)
            return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d touches row %d, the image of row 0: not in the lattice "
                         "mode", row0, col0, nrows, ncols, b->rows - 1);
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still use the old window
    for (void **p : {(void **)&b->win_acc, (void **)&b->win_omega, (void **)&b->win_ph, (void **)&b->win_held,
                     (void **)&b->win_held_disp})
        release(p);
    b->win_nf = 0;
    if (nfreq == 0) return bloch_window(b);
    const size_t acc = (size_t)b->count * 16 * nfreq * (size_t)nrows * ncols, om = (size_t)b->count * nfreq * sizeof(double);
    if ((rc = alloc(b, (void **)&b->win_acc, acc)) || (rc = alloc(b, (void **)&b->win_omega, om)) ||
        (rc = alloc(b, (void **)&b->win_ph, 2 * om))) {
        for (void **p : {(void **)&b->win_acc, (void **)&b->win_omega, (void **)&b->win_ph}) release(p);
        return rc;
    }
    BCHK(b, hipMemsetAsync(b->win_acc, 0, acc, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(b->win_omega, omega, om, hipMemcpyHostToDevice));
    b->win_r0 = row0; b->win_c0 = col0; b->win_nr = nrows; b->win_nc = ncols;
    b->win_every = every;
    b->win_step0 = b->step;
    b->win_nf = nfreq;
    return bloch_window(b);
}

int fdtd2d_batch_read_dft_window(fdtd2d_batch_t *b, double *re, double *im)
{
    if (!b || !re || !im) return FDTD2D_E_ARG;
    if (!b->win_nf) return bfail(b, FDTD2D_E_STATE, "no window DFT is set");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t per = (size_t)b->win_nf * b->win_nr * b->win_nc;   // one member's re (or im)
    std::vector<double> acc((size_t)b->count * 2 * per);
    BCHK(b, hipMemcpy(acc.data(), b->win_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int m = 0; m < b->count; ++m) {
        std::memcpy(re + m * per, acc.data() + 2 * m * per, per * sizeof(double));
        std::memcpy(im + m * per, acc.data() + (2 * m + 1) * per, per * sizeof(double));
    }
    return 0;
}

int fdtd2d_batch_set_probes(fdtd2d_batch_t *b, int nprobe, const int *cells, long long capacity)
{
    if (!b) return FDTD2D_E_ARG;
    if (nprobe < 0 || nprobe > FDTD2D_BATCH_MAX_PROBES)
        return bfail(b, FDTD2D_E_ARG, "nprobe %d outside 0..%d", nprobe, FDTD2D_BATCH_MAX_PROBES);
    std::vector<int> lin;
    if (nprobe > 0) {
        if (!cells) return bfail(b, FDTD2D_E_ARG, "cells must not be NULL");
        if (capacity < 1) return bfail(b, FDTD2D_E_ARG, "capacity must be >= 1, not %lld", capacity);
        if (capacity > (1LL << 40) / ((long long)b->count * nprobe))
            return bfail(b, FDTD2D_E_ARG, "capacity %lld is too large for %d x %d probes", capacity, b->count, nprobe);
        lin.resize((size_t)b->count * nprobe);
        for (size_t k = 0; k < lin.size(); ++k) {
            const int r = cells[2 * k], c = cells[2 * k + 1];
            if (r < 0 || r >= b->rows || c < 0 || c >= b->cols)
                return bfail(b, FDTD2D_E_ARG, "member %d probe %d: cell (%d,%d) outside the %dx%d grid",
                             (int)(k / nprobe), (int)(k % nprobe), r, c, b->rows, b->cols);
            lin[k] = r * b->cols + c;
        }
        const long long kl = b->lattice ? probe_in_lattice_image(b, lin) : -1;
        if (kl >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d probe %d: cell (%d,%d) lies in row %d or column %d, the images of row 0 "
                         "and column 0: not in the lattice mode", (int)(kl / nprobe), (int)(kl % nprobe),
                         lin[kl] / b->cols, lin[kl] % b->cols, b->rows - 1, b->cols - 1);
        const long long k = b->bloch ? probe_in_image(b, lin) : -1;
        if (k >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d probe %d: column %d is the image of column 0: not while a Bloch "
                         "phase is set", (int)(k / nprobe), (int)(k % nprobe), b->cols - 1);
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still record into the old buffer
    release((void **)&b->probe_cells);
    release((void **)&b->probe_trace);
    b->nprobe = 0;
    b->probe_host.clear();
    if (nprobe == 0) return bloch_probes(b);
    const size_t trace = lin.size() * (size_t)capacity * sizeof(double);
    if ((rc = alloc(b, (void **)&b->probe_cells, lin.size() * sizeof(int))) ||
        (rc = alloc(b, (void **)&b->probe_trace, trace))) {
        release((void **)&b->probe_cells);
        release((void **)&b->probe_trace);
        return rc;
    }
    BCHK(b, hipMemsetAsync(b->probe_trace, 0, trace, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(b->probe_cells, lin.data(), lin.size() * sizeof(int), hipMemcpyHostToDevice));
    b->probe_cap = capacity;
    b->probe_step0 = b->step;
    b->nprobe = nprobe;
    b->probe_host = lin;
    return bloch_probes(b);
}

int fdtd2d_batch_read_probes(fdtd2d_batch_t *b, double *out, long long first, long long count_samples)
{
    if (!b || !out) return FDTD2D_E_ARG;
    if (!b->nprobe) return bfail(b, FDTD2D_E_STATE, "no probes are set");
    if (first < 0 || count_samples < 0 || first + count_samples > b->probe_cap)
        return bfail(b, FDTD2D_E_ARG, "samples [%lld, %lld) outside the capacity %lld", first, first + count_samples,
                     b->probe_cap);
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    if (count_samples == 0) return 0;
    const size_t w = (size_t)count_samples * sizeof(double);
    BCHK(b, hipMemcpy2D(out, w, b->probe_trace + first, (size_t)b->probe_cap * sizeof(double), w,
                        (size_t)b->count * b->nprobe, hipMemcpyDeviceToHost));
    return 0;
}

// ---- fdtd2d_batch_adjoint.h ------------------------------------------------------------------------------------

int fdtd2d_batch_set_point_sources(fdtd2d_batch_t *b, int ncell, const int *cells, int nchan, const double *weights)
{
    if (!b) return FDTD2D_E_ARG;
    if (ncell < 0 || ncell > FDTD2D_BATCH_MAX_POINT_SOURCES)
        return bfail(b, FDTD2D_E_ARG, "ncell %d outside 0..%d", ncell, FDTD2D_BATCH_MAX_POINT_SOURCES);
    if (ncell > 0 && b->bloch) return refuse_bloch(b, "a point source");
    return batch_set_points(b, ncell, cells, nchan, weights);
}

}  // extern "C"

static int batch_set_points(fdtd2d_batch *b, int ncell, const int *cells, int nchan, const double *weights)
{
    if (ncell < 0 || ncell > FDTD2D_BATCH_MAX_POINT_SOURCES)
        return bfail(b, FDTD2D_E_ARG, "ncell %d outside 0..%d", ncell, FDTD2D_BATCH_MAX_POINT_SOURCES);
    std::vector<int> lin, own;
    std::vector<double> w;
    int ntab = ncell;                       // entries per member: a periodic batch lists column-0 cells at their images too
    if (ncell > 0) {
        if (nchan < 1 || nchan > FDTD2D_BATCH_MAX_CHANNELS)
            return bfail(b, FDTD2D_E_ARG, "nchan %d outside 1..%d", nchan, FDTD2D_BATCH_MAX_CHANNELS);
        if (!cells || !weights) return bfail(b, FDTD2D_E_ARG, "cells and weights must not be NULL");
        if (b->fsrc_nchan && nchan != b->fsrc_nchan)
            return bfail(b, FDTD2D_E_STATE, "%d channels, but the line sources that are set take %d: one run drives both",
                         nchan, b->fsrc_nchan);
        for (int m = 0; m < b->count; ++m) {
            int images = 0;
            for (int p = 0; p < ncell; ++p) {
                const int r = cells[2 * ((size_t)m * ncell + p)], c = cells[2 * ((size_t)m * ncell + p) + 1];
                if (r < 0 || r >= b->rows || c < 0 || c >= b->cols)
                    return bfail(b, FDTD2D_E_ARG, "member %d point source %d: cell (%d,%d) outside the %dx%d grid", m, p,
                                 r, c, b->rows, b->cols);
                if (b->periodic && c == b->cols - 1)
                    return bfail(b, FDTD2D_E_ARG, "member %d point source %d: cell (%d,%d) is in column %d, the image of "
                                 "column 0 of a periodic batch", m, p, r, c, b->cols - 1);
                images += b->periodic && c == 0;
            }
            if (ncell + images > FDTD2D_BATCH_MAX_POINT_SOURCES)
                return bfail(b, FDTD2D_E_ARG, "member %d: %d point sources and the %d images of those in column 0 exceed %d",
                             m, ncell, images, FDTD2D_BATCH_MAX_POINT_SOURCES);
            ntab = ncell + images > ntab ? ncell + images : ntab;
        }
        // every table in the order of the resident cell walk's owners: thread l % nthr, slot l / nthr.  Entries past a
        // member's own (fewer images than another member's) are silent: cell -1, no owner thread, zero weights.
        const int nthr = resident_threads(b->rows * b->cols);
        lin.resize((size_t)b->count * ntab);
        own.resize(lin.size());
        w.assign(lin.size() * nchan, 0.0);
        std::vector<int> cell((size_t)ntab), from((size_t)ntab), order((size_t)ntab);
        for (int m = 0; m < b->count; ++m) {
            int n = ncell;
            for (int p = 0; p < ncell; ++p) {
                const int r = cells[2 * ((size_t)m * ncell + p)], c = cells[2 * ((size_t)m * ncell + p) + 1];
                cell[p] = r * b->cols + c;
                from[p] = p;
                for (int q = 0; q < nchan; ++q)
                    if (!std::isfinite(weights[((size_t)m * ncell + p) * nchan + q]))
                        return bfail(b, FDTD2D_E_ARG, "member %d point source %d: weight %d is not finite", m, p, q);
                if (b->periodic && c == 0) {
                    cell[n] = r * b->cols + b->cols - 1;
                    from[n++] = p;
                }
            }
            for (; n < ntab; ++n) cell[n] = from[n] = -1;
            std::iota(order.begin(), order.end(), 0);
            auto key = [&](int p) {
                return cell[p] < 0 ? (1LL << 40) + p : (long long)(cell[p] % nthr) * 16 + cell[p] / nthr;
            };
            std::sort(order.begin(), order.end(), [&](int x, int y) { return key(x) < key(y); });
            for (int k = 0; k < ntab; ++k) {
                const int p = order[k];
                lin[(size_t)m * ntab + k] = cell[p];
                if (cell[p] < 0) {
                    own[(size_t)m * ntab + k] = 4096 * 16;       // past every thread of a workgroup
                    continue;
                }
                if (k && cell[order[k - 1]] == cell[p])
                    return bfail(b, FDTD2D_E_ARG, "member %d: cell (%d,%d) is listed twice", m, cell[p] / b->cols,
                                 cell[p] % b->cols);
                // slots past 15 belong to members that never run resident (16 cells per thread at most)
                own[(size_t)m * ntab + k] = (cell[p] % nthr) * 16 + (cell[p] / nthr < 16 ? cell[p] / nthr : 15);
                for (int q = 0; q < nchan; ++q)
                    w[((size_t)m * nchan + q) * ntab + k] = weights[((size_t)m * ncell + from[p]) * nchan + q];
            }
        }
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still read the old tables
    void **bufs[] = {(void **)&b->pts_cells, (void **)&b->pts_own, (void **)&b->pts_w, (void **)&b->pts_tab};
    for (void **p : bufs) release(p);
    b->npts = b->npts_user = b->pts_nchan = 0;
    if (ncell == 0) return 0;
    if ((rc = alloc(b, (void **)&b->pts_cells, lin.size() * sizeof(int))) ||
        (rc = alloc(b, (void **)&b->pts_own, own.size() * sizeof(int))) ||
        (rc = alloc(b, (void **)&b->pts_w, w.size() * sizeof(double))) ||
        (rc = alloc(b, (void **)&b->pts_tab, lin.size() * sizeof(double)))) {
        for (void **p : bufs) release(p);
        return rc;
    }
    BCHK(b, hipMemcpy(b->pts_cells, lin.data(), lin.size() * sizeof(int), hipMemcpyHostToDevice));
    BCHK(b, hipMemcpy(b->pts_own, own.data(), own.size() * sizeof(int), hipMemcpyHostToDevice));
    BCHK(b, hipMemcpy(b->pts_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    BCHK(b, hipMemset(b->pts_tab, 0, lin.size() * sizeof(double)));
    b->npts = ntab;
    b->npts_user = ncell;
    b->pts_nchan = nchan;
    return 0;
}

extern "C" {

int fdtd2d_batch_run_channels(fdtd2d_batch_t *b, int nsteps, const double *amps, const double *chan,
                              int chan_per_member)
{
    if (!b) return FDTD2D_E_ARG;
    if (nsteps < 0) return bfail(b, FDTD2D_E_ARG, "nsteps < 0");
    if (!chan) return bfail(b, FDTD2D_E_ARG, "chan must not be NULL");
    if (b->bloch) return refuse_bloch(b, "a run with channels");
    if (!b->npts && !b->fsrc_nchan)
        return bfail(b, FDTD2D_E_STATE, "no point sources are set: call fdtd2d_batch_set_point_sources first");
    int rc = need_ready(b);
    if (rc) return rc;
    for (int m = 0; m < b->count; ++m)
        if (b->courant[m] > 1.0)
            return bfail(b, FDTD2D_E_COURANT, "Courant stability condition not met for member %d: %.17g > 1.0", m,
                         b->courant[m]);
    if (nsteps == 0) return 0;
    const double *dev_amps = nullptr;
    if (amps && b->have_src) {
        if ((rc = stage(b, &b->amps, &b->amps_cap, amps, (size_t)b->count * nsteps * sizeof(double)))) return rc;
        dev_amps = b->amps;
    }
    const int nchan = b->npts ? b->pts_nchan : b->fsrc_nchan;     // equal when both are set
    const size_t per = (size_t)nchan * nsteps;
    if ((rc = stage(b, &b->chan, &b->chan_cap, chan, (chan_per_member ? b->count : 1) * per * sizeof(double))))
        return rc;
    fdtd::BatchPts P{};                     // nc = 0 without point sources: silent, like a run without channels
    if (b->npts) {
        P.cells = b->pts_cells;
        P.own = b->pts_own;
        P.w = b->pts_w;
        P.chan = b->chan;
        P.tab = b->pts_tab;
        P.chan_mstride = chan_per_member ? (long long)per : 0;
        P.chan_stride = nsteps;
        P.nc = b->npts;
        P.nchan = b->pts_nchan;
    }
    if (b->fsrc_nchan) {                    // line sources (fdtd2d_batch_flux_adjoint.h): the same channels
        fdtd::BatchFluxSrc S{b->fsrc_we, b->fsrc_wh, b->chan, b->fsrc_geom, chan_per_member ? (long long)per : 0,
                             nsteps, nchan, b->flux_cells};
        return b->dtype == FDTD2D_F32 ? run_impl<float>(b, nsteps, dev_amps, nsteps, &P, &S)
                                      : run_impl<double>(b, nsteps, dev_amps, nsteps, &P, &S);
    }
    return b->dtype == FDTD2D_F32 ? run_impl<float>(b, nsteps, dev_amps, nsteps, &P)
                                  : run_impl<double>(b, nsteps, dev_amps, nsteps, &P);
}

int fdtd2d_batch_hold_dft_window(fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->hz) return refuse_hz(b, "the held window (the adjoint)");
    if (b->bloch) return refuse_bloch(b, "the held window");
    if (b->dcj) return refuse_dispersive(b, "the held window (the adjoint of a dispersive medium)");
    if (!b->win_nf) return bfail(b, FDTD2D_E_STATE, "no window DFT is set");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t bytes = (size_t)b->count * win_acc_bytes(b);
    if (!b->win_held && (rc = alloc(b, (void **)&b->win_held, bytes))) return rc;
    BCHK(b, hipMemcpyAsync(b->win_held, b->win_acc, bytes, hipMemcpyDeviceToDevice, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int fdtd2d_batch_dft_window_product(fdtd2d_batch_t *b, const double *coef_re, const double *coef_im, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!coef_re || !coef_im || !out) return bfail(b, FDTD2D_E_ARG, "coef_re, coef_im and out must not be NULL");
    if (b->hz) return refuse_hz(b, "the window product (the adjoint)");
    if (b->bloch) return refuse_bloch(b, "the window product");
    if (b->dcj) return refuse_dispersive(b, "the window product (the adjoint of a dispersive medium)");
    if (!b->win_nf) return bfail(b, FDTD2D_E_STATE, "no window DFT is set");
    if (!b->win_held) return bfail(b, FDTD2D_E_STATE, "no held window: call fdtd2d_batch_hold_dft_window first");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t W = (size_t)b->win_nr * b->win_nc, nk = (size_t)b->count * b->win_nf;
    std::vector<double> coef(2 * nk);
    for (size_t k = 0; k < nk; ++k) {
        coef[2 * k] = coef_re[k];
        coef[2 * k + 1] = coef_im[k];
    }
    double *dcoef = nullptr, *dout = nullptr;
    if ((rc = alloc(b, (void **)&dcoef, coef.size() * sizeof(double)))) return rc;
    if ((rc = alloc(b, (void **)&dout, (size_t)b->count * W * sizeof(double)))) {
        release((void **)&dcoef);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(dcoef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) {
        fdtd::batch_window_product_launch(b->win_held, b->win_acc, dcoef, dout, b->count, b->win_nf, W, b->stream);
        e = hipGetLastError();
        b->launches++;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)b->count * W * sizeof(double), hipMemcpyDeviceToHost);
    release((void **)&dcoef);
    release((void **)&dout);
    if (e != hipSuccess) return bfail(b, -(1000 + (int)e), "window product failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- fdtd2d_batch_design.h -------------------------------------------------------------------------------------

int fdtd2d_batch_probe_spectra(fdtd2d_batch_t *b, int nfreq, const double *omega, long long first,
                               long long count_samples, double *re, double *im, double *peak)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->bloch) return refuse_bloch(b, "fdtd2d_batch_probe_spectra");
    if (!b->nprobe) return bfail(b, FDTD2D_E_STATE, "no probes are set");
    if (nfreq < 0 || nfreq > FDTD2D_BATCH_MAX_DFT_FREQS)
        return bfail(b, FDTD2D_E_ARG, "nfreq %d outside 0..%d", nfreq, FDTD2D_BATCH_MAX_DFT_FREQS);
    if (nfreq > 0 && (!omega || !re || !im)) return bfail(b, FDTD2D_E_ARG, "omega, re and im must not be NULL");
    if (nfreq == 0 && !peak) return bfail(b, FDTD2D_E_ARG, "nfreq 0 asks for the peak alone: peak must not be NULL");
    for (size_t k = 0; k < (size_t)b->count * nfreq; ++k)
        if (!std::isfinite(omega[k]))
            return bfail(b, FDTD2D_E_ARG, "member %d: frequency %d is not finite", (int)(k / nfreq), (int)(k % nfreq));
    const long long recorded = fdtd2d_batch_info(b, FDTD2D_BATCH_INFO_PROBE_SAMPLES);
    if (first < 0 || count_samples < 0 || first > recorded || count_samples > recorded - first)
        return bfail(b, FDTD2D_E_ARG, "samples [%lld, %lld) outside the %lld recorded so far", first, first + count_samples,
                     recorded);
    int rc = use_device(b);
    if (rc) return rc;
    // scratch: omega (count x nfreq), re, im (count x nprobe x nfreq each), peak (count)
    const size_t nom = (size_t)b->count * nfreq, nsp = nom * b->nprobe;
    if ((rc = scratch(b, (nom + 2 * nsp + b->count) * sizeof(double)))) return rc;
    double *d = (double *)b->dsg;
    if (nom) BCHK(b, hipMemcpyAsync(d, omega, nom * sizeof(double), hipMemcpyHostToDevice, b->stream));
    fdtd::BatchSpectra a;
    a.trace = b->probe_trace;
    a.omega = d;
    a.re = d + nom;
    a.im = d + nom + nsp;
    a.peak = peak ? d + nom + 2 * nsp : nullptr;
    a.B = b->count; a.np = b->nprobe; a.nf = nfreq;
    a.cap = b->probe_cap; a.first = first; a.count = count_samples;
    a.step0 = b->probe_step0;
    a.dt = b->dt;
    fdtd::batch_probe_spectra_launch(a, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    if (nsp) {
        BCHK(b, hipMemcpy(re, a.re, nsp * sizeof(double), hipMemcpyDeviceToHost));
        BCHK(b, hipMemcpy(im, a.im, nsp * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (peak) BCHK(b, hipMemcpy(peak, a.peak, (size_t)b->count * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int fdtd2d_batch_field_absmax(fdtd2d_batch_t *b, int field, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!out) return bfail(b, FDTD2D_E_ARG, "out must not be NULL");
    if (b->bloch) return refuse_bloch(b, "fdtd2d_batch_field_absmax");
    if (field != FDTD2D_FIELD_EZ && field != FDTD2D_FIELD_HX && field != FDTD2D_FIELD_HY)
        return bfail(b, FDTD2D_E_ARG, "field %d: FDTD2D_FIELD_EZ, _HX or _HY", field);
    int rc = use_device(b);
    if (rc) return rc;
    if ((rc = scratch(b, (size_t)b->count * sizeof(double)))) return rc;
    const void *f = field == FDTD2D_FIELD_EZ ? b->ez[b->cur] : field == FDTD2D_FIELD_HX ? b->hx : b->hy;
    fdtd::batch_field_absmax_launch(f, b->dtype == FDTD2D_F64, (double *)b->dsg, b->count,
                                    b->rows - (field == FDTD2D_FIELD_HY), b->cols - (field == FDTD2D_FIELD_HX), b->pitch,
                                    b->mstride, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(out, b->dsg, (size_t)b->count * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int fdtd2d_batch_set_eps_window(fdtd2d_batch_t *b, int row0, int col0, int nrows, int ncols, const void *eps,
                                int host_dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->have_mat || b->uniform)
        return bfail(b, FDTD2D_E_STATE, "no material arrays to patch: call fdtd2d_batch_set_materials first");
    if (!eps) return bfail(b, FDTD2D_E_ARG, "eps must not be NULL");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    if (nrows < 1 || ncols < 1 || row0 < 0 || col0 < 0 || (long long)row0 + nrows > b->rows ||
        (long long)col0 + ncols > b->cols)
        return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d is empty or outside the %dx%d grid", row0, col0, nrows, ncols,
                     b->rows, b->cols);
    if (row0 == 0 && col0 == 0)
        return bfail(b, FDTD2D_E_ARG, "the window holds cell [0, 0], which sets the Mur factor and the PML grading");
    const size_t W = (size_t)nrows * ncols, per = (size_t)b->rows * b->cols;
    std::vector<unsigned char> stage_w((size_t)b->count * W * b->esz);
    std::vector<double> wmin((size_t)b->count, 1e300);
    for (int m = 0; m < b->count; ++m)
        for (size_t t = 0; t < W; ++t) {
            const double e = as_engine(b, get_elem(eps, host_dtype, m * W + t));
            if (!(e > 0) || !std::isfinite(e))
                return bfail(b, FDTD2D_E_ARG, "eps must be positive and finite (member %d, window cell %zu)", m, t);
            if (b->dtype == FDTD2D_F32) ((float *)stage_w.data())[m * W + t] = (float)e;
            else ((double *)stage_w.data())[m * W + t] = e;
            wmin[m] = e < wmin[m] ? e : wmin[m];
        }
    int rc;
    if (b->dcj &&           // the pole's stability with the new permittivity, before anything changes
        (rc = disp_check_stability(
             b, b->disp_omega0, b->mu_min, row0, col0, nrows, ncols,
             [&](int m, int i, int j) {
                 return as_engine(b, get_elem(eps, host_dtype, m * W + (size_t)(i - row0) * ncols + (j - col0)));
             },
             [&](int m, int i, int j) { return b->wp2_host[m * per + (size_t)i * b->cols + j]; })))
        return rc;
    if ((rc = use_device(b))) return rc;
    if ((rc = scratch(b, stage_w.size()))) return rc;      // waits for launches that still read the coefficients
    BCHK(b, hipMemcpyAsync(b->dsg, stage_w.data(), stage_w.size(), hipMemcpyHostToDevice, b->stream));
    fdtd::batch_eps_window_launch(b->ce, b->dsg, b->dtype == FDTD2D_F64, b->count, row0, col0, nrows, ncols, b->pitch,
                                  b->mstride, b->dt, b->dx, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    // the host copy and the Courant number of the full updated member
    const int win[4] = {row0, col0, nrows, ncols};
    if (b->eps_out_min.empty() || std::memcmp(win, b->out_win, sizeof win) != 0) {
        b->eps_out_min.assign((size_t)b->count, 1e300);
        for (int m = 0; m < b->count; ++m)
            for (int i = 0; i < b->rows; ++i) {
                const bool in_rows = i >= row0 && i < row0 + nrows;
                const double *row = b->eps_host.data() + m * per + (size_t)i * b->cols;
                for (int j = 0; j < b->cols; ++j) {
                    if (in_rows && j >= col0 && j < col0 + ncols) continue;
                    b->eps_out_min[m] = row[j] < b->eps_out_min[m] ? row[j] : b->eps_out_min[m];
                }
            }
        std::memcpy(b->out_win, win, sizeof win);
    }
    for (int m = 0; m < b->count; ++m) {
        for (int i = 0; i < nrows; ++i)
            for (int j = 0; j < ncols; ++j)
                b->eps_host[m * per + (size_t)(row0 + i) * b->cols + (col0 + j)] =
                    as_engine(b, get_elem(eps, host_dtype, m * W + (size_t)i * ncols + j));
        const double emin = wmin[m] < b->eps_out_min[m] ? wmin[m] : b->eps_out_min[m];
        b->courant[m] = courant_of(emin, b->mu_min[m], b->dt, b->dx);
    }
    return b->ca ? lossy_reform(b, row0, col0, nrows, ncols) : 0;
}

// ---- fdtd2d_batch_lossy.h --------------------------------------------------------------------------------------

int fdtd2d_batch_set_conductivity(fdtd2d_batch_t *b, const void *sigma, int dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->hz) return refuse_hz(b, "fdtd2d_batch_set_conductivity (there it would be a magnetic loss; the electric one is "
                                   "fdtd2d_batch_set_hz_conductivity)");
    if (!sigma) {                           // remove it: the other kernels again
        if (!b->ca) return 0;
        int rc = use_device(b);
        if (rc) return rc;
        if (b->periodic || b->dcj || b->flux_nl) {   // such a batch keeps its arrays, with ca = 1 and cb = ce
            std::fill(b->sigma_host.begin(), b->sigma_host.end(), 0.0);
            b->sigma_implicit = true;
            return lossy_reform(b, 0, 0, b->rows, b->cols);
        }
        BCHK(b, hipStreamSynchronize(b->stream));
        release(&b->ca);
        release(&b->cb);
        b->sigma_host.clear();
        return 0;
    }
    int rc = set_sigma(b, nullptr, sigma, dtype);
    if (!rc) b->sigma_implicit = false;
    return rc;
}

int fdtd2d_batch_set_conductivity_window(fdtd2d_batch_t *b, const int window[4], const void *sigma, int dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (!window) return bfail(b, FDTD2D_E_ARG, "window must not be NULL");
    if (b->hz) return refuse_hz(b, "fdtd2d_batch_set_conductivity_window");
    int rc = set_sigma(b, window, sigma, dtype);
    if (!rc) b->sigma_implicit = false;
    return rc;
}

// ---- fdtd2d_batch_dispersive.h ---------------------------------------------------------------------------------

int fdtd2d_batch_set_dispersion(fdtd2d_batch_t *b, const void *wp2, int dtype, const double *gamma, const double *omega0)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->hz) return refuse_hz(b, "fdtd2d_batch_set_dispersion (use fdtd2d_batch_set_hz_dispersion)");
    if (!wp2 && !gamma && !omega0) {        // remove the pole: the other kernels again
        if (b->bdisp) return refuse_bloch_pole(b, "fdtd2d_batch_set_dispersion", "fdtd2d_batch_set_bloch_dispersion");
        if (!b->dcj) return 0;
        int rc = use_device(b);
        if (rc) return rc;
        BCHK(b, hipStreamSynchronize(b->stream));
        disp_release(b);
        if (b->sigma_implicit && !b->periodic && !b->flux_nl) {     // the all-zero conductivity the pole brought
            release(&b->ca);
            release(&b->cb);
            b->sigma_host.clear();
            b->sigma_implicit = false;
        }
        return 0;
    }
    if (!wp2 || !gamma || !omega0)
        return bfail(b, FDTD2D_E_ARG, "wp2, gamma and omega0 must all be given (or all NULL)");
    return set_disp(b, nullptr, wp2, dtype, gamma, omega0);
}

int fdtd2d_batch_set_dispersion_window(fdtd2d_batch_t *b, const int window[4], const void *wp2, int dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (!window) return bfail(b, FDTD2D_E_ARG, "window must not be NULL");
    if (b->hz) return refuse_hz(b, "fdtd2d_batch_set_dispersion_window");
    return set_disp(b, window, wp2, dtype, nullptr, nullptr);
}

int fdtd2d_batch_transfer_dispersion(fdtd2d_batch_t *b, void *jh, void *q, int host_dtype, int to_device)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->hz) return refuse_hz(b, "fdtd2d_batch_transfer_dispersion (use fdtd2d_batch_transfer_hz_dispersion)");
    if (b->bdisp)
        return refuse_bloch_pole(b, "fdtd2d_batch_transfer_dispersion", "fdtd2d_batch_transfer_bloch_dispersion");
    if (!b->dcj) return bfail(b, FDTD2D_E_STATE, "no pole is set: call fdtd2d_batch_set_dispersion first");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    int rc = use_device(b);
    if (rc) return rc;
    void *dev[2] = {b->djh, b->dq}, *host[2] = {jh, q};
    for (int k = 0; k < 2; ++k) {
        if (!host[k]) continue;
        if (!to_device) rc = copy_out(b, dev[k], host[k], host_dtype, b->rows, b->cols);
        else if (!(rc = copy_in(b, dev[k], host[k], host_dtype, b->rows, b->cols)) && b->periodic)
            rc = copy_image(b, dev[k]);
        if (rc) return rc;
    }
    return 0;
}

// ---- fdtd2d_batch_hz.h -----------------------------------------------------------------------------------------

int fdtd2d_batch_polarization(const fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    return b->hz ? FDTD2D_POL_HZ : FDTD2D_POL_EZ;
}

int fdtd2d_batch_set_polarization(fdtd2d_batch_t *b, int polarization)
{
    if (!b) return FDTD2D_E_ARG;
    if (polarization != FDTD2D_POL_EZ && polarization != FDTD2D_POL_HZ)
        return bfail(b, FDTD2D_E_ARG, "polarization must be FDTD2D_POL_EZ or FDTD2D_POL_HZ, not %d", polarization);
    const bool hz = polarization == FDTD2D_POL_HZ;
    const char *to = hz ? "the Hz polarisation" : "the Ez polarisation";
    // the refusals, before anything changes
    if (b->boundary != FDTD2D_BOUNDARY_NONE)
        return bfail(b, FDTD2D_E_STATE, "a change of polarisation needs a batch created with FDTD2D_BOUNDARY_NONE: the Mur "
                     "frame has no Hz kernels");
    if (b->lattice && b->hz && hz) return 0;
    if (b->lattice && b->hz)
        return refuse_bloch(b, "a change of polarisation (turn the mode of fdtd2d_batch_set_hz_lattice off first)");
    if (b->lattice) return refuse_bloch(b, "a change of polarisation (the lattice mode has no Hz kernels)");
    if (b->bloch && b->hz && hz) return 0;
    if (b->bloch && b->hz)
        return refuse_bloch(b, "a change of polarisation (turn the phase of fdtd2d_batch_set_hz_bloch off first)");
    if (b->bloch) return refuse_bloch(b, "a change of polarisation (a Bloch phase has no Hz kernels)");
    if (hz == b->hz) return 0;
    if (b->flux_nl || b->fsrc_nchan) return refuse_flux(b, "a change of polarisation");
    if (b->win_held || b->win_held_disp || b->win_held_im)
        return bfail(b, FDTD2D_E_STATE, "%s is not available beside a held window: set the window again first", to);
    if (b->dcj)
        return bfail(b, FDTD2D_E_STATE, "%s is not available while a pole of the other polarisation is set: remove it first",
                     to);
    if (b->ca && !b->sigma_implicit)
        return bfail(b, FDTD2D_E_STATE, "%s is not available while a conductivity of the other polarisation is set: remove "
                     "it first", to);
    int rc = fdtd2d_batch_reset(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    b->hz = hz;
    if (hz && b->have_mat && !b->ca && (rc = periodic_coefficients(b))) {     // ca = 1, cb = ce
        b->hz = false;
        return rc;
    }
    if (!hz && b->sigma_implicit && !b->periodic) {      // the all-zero conductivity the Hz polarisation brought
        release(&b->ca);
        release(&b->cb);
        b->sigma_host.clear();
        b->sigma_implicit = false;
    }
    return 0;
}

int fdtd2d_batch_set_hz_conductivity(fdtd2d_batch_t *b, const void *sigma, int dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->hz)
        return bfail(b, FDTD2D_E_STATE, "fdtd2d_batch_set_hz_conductivity needs the Hz polarisation "
                     "(fdtd2d_batch_set_polarization); the Ez polarisation takes fdtd2d_batch_set_conductivity");
    if (!sigma) {                           // remove it: the batch keeps its arrays, with ca = 1 and cb = ce
        if (!b->ca || b->sigma_implicit) return 0;
        int rc = use_device(b);
        if (rc) return rc;
        std::fill(b->sigma_host.begin(), b->sigma_host.end(), 0.0);
        b->sigma_implicit = true;
        return lossy_reform(b, 0, 0, b->rows, b->cols);
    }
    int rc = set_sigma(b, nullptr, sigma, dtype);
    if (!rc) b->sigma_implicit = false;
    return rc;
}

int fdtd2d_batch_set_hz_dispersion(fdtd2d_batch_t *b, const void *wp2, int dtype, const double *gamma,
                                   const double *omega0)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->hz)
        return bfail(b, FDTD2D_E_STATE, "fdtd2d_batch_set_hz_dispersion needs the Hz polarisation "
                     "(fdtd2d_batch_set_polarization); the Ez polarisation takes fdtd2d_batch_set_dispersion");
    if (!wp2 && !gamma && !omega0) {        // remove the pole: the seven-array kernels again
        if (!b->dcj) return 0;
        int rc = use_device(b);
        if (rc) return rc;
        BCHK(b, hipStreamSynchronize(b->stream));
        disp_release(b);
        return 0;
    }
    if (!wp2 || !gamma || !omega0)
        return bfail(b, FDTD2D_E_ARG, "wp2, gamma and omega0 must all be given (or all NULL)");
    return set_disp(b, nullptr, wp2, dtype, gamma, omega0);
}

int fdtd2d_batch_transfer_hz_dispersion(fdtd2d_batch_t *b, void *jx, void *qx, void *jy, void *qy, int host_dtype,
                                        int to_device)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->hz || !b->dcj)
        return bfail(b, FDTD2D_E_STATE, "no pole of the Hz polarisation is set: call fdtd2d_batch_set_hz_dispersion first");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    int rc = use_device(b);
    if (rc) return rc;
    void *dev[4] = {b->djh, b->dq, b->djy, b->dqy}, *host[4] = {jx, qx, jy, qy};
    for (int k = 0; k < 4; ++k) {
        if (!host[k]) continue;
        rc = to_device ? copy_in(b, dev[k], host[k], host_dtype, b->rows, b->cols)
                       : copy_out(b, dev[k], host[k], host_dtype, b->rows, b->cols);
        if (rc) return rc;
    }
    return 0;
}

// ---- fdtd2d_batch_dispersive_adjoint.h -------------------------------------------------------------------------

namespace {
// what both calls refuse: complex fields, a batch without a pole, a batch without a window
int dispersive_window_state(fdtd2d_batch *b, const char *what, const char *plain)
{
    if (b->bloch) return refuse_bloch(b, what);
    if (!b->dcj)
        return bfail(b, FDTD2D_E_STATE, "%s needs a dispersive pole (fdtd2d_batch_set_dispersion): a batch without one "
                     "takes %s", what, plain);
    if (!b->win_nf) return bfail(b, FDTD2D_E_STATE, "no window DFT is set");
    return 0;
}
}  // namespace

int fdtd2d_batch_hold_dispersive_window(fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->hz) return refuse_hz(b, "the held dispersive window (the adjoint)");
    int rc = dispersive_window_state(b, "the held dispersive window", "fdtd2d_batch_hold_dft_window");
    if (rc) return rc;
    if ((rc = use_device(b))) return rc;
    const size_t bytes = (size_t)b->count * win_acc_bytes(b);
    if (!b->win_held_disp && (rc = alloc(b, (void **)&b->win_held_disp, bytes))) return rc;
    BCHK(b, hipMemcpyAsync(b->win_held_disp, b->win_acc, bytes, hipMemcpyDeviceToDevice, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int fdtd2d_batch_dispersive_window_product(fdtd2d_batch_t *b, int ncoef, const double *coef_re, const double *coef_im,
                                           const double *scale, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!coef_re || !coef_im || !scale || !out)
        return bfail(b, FDTD2D_E_ARG, "coef_re, coef_im, scale and out must not be NULL");
    if (ncoef < 1 || ncoef > FDTD2D_BATCH_MAX_PRODUCT_SETS)
        return bfail(b, FDTD2D_E_ARG, "ncoef %d outside 1..%d", ncoef, (int)FDTD2D_BATCH_MAX_PRODUCT_SETS);
    if (b->hz) return refuse_hz(b, "the dispersive window product (the adjoint)");
    int rc = dispersive_window_state(b, "the dispersive window product", "fdtd2d_batch_dft_window_product");
    if (rc) return rc;
    if (!b->win_held_disp)
        return bfail(b, FDTD2D_E_STATE, "no held dispersive window: call fdtd2d_batch_hold_dispersive_window first");
    if ((rc = use_device(b))) return rc;
    const size_t W = (size_t)b->win_nr * b->win_nc, nk = (size_t)ncoef * b->count * b->win_nf;
    const size_t ns = (size_t)b->count * ncoef, nout = (size_t)ncoef * b->count * W;
    std::vector<double> host(2 * nk + ns);      // the interleaved coefficients, then the scales: one upload
    for (size_t k = 0; k < nk; ++k) {
        host[2 * k] = coef_re[k];
        host[2 * k + 1] = coef_im[k];
    }
    std::copy(scale, scale + ns, host.begin() + 2 * nk);
    // scratch, as fdtd2d_batch_bloch_window_product: coef (ncoef x count x nf x 2), scale (count x ncoef), out
    if ((rc = scratch(b, (host.size() + nout) * sizeof(double)))) return rc;
    double *dcoef = (double *)b->dsg, *dout = dcoef + host.size();
    BCHK(b, hipMemcpyAsync(dcoef, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    fdtd::batch_window_product_multi_launch(b->win_held_disp, b->win_acc, dcoef, dcoef + 2 * nk, dout, b->count,
                                            b->win_nf, W, ncoef, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// ---- fdtd2d_batch_bloch_dispersive.h ---------------------------------------------------------------------------

int fdtd2d_batch_set_bloch_dispersion(fdtd2d_batch_t *b, const void *wp2, int dtype, const double *gamma,
                                      const double *omega0)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bloch)
        return bfail(b, FDTD2D_E_STATE, "fdtd2d_batch_set_bloch_dispersion needs a Bloch phase or the lattice mode: a batch "
                     "with real fields takes fdtd2d_batch_set_dispersion");
    if (b->hz) return refuse_hz(b, "fdtd2d_batch_set_bloch_dispersion (use fdtd2d_batch_set_hz_dispersion)");
    if (!wp2 && !gamma && !omega0) {        // remove the pole: the Bloch or lattice kernels again
        if (!b->bdisp) return 0;
        int rc = use_device(b);
        if (rc) return rc;
        BCHK(b, hipStreamSynchronize(b->stream));
        disp_release(b);
        return 0;
    }
    if (!wp2 || !gamma || !omega0)
        return bfail(b, FDTD2D_E_ARG, "wp2, gamma and omega0 must all be given (or all NULL)");
    if (b->npts)
        return bfail(b, FDTD2D_E_STATE, "a dispersive pole is not available beside Bloch point sources (remove them: the "
                     "adjoint of a dispersive medium is not implemented)");
    if (b->win_held)
        return bfail(b, FDTD2D_E_STATE, "a dispersive pole is not available beside the held window (set the window again: "
                     "the adjoint of a dispersive medium is not implemented)");
    return set_disp(b, nullptr, wp2, dtype, gamma, omega0, true);
}

int fdtd2d_batch_set_bloch_dispersion_window(fdtd2d_batch_t *b, const int window[4], const void *wp2, int dtype)
{
    if (!b) return FDTD2D_E_ARG;
    if (!window) return bfail(b, FDTD2D_E_ARG, "window must not be NULL");
    if (!b->bdisp) return bfail(b, FDTD2D_E_STATE, "no pole is set: call fdtd2d_batch_set_bloch_dispersion first");
    return set_disp(b, window, wp2, dtype, nullptr, nullptr, true);
}

int fdtd2d_batch_transfer_bloch_dispersion(fdtd2d_batch_t *b, void *jh_re, void *jh_im, void *q_re, void *q_im,
                                           int host_dtype, int to_device)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bdisp) return bfail(b, FDTD2D_E_STATE, "no pole is set: call fdtd2d_batch_set_bloch_dispersion first");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    int rc = use_device(b);
    if (rc) return rc;
    void *re[2] = {b->djh, b->dq}, *im[2] = {b->djh_im, b->dq_im}, *host[2][2] = {{jh_re, jh_im}, {q_re, q_im}};
    for (int k = 0; k < 2; ++k)
        for (int part = 0; part < 2; ++part) {
            void *h = host[k][part], *dev = part ? im[k] : re[k];
            if (!h) continue;
            if (to_device) {
                if ((rc = copy_in(b, dev, h, host_dtype, b->rows, b->cols)) || (rc = copy_image(b, dev))) return rc;
                if (b->lattice && (rc = copy_row_image(b, dev))) return rc;
            } else if ((rc = b->lattice ? copy_out_lattice(b, re[k], im[k], h, host_dtype, part)
                                        : copy_out_bloch(b, re[k], im[k], h, host_dtype, part)))
                return rc;
        }
    return 0;
}

// ---- fdtd2d_batch_periodic.h -----------------------------------------------------------------------------------

int fdtd2d_batch_set_periodic(fdtd2d_batch_t *b, int on)
{
    if (!b) return FDTD2D_E_ARG;
    if (b->boundary != FDTD2D_BOUNDARY_NONE)
        return bfail(b, FDTD2D_E_STATE, "periodic columns need a batch created with FDTD2D_BOUNDARY_NONE: the Mur frame "
                     "and a periodic boundary exclude each other");
    if ((on != 0) == b->periodic) return 0;
    if (!on && b->hz && b->lattice)
        return refuse_bloch(b, "turning periodic columns off (turn the mode of fdtd2d_batch_set_hz_lattice off first)");
    if (!on && b->hz && b->bloch)
        return refuse_bloch(b, "turning periodic columns off (turn the phase of fdtd2d_batch_set_hz_bloch off first)");
    if (b->flux_nl) return refuse_flux(b, "switching periodic columns");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    if (!on && b->bdisp)
        return refuse_dispersive(b, "turning periodic columns (and with them the phase or the lattice mode) off");
    if (!on && b->dcj) {                    // the refusals of a dispersive batch, before anything changes
        if (b->pml_L == 0)
            return refuse_dispersive(b, "turning periodic columns off without a layer (a plain box has no dispersive "
                                        "kernels)");
        b->periodic = false;
        const int mg = sigma_margin(b, b->pml_L);
        const long long t = wp2_outside(b, mg);
        b->periodic = true;
        if (t >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d: wp2 is non-zero within %d cells of an edge (the PML layer, the "
                         "frame and cell [0, 0])", (int)(t / ((long long)b->rows * b->cols)), mg);
    }
    if (!on && b->lattice) {
        const long long t = lattice_sigma_outside(b);
        if (t >= 0) return refuse_lattice_off(b, t);
    }
    if (!on) {
        if (b->bloch && (rc = bloch_off(b))) return rc;
        if ((rc = fdtd2d_batch_set_point_sources(b, 0, nullptr, 0, nullptr))) return rc;
        b->periodic = false;
        if (b->sigma_implicit && !b->dcj && !b->hz) {
            release(&b->ca);
            release(&b->cb);
            b->sigma_host.clear();
            b->sigma_implicit = false;
        }
        if (b->pml_L == 0) {
            for (void **p : {&b->ezx, &b->pml_row, &b->pml_col}) release(p);
        }
        return 0;
    }
    // the refusals, before anything changes
    for (int m = 0; m < b->count && !b->rect_host.empty(); ++m) {
        const int *r = b->rect_host.data() + 4 * m;
        if (r[2] > 0 && r[1] + r[3] > b->cols - 1)
            return bfail(b, FDTD2D_E_ARG, "member %d: source (%d,%d)+%dx%d reaches column %d, the image of column 0 of a "
                         "periodic batch", m, r[0], r[1], r[2], r[3], b->cols - 1);
    }
    if (b->ezx) {
        std::vector<unsigned char> colf((size_t)b->count * 4 * b->cols * b->esz);
        BCHK(b, hipMemcpy(colf.data(), b->pml_col, colf.size(), hipMemcpyDeviceToHost));
        const long long k = colf_not_one(b, colf.data());
        if (k >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d: column factor %d of the layer is not exactly 1: a periodic batch has "
                         "its layer on rows alone", (int)(k / (4 * b->cols)), (int)(k % (4 * b->cols)));
    }
    b->periodic = true;
    if (b->ca) {
        const int mg = sigma_margin(b, b->ezx ? b->pml_L : 0);
        const long long t = sigma_outside(b, mg);
        if (t >= 0) {
            b->periodic = false;
            return bfail(b, FDTD2D_E_ARG, "member %d: sigma is non-zero within %d rows of the top or bottom edge",
                         (int)(t / ((long long)b->rows * b->cols)), mg);
        }
    }
    auto undo = [&](int code) {
        b->periodic = false;
        return code;
    };
    if ((rc = fdtd2d_batch_set_point_sources(b, 0, nullptr, 0, nullptr))) return undo(rc);
    if (!b->ezx && (rc = unit_layer(b))) return undo(rc);
    if ((rc = copy_image(b, b->ez[b->cur])) || (rc = copy_image(b, b->ezx))) return undo(rc);
    // (the pole state of the Hz polarisation has no image column)
    if (b->dcj && !b->hz && ((rc = copy_image(b, b->djh)) || (rc = copy_image(b, b->dq)))) return undo(rc);
    if (b->have_mat && !b->ca && (rc = periodic_coefficients(b))) return undo(rc);
    return 0;
}

// ---- fdtd2d_batch_bloch.h ----------------------------------------------------------------------------------------

int fdtd2d_batch_set_bloch(fdtd2d_batch_t *b, const double *cos_phi, const double *sin_phi)
{
    if (!b) return FDTD2D_E_ARG;
    if (!cos_phi != !sin_phi) return bfail(b, FDTD2D_E_ARG, "cos_phi and sin_phi must both be given (or both NULL)");
    int rc = use_device(b);
    if (rc) return rc;
    if (b->lattice && b->hz) return refuse_bloch(b, "fdtd2d_batch_set_bloch or fdtd2d_batch_set_hz_bloch (use fdtd2d_batch_set_hz_lattice)");
    if (b->lattice) return refuse_bloch(b, "fdtd2d_batch_set_bloch (use fdtd2d_batch_set_lattice)");
    if (b->hz && b->bloch && !b->hz_bloch_call) return refuse_hz(b, "fdtd2d_batch_set_bloch (use fdtd2d_batch_set_hz_bloch)");
    if (!cos_phi && b->bflux) return refuse_flux(b, "turning the Bloch phase off");
    if (!cos_phi && b->bdisp) return refuse_dispersive(b, "turning the Bloch phase off");
    if (!cos_phi) return b->bloch ? bloch_off(b) : 0;
    if (b->hz && !b->hz_bloch_call) return refuse_hz(b, "a Bloch phase");
    if (b->dcj && !b->bdisp && !b->hz) return refuse_dispersive(b, "a Bloch phase");
    if (b->flux_nl && !b->bflux && !b->hzbflux) return refuse_flux(b, "a Bloch phase");
    if (!b->periodic)
        return bfail(b, FDTD2D_E_STATE, "a Bloch phase needs periodic columns: call fdtd2d_batch_set_periodic first");
    for (int m = 0; m < b->count; ++m)
        if (!std::isfinite(cos_phi[m]) || !std::isfinite(sin_phi[m]))
            return bfail(b, FDTD2D_E_ARG, "member %d: the rotation (%g, %g) is not finite", m, cos_phi[m], sin_phi[m]);
    if (!b->bloch) {
        if (b->dft) return refuse_bloch(b, "the whole-grid transform (remove it, use fdtd2d_batch_set_dft_window)");
        if (b->npts) return refuse_bloch(b, "a point source (remove them)");
        if (b->win_held) return refuse_bloch(b, "the held window (set the window again)");
        if (b->win_nf && b->win_c0 + b->win_nc > b->cols - 1)
            return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d touches column %d, the image of column 0: not with a Bloch "
                         "phase", b->win_r0, b->win_c0, b->win_nr, b->win_nc, b->cols - 1);
        const long long k = probe_in_image(b, b->probe_host);
        if (k >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d probe %d: column %d is the image of column 0: not with a Bloch "
                         "phase", (int)(k / b->nprobe), (int)(k % b->nprobe), b->cols - 1);
    }
    std::vector<double> rho((size_t)b->count * 2);
    std::vector<unsigned char> rt(rho.size() * b->esz), rtc(rt.size());     // (c, s) and (c, -s): negation is exact
    for (size_t k = 0; k < rho.size(); ++k) {
        rho[k] = as_engine(b, k % 2 ? sin_phi[k / 2] : cos_phi[k / 2]);
        const double conj = k % 2 ? -rho[k] : rho[k];
        if (b->dtype == FDTD2D_F32) {
            ((float *)rt.data())[k] = (float)rho[k];
            ((float *)rtc.data())[k] = (float)conj;
        } else {
            ((double *)rt.data())[k] = rho[k];
            ((double *)rtc.data())[k] = conj;
        }
    }
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still read the old rotations
    if (!b->bloch) {
        const size_t wn = (size_t)b->count * 2 * (b->cols - 1);
        auto undo = [&](int code) {
            bloch_off(b);
            return code;
        };
        for (void **p : {&b->ez_im, &b->hx_im, &b->hy_im, &b->ezx_im}) {
            if ((rc = alloc(b, p, b->field_bytes))) return undo(rc);
            if (hipMemsetAsync(*p, 0, b->field_bytes, b->stream) != hipSuccess)
                return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary fields failed"));
        }
        if (hipStreamSynchronize(b->stream) != hipSuccess)
            return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary fields failed"));
        if ((rc = alloc(b, &b->rho, rt.size())) || (rc = alloc(b, &b->rho_conj, rt.size())) ||
            (rc = alloc(b, (void **)&b->bloch_w, wn * sizeof(double))))
            return undo(rc);
        if (b->hz && b->dcj) {                  // fdtd2d_batch_hz_bloch.h: the imaginary parts of Jx, Qx, Jy, Qy as zero
            for (void **p : {&b->djh_im, &b->dq_im, &b->djy_im, &b->dqy_im}) {
                if ((rc = alloc(b, p, b->field_bytes))) return undo(rc);
                if (hipMemsetAsync(*p, 0, b->field_bytes, b->stream) != hipSuccess)
                    return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary pole state failed"));
            }
            if (hipStreamSynchronize(b->stream) != hipSuccess)
                return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary pole state failed"));
        }
        b->bloch = true;
        if ((rc = fdtd2d_batch_set_bloch_source(b, nullptr, nullptr)) || (rc = bloch_window(b)) || (rc = bloch_probes(b)))
            return undo(rc);
    }
    BCHK(b, hipMemcpy(b->rho, rt.data(), rt.size(), hipMemcpyHostToDevice));
    BCHK(b, hipMemcpy(b->rho_conj, rtc.data(), rtc.size(), hipMemcpyHostToDevice));
    b->rho_host.swap(rho);
    b->run_conj = false;
    return 0;
}

int fdtd2d_batch_set_bloch_source(fdtd2d_batch_t *b, const double *wr, const double *wi)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (!wr != !wi) return bfail(b, FDTD2D_E_ARG, "wr and wi must both be given (or both NULL)");
    const size_t Q = (size_t)b->cols - 1;
    std::vector<double> w((size_t)b->count * 2 * Q);
    for (int m = 0; m < b->count; ++m)
        for (size_t j = 0; j < Q; ++j) {
            const double r = wr ? wr[m * Q + j] : 1.0, i = wi ? wi[m * Q + j] : 0.0;
            if (!std::isfinite(r) || !std::isfinite(i))
                return bfail(b, FDTD2D_E_ARG, "member %d: the source weight of column %zu is not finite", m, j);
            w[(size_t)m * 2 * Q + j] = r;
            w[(size_t)m * 2 * Q + Q + j] = i;
        }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still read the old weights
    BCHK(b, hipMemcpy(b->bloch_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

int fdtd2d_batch_run_bloch(fdtd2d_batch_t *b, int nsteps, const double *amps_re, const double *amps_im)
{
    int rc = need_ready(b);
    if (rc) return rc;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (nsteps < 0) return bfail(b, FDTD2D_E_ARG, "nsteps < 0");
    if (amps_im && !amps_re) return bfail(b, FDTD2D_E_ARG, "amps_im needs amps_re (zeros for a purely imaginary source)");
    for (int m = 0; m < b->count; ++m)
        if (b->courant[m] > 1.0)
            return bfail(b, FDTD2D_E_COURANT, "Courant stability condition not met for member %d: %.17g > 1.0", m,
                         b->courant[m]);
    if (nsteps == 0) return 0;
    const double *dev_amps = nullptr;
    b->run_amps_im = nullptr;
    if (amps_re && b->have_src) {
        const size_t bytes = (size_t)b->count * nsteps * sizeof(double);
        if ((rc = stage(b, &b->amps, &b->amps_cap, amps_re, bytes))) return rc;
        dev_amps = b->amps;
        if (amps_im) {
            if ((rc = stage(b, &b->amps_im, &b->amps_im_cap, amps_im, bytes))) return rc;
            b->run_amps_im = b->amps_im;
        }
    }
    return b->dtype == FDTD2D_F32 ? run_impl<float>(b, nsteps, dev_amps, nsteps)
                                  : run_impl<double>(b, nsteps, dev_amps, nsteps);
}

int fdtd2d_batch_transfer_bloch(fdtd2d_batch_t *b, void *Ez_im, void *Hx_im, void *Hy_im, void *Ezx_im, int host_dtype,
                                int to_device)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    if (b->lattice && Ezx_im) return refuse_bloch(b, "Ezx (pass Ezx_im as NULL)");
    int rc = use_device(b);
    if (rc) return rc;
    if (to_device) {
        if (Ez_im && ((rc = copy_in(b, b->ez_im, Ez_im, host_dtype, b->rows, b->cols)) || (rc = copy_image(b, b->ez_im))))
            return rc;
        if (Ez_im && b->lattice && (rc = copy_row_image(b, b->ez_im))) return rc;
        if (Hx_im && (rc = copy_in(b, b->hx_im, Hx_im, host_dtype, b->rows, b->cols - 1))) return rc;
        if (Hy_im && (rc = copy_in(b, b->hy_im, Hy_im, host_dtype, b->rows - 1, b->cols))) return rc;
        if (Ezx_im && ((rc = copy_in(b, b->ezx_im, Ezx_im, host_dtype, b->rows, b->cols)) ||
                       (rc = copy_image(b, b->ezx_im))))
            return rc;
        return 0;
    }
    if (Ez_im && b->lattice) {
        if ((rc = copy_out_lattice(b, b->ez[b->cur], b->ez_im, Ez_im, host_dtype, 1))) return rc;
    } else if (Ez_im) {
        if ((rc = copy_out_bloch(b, b->ez[b->cur], b->ez_im, Ez_im, host_dtype, 1))) return rc;
    }
    if (Hx_im && (rc = copy_out(b, b->hx_im, Hx_im, host_dtype, b->rows, b->cols - 1))) return rc;
    if (Hy_im && (rc = copy_out(b, b->hy_im, Hy_im, host_dtype, b->rows - 1, b->cols))) return rc;
    if (Ezx_im && (rc = copy_out_bloch(b, b->ezx, b->ezx_im, Ezx_im, host_dtype, 1))) return rc;
    return 0;
}

int fdtd2d_batch_read_dft_window_bloch(fdtd2d_batch_t *b, double *re, double *im)
{
    if (!b || !re || !im) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (!b->win_nf || !b->win_acc_im) return bfail(b, FDTD2D_E_STATE, "no window DFT is set");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t per = (size_t)b->win_nf * b->win_nr * b->win_nc;   // one member's re (or im)
    std::vector<double> acc((size_t)b->count * 2 * per);
    BCHK(b, hipMemcpy(acc.data(), b->win_acc_im, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int m = 0; m < b->count; ++m) {
        std::memcpy(re + m * per, acc.data() + 2 * m * per, per * sizeof(double));
        std::memcpy(im + m * per, acc.data() + (2 * m + 1) * per, per * sizeof(double));
    }
    return 0;
}

int fdtd2d_batch_read_probes_bloch(fdtd2d_batch_t *b, double *out, long long first, long long count_samples)
{
    if (!b || !out) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (!b->nprobe || !b->probe_trace_im) return bfail(b, FDTD2D_E_STATE, "no probes are set");
    if (first < 0 || count_samples < 0 || first + count_samples > b->probe_cap)
        return bfail(b, FDTD2D_E_ARG, "samples [%lld, %lld) outside the capacity %lld", first, first + count_samples,
                     b->probe_cap);
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    if (count_samples == 0) return 0;
    const size_t w = (size_t)count_samples * sizeof(double);
    BCHK(b, hipMemcpy2D(out, w, b->probe_trace_im + first, (size_t)b->probe_cap * sizeof(double), w,
                        (size_t)b->count * b->nprobe, hipMemcpyDeviceToHost));
    return 0;
}

// ---- fdtd2d_batch_hz_bloch.h -------------------------------------------------------------------------------------
// The phase shares the host state of fdtd2d_batch_bloch.h (`bloch` beside `hz`): the entry points below make their own
// refusals and then run the bodies above, which refuse an Hz batch unless `hz_bloch_call` is set.

namespace {
struct HzBlochCall {
    fdtd2d_batch *b;
    explicit HzBlochCall(fdtd2d_batch *bb) : b(bb) { b->hz_bloch_call = true; }
    ~HzBlochCall() { b->hz_bloch_call = false; }
};

int need_hz_bloch(fdtd2d_batch *b, const char *what)
{
    if (!b->hz || !b->bloch)
        return bfail(b, FDTD2D_E_STATE, "%s needs the phase of the Hz polarisation: call fdtd2d_batch_set_hz_bloch first", what);
    return 0;
}
}  // namespace

int fdtd2d_batch_set_hz_bloch(fdtd2d_batch_t *b, const double *cos_phi, const double *sin_phi)
{
    if (!b) return FDTD2D_E_ARG;
    if (!cos_phi != !sin_phi) return bfail(b, FDTD2D_E_ARG, "cos_phi and sin_phi must both be given (or both NULL)");
    if (!b->hz)
        return bfail(b, FDTD2D_E_STATE, "fdtd2d_batch_set_hz_bloch needs the Hz polarisation "
                     "(fdtd2d_batch_set_polarization); the Ez polarisation takes fdtd2d_batch_set_bloch");
    if (!cos_phi && !b->bloch) return 0;
    if (cos_phi && b->hzflux) return refuse_flux(b, "a Bloch phase");
    if (!cos_phi && b->hzbflux) return refuse_flux(b, "turning the Bloch phase off");
    HzBlochCall call(b);
    return fdtd2d_batch_set_bloch(b, cos_phi, sin_phi);
}

int fdtd2d_batch_set_hz_bloch_source(fdtd2d_batch_t *b, const double *wr, const double *wi)
{
    if (!b) return FDTD2D_E_ARG;
    int rc = need_hz_bloch(b, "fdtd2d_batch_set_hz_bloch_source");
    if (rc) return rc;
    HzBlochCall call(b);
    return fdtd2d_batch_set_bloch_source(b, wr, wi);
}

int fdtd2d_batch_run_hz_bloch(fdtd2d_batch_t *b, int nsteps, const double *amps_re, const double *amps_im)
{
    if (!b) return FDTD2D_E_ARG;
    int rc = need_hz_bloch(b, "fdtd2d_batch_run_hz_bloch");
    if (rc) return rc;
    HzBlochCall call(b);
    return fdtd2d_batch_run_bloch(b, nsteps, amps_re, amps_im);
}

int fdtd2d_batch_transfer_hz_bloch(fdtd2d_batch_t *b, void *Hz_im, void *Ex_im, void *Ey_im, void *Hzx_im,
                                   int host_dtype, int to_device)
{
    if (!b) return FDTD2D_E_ARG;
    int rc = need_hz_bloch(b, "fdtd2d_batch_transfer_hz_bloch");
    if (rc) return rc;
    HzBlochCall call(b);
    return fdtd2d_batch_transfer_bloch(b, Hz_im, Ex_im, Ey_im, Hzx_im, host_dtype, to_device);
}

int fdtd2d_batch_transfer_hz_bloch_dispersion(fdtd2d_batch_t *b, void *jx_im, void *qx_im, void *jy_im, void *qy_im,
                                              int host_dtype, int to_device)
{
    if (!b) return FDTD2D_E_ARG;
    int rc = need_hz_bloch(b, "fdtd2d_batch_transfer_hz_bloch_dispersion");
    if (rc) return rc;
    if (!b->dcj || !b->djh_im || !b->dq_im || !b->djy_im || !b->dqy_im)
        return bfail(b, FDTD2D_E_STATE, "no pole of the Hz polarisation is set: call fdtd2d_batch_set_hz_dispersion first");
    if (host_dtype != FDTD2D_F32 && host_dtype != FDTD2D_F64) return bfail(b, FDTD2D_E_ARG, "bad host_dtype");
    if ((rc = use_device(b))) return rc;
    void *dev[4] = {b->djh_im, b->dq_im, b->djy_im, b->dqy_im}, *host[4] = {jx_im, qx_im, jy_im, qy_im};
    for (int k = 0; k < 4; ++k) {
        if (!host[k]) continue;
        rc = to_device ? copy_in(b, dev[k], host[k], host_dtype, b->rows, b->cols)
                       : copy_out(b, dev[k], host[k], host_dtype, b->rows, b->cols);
        if (rc) return rc;
    }
    return 0;
}

int fdtd2d_batch_read_dft_window_hz_bloch(fdtd2d_batch_t *b, double *re, double *im)
{
    if (!b || !re || !im) return FDTD2D_E_ARG;
    int rc = need_hz_bloch(b, "fdtd2d_batch_read_dft_window_hz_bloch");
    if (rc) return rc;
    HzBlochCall call(b);
    return fdtd2d_batch_read_dft_window_bloch(b, re, im);
}

int fdtd2d_batch_read_probes_hz_bloch(fdtd2d_batch_t *b, double *out, long long first, long long count_samples)
{
    if (!b || !out) return FDTD2D_E_ARG;
    int rc = need_hz_bloch(b, "fdtd2d_batch_read_probes_hz_bloch");
    if (rc) return rc;
    HzBlochCall call(b);
    return fdtd2d_batch_read_probes_bloch(b, out, first, count_samples);
}

// ---- fdtd2d_batch_lattice.h --------------------------------------------------------------------------------------

int fdtd2d_batch_set_lattice(fdtd2d_batch_t *b, const double *cos_r, const double *sin_r, const double *cos_c,
                             const double *sin_c)
{
    if (!b) return FDTD2D_E_ARG;
    const int given = !!cos_r + !!sin_r + !!cos_c + !!sin_c;
    if (given != 0 && given != 4)
        return bfail(b, FDTD2D_E_ARG, "cos_r, sin_r, cos_c and sin_c must all be given (or all NULL)");
    if (b->hz && (given || b->lattice)) return refuse_hz(b, "the lattice mode of the Ez polarisation (use fdtd2d_batch_set_hz_lattice)");
    int rc = use_device(b);
    if (rc) return rc;
    if (!given) {
        if (!b->lattice) return 0;
        if (b->bdisp) return refuse_dispersive(b, "turning the lattice mode off");
        const long long t = lattice_sigma_outside(b);
        if (t >= 0) return refuse_lattice_off(b, t);
        return bloch_off(b);
    }
    if (b->bloch && !b->lattice) return refuse_bloch(b, "the lattice mode (turn the phase of fdtd2d_batch_set_bloch off)");
    if (b->dcj && !b->bdisp) return refuse_dispersive(b, "the lattice mode");
    if (b->flux_nl) return refuse_flux(b, "the lattice mode");
    if (!b->periodic)
        return bfail(b, FDTD2D_E_STATE, "the lattice mode needs periodic columns: call fdtd2d_batch_set_periodic first");
    if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    const int R = b->rows, C = b->cols;
    if (!b->lattice) {
        if (b->pml_L > 0)
            return bfail(b, FDTD2D_E_STATE, "the lattice mode has no layer: remove it (fdtd2d_batch_set_pml with NULL) first");
        if (b->dft)
            return bfail(b, FDTD2D_E_STATE, "the whole-grid transform is not available in the lattice mode (remove it, use "
                         "fdtd2d_batch_set_dft_window)");
        if (b->npts) return bfail(b, FDTD2D_E_STATE, "a point source is not available in the lattice mode (remove them)");
        if (b->win_held)
            return bfail(b, FDTD2D_E_STATE, "the held window is not available in the lattice mode (set the window again)");
    }
    for (int m = 0; m < b->count; ++m)
        if (!std::isfinite(cos_r[m]) || !std::isfinite(sin_r[m]) || !std::isfinite(cos_c[m]) || !std::isfinite(sin_c[m]))
            return bfail(b, FDTD2D_E_ARG, "member %d: the rotations (%g, %g), (%g, %g) are not finite", m, cos_r[m], sin_r[m],
                         cos_c[m], sin_c[m]);
    if (!b->lattice) {
        if (b->win_nf && (b->win_c0 + b->win_nc > C - 1 || b->win_r0 + b->win_nr > R - 1))
            return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d touches row %d or column %d, the images of row 0 and column "
                         "0: not in the lattice mode", b->win_r0, b->win_c0, b->win_nr, b->win_nc, R - 1, C - 1);
        const long long k = probe_in_lattice_image(b, b->probe_host);
        if (k >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d probe %d: cell (%d,%d) lies in row %d or column %d, the images of row 0 "
                         "and column 0: not in the lattice mode", (int)(k / b->nprobe), (int)(k % b->nprobe),
                         b->probe_host[k] / C, b->probe_host[k] % C, R - 1, C - 1);
        for (int m = 0; m < b->count && !b->rect_host.empty(); ++m) {
            const int *r = b->rect_host.data() + 4 * m;
            if (r[2] > 0 && r[0] + r[2] > R - 1)
                return bfail(b, FDTD2D_E_ARG, "member %d: source (%d,%d)+%dx%d reaches row %d, the image of row 0 of a "
                             "lattice batch", m, r[0], r[1], r[2], r[3], R - 1);
        }
    }
    // (c, s) of the row seam and of the column seam, as the engine stores them
    std::vector<double> rr((size_t)b->count * 2), rc2(rr.size());
    std::vector<unsigned char> rrt(rr.size() * b->esz), rct(rrt.size());
    for (size_t k = 0; k < rr.size(); ++k) {
        rr[k] = as_engine(b, k % 2 ? sin_r[k / 2] : cos_r[k / 2]);
        rc2[k] = as_engine(b, k % 2 ? sin_c[k / 2] : cos_c[k / 2]);
        if (b->dtype == FDTD2D_F32) {
            ((float *)rrt.data())[k] = (float)rr[k];
            ((float *)rct.data())[k] = (float)rc2[k];
        } else {
            ((double *)rrt.data())[k] = rr[k];
            ((double *)rct.data())[k] = rc2[k];
        }
    }
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still read the old rotations
    if (!b->lattice) {
        const size_t wn = (size_t)b->count * 2 * (C - 1);
        auto undo = [&](int code) {
            bloch_off(b);
            return code;
        };
        for (void **p : {&b->ez_im, &b->hx_im, &b->hy_im}) {
            if ((rc = alloc(b, p, b->field_bytes))) return undo(rc);
            if (hipMemsetAsync(*p, 0, b->field_bytes, b->stream) != hipSuccess)
                return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary fields failed"));
        }
        if (hipStreamSynchronize(b->stream) != hipSuccess)
            return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary fields failed"));
        if ((rc = alloc(b, &b->rho, rct.size())) || (rc = alloc(b, &b->rho_r, rrt.size())) ||
            (rc = alloc(b, (void **)&b->bloch_w, wn * sizeof(double))))
            return undo(rc);
        b->bloch = b->lattice = true;
        if ((rc = fdtd2d_batch_set_bloch_source(b, nullptr, nullptr)) || (rc = bloch_window(b)) || (rc = bloch_probes(b)) ||
            (rc = copy_image(b, b->ez[b->cur])) || (rc = copy_row_image(b, b->ez[b->cur])))
            return undo(rc);
    }
    BCHK(b, hipMemcpy(b->rho, rct.data(), rct.size(), hipMemcpyHostToDevice));
    BCHK(b, hipMemcpy(b->rho_r, rrt.data(), rrt.size(), hipMemcpyHostToDevice));
    b->rho_host.swap(rc2);
    b->rho_r_host.swap(rr);
    b->run_conj = false;
    return 0;
}

int fdtd2d_batch_is_lattice(const fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    return b->lattice && !b->hz ? 1 : 0;
}

// ---- fdtd2d_batch_hz_lattice.h -----------------------------------------------------------------------------------
// The mode shares the host state of the Hz Bloch phase and of the lattice mode (`hz`, `bloch` and `lattice` together):
// rho / rho_host hold the column rotation, rho_r / rho_r_host the row rotation, and the complex traffic goes through the
// entry points of fdtd2d_batch_hz_bloch.h, whose bodies deliver both image kinds while `lattice` is set.

int fdtd2d_batch_set_hz_lattice(fdtd2d_batch_t *b, const double *cos_r, const double *sin_r, const double *cos_c,
                                const double *sin_c)
{
    if (!b) return FDTD2D_E_ARG;
    const int given = !!cos_r + !!sin_r + !!cos_c + !!sin_c;
    if (given != 0 && given != 4)
        return bfail(b, FDTD2D_E_ARG, "cos_r, sin_r, cos_c and sin_c must all be given (or all NULL)");
    if (!b->hz)
        return bfail(b, FDTD2D_E_STATE, "fdtd2d_batch_set_hz_lattice needs the Hz polarisation "
                     "(fdtd2d_batch_set_polarization); the Ez polarisation takes fdtd2d_batch_set_lattice");
    int rc = use_device(b);
    if (rc) return rc;
    const bool on = b->lattice;
    const int R = b->rows, C = b->cols;
    if (!given) {
        if (!on) return 0;
        // a plain periodic Hz batch again: sigma and wp2 must lie where that batch allows them
        b->lattice = false;
        const int mg = sigma_margin(b, 0);
        const long long ts = b->ca ? sigma_outside(b, mg) : -1, tw = b->dcj ? wp2_outside(b, mg) : -1;
        b->lattice = true;
        if (ts >= 0 || tw >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d: %s is non-zero within %d rows of the top or bottom edge, where a periodic "
                         "Hz batch without the lattice mode allows none: remove it first",
                         (int)((ts >= 0 ? ts : tw) / ((long long)R * C)), ts >= 0 ? "sigma" : "wp2", mg);
        return bloch_off(b);
    }
    if (!b->periodic)
        return bfail(b, FDTD2D_E_STATE, "the lattice mode needs periodic columns: call fdtd2d_batch_set_periodic first");
    if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    if (!on) {
        if (b->pml_L > 0)
            return bfail(b, FDTD2D_E_STATE, "the lattice mode has no layer: remove it (fdtd2d_batch_set_pml with NULL) first");
        if (b->bloch)
            return refuse_bloch(b, "the lattice mode of the Hz polarisation (turn the phase of fdtd2d_batch_set_hz_bloch off)");
        if (b->flux_nl) return refuse_flux(b, "the lattice mode of the Hz polarisation");
        if (b->dft)
            return bfail(b, FDTD2D_E_STATE, "the whole-grid transform is not available in the lattice mode (remove it, use "
                         "fdtd2d_batch_set_dft_window)");
        if (b->npts) return bfail(b, FDTD2D_E_STATE, "a point source is not available in the lattice mode (remove them)");
        if (b->win_held)
            return bfail(b, FDTD2D_E_STATE, "the held window is not available in the lattice mode (set the window again)");
    }
    for (int m = 0; m < b->count; ++m)
        if (!std::isfinite(cos_r[m]) || !std::isfinite(sin_r[m]) || !std::isfinite(cos_c[m]) || !std::isfinite(sin_c[m]))
            return bfail(b, FDTD2D_E_ARG, "member %d: the rotations (%g, %g), (%g, %g) are not finite", m, cos_r[m], sin_r[m],
                         cos_c[m], sin_c[m]);
    if (!on) {
        if (b->win_nf && (b->win_c0 + b->win_nc > C - 1 || b->win_r0 + b->win_nr > R - 1))
            return bfail(b, FDTD2D_E_ARG, "window (%d,%d)+%dx%d touches row %d or column %d, the images of row 0 and column "
                         "0: not in the lattice mode", b->win_r0, b->win_c0, b->win_nr, b->win_nc, R - 1, C - 1);
        const long long k = probe_in_lattice_image(b, b->probe_host);
        if (k >= 0)
            return bfail(b, FDTD2D_E_ARG, "member %d probe %d: cell (%d,%d) lies in row %d or column %d, the images of row 0 "
                         "and column 0: not in the lattice mode", (int)(k / b->nprobe), (int)(k % b->nprobe),
                         b->probe_host[k] / C, b->probe_host[k] % C, R - 1, C - 1);
        for (int m = 0; m < b->count && !b->rect_host.empty(); ++m) {
            const int *r = b->rect_host.data() + 4 * m;
            if (r[2] > 0 && r[0] + r[2] > R - 1)
                return bfail(b, FDTD2D_E_ARG, "member %d: source (%d,%d)+%dx%d reaches row %d, the image of row 0 of a "
                             "lattice batch", m, r[0], r[1], r[2], r[3], R - 1);
        }
    }
    // (c, s) of the row seam and of the column seam, as the engine stores them
    std::vector<double> rr((size_t)b->count * 2), rc2(rr.size());
    std::vector<unsigned char> rrt(rr.size() * b->esz), rct(rrt.size());
    for (size_t k = 0; k < rr.size(); ++k) {
        rr[k] = as_engine(b, k % 2 ? sin_r[k / 2] : cos_r[k / 2]);
        rc2[k] = as_engine(b, k % 2 ? sin_c[k / 2] : cos_c[k / 2]);
        if (b->dtype == FDTD2D_F32) {
            ((float *)rrt.data())[k] = (float)rr[k];
            ((float *)rct.data())[k] = (float)rc2[k];
        } else {
            ((double *)rrt.data())[k] = rr[k];
            ((double *)rct.data())[k] = rc2[k];
        }
    }
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still read the old rotations
    if (!on) {
        const size_t wn = (size_t)b->count * 2 * (C - 1);
        auto undo = [&](int code) {
            bloch_off(b);
            return code;
        };
        for (void **p : {&b->ez_im, &b->hx_im, &b->hy_im, &b->djh_im, &b->dq_im, &b->djy_im, &b->dqy_im}) {
            if (!b->dcj && p != &b->ez_im && p != &b->hx_im && p != &b->hy_im) continue;   // the pole's imaginary state
            if ((rc = alloc(b, p, b->field_bytes))) return undo(rc);
            if (hipMemsetAsync(*p, 0, b->field_bytes, b->stream) != hipSuccess)
                return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary fields failed"));
        }
        if (hipStreamSynchronize(b->stream) != hipSuccess)
            return undo(bfail(b, FDTD2D_E_NOMEM, "hipMemset of the imaginary fields failed"));
        if ((rc = alloc(b, &b->rho, rct.size())) || (rc = alloc(b, &b->rho_r, rrt.size())) ||
            (rc = alloc(b, (void **)&b->bloch_w, wn * sizeof(double))))
            return undo(rc);
        b->bloch = b->lattice = true;
        HzBlochCall call(b);
        if ((rc = fdtd2d_batch_set_bloch_source(b, nullptr, nullptr)) || (rc = bloch_window(b)) || (rc = bloch_probes(b)) ||
            (rc = copy_image(b, b->ez[b->cur])) || (rc = copy_row_image(b, b->ez[b->cur])))
            return undo(rc);
    }
    BCHK(b, hipMemcpy(b->rho, rct.data(), rct.size(), hipMemcpyHostToDevice));
    BCHK(b, hipMemcpy(b->rho_r, rrt.data(), rrt.size(), hipMemcpyHostToDevice));
    b->rho_host.swap(rc2);
    b->rho_r_host.swap(rr);
    b->run_conj = false;
    return 0;
}

int fdtd2d_batch_is_hz_lattice(const fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    return b->lattice && b->hz ? 1 : 0;
}

// ---- fdtd2d_batch_bloch_adjoint.h ----------------------------------------------------------------------------------

int fdtd2d_batch_set_bloch_point_sources(fdtd2d_batch_t *b, int ncell, const int *cells, int nchan,
                                         const double *weights)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (ncell > 0 && b->lattice) return refuse_bloch(b, "a point source");
    if (ncell > 0 && b->bflux) return refuse_flux(b, "a Bloch point source");
    if (ncell > 0 && b->bdisp) return refuse_dispersive(b, "a point source (the adjoint of a dispersive medium)");
    return batch_set_points(b, ncell, cells, nchan, weights);     // a periodic batch: column C-1 is refused there
}

int fdtd2d_batch_run_bloch_channels(fdtd2d_batch_t *b, int nsteps, const double *amps_re, const double *amps_im,
                                    const double *chan, int chan_per_member, int conjugate)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (b->lattice) return refuse_bloch(b, "a run with channels");
    const bool lsrc = b->bflux && b->fsrc_nchan;   // line sources on the Bloch lines: they take the channels
    if (b->bflux && !lsrc) return refuse_flux(b, "a run with channels");
    if (b->bdisp && !lsrc) return refuse_dispersive(b, "a run with channels (the adjoint of a dispersive medium)");
    if (nsteps < 0) return bfail(b, FDTD2D_E_ARG, "nsteps < 0");
    if (!chan) return bfail(b, FDTD2D_E_ARG, "chan must not be NULL");
    if (amps_im && !amps_re) return bfail(b, FDTD2D_E_ARG, "amps_im needs amps_re (zeros for a purely imaginary source)");
    if (!b->npts && !lsrc)
        return bfail(b, FDTD2D_E_STATE, "no point sources are set: call fdtd2d_batch_set_bloch_point_sources first");
    int rc = need_ready(b);
    if (rc) return rc;
    for (int m = 0; m < b->count; ++m)
        if (b->courant[m] > 1.0)
            return bfail(b, FDTD2D_E_COURANT, "Courant stability condition not met for member %d: %.17g > 1.0", m,
                         b->courant[m]);
    if (nsteps == 0) return 0;
    const double *dev_amps = nullptr;
    b->run_amps_im = nullptr;
    if (amps_re && b->have_src) {
        const size_t bytes = (size_t)b->count * nsteps * sizeof(double);
        if ((rc = stage(b, &b->amps, &b->amps_cap, amps_re, bytes))) return rc;
        dev_amps = b->amps;
        if (amps_im) {
            if ((rc = stage(b, &b->amps_im, &b->amps_im_cap, amps_im, bytes))) return rc;
            b->run_amps_im = b->amps_im;
        }
    }
    const size_t per = (size_t)(lsrc ? b->fsrc_nchan : b->pts_nchan) * nsteps;
    if ((rc = stage(b, &b->chan, &b->chan_cap, chan, (chan_per_member ? b->count : 1) * per * sizeof(double))))
        return rc;
    if (lsrc) {                             // fdtd2d_batch_bloch_flux_adjoint.h: Bloch lines exclude point sources
        fdtd::BatchBlochFluxSrc S{b->fsrc_we, b->fsrc_we_im, b->fsrc_wh, b->fsrc_wh_im, b->chan, b->fsrc_geom,
                                  chan_per_member ? (long long)per : 0, nsteps, b->fsrc_nchan, b->flux_cells};
        return b->dtype == FDTD2D_F32 ? run_bloch_flux<float>(b, nsteps, dev_amps, nsteps, &S, conjugate != 0)
                                      : run_bloch_flux<double>(b, nsteps, dev_amps, nsteps, &S, conjugate != 0);
    }
    fdtd::BatchPts P;
    P.cells = b->pts_cells;
    P.own = b->pts_own;
    P.w = b->pts_w;
    P.chan = b->chan;
    P.tab = b->pts_tab;
    P.chan_mstride = chan_per_member ? (long long)per : 0;
    P.chan_stride = nsteps;
    P.nc = b->npts;
    P.nchan = b->pts_nchan;
    return b->dtype == FDTD2D_F32 ? run_bloch<float>(b, nsteps, dev_amps, nsteps, &P, conjugate != 0)
                                  : run_bloch<double>(b, nsteps, dev_amps, nsteps, &P, conjugate != 0);
}

int fdtd2d_batch_hold_bloch_window(fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (b->lattice) return refuse_bloch(b, "the held window");
    if (b->bflux && !b->fsrc_nchan) return refuse_flux(b, "the held window");   // accepted once line sources are set
    if (b->bdisp) return refuse_dispersive(b, "the held window (the adjoint of a dispersive medium)");
    if (!b->win_nf || !b->win_acc_im) return bfail(b, FDTD2D_E_STATE, "no window DFT is set");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t bytes = (size_t)b->count * win_acc_bytes(b);
    if (!b->win_held && (rc = alloc(b, (void **)&b->win_held, bytes))) return rc;
    if (!b->win_held_im && (rc = alloc(b, (void **)&b->win_held_im, bytes))) return rc;
    BCHK(b, hipMemcpyAsync(b->win_held, b->win_acc, bytes, hipMemcpyDeviceToDevice, b->stream));
    BCHK(b, hipMemcpyAsync(b->win_held_im, b->win_acc_im, bytes, hipMemcpyDeviceToDevice, b->stream));
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int fdtd2d_batch_bloch_window_product(fdtd2d_batch_t *b, const double *coef_re, const double *coef_im, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!coef_re || !coef_im || !out) return bfail(b, FDTD2D_E_ARG, "coef_re, coef_im and out must not be NULL");
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (b->lattice) return refuse_bloch(b, "the window product");
    if (b->bdisp) return refuse_dispersive(b, "the window product (the adjoint of a dispersive medium)");
    if (!b->win_nf || !b->win_acc_im) return bfail(b, FDTD2D_E_STATE, "no window DFT is set");
    if (!b->win_held || !b->win_held_im)
        return bfail(b, FDTD2D_E_STATE, "no held window: call fdtd2d_batch_hold_bloch_window first");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t W = (size_t)b->win_nr * b->win_nc, nk = (size_t)b->count * b->win_nf;
    std::vector<double> coef(2 * nk);
    for (size_t k = 0; k < nk; ++k) {
        coef[2 * k] = coef_re[k];
        coef[2 * k + 1] = coef_im[k];
    }
    // scratch: coef (count x nf x 2), out (count x W)
    if ((rc = scratch(b, (coef.size() + (size_t)b->count * W) * sizeof(double)))) return rc;
    double *dcoef = (double *)b->dsg, *dout = dcoef + coef.size();
    BCHK(b, hipMemcpyAsync(dcoef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    fdtd::batch_bloch_window_product_launch(b->win_held, b->win_held_im, b->win_acc, b->win_acc_im, dcoef, dout, b->count,
                                            b->win_nf, W, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(out, dout, (size_t)b->count * W * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int fdtd2d_batch_bloch_probe_spectra(fdtd2d_batch_t *b, int nfreq, const double *omega, long long first,
                                     long long count_samples, double *re, double *im, double *peak)
{
    if (!b) return FDTD2D_E_ARG;
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (!b->nprobe || !b->probe_trace_im) return bfail(b, FDTD2D_E_STATE, "no probes are set");
    if (nfreq < 0 || nfreq > FDTD2D_BATCH_MAX_DFT_FREQS)
        return bfail(b, FDTD2D_E_ARG, "nfreq %d outside 0..%d", nfreq, FDTD2D_BATCH_MAX_DFT_FREQS);
    if (nfreq > 0 && (!omega || !re || !im)) return bfail(b, FDTD2D_E_ARG, "omega, re and im must not be NULL");
    if (nfreq == 0 && !peak) return bfail(b, FDTD2D_E_ARG, "nfreq 0 asks for the peak alone: peak must not be NULL");
    for (size_t k = 0; k < (size_t)b->count * nfreq; ++k)
        if (!std::isfinite(omega[k]))
            return bfail(b, FDTD2D_E_ARG, "member %d: frequency %d is not finite", (int)(k / nfreq), (int)(k % nfreq));
    const long long recorded = fdtd2d_batch_info(b, FDTD2D_BATCH_INFO_PROBE_SAMPLES);
    if (first < 0 || count_samples < 0 || first > recorded || count_samples > recorded - first)
        return bfail(b, FDTD2D_E_ARG, "samples [%lld, %lld) outside the %lld recorded so far", first, first + count_samples,
                     recorded);
    int rc = use_device(b);
    if (rc) return rc;
    // scratch: omega (count x nfreq), then per part re, im (count x nprobe x nfreq each) and peak (count)
    const size_t nom = (size_t)b->count * nfreq, nsp = nom * b->nprobe, part = 2 * nsp + b->count;
    if ((rc = scratch(b, (nom + 2 * part) * sizeof(double)))) return rc;
    double *d = (double *)b->dsg;
    if (nom) BCHK(b, hipMemcpyAsync(d, omega, nom * sizeof(double), hipMemcpyHostToDevice, b->stream));
    for (int q = 0; q < 2; ++q) {
        fdtd::BatchSpectra a;
        a.trace = q ? b->probe_trace_im : b->probe_trace;
        a.omega = d;
        a.re = d + nom + q * part;
        a.im = a.re + nsp;
        a.peak = peak ? a.im + nsp : nullptr;
        a.B = b->count; a.np = b->nprobe; a.nf = nfreq;
        a.cap = b->probe_cap; a.first = first; a.count = count_samples;
        a.step0 = b->probe_step0;
        a.dt = b->dt;
        fdtd::batch_probe_spectra_launch(a, b->stream);
        BCHK(b, hipGetLastError());
        b->launches++;
    }
    BCHK(b, hipStreamSynchronize(b->stream));
    std::vector<double> h(2 * part);
    BCHK(b, hipMemcpy(h.data(), d + nom, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    const double *sr = h.data(), *si = h.data() + part;      // S(re) and S(im): re[nsp], im[nsp], peak[count]
    for (size_t k = 0; k < nsp; ++k) {
        re[k] = sr[k] - si[nsp + k];
        im[k] = sr[nsp + k] + si[k];
    }
    for (int m = 0; peak && m < b->count; ++m) peak[m] = std::max(sr[2 * nsp + m], si[2 * nsp + m]);
    return 0;
}

int fdtd2d_batch_bloch_field_absmax(fdtd2d_batch_t *b, int field, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!out) return bfail(b, FDTD2D_E_ARG, "out must not be NULL");
    if (!b->bloch) return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first");
    if (b->hz && !b->hz_bloch_call)
        return refuse_hz(b, "this entry point of the Ez Bloch phase (fdtd2d_batch_hz_bloch.h has the Hz ones)");
    if (field != FDTD2D_FIELD_EZ && field != FDTD2D_FIELD_HX && field != FDTD2D_FIELD_HY)
        return bfail(b, FDTD2D_E_ARG, "field %d: FDTD2D_FIELD_EZ, _HX or _HY", field);
    int rc = use_device(b);
    if (rc) return rc;
    if ((rc = scratch(b, 2 * (size_t)b->count * sizeof(double)))) return rc;
    const void *re = field == FDTD2D_FIELD_EZ ? b->ez[b->cur] : field == FDTD2D_FIELD_HX ? b->hx : b->hy;
    const void *im = field == FDTD2D_FIELD_EZ ? b->ez_im : field == FDTD2D_FIELD_HX ? b->hx_im : b->hy_im;
    for (int q = 0; q < 2; ++q) {
        // Ez: columns 0..C-2 (the image slot holds a copy of column 0); Hx has C-1 columns, Hy has R-1 rows; a lattice
        // batch: rows 0..R-2 and columns 0..C-2 of each
        fdtd::batch_field_absmax_launch(q ? im : re, b->dtype == FDTD2D_F64, (double *)b->dsg + (size_t)q * b->count,
                                        b->count, b->rows - (field == FDTD2D_FIELD_HY || b->lattice),
                                        b->cols - (field != FDTD2D_FIELD_HY || b->lattice), b->pitch, b->mstride,
                                        b->stream);
        BCHK(b, hipGetLastError());
        b->launches++;
    }
    BCHK(b, hipStreamSynchronize(b->stream));
    std::vector<double> h(2 * (size_t)b->count);
    BCHK(b, hipMemcpy(h.data(), b->dsg, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int m = 0; m < b->count; ++m) out[m] = std::max(h[m], h[(size_t)b->count + m]);
    return 0;
}

int fdtd2d_batch_sync(fdtd2d_batch_t *b)
{
    if (!b) return FDTD2D_E_ARG;
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

}  // extern "C"

// ---- fdtd2d_batch_flux.h ------------------------------------------------------------------------------------------

extern "C" {

int fdtd2d_batch_set_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                int every)
{
    if (!b) return FDTD2D_E_ARG;
    if (nlines < 0 || nlines > FDTD2D_BATCH_MAX_FLUX_LINES)
        return bfail(b, FDTD2D_E_ARG, "nlines %d outside 0..%d", nlines, FDTD2D_BATCH_MAX_FLUX_LINES);
    long long cells = 0;
    if (nlines > 0) {
        if (b->hz) return refuse_hz(b, "flux lines (the sign and the averaged component differ)");
        if (b->boundary != FDTD2D_BOUNDARY_NONE)
            return bfail(b, FDTD2D_E_STATE, "flux lines need a PML or periodic batch: the kernels of the Mur frame carry none");
        if (b->lattice) return bfail(b, FDTD2D_E_STATE, "flux lines are not available in the lattice mode");
        if (b->bloch) return bfail(b, FDTD2D_E_STATE, "flux lines are not available with a Bloch phase");
        if (!b->ezx && !b->periodic)
            return bfail(b, FDTD2D_E_STATE, "flux lines need a PML layer (fdtd2d_batch_set_pml) or periodic columns");
        if (nfreq < 1 || nfreq > FDTD2D_BATCH_MAX_FLUX_FREQS)
            return bfail(b, FDTD2D_E_ARG, "nfreq %d outside 1..%d", nfreq, FDTD2D_BATCH_MAX_FLUX_FREQS);
        if (!lines || !omega) return bfail(b, FDTD2D_E_ARG, "lines and omega must not be NULL");
        if (every < 1) return bfail(b, FDTD2D_E_ARG, "every must be >= 1");
        const int R = b->rows, C = b->cols;
        for (int k = 0; k < nlines; ++k) {
            const int o = lines[4 * k], at = lines[4 * k + 1], first = lines[4 * k + 2], n = lines[4 * k + 3];
            if (o != 0 && o != 1) return bfail(b, FDTD2D_E_ARG, "line %d: orientation %d (0 row, 1 column)", k, o);
            if (o == 0 && (at < 1 || at > R - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: row %d outside 1..%d", k, at, R - 2);
            const int lo = b->periodic ? 0 : 1;
            if (o == 1 && (at < lo || at > C - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: column %d outside %d..%d%s", k, at, lo, C - 2,
                             b->periodic ? " (column C-1 is the image of column 0)" : "");
            const int extent = o == 1 ? R : b->periodic ? C - 1 : C;
            if (n < 1 || first < 0 || (long long)first + n > extent)
                return bfail(b, FDTD2D_E_ARG, "line %d: cells [%d, %d + %d) are empty or run past %d", k, first, first, n,
                             extent);
            cells += n;
        }
        if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    } else if (!b->flux_nl || b->hzflux || b->hzbflux) {   // the lines of the Hz headers are not this call's to remove
        return 0;
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still use the old lines
    if (nlines == 0) {
        for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph, (void **)&b->flux_acc_im})
            release(p);
        b->flux_nl = b->flux_nff = b->flux_cells = 0;
        b->bflux = false;
        fsrc_drop(b);                                         // the line sources go with their lines
        if (b->sigma_implicit && !b->periodic && !b->dcj) {   // the all-zero conductivity the lines brought
            release(&b->ca);
            release(&b->cb);
            b->sigma_host.clear();
            b->sigma_implicit = false;
        }
        return 0;
    }
    if (!b->ca) {                               // a lossless PML batch: the lossy kernels with ca = 1, cb = ce
        const std::vector<double> zero((size_t)b->count * b->rows * b->cols, 0.0);
        if ((rc = set_sigma(b, nullptr, zero.data(), FDTD2D_F64))) return rc;
        b->sigma_implicit = true;
    }
    const size_t acc = (size_t)b->count * 32 * nfreq * (size_t)cells, om = (size_t)b->count * nfreq * sizeof(double);
    double *nacc = nullptr, *nom = nullptr, *nph = nullptr;
    if ((rc = alloc(b, (void **)&nacc, acc)) || (rc = alloc(b, (void **)&nom, om)) ||
        (rc = alloc(b, (void **)&nph, 2 * om))) {
        for (void **p : {(void **)&nacc, (void **)&nom, (void **)&nph}) release(p);
        return rc;
    }
    hipError_t e = hipMemsetAsync(nacc, 0, acc, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(nom, omega, om, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        for (void **p : {(void **)&nacc, (void **)&nom, (void **)&nph}) release(p);
        return bfail(b, -(1000 + (int)e), "setting up the flux lines failed: %s", hipGetErrorString(e));
    }
    for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph}) release(p);
    fsrc_drop(b);                               // line sources belong to the lines they were set on
    b->flux_acc = nacc;
    b->flux_omega = nom;
    b->flux_ph = nph;
    std::copy(lines, lines + 4 * nlines, b->flux_line);
    b->flux_nl = nlines;
    b->flux_nff = nfreq;
    b->flux_cells = (int)cells;
    b->flux_every = every;
    b->flux_step0 = b->step;
    return 0;
}

int fdtd2d_batch_read_flux_lines(fdtd2d_batch_t *b, double *ez_re, double *ez_im, double *ht_re, double *ht_im)
{
    if (!b || !ez_re || !ez_im || !ht_re || !ht_im) return FDTD2D_E_ARG;
    if (!b->flux_nl) return bfail(b, FDTD2D_E_STATE, "no flux lines are set");
    if (b->bflux) return bfail(b, FDTD2D_E_STATE, "the lines are Bloch lines: use fdtd2d_batch_read_bloch_flux_lines");
    if (b->hzflux) return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz polarisation: use fdtd2d_batch_read_hz_flux_lines");
    if (b->hzbflux)
        return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz Bloch phase: use fdtd2d_batch_read_hz_bloch_flux_lines");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t per = (size_t)b->flux_nff * b->flux_cells;   // one member's Ez re (or any of the four)
    std::vector<double> acc((size_t)b->count * 4 * per);
    BCHK(b, hipMemcpy(acc.data(), b->flux_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    double *out[4] = {ez_re, ez_im, ht_re, ht_im};
    for (int m = 0; m < b->count; ++m)
        for (int k = 0; k < 4; ++k)
            std::memcpy(out[k] + m * per, acc.data() + (4 * (size_t)m + k) * per, per * sizeof(double));
    return 0;
}

int fdtd2d_batch_flux(fdtd2d_batch_t *b, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!out) return bfail(b, FDTD2D_E_ARG, "out must not be NULL");
    if (!b->flux_nl) return bfail(b, FDTD2D_E_STATE, "no flux lines are set");
    if (b->bflux) return bfail(b, FDTD2D_E_STATE, "the lines are Bloch lines: use fdtd2d_batch_bloch_flux");
    if (b->hzflux) return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz polarisation: use fdtd2d_batch_hz_flux");
    if (b->hzbflux) return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz Bloch phase: use fdtd2d_batch_hz_bloch_flux");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t n = (size_t)b->count * b->flux_nl * b->flux_nff;
    if ((rc = scratch(b, n * sizeof(double)))) return rc;
    fdtd::batch_flux_launch(flux_view(b), (double *)b->dsg, b->count, b->dt, b->dx, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(out, b->dsg, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// ---- fdtd2d_batch_hz_flux.h ---------------------------------------------------------------------------------------
// The lines share the host state of fdtd2d_batch_flux.h's (`flux_nl` is set too, so the capacity rule, the info ids, the
// placement option, fdtd2d_batch_reset and the refusals while lines are set serve them as they are); run_hz takes the
// kernels of batch_hz_flux.hip while `hzflux` is set.

extern "C" {

int fdtd2d_batch_set_hz_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                   int every)
{
    if (!b) return FDTD2D_E_ARG;
    if (nlines < 0 || nlines > FDTD2D_BATCH_MAX_FLUX_LINES)
        return bfail(b, FDTD2D_E_ARG, "nlines %d outside 0..%d", nlines, FDTD2D_BATCH_MAX_FLUX_LINES);
    long long cells = 0;
    if (nlines > 0) {
        if (b->hz && b->bloch) return refuse_bloch(b, "fdtd2d_batch_set_hz_flux_lines");
        if (!b->hz)
            return bfail(b, FDTD2D_E_STATE, "fdtd2d_batch_set_hz_flux_lines needs the Hz polarisation "
                         "(fdtd2d_batch_set_polarization): the lines of the Ez polarisation are fdtd2d_batch_set_flux_lines'");
        if (!b->ezx && !b->periodic)
            return bfail(b, FDTD2D_E_STATE, "flux lines need a PML layer (fdtd2d_batch_set_pml) or periodic columns");
        if (nfreq < 1 || nfreq > FDTD2D_BATCH_MAX_FLUX_FREQS)
            return bfail(b, FDTD2D_E_ARG, "nfreq %d outside 1..%d", nfreq, FDTD2D_BATCH_MAX_FLUX_FREQS);
        if (!lines || !omega) return bfail(b, FDTD2D_E_ARG, "lines and omega must not be NULL");
        if (every < 1) return bfail(b, FDTD2D_E_ARG, "every must be >= 1");
        const int R = b->rows, C = b->cols;
        for (int k = 0; k < nlines; ++k) {
            const int o = lines[4 * k], at = lines[4 * k + 1], first = lines[4 * k + 2], n = lines[4 * k + 3];
            if (o != 0 && o != 1) return bfail(b, FDTD2D_E_ARG, "line %d: orientation %d (0 row, 1 column)", k, o);
            if (o == 0 && (at < 1 || at > R - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: row %d outside 1..%d", k, at, R - 2);
            const int lo = b->periodic ? 0 : 1;
            if (o == 1 && (at < lo || at > C - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: column %d outside %d..%d%s", k, at, lo, C - 2,
                             b->periodic ? " (column C-1 is the image of column 0)" : "");
            const int extent = o == 1 ? R : b->periodic ? C - 1 : C;
            if (n < 1 || first < 0 || (long long)first + n > extent)
                return bfail(b, FDTD2D_E_ARG, "line %d: cells [%d, %d + %d) are empty or run past %d", k, first, first, n,
                             extent);
            cells += n;
        }
        if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    } else if (!b->hzflux) {
        return 0;
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still use the old lines
    if (nlines == 0) {
        for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph}) release(p);
        b->flux_nl = b->flux_nff = b->flux_cells = 0;
        b->hzflux = false;
        return 0;
    }
    const size_t acc = (size_t)b->count * 32 * nfreq * (size_t)cells, om = (size_t)b->count * nfreq * sizeof(double);
    double *nacc = nullptr, *nom = nullptr, *nph = nullptr;
    if ((rc = alloc(b, (void **)&nacc, acc)) || (rc = alloc(b, (void **)&nom, om)) ||
        (rc = alloc(b, (void **)&nph, 2 * om))) {
        for (void **p : {(void **)&nacc, (void **)&nom, (void **)&nph}) release(p);
        return rc;
    }
    hipError_t e = hipMemsetAsync(nacc, 0, acc, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(nom, omega, om, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        for (void **p : {(void **)&nacc, (void **)&nom, (void **)&nph}) release(p);
        return bfail(b, -(1000 + (int)e), "setting up the flux lines failed: %s", hipGetErrorString(e));
    }
    for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph}) release(p);
    b->flux_acc = nacc;
    b->flux_omega = nom;
    b->flux_ph = nph;
    std::copy(lines, lines + 4 * nlines, b->flux_line);
    b->flux_nl = nlines;
    b->flux_nff = nfreq;
    b->flux_cells = (int)cells;
    b->flux_every = every;
    b->flux_step0 = b->step;
    b->hzflux = true;
    return 0;
}

int fdtd2d_batch_read_hz_flux_lines(fdtd2d_batch_t *b, double *hz_re, double *hz_im, double *et_re, double *et_im)
{
    if (!b || !hz_re || !hz_im || !et_re || !et_im) return FDTD2D_E_ARG;
    if (b->hzbflux)
        return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz Bloch phase: use fdtd2d_batch_read_hz_bloch_flux_lines");
    if (!b->hzflux) return bfail(b, FDTD2D_E_STATE, "no flux lines of the Hz polarisation are set");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t per = (size_t)b->flux_nff * b->flux_cells;   // one member's Hz re (or any of the four)
    std::vector<double> acc((size_t)b->count * 4 * per);
    BCHK(b, hipMemcpy(acc.data(), b->flux_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    double *out[4] = {hz_re, hz_im, et_re, et_im};
    for (int m = 0; m < b->count; ++m)
        for (int k = 0; k < 4; ++k)
            std::memcpy(out[k] + m * per, acc.data() + (4 * (size_t)m + k) * per, per * sizeof(double));
    return 0;
}

int fdtd2d_batch_hz_flux(fdtd2d_batch_t *b, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!out) return bfail(b, FDTD2D_E_ARG, "out must not be NULL");
    if (b->hzbflux) return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz Bloch phase: use fdtd2d_batch_hz_bloch_flux");
    if (!b->hzflux) return bfail(b, FDTD2D_E_STATE, "no flux lines of the Hz polarisation are set");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t n = (size_t)b->count * b->flux_nl * b->flux_nff;
    if ((rc = scratch(b, n * sizeof(double)))) return rc;
    fdtd::batch_hz_flux_launch(flux_view(b), (double *)b->dsg, b->count, b->dt, b->dx, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(out, b->dsg, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// ---- fdtd2d_batch_hz_bloch_flux.h ---------------------------------------------------------------------------------
// The lines share the host state of fdtd2d_batch_flux.h's (`flux_nl` is set too, so the capacity rule, the info ids, the
// placement option and the refusals while lines are set serve them as they are) and flux_acc_im of the Ez Bloch lines;
// run_impl takes the kernels of batch_hz_bloch_flux.hip while `hzbflux` is set.

extern "C" {

int fdtd2d_batch_set_hz_bloch_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                         int every)
{
    if (!b) return FDTD2D_E_ARG;
    if (nlines < 0 || nlines > FDTD2D_BATCH_MAX_FLUX_LINES)
        return bfail(b, FDTD2D_E_ARG, "nlines %d outside 0..%d", nlines, FDTD2D_BATCH_MAX_FLUX_LINES);
    long long cells = 0;
    if (nlines > 0) {
        if (!b->hz || !b->bloch || !b->periodic || b->lattice)
            return bfail(b, FDTD2D_E_STATE, "fdtd2d_batch_set_hz_bloch_flux_lines needs the phase of the Hz polarisation: "
                         "call fdtd2d_batch_set_hz_bloch first (without a phase use fdtd2d_batch_set_hz_flux_lines, in the Ez "
                         "polarisation fdtd2d_batch_set_bloch_flux_lines)");
        if (nfreq < 1 || nfreq > FDTD2D_BATCH_MAX_FLUX_FREQS)
            return bfail(b, FDTD2D_E_ARG, "nfreq %d outside 1..%d", nfreq, FDTD2D_BATCH_MAX_FLUX_FREQS);
        if (!lines || !omega) return bfail(b, FDTD2D_E_ARG, "lines and omega must not be NULL");
        if (every < 1) return bfail(b, FDTD2D_E_ARG, "every must be >= 1");
        const int R = b->rows, C = b->cols;
        for (int k = 0; k < nlines; ++k) {
            const int o = lines[4 * k], at = lines[4 * k + 1], first = lines[4 * k + 2], n = lines[4 * k + 3];
            if (o != 0 && o != 1) return bfail(b, FDTD2D_E_ARG, "line %d: orientation %d (0 row, 1 column)", k, o);
            if (o == 0 && (at < 1 || at > R - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: row %d outside 1..%d", k, at, R - 2);
            if (o == 1 && (at < 0 || at > C - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: column %d outside 0..%d (column C-1 is the image of column 0)", k, at,
                             C - 2);
            const int extent = o == 1 ? R : C - 1;
            if (n < 1 || first < 0 || (long long)first + n > extent)
                return bfail(b, FDTD2D_E_ARG, "line %d: cells [%d, %d + %d) are empty or run past %d", k, first, first, n,
                             extent);
            cells += n;
        }
        if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    } else if (!b->hzbflux) {
        return 0;
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still use the old lines
    if (nlines == 0) {
        for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph, (void **)&b->flux_acc_im})
            release(p);
        b->flux_nl = b->flux_nff = b->flux_cells = 0;
        b->hzbflux = false;
        return 0;
    }
    // the new buffers before the old ones go: a refused call keeps the old lines
    const size_t acc = (size_t)b->count * 32 * nfreq * (size_t)cells, om = (size_t)b->count * nfreq * sizeof(double);
    double *nacc = nullptr, *nacci = nullptr, *nom = nullptr, *nph = nullptr;
    auto drop = [&]() {
        for (void **p : {(void **)&nacc, (void **)&nacci, (void **)&nom, (void **)&nph}) release(p);
    };
    if ((rc = alloc(b, (void **)&nacc, acc)) || (rc = alloc(b, (void **)&nacci, acc)) ||
        (rc = alloc(b, (void **)&nom, om)) || (rc = alloc(b, (void **)&nph, 2 * om))) {
        drop();
        return rc;
    }
    hipError_t e = hipMemsetAsync(nacc, 0, acc, b->stream);
    if (e == hipSuccess) e = hipMemsetAsync(nacci, 0, acc, b->stream);
    if (e == hipSuccess) e = hipMemsetAsync(nph, 0, 2 * om, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(nom, omega, om, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        drop();
        return bfail(b, -(1000 + (int)e), "setting up the flux lines of the Hz Bloch phase failed: %s", hipGetErrorString(e));
    }
    for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph, (void **)&b->flux_acc_im})
        release(p);
    b->flux_acc = nacc;
    b->flux_acc_im = nacci;
    b->flux_omega = nom;
    b->flux_ph = nph;
    std::copy(lines, lines + 4 * nlines, b->flux_line);
    b->flux_nl = nlines;
    b->flux_nff = nfreq;
    b->flux_cells = (int)cells;
    b->flux_every = every;
    b->flux_step0 = b->step;
    b->hzbflux = true;
    return 0;
}

int fdtd2d_batch_read_hz_bloch_flux_lines(fdtd2d_batch_t *b, int part, double *hz_re, double *hz_im, double *et_re,
                                          double *et_im)
{
    if (!b || !hz_re || !hz_im || !et_re || !et_im) return FDTD2D_E_ARG;
    if (part != 0 && part != 1) return bfail(b, FDTD2D_E_ARG, "part %d (0 real, 1 imaginary)", part);
    if (!b->hzbflux) return bfail(b, FDTD2D_E_STATE, "no flux lines of the Hz Bloch phase are set");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t per = (size_t)b->flux_nff * b->flux_cells;   // one member's Hz re (or any of the four)
    std::vector<double> acc((size_t)b->count * 4 * per);
    BCHK(b, hipMemcpy(acc.data(), part ? b->flux_acc_im : b->flux_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    double *out[4] = {hz_re, hz_im, et_re, et_im};
    for (int m = 0; m < b->count; ++m)
        for (int k = 0; k < 4; ++k)
            std::memcpy(out[k] + m * per, acc.data() + (4 * (size_t)m + k) * per, per * sizeof(double));
    return 0;
}

int fdtd2d_batch_hz_bloch_flux(fdtd2d_batch_t *b, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!out) return bfail(b, FDTD2D_E_ARG, "out must not be NULL");
    if (!b->hzbflux) return bfail(b, FDTD2D_E_STATE, "no flux lines of the Hz Bloch phase are set");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t n = (size_t)b->count * b->flux_nl * b->flux_nff;
    if ((rc = scratch(b, n * sizeof(double)))) return rc;
    fdtd::batch_hz_bloch_flux_launch(flux_view(b), b->flux_acc_im, (double *)b->dsg, b->count, b->dt, b->dx, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(out, b->dsg, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// ---- fdtd2d_batch_bloch_flux.h ------------------------------------------------------------------------------------

extern "C" {

int fdtd2d_batch_set_bloch_flux_lines(fdtd2d_batch_t *b, int nlines, const int *lines, int nfreq, const double *omega,
                                      int every)
{
    if (!b) return FDTD2D_E_ARG;
    if (nlines < 0 || nlines > FDTD2D_BATCH_MAX_FLUX_LINES)
        return bfail(b, FDTD2D_E_ARG, "nlines %d outside 0..%d", nlines, FDTD2D_BATCH_MAX_FLUX_LINES);
    long long cells = 0;
    if (nlines > 0) {
        if (b->hz) return refuse_hz(b, "Bloch flux lines");
        if (b->boundary != FDTD2D_BOUNDARY_NONE || !b->periodic)
            return bfail(b, FDTD2D_E_STATE, "Bloch flux lines need a batch with periodic columns and a Bloch phase");
        if (b->lattice) return bfail(b, FDTD2D_E_STATE, "Bloch flux lines are not available in the lattice mode");
        if (!b->bloch)
            return bfail(b, FDTD2D_E_STATE, "no Bloch phase is set: call fdtd2d_batch_set_bloch first (without a phase use "
                         "fdtd2d_batch_set_flux_lines)");
        if (b->npts) return bfail(b, FDTD2D_E_STATE, "Bloch flux lines are not available with Bloch point sources (remove them)");
        if (b->win_held || b->win_held_im)
            return bfail(b, FDTD2D_E_STATE, "Bloch flux lines are not available with a held Bloch window (set the window again)");
        if (nfreq < 1 || nfreq > FDTD2D_BATCH_MAX_FLUX_FREQS)
            return bfail(b, FDTD2D_E_ARG, "nfreq %d outside 1..%d", nfreq, FDTD2D_BATCH_MAX_FLUX_FREQS);
        if (!lines || !omega) return bfail(b, FDTD2D_E_ARG, "lines and omega must not be NULL");
        if (every < 1) return bfail(b, FDTD2D_E_ARG, "every must be >= 1");
        const int R = b->rows, C = b->cols;
        for (int k = 0; k < nlines; ++k) {
            const int o = lines[4 * k], at = lines[4 * k + 1], first = lines[4 * k + 2], n = lines[4 * k + 3];
            if (o != 0 && o != 1) return bfail(b, FDTD2D_E_ARG, "line %d: orientation %d (0 row, 1 column)", k, o);
            if (o == 0 && (at < 1 || at > R - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: row %d outside 1..%d", k, at, R - 2);
            if (o == 1 && (at < 0 || at > C - 2))
                return bfail(b, FDTD2D_E_ARG, "line %d: column %d outside 0..%d (column C-1 is the image of column 0)", k, at,
                             C - 2);
            const int extent = o == 1 ? R : C - 1;
            if (n < 1 || first < 0 || (long long)first + n > extent)
                return bfail(b, FDTD2D_E_ARG, "line %d: cells [%d, %d + %d) are empty or run past %d", k, first, first, n,
                             extent);
            cells += n;
        }
        if (!b->have_mat) return bfail(b, FDTD2D_E_STATE, "materials not set: call fdtd2d_batch_set_materials first");
    } else if (!b->bflux) {
        return 0;
    }
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));   // a running launch may still use the old lines
    if (nlines == 0) {
        for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph, (void **)&b->flux_acc_im})
            release(p);
        b->flux_nl = b->flux_nff = b->flux_cells = 0;
        b->bflux = false;
        fsrc_drop(b);                           // the line sources go with their lines
        return 0;
    }
    // the new buffers before the old ones go: a refused call keeps the old lines
    const size_t acc = (size_t)b->count * 32 * nfreq * (size_t)cells, om = (size_t)b->count * nfreq * sizeof(double);
    double *nacc = nullptr, *nacci = nullptr, *nom = nullptr, *nph = nullptr;
    auto drop = [&]() {
        for (void **p : {(void **)&nacc, (void **)&nacci, (void **)&nom, (void **)&nph}) release(p);
    };
    if ((rc = alloc(b, (void **)&nacc, acc)) || (rc = alloc(b, (void **)&nacci, acc)) ||
        (rc = alloc(b, (void **)&nom, om)) || (rc = alloc(b, (void **)&nph, 2 * om))) {
        drop();
        return rc;
    }
    hipError_t e = hipMemsetAsync(nacc, 0, acc, b->stream);
    if (e == hipSuccess) e = hipMemsetAsync(nacci, 0, acc, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(nom, omega, om, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        drop();
        return bfail(b, -(1000 + (int)e), "setting up the Bloch flux lines failed: %s", hipGetErrorString(e));
    }
    for (void **p : {(void **)&b->flux_acc, (void **)&b->flux_omega, (void **)&b->flux_ph, (void **)&b->flux_acc_im})
        release(p);
    fsrc_drop(b);                               // line sources belong to the lines they were set on
    b->flux_acc = nacc;
    b->flux_acc_im = nacci;
    b->flux_omega = nom;
    b->flux_ph = nph;
    std::copy(lines, lines + 4 * nlines, b->flux_line);
    b->flux_nl = nlines;
    b->flux_nff = nfreq;
    b->flux_cells = (int)cells;
    b->flux_every = every;
    b->flux_step0 = b->step;
    b->bflux = true;
    return 0;
}

int fdtd2d_batch_read_bloch_flux_lines(fdtd2d_batch_t *b, int part, double *ez_re, double *ez_im, double *ht_re,
                                       double *ht_im)
{
    if (!b || !ez_re || !ez_im || !ht_re || !ht_im) return FDTD2D_E_ARG;
    if (part != 0 && part != 1) return bfail(b, FDTD2D_E_ARG, "part %d (0 real, 1 imaginary)", part);
    if (b->hzbflux)
        return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz Bloch phase: use fdtd2d_batch_read_hz_bloch_flux_lines");
    if (!b->bflux) return bfail(b, FDTD2D_E_STATE, "no Bloch flux lines are set");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t per = (size_t)b->flux_nff * b->flux_cells;   // one member's Ez re (or any of the four)
    std::vector<double> acc((size_t)b->count * 4 * per);
    BCHK(b, hipMemcpy(acc.data(), part ? b->flux_acc_im : b->flux_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    double *out[4] = {ez_re, ez_im, ht_re, ht_im};
    for (int m = 0; m < b->count; ++m)
        for (int k = 0; k < 4; ++k)
            std::memcpy(out[k] + m * per, acc.data() + (4 * (size_t)m + k) * per, per * sizeof(double));
    return 0;
}

int fdtd2d_batch_bloch_flux(fdtd2d_batch_t *b, double *out)
{
    if (!b) return FDTD2D_E_ARG;
    if (!out) return bfail(b, FDTD2D_E_ARG, "out must not be NULL");
    if (b->hzbflux) return bfail(b, FDTD2D_E_STATE, "the lines are those of the Hz Bloch phase: use fdtd2d_batch_hz_bloch_flux");
    if (!b->bflux) return bfail(b, FDTD2D_E_STATE, "no Bloch flux lines are set");
    int rc = use_device(b);
    if (rc) return rc;
    const size_t n = (size_t)b->count * b->flux_nl * b->flux_nff;
    if ((rc = scratch(b, n * sizeof(double)))) return rc;
    fdtd::batch_bloch_flux_launch(flux_view(b), b->flux_acc_im, (double *)b->dsg, b->count, b->dt, b->dx, b->stream);
    BCHK(b, hipGetLastError());
    b->launches++;
    BCHK(b, hipStreamSynchronize(b->stream));
    BCHK(b, hipMemcpy(out, b->dsg, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// ---- fdtd2d_batch_flux_adjoint.h ----------------------------------------------------------------------------------

namespace {

// what line sources need: plain flux lines (hence a PML or periodic batch without a Bloch phase) and, when point sources
// are set too, their channel count
int fsrc_refuse(fdtd2d_batch *b, int nchan)
{
    if (b->hz) return refuse_hz(b, "line sources on flux lines");
    if (!b->flux_nl || b->bflux)
        return bfail(b, FDTD2D_E_STATE, "line sources live on flux lines: call fdtd2d_batch_set_flux_lines first (a PML or "
                     "periodic batch without a Bloch phase)");
    if (b->npts && b->pts_nchan != nchan)
        return bfail(b, FDTD2D_E_STATE, "%d channels, but the point sources that are set take %d: one run drives both",
                     nchan, b->pts_nchan);
    return 0;
}

// replaces the line sources by the device arrays given (either may be nullptr) and uploads the lines' geometry for
// them; on failure the arrays are released and the previous sources stay
int fsrc_install(fdtd2d_batch *b, double *we, double *wh, int nchan, double *we_im = nullptr, double *wh_im = nullptr)
{
    int geom[fdtd::BATCH_FLUXSRC_GEOM] = {};
    int off = 0;
    for (int k = 0; k < b->flux_nl; ++k) {
        for (int q = 0; q < 4; ++q) geom[5 * k + q] = b->flux_line[4 * k + q];
        geom[5 * k + 4] = off;
        off += b->flux_line[4 * k + 3];
    }
    geom[5 * FDTD2D_BATCH_MAX_FLUX_LINES] = b->flux_nl;
    int *ng = nullptr;
    int rc = alloc(b, (void **)&ng, sizeof geom);
    hipError_t e = rc ? hipSuccess : hipMemcpy(ng, geom, sizeof geom, hipMemcpyHostToDevice);
    if (rc || e != hipSuccess) {
        for (void **p : {(void **)&we, (void **)&wh, (void **)&ng, (void **)&we_im, (void **)&wh_im}) release(p);
        return rc ? rc : bfail(b, -(1000 + (int)e), "setting up the line sources failed: %s", hipGetErrorString(e));
    }
    fsrc_drop(b);
    b->fsrc_we = we;
    b->fsrc_wh = wh;
    b->fsrc_we_im = we_im;
    b->fsrc_wh_im = wh_im;
    b->fsrc_geom = ng;
    b->fsrc_nchan = nchan;
    return 0;
}

}  // namespace

extern "C" {

int fdtd2d_batch_set_flux_line_sources(fdtd2d_batch_t *b, int nchan, const double *we, const double *wh)
{
    if (!b) return FDTD2D_E_ARG;
    if ((!we && !wh) || nchan == 0) {           // remove
        if (!b->fsrc_nchan) return 0;
        int rc = use_device(b);
        if (rc) return rc;
        BCHK(b, hipStreamSynchronize(b->stream));
        fsrc_drop(b);
        return 0;
    }
    if (nchan < 1 || nchan > FDTD2D_BATCH_MAX_CHANNELS)
        return bfail(b, FDTD2D_E_ARG, "nchan %d outside 1..%d", nchan, FDTD2D_BATCH_MAX_CHANNELS);
    int rc = fsrc_refuse(b, nchan);
    if (rc) return rc;
    const size_t n = (size_t)b->count * b->flux_cells * nchan;
    for (const double *w : {we, wh})
        for (size_t k = 0; w && k < n; ++k)
            if (!std::isfinite(w[k]))
                return bfail(b, FDTD2D_E_ARG, "member %zu: a line source weight is not finite",
                             k / ((size_t)b->flux_cells * nchan));
    if ((rc = use_device(b))) return rc;
    double *ne = nullptr, *nh = nullptr;
    if ((we && (rc = alloc(b, (void **)&ne, n * sizeof(double)))) ||
        (wh && (rc = alloc(b, (void **)&nh, n * sizeof(double))))) {
        for (void **p : {(void **)&ne, (void **)&nh}) release(p);
        return rc;
    }
    hipError_t e = hipStreamSynchronize(b->stream);   // a running launch may still read the old weights
    if (e == hipSuccess && we) e = hipMemcpy(ne, we, n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && wh) e = hipMemcpy(nh, wh, n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        for (void **p : {(void **)&ne, (void **)&nh}) release(p);
        return bfail(b, -(1000 + (int)e), "setting up the line sources failed: %s", hipGetErrorString(e));
    }
    return fsrc_install(b, ne, nh, nchan);
}

int fdtd2d_batch_read_flux_line_sources(fdtd2d_batch_t *b, double *we, double *wh)
{
    if (!b || !we || !wh) return FDTD2D_E_ARG;
    if (!b->fsrc_nchan || b->bflux) return bfail(b, FDTD2D_E_STATE, "no line sources are set");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->count * b->flux_cells * b->fsrc_nchan;
    const double *from[2] = {b->fsrc_we, b->fsrc_wh};
    double *to[2] = {we, wh};
    for (int k = 0; k < 2; ++k) {
        if (from[k]) BCHK(b, hipMemcpy(to[k], from[k], n * sizeof(double), hipMemcpyDeviceToHost));
        else std::fill(to[k], to[k] + n, 0.0);
    }
    return 0;
}

int fdtd2d_batch_flux_line_weights(fdtd2d_batch_t *b, const double *dJdP, const double *solve, int solve_per_member,
                                   const double *scale_e, const double *scale_h)
{
    if (!b) return FDTD2D_E_ARG;
    if (!dJdP || !solve) return bfail(b, FDTD2D_E_ARG, "dJdP and solve must not be NULL");
    const int nchan = 2 * b->flux_nff;
    int rc = fsrc_refuse(b, nchan);
    if (rc) return rc;
    if ((rc = use_device(b))) return rc;
    const size_t nj = (size_t)b->count * b->flux_nl * b->flux_nff, ns = (size_t)(solve_per_member ? b->count : 1) * nchan * nchan;
    const size_t nc = (size_t)b->count * b->flux_cells, nw = nc * nchan;
    // the inputs in the design loop's scratch: dJdP, solve, scale_e, scale_h
    if ((rc = scratch(b, (nj + ns + 2 * nc) * sizeof(double)))) return rc;
    double *dj = (double *)b->dsg, *ds = dj + nj, *dse = ds + ns, *dsh = dse + nc;
    double *ne = nullptr, *nh = nullptr;
    if ((rc = alloc(b, (void **)&ne, nw * sizeof(double))) || (rc = alloc(b, (void **)&nh, nw * sizeof(double)))) {
        for (void **p : {(void **)&ne, (void **)&nh}) release(p);
        return rc;
    }
    hipError_t e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(dj, dJdP, nj * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ds, solve, ns * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && scale_e) e = hipMemcpy(dse, scale_e, nc * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && scale_h) e = hipMemcpy(dsh, scale_h, nc * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const fdtd::BatchFluxWeights W{dj, ds, scale_e ? dse : nullptr, scale_h ? dsh : nullptr, ne, nh,
                                       solve_per_member ? (long long)nchan * nchan : 0};
        fdtd::batch_flux_line_weights_launch(flux_view(b), W, b->count, b->dt, b->dx, b->stream);
        e = hipGetLastError();
        if (e == hipSuccess) b->launches++;
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    }
    if (e != hipSuccess) {
        for (void **p : {(void **)&ne, (void **)&nh}) release(p);
        return bfail(b, -(1000 + (int)e), "forming the line source weights failed: %s", hipGetErrorString(e));
    }
    return fsrc_install(b, ne, nh, nchan);
}

}  // extern "C"

// ---- fdtd2d_batch_bloch_flux_adjoint.h ----------------------------------------------------------------------------

extern "C" {

int fdtd2d_batch_set_bloch_flux_line_sources(fdtd2d_batch_t *b, int nchan, const double *we_re, const double *we_im,
                                             const double *wh_re, const double *wh_im)
{
    if (!b) return FDTD2D_E_ARG;
    const double *host[4] = {we_re, wh_re, we_im, wh_im};
    if ((!we_re && !we_im && !wh_re && !wh_im) || nchan == 0) {   // remove
        if (!b->bflux || !b->fsrc_nchan) return 0;
        int rc = use_device(b);
        if (rc) return rc;
        BCHK(b, hipStreamSynchronize(b->stream));
        fsrc_drop(b);
        return 0;
    }
    if (nchan < 1 || nchan > FDTD2D_BATCH_MAX_CHANNELS)
        return bfail(b, FDTD2D_E_ARG, "nchan %d outside 1..%d", nchan, FDTD2D_BATCH_MAX_CHANNELS);
    if (!b->bflux)
        return bfail(b, FDTD2D_E_STATE, "Bloch line sources live on Bloch flux lines: call "
                     "fdtd2d_batch_set_bloch_flux_lines first");
    const size_t n = (size_t)b->count * b->flux_cells * nchan;
    for (const double *w : host)
        for (size_t k = 0; w && k < n; ++k)
            if (!std::isfinite(w[k]))
                return bfail(b, FDTD2D_E_ARG, "member %zu: a line source weight is not finite",
                             k / ((size_t)b->flux_cells * nchan));
    int rc = use_device(b);
    if (rc) return rc;
    double *dev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto drop = [&]() {
        for (double *&p : dev) release((void **)&p);
    };
    for (int k = 0; k < 4; ++k)
        if (host[k] && (rc = alloc(b, (void **)&dev[k], n * sizeof(double)))) {
            drop();
            return rc;
        }
    hipError_t e = hipStreamSynchronize(b->stream);   // a running launch may still read the old weights
    for (int k = 0; k < 4; ++k)
        if (e == hipSuccess && host[k]) e = hipMemcpy(dev[k], host[k], n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        drop();
        return bfail(b, -(1000 + (int)e), "setting up the line sources failed: %s", hipGetErrorString(e));
    }
    return fsrc_install(b, dev[0], dev[1], nchan, dev[2], dev[3]);
}

int fdtd2d_batch_read_bloch_flux_line_sources(fdtd2d_batch_t *b, double *we_re, double *we_im, double *wh_re,
                                              double *wh_im)
{
    if (!b || !we_re || !we_im || !wh_re || !wh_im) return FDTD2D_E_ARG;
    if (!b->bflux || !b->fsrc_nchan) return bfail(b, FDTD2D_E_STATE, "no line sources are set on Bloch flux lines");
    int rc = use_device(b);
    if (rc) return rc;
    BCHK(b, hipStreamSynchronize(b->stream));
    const size_t n = (size_t)b->count * b->flux_cells * b->fsrc_nchan;
    const double *from[4] = {b->fsrc_we, b->fsrc_we_im, b->fsrc_wh, b->fsrc_wh_im};
    double *to[4] = {we_re, we_im, wh_re, wh_im};
    for (int k = 0; k < 4; ++k) {
        if (from[k]) BCHK(b, hipMemcpy(to[k], from[k], n * sizeof(double), hipMemcpyDeviceToHost));
        else std::fill(to[k], to[k] + n, 0.0);
    }
    return 0;
}

int fdtd2d_batch_bloch_flux_line_weights(fdtd2d_batch_t *b, const double *dJdP, const double *solve,
                                         int solve_per_member, const double *scale_e, const double *scale_h)
{
    if (!b) return FDTD2D_E_ARG;
    if (!dJdP || !solve) return bfail(b, FDTD2D_E_ARG, "dJdP and solve must not be NULL");
    if (!b->bflux || !b->flux_acc_im)
        return bfail(b, FDTD2D_E_STATE, "Bloch line sources live on Bloch flux lines: call "
                     "fdtd2d_batch_set_bloch_flux_lines first");
    const int nchan = 2 * b->flux_nff;
    int rc = use_device(b);
    if (rc) return rc;
    const size_t nj = (size_t)b->count * b->flux_nl * b->flux_nff, ns = (size_t)(solve_per_member ? b->count : 1) * nchan * nchan;
    const size_t nc = (size_t)b->count * b->flux_cells, nw = nc * nchan;
    // the inputs in the design loop's scratch: dJdP, solve, scale_e, scale_h
    if ((rc = scratch(b, (nj + ns + 2 * nc) * sizeof(double)))) return rc;
    double *dj = (double *)b->dsg, *ds = dj + nj, *dse = ds + ns, *dsh = dse + nc;
    double *ne = nullptr, *nh = nullptr;
    if ((rc = alloc(b, (void **)&ne, nw * sizeof(double))) || (rc = alloc(b, (void **)&nh, nw * sizeof(double)))) {
        for (void **p : {(void **)&ne, (void **)&nh}) release(p);
        return rc;
    }
    hipError_t e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(dj, dJdP, nj * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ds, solve, ns * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && scale_e) e = hipMemcpy(dse, scale_e, nc * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && scale_h) e = hipMemcpy(dsh, scale_h, nc * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const fdtd::BatchFluxWeights W{dj, ds, scale_e ? dse : nullptr, scale_h ? dsh : nullptr, ne, nh,
                                       solve_per_member ? (long long)nchan * nchan : 0};
        fdtd::batch_bloch_flux_line_weights_launch(flux_view(b), b->flux_acc_im, W, b->count, b->dt, b->dx, b->stream);
        e = hipGetLastError();
        if (e == hipSuccess) b->launches++;
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    }
    if (e != hipSuccess) {
        for (void **p : {(void **)&ne, (void **)&nh}) release(p);
        return bfail(b, -(1000 + (int)e), "forming the line source weights failed: %s", hipGetErrorString(e));
    }
    return fsrc_install(b, ne, nh, nchan);
}

}  // extern "C"
