// The instantiations and launches of the design-loop kernels (include/fdtd2d_batch_design.h,
// kernels_batch_design.hpp), in a translation unit of their own: they compile beside batch.hip, batch_monitor.hip and
// batch_adjoint.hip, whose kernels keep their code.
#include "kernels_batch_design.hpp"

namespace fdtd {

namespace {
// one workgroup per member; a workgroup walks the members beyond the grid
int member_blocks(int B) { return B < 65535 ? B : 65535; }
}  // namespace

void batch_probe_spectra_launch(const BatchSpectra &a, hipStream_t stream)
{
    const dim3 grid(member_blocks(a.B)), block(BATCH_DSG_THREADS);
    const int pf = a.np * a.nf;
    if (pf <= BATCH_DSG_THREADS) hipLaunchKernelGGL(k_batch_probe_spectra<1>, grid, block, 0, stream, a);
    else if (pf <= 2 * BATCH_DSG_THREADS) hipLaunchKernelGGL(k_batch_probe_spectra<2>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_batch_probe_spectra<4>, grid, block, 0, stream, a);
}

void batch_field_absmax_launch(const void *f, bool dtype_f64, double *out, int B, int nrows, int ncols, long long pitch,
                               size_t mstride, hipStream_t stream)
{
    const dim3 grid(member_blocks(B)), block(BATCH_DSG_THREADS);
    if (dtype_f64)
        hipLaunchKernelGGL(k_batch_field_absmax<double>, grid, block, 0, stream, (const double *)f, out, B, nrows, ncols,
                           pitch, mstride);
    else
        hipLaunchKernelGGL(k_batch_field_absmax<float>, grid, block, 0, stream, (const float *)f, out, B, nrows, ncols,
                           pitch, mstride);
}

void batch_eps_window_launch(void *ce, const void *w, bool dtype_f64, int B, int r0, int c0, int nr, int nc,
                             long long pitch, size_t mstride, double dt, double dx, hipStream_t stream)
{
    const size_t n = (size_t)B * nr * nc;
    const size_t want = (n + BATCH_DSG_THREADS - 1) / BATCH_DSG_THREADS;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(BATCH_DSG_THREADS);
    if (dtype_f64)
        hipLaunchKernelGGL(k_batch_eps_window<double>, grid, block, 0, stream, (double *)ce, (const double *)w, B, r0, c0,
                           nr, nc, pitch, mstride, dt, dx);
    else
        hipLaunchKernelGGL(k_batch_eps_window<float>, grid, block, 0, stream, (float *)ce, (const float *)w, B, r0, c0,
                           nr, nc, pitch, mstride, (float)dt, (float)dx);
}

}  // namespace fdtd
