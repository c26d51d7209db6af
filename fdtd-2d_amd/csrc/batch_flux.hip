// The instantiations of the flux-line batch kernels and the launch of the flux kernel (include/fdtd2d_batch_flux.h,
// kernels_batch_flux.hpp), in a translation unit of their own: they compile beside batch.hip, batch_monitor.hip,
// batch_adjoint.hip, batch_lossy.hip, batch_periodic.hip and batch_dispersive.hip, whose kernels keep their code.
#include "kernels_batch_flux.hpp"

namespace fdtd {

// ---- the flux -----------------------------------------------------------------------------------------------------
// One workgroup per member; thread t < nl * nff forms P of line t / nff at frequency t % nff: the cells in ascending
// order, s = 0.0; s = s + (er * xr + ei * xi) with x = H (gc + i gs), g = exp(+i omega dt / 2); P = sign * dx * s.
// out: count x nl x nff.
__global__ __launch_bounds__(64) void k_batch_flux(BatchFlux f, double *__restrict__ out, int B, double dt, double dx)
{
    const int t = threadIdx.x;
    if (t >= f.nl * f.nff) return;
    const int line = t / f.nff, q = t - line * f.nff;
    int off = 0, cnt = 0, col = 0;
#pragma unroll
    for (int k = 0; k < BATCH_FLUX_MAX_LINES; ++k)
        if (k == line) {
            off = f.offset[k];
            cnt = f.count[k];
            col = f.orient[k];
        }
    const size_t W = (size_t)f.cells;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const double half = f.omega[(size_t)b * f.nff + q] * dt * 0.5;
        const double gc = cos(half), gs = sin(half);
        const double *a = f.member_acc(b);
        const double *er = a + (size_t)q * W + off, *ei = a + (size_t)(f.nff + q) * W + off;
        const double *hr = a + (size_t)(2 * f.nff + q) * W + off, *hi = a + (size_t)(3 * f.nff + q) * W + off;
        double s = 0.0;
        for (int c = 0; c < cnt; ++c) {
            const double xr = hr[c] * gc - hi[c] * gs, xi = hr[c] * gs + hi[c] * gc;
            s = s + (er[c] * xr + ei[c] * xi);
        }
        out[((size_t)b * f.nl + line) * f.nff + q] = (col ? -1.0 : 1.0) * dx * s;
    }
}

void batch_flux_launch(const BatchFlux &f, double *out, int B, double dt, double dx, hipStream_t stream)
{
    hipLaunchKernelGGL(k_batch_flux, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(64), 0, stream, f, out, B, dt, dx);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchFluxKernels &batch_flux_kernels()
{
    static const BatchFluxKernels k = {
        {{FDTD2D_STUB(k_batch_resident_flux<T, 4, false, false>), FDTD2D_STUB(k_batch_resident_flux<T, 8, false, false>),
          FDTD2D_STUB(k_batch_resident_flux<T, 16, false, false>)},
         {FDTD2D_STUB(k_batch_resident_flux<T, 4, true, false>), FDTD2D_STUB(k_batch_resident_flux<T, 8, true, false>),
          FDTD2D_STUB(k_batch_resident_flux<T, 16, true, false>)}},
        {FDTD2D_STUB(k_batch_resident_flux<T, 4, false, true>), FDTD2D_STUB(k_batch_resident_flux<T, 4, true, true>)},
        {FDTD2D_STUB(k_batch_h_flux<T, false>), FDTD2D_STUB(k_batch_h_flux<T, true>)},
        {{FDTD2D_STUB(k_batch_e_flux<T, false, false>), FDTD2D_STUB(k_batch_e_flux<T, false, true>)},
         {FDTD2D_STUB(k_batch_e_flux<T, true, false>), FDTD2D_STUB(k_batch_e_flux<T, true, true>)}},
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchFluxKernels &batch_flux_kernels<float>();
template const BatchFluxKernels &batch_flux_kernels<double>();

}  // namespace fdtd
