// The instantiations of the flux-line kernels of the Hz polarisation and the launch of their flux kernel
// (include/fdtd2d_batch_hz_flux.h, kernels_batch_hz_flux.hpp), in a translation unit of their own: they compile beside
// batch.hip and the other batch_*.hip, whose kernels keep their code.
#include "kernels_batch_hz_flux.hpp"

namespace fdtd {

// ---- the flux -----------------------------------------------------------------------------------------------------
// k_batch_flux (batch_flux.hip) with the signs of the Hz polarisation, S_y = -Ex Hz and S_x = Ey Hz: one workgroup per
// member; thread t < nl * nff forms P of line t / nff at frequency t % nff: the cells in ascending order, s = 0.0;
// s = s + (hr * xr + hi * xi) with h = the transform of Hz, x = Et (gc + i gs), g = exp(+i omega dt / 2);
// P = sign * dx * s, sign = -1 for a row line and +1 for a column line.  out: count x nl x nff.
__global__ __launch_bounds__(64) void k_batch_hz_flux(BatchFlux f, double *__restrict__ out, int B, double dt, double dx)
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
        const double *hr = a + (size_t)q * W + off, *hi = a + (size_t)(f.nff + q) * W + off;
        const double *er = a + (size_t)(2 * f.nff + q) * W + off, *ei = a + (size_t)(3 * f.nff + q) * W + off;
        double s = 0.0;
        for (int c = 0; c < cnt; ++c) {
            const double xr = er[c] * gc - ei[c] * gs, xi = er[c] * gs + ei[c] * gc;
            s = s + (hr[c] * xr + hi[c] * xi);
        }
        out[((size_t)b * f.nl + line) * f.nff + q] = (col ? 1.0 : -1.0) * dx * s;
    }
}

void batch_hz_flux_launch(const BatchFlux &f, double *out, int B, double dt, double dx, hipStream_t stream)
{
    hipLaunchKernelGGL(k_batch_hz_flux, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(64), 0, stream, f, out, B, dt, dx);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchHzFluxKernels &batch_hz_flux_kernels()
{
    static const BatchHzFluxKernels k = {
        {{{FDTD2D_STUB(k_batch_resident_hz_flux<T, false, false, 4>),
           FDTD2D_STUB(k_batch_resident_hz_flux<T, false, false, 8>)},
          {FDTD2D_STUB(k_batch_resident_hz_flux<T, false, true, 4>), nullptr}},
         {{FDTD2D_STUB(k_batch_resident_hz_flux<T, true, false, 4>),
           FDTD2D_STUB(k_batch_resident_hz_flux<T, true, false, 8>)},
          {FDTD2D_STUB(k_batch_resident_hz_flux<T, true, true, 4>), nullptr}}},
        {{FDTD2D_STUB(k_batch_e_hz_flux<T, false, false>), FDTD2D_STUB(k_batch_e_hz_flux<T, false, true>)},
         {FDTD2D_STUB(k_batch_e_hz_flux<T, true, false>), FDTD2D_STUB(k_batch_e_hz_flux<T, true, true>)}},
        {FDTD2D_STUB(k_batch_h_hz_flux<T, false>), FDTD2D_STUB(k_batch_h_hz_flux<T, true>)},
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchHzFluxKernels &batch_hz_flux_kernels<float>();
template const BatchHzFluxKernels &batch_hz_flux_kernels<double>();

}  // namespace fdtd
