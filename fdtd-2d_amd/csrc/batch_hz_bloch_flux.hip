// The instantiations of the flux-line kernels of an Hz Bloch batch and the launch of their flux kernel
// (include/fdtd2d_batch_hz_bloch_flux.h, kernels_batch_hz_bloch_flux.hpp), in a translation unit of their own: they
// compile beside batch_hz_bloch.hip, batch_hz_flux.hip and batch_bloch_flux.hip, whose kernels keep their code.
#include "kernels_batch_hz_bloch_flux.hpp"

namespace fdtd {

// ---- the flux -----------------------------------------------------------------------------------------------------
// k_batch_hz_flux on complex fields.  One workgroup per member; thread t < nl * nff forms P of line t / nff at frequency
// t % nff.  The transform of a complex field is the transform of its real part plus i times that of its imaginary part:
// H = (ar_re - ai_im) + i (ar_im + ai_re) with ar / ai the sums of the real / imaginary part, E likewise.  Then, the
// cells in ascending order, s = 0.0; s = s + (hr * xr + hi * xi) with x = E (gc + i gs), g = exp(+i omega dt / 2);
// P = sign * dx * s, sign = -1 for a row line and +1 for a column line.  out: count x nl x nff.
__global__ __launch_bounds__(64) void k_batch_hz_bloch_flux(BatchFlux f, const double *__restrict__ facc_im,
                                                            double *__restrict__ out, int B, double dt, double dx)
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
    const size_t ohr = (size_t)q * W + off, ohi = (size_t)(f.nff + q) * W + off;
    const size_t oer = (size_t)(2 * f.nff + q) * W + off, oei = (size_t)(3 * f.nff + q) * W + off;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const double half = f.omega[(size_t)b * f.nff + q] * dt * 0.5;
        const double gc = cos(half), gs = sin(half);
        const double *a = f.member_acc(b), *ai = facc_im + (size_t)b * f.member_size();
        double s = 0.0;
        for (int c = 0; c < cnt; ++c) {
            const double hr = a[ohr + c] - ai[ohi + c], hi = a[ohi + c] + ai[ohr + c];
            const double er = a[oer + c] - ai[oei + c], ei = a[oei + c] + ai[oer + c];
            const double xr = er * gc - ei * gs, xi = er * gs + ei * gc;
            s = s + (hr * xr + hi * xi);
        }
        out[((size_t)b * f.nl + line) * f.nff + q] = (col ? 1.0 : -1.0) * dx * s;
    }
}

void batch_hz_bloch_flux_launch(const BatchFlux &f, const double *facc_im, double *out, int B, double dt, double dx,
                                hipStream_t stream)
{
    hipLaunchKernelGGL(k_batch_hz_bloch_flux, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(64), 0, stream, f, facc_im,
                       out, B, dt, dx);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchHzBlochFluxKernels &batch_hz_bloch_flux_kernels()
{
    static const BatchHzBlochFluxKernels k = {
        {FDTD2D_STUB(k_batch_resident_hz_bloch_flux<T, false>), FDTD2D_STUB(k_batch_resident_hz_bloch_flux<T, true>)},
        {FDTD2D_STUB(k_batch_e_hz_bloch_flux<T, false>), FDTD2D_STUB(k_batch_e_hz_bloch_flux<T, true>)},
        FDTD2D_STUB(k_batch_h_hz_bloch_flux<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchHzBlochFluxKernels &batch_hz_bloch_flux_kernels<float>();
template const BatchHzBlochFluxKernels &batch_hz_bloch_flux_kernels<double>();

}  // namespace fdtd
