// The instantiations of the line-source kernels of a Bloch batch and the kernel that forms the adjoint weights of a flux
// objective from the complex lines' sums (include/fdtd2d_batch_bloch_flux_adjoint.h,
// kernels_batch_bloch_flux_adjoint.hpp), in a translation unit of their own: they compile beside batch_bloch_flux.hip and
// batch_flux_adjoint.hip, whose kernels keep their code.
#include "kernels_batch_bloch_flux_adjoint.hpp"

namespace fdtd {

// ---- the weights ----------------------------------------------------------------------------------------------------
// k_batch_flux_line_weights on the sums of both parts.  One workgroup per member; a thread forms one weight: part (0: we
// from H, 1: wh from E), entry w, channel c.  The raw sum the part reads is X = (ar_re - ai_im) + i (ar_im + ai_re) with
// ar / ai the sums of the real / imaginary part of the field, as k_batch_bloch_flux forms it; then, with
// g = exp(+i omega dt / 2) and cf = scale[w] * (dJdP[line][k] * (sign * dx)):
//     x = X g;  tr = cf * xr;  ti = -(cf * xi);  s = 0.0;  s = s + solve[c][k] * tr (k ascending);
//     then s = s + solve[c][nff + k] * ti (k ascending)
__global__ __launch_bounds__(256) void k_batch_bloch_flux_line_weights(BatchFlux f, const double *__restrict__ facc_im,
                                                                       BatchFluxWeights W, int B, double dt, double dx)
{
    const int K = 2 * f.nff, per = f.cells * K;
    const size_t Wd = (size_t)f.cells;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const double *a = f.member_acc(b), *ai = facc_im + (size_t)b * f.member_size();
        const double *sol = W.solve + (size_t)b * (size_t)W.solve_mstride;
        for (int t = threadIdx.x; t < 2 * per; t += blockDim.x) {
            const int part = t / per, r = t - part * per, w = r / K, c = r - w * K;
            int line = 0, col = 0;
#pragma unroll
            for (int k = 0; k < BATCH_FLUX_MAX_LINES; ++k)
                if (k < f.nl && w >= f.offset[k] && w < f.offset[k] + f.count[k]) {
                    line = k;
                    col = f.orient[k];
                }
            const double *scale = part ? W.scale_h : W.scale_e;
            const double sc = scale ? scale[(size_t)b * Wd + w] : 1.0;
            const double sdx = (col ? -1.0 : 1.0) * dx;
            const int re0 = part ? 0 : 2 * f.nff;     // E: blocks 0, nff; H: blocks 2 nff, 3 nff
            double s = 0.0;
            for (int pass = 0; pass < 2; ++pass)
                for (int k = 0; k < f.nff; ++k) {
                    const double half = f.omega[(size_t)b * f.nff + k] * dt * 0.5;
                    const double gc = cos(half), gs = sin(half);
                    const size_t ore = (size_t)(re0 + k) * Wd + w, oim = (size_t)(re0 + f.nff + k) * Wd + w;
                    const double xr0 = a[ore] - ai[oim], xi0 = a[oim] + ai[ore];
                    const double xr = xr0 * gc - xi0 * gs, xi = xr0 * gs + xi0 * gc;
                    const double cf = sc * (W.dJdP[((size_t)b * f.nl + line) * f.nff + k] * sdx);
                    if (pass == 0) s = s + sol[(size_t)c * K + k] * (cf * xr);
                    else s = s + sol[(size_t)c * K + f.nff + k] * (-(cf * xi));
                }
            (part ? W.wh : W.we)[((size_t)b * Wd + w) * K + c] = s;
        }
    }
}

void batch_bloch_flux_line_weights_launch(const BatchFlux &f, const double *facc_im, const BatchFluxWeights &W, int B,
                                          double dt, double dx, hipStream_t stream)
{
    hipLaunchKernelGGL(k_batch_bloch_flux_line_weights, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, stream, f,
                       facc_im, W, B, dt, dx);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchBlochFluxKernels &batch_bloch_flux_src_kernels()
{
    static const BatchBlochFluxKernels k = {
        {FDTD2D_STUB(k_batch_resident_bloch_flux_src<T, false>), FDTD2D_STUB(k_batch_resident_bloch_flux_src<T, true>)},
        FDTD2D_STUB(k_batch_h_bloch_flux_src<T>),
        {FDTD2D_STUB(k_batch_e_bloch_flux_src<T, false>), FDTD2D_STUB(k_batch_e_bloch_flux_src<T, true>)},
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchBlochFluxKernels &batch_bloch_flux_src_kernels<float>();
template const BatchBlochFluxKernels &batch_bloch_flux_src_kernels<double>();

}  // namespace fdtd
