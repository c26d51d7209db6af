// The point-source instantiations of the Bloch batch kernels and the product of two complex windows
// (include/fdtd2d_batch_bloch_adjoint.h, kernels_batch_bloch_adjoint.hpp), in a translation unit of their own beside
// batch_bloch.hip and batch_adjoint.hip, whose kernels keep their code.
#include "kernels_batch_bloch_adjoint.hpp"

namespace fdtd {

// the held complex window times the current one (fdtd2d_batch_bloch_window_product):
// out[b][w] = sum_k Re(coef * H * E), H = a + i b the held window, E the current one, a = W(re) and b = W(im) each an
// accumulator pair.  Every window: per member re[nf][W] then im[nf][W]; coef: count x nf x {re, im}.
// grid (ceil(W / 256), min(B, 65535)).  The fused build writes its fma out, so that each build defines one order.
__global__ __launch_bounds__(256) void k_batch_bloch_window_product(const double *__restrict__ held_re,
                                                                    const double *__restrict__ held_im,
                                                                    const double *__restrict__ cur_re,
                                                                    const double *__restrict__ cur_im,
                                                                    const double *__restrict__ coef,
                                                                    double *__restrict__ out, int B, int nf, size_t W)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const size_t o = (size_t)b * 2 * nf * W;
        const double *ha = held_re + o, *hb = held_im + o, *ca = cur_re + o, *cb = cur_im + o;
        double s = 0.0;
        for (int k = 0; k < nf; ++k) {
            const size_t r = (size_t)k * W + w, i = (size_t)(nf + k) * W + w;
            const double hr = ha[r] - hb[i], hi = ha[i] + hb[r];
            const double cr = ca[r] - cb[i], ci = ca[i] + cb[r];
            const double kr = coef[((size_t)b * nf + k) * 2], ki = coef[((size_t)b * nf + k) * 2 + 1];
#ifdef FDTD2D_FUSED
            const double tr = __builtin_fma(hr, cr, -(hi * ci)), ti = __builtin_fma(hr, ci, hi * cr);
            s = s + __builtin_fma(kr, tr, -(ki * ti));
#else
            const double tr = hr * cr - hi * ci, ti = hr * ci + hi * cr;
            s = s + (kr * tr - ki * ti);
#endif
        }
        out[(size_t)b * W + w] = s;
    }
}

void batch_bloch_window_product_launch(const double *held_re, const double *held_im, const double *cur_re,
                                       const double *cur_im, const double *coef, double *out, int B, int nf, size_t W,
                                       hipStream_t stream)
{
    const dim3 grid((unsigned)((W + 255) / 256), B < 65535 ? B : 65535);
    hipLaunchKernelGGL(k_batch_bloch_window_product, grid, dim3(256), 0, stream, held_re, held_im, cur_re, cur_im, coef,
                       out, B, nf, W);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

// 4 cells per thread alone, as batch_bloch.hip explains
template <class T> const BatchBlochKernels &batch_bloch_pts_kernels()
{
    static const BatchBlochKernels k = {
        FDTD2D_STUB(k_batch_resident_bloch_pts<T, 4>),
        FDTD2D_STUB(k_batch_h_bloch_pts<T>),
        FDTD2D_STUB(k_batch_e_bloch_pts<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchBlochKernels &batch_bloch_pts_kernels<float>();
template const BatchBlochKernels &batch_bloch_pts_kernels<double>();

}  // namespace fdtd
