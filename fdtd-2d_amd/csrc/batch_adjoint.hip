// The point-source instantiations of the monitored batch kernels and the window product kernel
// (include/fdtd2d_batch_adjoint.h, kernels_batch_adjoint.hpp), in a translation unit of their own: they compile beside
// batch.hip and batch_monitor.hip, whose kernels keep their code.
#include "kernels_batch_adjoint.hpp"

namespace fdtd {

// the held window times the current one (fdtd2d_batch_dft_window_product): out[b][w] = sum_k Re(coef * held * cur).
// held, cur: per member re[nf][W] then im[nf][W]; coef: count x nf x {re, im}.  grid (ceil(W / 256), min(B, 65535)).
__global__ __launch_bounds__(256) void k_batch_window_product(const double *__restrict__ held,
                                                              const double *__restrict__ cur,
                                                              const double *__restrict__ coef,
                                                              double *__restrict__ out, int B, int nf, size_t W)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const double *h = held + (size_t)b * 2 * nf * W, *c = cur + (size_t)b * 2 * nf * W;
        double s = 0.0;
        for (int k = 0; k < nf; ++k) {
            const double hr = h[(size_t)k * W + w], hi = h[(size_t)(nf + k) * W + w];
            const double cr = c[(size_t)k * W + w], ci = c[(size_t)(nf + k) * W + w];
            const double tr = hr * cr - hi * ci, ti = hr * ci + hi * cr;
            s = s + (coef[((size_t)b * nf + k) * 2] * tr - coef[((size_t)b * nf + k) * 2 + 1] * ti);
        }
        out[(size_t)b * W + w] = s;
    }
}

void batch_window_product_launch(const double *held, const double *cur, const double *coef, double *out, int B, int nf,
                                 size_t W, hipStream_t stream)
{
    const dim3 grid((unsigned)((W + 255) / 256), B < 65535 ? B : 65535);
    hipLaunchKernelGGL(k_batch_window_product, grid, dim3(256), 0, stream, held, cur, coef, out, B, nf, W);
}

// k_batch_window_product for up to three coefficient sets (fdtd2d_batch_dispersive_window_product): every pair of
// window values is read once and feeds all ncoef sums, so the eps, sigma and wp2 gradients of a dispersive batch cost one
// pass over the two windows.  out[c][b][w] = scale[b][c] * sum_k Re(coef[c][b][k] * held * cur), each sum with the
// operations and the order of k_batch_window_product: with one set and scale 1 it writes that kernel's bits.
// coef: ncoef x count x nf x {re, im}; scale: count x ncoef; out: ncoef x count x W.  The set loop is unrolled over its
// three slots with a uniform bound, so the sums stay in registers (no scratch).  Same grid.
__global__ __launch_bounds__(256) void k_batch_window_product_multi(const double *__restrict__ held,
                                                                    const double *__restrict__ cur,
                                                                    const double *__restrict__ coef,
                                                                    const double *__restrict__ scale,
                                                                    double *__restrict__ out, int B, int nf, size_t W,
                                                                    int ncoef)
{
    constexpr int MAXSETS = 3;
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const double *h = held + (size_t)b * 2 * nf * W, *c = cur + (size_t)b * 2 * nf * W;
        double s[MAXSETS] = {0.0, 0.0, 0.0};
        for (int k = 0; k < nf; ++k) {
            const double hr = h[(size_t)k * W + w], hi = h[(size_t)(nf + k) * W + w];
            const double cr = c[(size_t)k * W + w], ci = c[(size_t)(nf + k) * W + w];
            const double tr = hr * cr - hi * ci, ti = hr * ci + hi * cr;
#pragma unroll
            for (int q = 0; q < MAXSETS; ++q) {
                if (q < ncoef) {
                    const double *kq = coef + (((size_t)q * B + b) * nf + k) * 2;
                    s[q] = s[q] + (kq[0] * tr - kq[1] * ti);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < MAXSETS; ++q)
            if (q < ncoef) out[((size_t)q * B + b) * W + w] = scale[(size_t)b * ncoef + q] * s[q];
    }
}

void batch_window_product_multi_launch(const double *held, const double *cur, const double *coef, const double *scale,
                                       double *out, int B, int nf, size_t W, int ncoef, hipStream_t stream)
{
    const dim3 grid((unsigned)((W + 255) / 256), B < 65535 ? B : 65535);
    hipLaunchKernelGGL(k_batch_window_product_multi, grid, dim3(256), 0, stream, held, cur, coef, scale, out, B, nf, W,
                       ncoef);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchMonKernels &batch_pts_kernels()
{
    static const BatchMonKernels k = {
        {{FDTD2D_STUB(k_batch_resident_mon_pts<T, false, 4>), FDTD2D_STUB(k_batch_resident_mon_pts<T, false, 8>),
          FDTD2D_STUB(k_batch_resident_mon_pts<T, false, 16>)},
         {FDTD2D_STUB(k_batch_resident_mon_pts<T, true, 4>), FDTD2D_STUB(k_batch_resident_mon_pts<T, true, 8>),
          FDTD2D_STUB(k_batch_resident_mon_pts<T, true, 16>)}},
        {{FDTD2D_STUB(k_batch_resident_pml_mon_pts<T, false, 4>), FDTD2D_STUB(k_batch_resident_pml_mon_pts<T, false, 8>),
          FDTD2D_STUB(k_batch_resident_pml_mon_pts<T, false, 16>)},
         {FDTD2D_STUB(k_batch_resident_pml_mon_pts<T, true, 4>), FDTD2D_STUB(k_batch_resident_pml_mon_pts<T, true, 8>),
          FDTD2D_STUB(k_batch_resident_pml_mon_pts<T, true, 16>)}},
        {FDTD2D_STUB(k_batch_h_mon_pts<T, false>), FDTD2D_STUB(k_batch_h_mon_pts<T, true>)},
        {FDTD2D_STUB(k_batch_e_mon_pts<T, false>), FDTD2D_STUB(k_batch_e_mon_pts<T, true>)},
        {FDTD2D_STUB(k_batch_h_pml_mon_pts<T, false>), FDTD2D_STUB(k_batch_h_pml_mon_pts<T, true>)},
        {FDTD2D_STUB(k_batch_e_pml_mon_pts<T, false>), FDTD2D_STUB(k_batch_e_pml_mon_pts<T, true>)},
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchMonKernels &batch_pts_kernels<float>();
template const BatchMonKernels &batch_pts_kernels<double>();

}  // namespace fdtd
