// The instantiations of the lossy batch kernels and the launch of the conductivity window kernel
// (include/fdtd2d_batch_lossy.h, kernels_batch_lossy.hpp), in a translation unit of their own: they compile beside
// batch.hip, batch_monitor.hip, batch_adjoint.hip and batch_design.hip, whose kernels keep their code.
#include "kernels_batch_lossy.hpp"

namespace fdtd {

void batch_sigma_window_launch(void *ca, void *cb, const void *ce, const double *w, bool dtype_f64, int B, int r0,
                               int c0, int nr, int nc, long long pitch, size_t mstride, double dt, hipStream_t stream)
{
    const size_t n = (size_t)B * nr * nc;
    const size_t want = (n + 255) / 256;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(256);
    if (dtype_f64)
        hipLaunchKernelGGL(k_batch_sigma_window<double>, grid, block, 0, stream, (double *)ca, (double *)cb,
                           (const double *)ce, w, B, r0, c0, nr, nc, pitch, mstride, dt);
    else
        hipLaunchKernelGGL(k_batch_sigma_window<float>, grid, block, 0, stream, (float *)ca, (float *)cb,
                           (const float *)ce, w, B, r0, c0, nr, nc, pitch, mstride, dt);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchLossyKernels &batch_lossy_kernels()
{
    static const BatchLossyKernels k = {
        {FDTD2D_STUB(k_batch_resident_lossy<T, 4>), FDTD2D_STUB(k_batch_resident_lossy<T, 8>),
         FDTD2D_STUB(k_batch_resident_lossy<T, 16>)},
        {FDTD2D_STUB(k_batch_resident_pml_lossy<T, 4>), FDTD2D_STUB(k_batch_resident_pml_lossy<T, 8>),
         FDTD2D_STUB(k_batch_resident_pml_lossy<T, 16>)},
        FDTD2D_STUB(k_batch_e_lossy<T>),
        FDTD2D_STUB(k_batch_e_pml_lossy<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchLossyKernels &batch_lossy_kernels<float>();
template const BatchLossyKernels &batch_lossy_kernels<double>();

}  // namespace fdtd
