// The instantiations of the dispersive batch kernels and the launch of the strength window kernel
// (include/fdtd2d_batch_dispersive.h, kernels_batch_dispersive.hpp), in a translation unit of their own: they compile
// beside batch.hip, batch_monitor.hip, batch_adjoint.hip, batch_design.hip, batch_lossy.hip and batch_periodic.hip,
// whose kernels keep their code.
#include "kernels_batch_dispersive.hpp"

namespace fdtd {

void batch_wp2_window_launch(void *cj, const double *w, const double *bq, bool dtype_f64, int B, int r0, int c0, int nr,
                             int nc, long long pitch, size_t mstride, double dx, double eps0, hipStream_t stream)
{
    const size_t n = (size_t)B * nr * nc;
    const size_t want = (n + 255) / 256;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(256);
    if (dtype_f64)
        hipLaunchKernelGGL(k_batch_wp2_window<double>, grid, block, 0, stream, (double *)cj, w, bq, B, r0, c0, nr, nc,
                           pitch, mstride, dx, eps0);
    else
        hipLaunchKernelGGL(k_batch_wp2_window<float>, grid, block, 0, stream, (float *)cj, w, bq, B, r0, c0, nr, nc,
                           pitch, mstride, dx, eps0);
}

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchDispersiveKernels &batch_dispersive_kernels()
{
    static const BatchDispersiveKernels k = {
        FDTD2D_STUB(k_batch_resident_pml_dispersive<T, 4>),
        FDTD2D_STUB(k_batch_resident_periodic_dispersive<T, 4>),
        FDTD2D_STUB(k_batch_e_pml_dispersive<T>),
        FDTD2D_STUB(k_batch_e_periodic_dispersive<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchDispersiveKernels &batch_dispersive_kernels<float>();
template const BatchDispersiveKernels &batch_dispersive_kernels<double>();

}  // namespace fdtd
