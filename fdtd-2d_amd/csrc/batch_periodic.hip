// The instantiations of the periodic batch kernels (include/fdtd2d_batch_periodic.h, kernels_batch_periodic.hpp), in a
// translation unit of their own: they compile beside batch.hip, batch_monitor.hip, batch_adjoint.hip, batch_design.hip
// and batch_lossy.hip, whose kernels keep their code.
#include "kernels_batch_periodic.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchPeriodicKernels &batch_periodic_kernels()
{
    static const BatchPeriodicKernels k = {
        {FDTD2D_STUB(k_batch_resident_periodic<T, 4>), FDTD2D_STUB(k_batch_resident_periodic<T, 8>),
         FDTD2D_STUB(k_batch_resident_periodic<T, 16>)},
        FDTD2D_STUB(k_batch_h_periodic<T>),
        FDTD2D_STUB(k_batch_e_periodic<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchPeriodicKernels &batch_periodic_kernels<float>();
template const BatchPeriodicKernels &batch_periodic_kernels<double>();

}  // namespace fdtd
