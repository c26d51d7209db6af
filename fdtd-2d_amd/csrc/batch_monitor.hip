// The monitored instantiations of the batch kernels (include/fdtd2d_batch_monitor.h, kernels_batch_monitor.hpp), in a
// translation unit of their own: they compile beside batch.hip, whose unmonitored kernels keep their code.
#include "kernels_batch_monitor.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchMonKernels &batch_mon_kernels()
{
    static const BatchMonKernels k = {
        {{FDTD2D_STUB(k_batch_resident_mon<T, false, 4>), FDTD2D_STUB(k_batch_resident_mon<T, false, 8>),
          FDTD2D_STUB(k_batch_resident_mon<T, false, 16>)},
         {FDTD2D_STUB(k_batch_resident_mon<T, true, 4>), FDTD2D_STUB(k_batch_resident_mon<T, true, 8>),
          FDTD2D_STUB(k_batch_resident_mon<T, true, 16>)}},
        {{FDTD2D_STUB(k_batch_resident_pml_mon<T, false, 4>), FDTD2D_STUB(k_batch_resident_pml_mon<T, false, 8>),
          FDTD2D_STUB(k_batch_resident_pml_mon<T, false, 16>)},
         {FDTD2D_STUB(k_batch_resident_pml_mon<T, true, 4>), FDTD2D_STUB(k_batch_resident_pml_mon<T, true, 8>),
          FDTD2D_STUB(k_batch_resident_pml_mon<T, true, 16>)}},
        {FDTD2D_STUB(k_batch_h_mon<T, false>), FDTD2D_STUB(k_batch_h_mon<T, true>)},
        {FDTD2D_STUB(k_batch_e_mon<T, false>), FDTD2D_STUB(k_batch_e_mon<T, true>)},
        {FDTD2D_STUB(k_batch_h_pml_mon<T, false>), FDTD2D_STUB(k_batch_h_pml_mon<T, true>)},
        {FDTD2D_STUB(k_batch_e_pml_mon<T, false>), FDTD2D_STUB(k_batch_e_pml_mon<T, true>)},
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchMonKernels &batch_mon_kernels<float>();
template const BatchMonKernels &batch_mon_kernels<double>();

}  // namespace fdtd
