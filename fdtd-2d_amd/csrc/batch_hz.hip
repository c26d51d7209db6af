// The instantiations of the Hz-polarisation batch kernels (include/fdtd2d_batch_hz.h, kernels_batch_hz.hpp), in a
// translation unit of their own: they compile beside batch.hip and the other batch_*.hip, whose kernels keep their code.
#include "kernels_batch_hz.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchHzKernels &batch_hz_kernels()
{
    static const BatchHzKernels k = {
        {{{FDTD2D_STUB(k_batch_resident_hz<T, false, false, 4>), FDTD2D_STUB(k_batch_resident_hz<T, false, false, 8>)},
          {FDTD2D_STUB(k_batch_resident_hz<T, false, true, 4>), nullptr}},
         {{FDTD2D_STUB(k_batch_resident_hz<T, true, false, 4>), FDTD2D_STUB(k_batch_resident_hz<T, true, false, 8>)},
          {FDTD2D_STUB(k_batch_resident_hz<T, true, true, 4>), nullptr}}},
        {{FDTD2D_STUB(k_batch_e_hz<T, false, false>), FDTD2D_STUB(k_batch_e_hz<T, false, true>)},
         {FDTD2D_STUB(k_batch_e_hz<T, true, false>), FDTD2D_STUB(k_batch_e_hz<T, true, true>)}},
        {FDTD2D_STUB(k_batch_h_hz<T, false>), FDTD2D_STUB(k_batch_h_hz<T, true>)},
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchHzKernels &batch_hz_kernels<float>();
template const BatchHzKernels &batch_hz_kernels<double>();

}  // namespace fdtd
