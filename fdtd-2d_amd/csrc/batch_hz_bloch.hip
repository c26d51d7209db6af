// The instantiations of the Hz-polarisation Bloch batch kernels (include/fdtd2d_batch_hz_bloch.h,
// kernels_batch_hz_bloch.hpp), in a translation unit of their own: they compile beside batch.hip and the other
// batch_*.hip, whose kernels keep their code.
#include "kernels_batch_hz_bloch.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

template <class T> const BatchHzBlochKernels &batch_hz_bloch_kernels()
{
    static const BatchHzBlochKernels k = {
        {FDTD2D_STUB(k_batch_resident_hz_bloch<T, false, 4>), FDTD2D_STUB(k_batch_resident_hz_bloch<T, true, 4>)},
        {FDTD2D_STUB(k_batch_e_hz_bloch<T, false>), FDTD2D_STUB(k_batch_e_hz_bloch<T, true>)},
        FDTD2D_STUB(k_batch_h_hz_bloch<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchHzBlochKernels &batch_hz_bloch_kernels<float>();
template const BatchHzBlochKernels &batch_hz_bloch_kernels<double>();

}  // namespace fdtd
