// The instantiations of the Bloch batch kernels (include/fdtd2d_batch_bloch.h, kernels_batch_bloch.hpp), in a
// translation unit of their own beside batch_periodic.hip: the periodic kernels keep their code.
#include "kernels_batch_bloch.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

// The resident kernel exists for 4 cells per thread alone: 11 arrays of a member must fit BATCH_LDS_LIMIT, which admits
// fewer than 163840 / 11 / 4 = 3724 float32 (1862 float64) cells, and resident_threads gives such a member at least a
// quarter of its cells in threads (1024 threads from 3073 cells on).  The 8- and 16-cell walks could never run.
template <class T> const BatchBlochKernels &batch_bloch_kernels()
{
    static const BatchBlochKernels k = {
        FDTD2D_STUB(k_batch_resident_bloch<T, 4>),
        FDTD2D_STUB(k_batch_h_bloch<T>),
        FDTD2D_STUB(k_batch_e_bloch<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchBlochKernels &batch_bloch_kernels<float>();
template const BatchBlochKernels &batch_bloch_kernels<double>();

}  // namespace fdtd
