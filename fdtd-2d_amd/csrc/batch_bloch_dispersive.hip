// The instantiations of the dispersive Bloch and lattice batch kernels (include/fdtd2d_batch_bloch_dispersive.h,
// kernels_batch_bloch_dispersive.hpp), in a translation unit of their own beside batch_bloch.hip, batch_lattice.hip and
// batch_dispersive.hip, whose kernels keep their code.
#include "kernels_batch_bloch_dispersive.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

// 16 (Bloch) or 14 (lattice) arrays of a member must fit BATCH_LDS_LIMIT: fewer than 2560 / 2926 float32 cells, which
// resident_threads gives at least a quarter as many threads: 4 cells per thread is the only instance
template <class T> const BatchBlochDispersiveKernels &batch_bloch_dispersive_kernels()
{
    static const BatchBlochDispersiveKernels k = {
        FDTD2D_STUB(k_batch_resident_bloch_dispersive<T, 4>),
        FDTD2D_STUB(k_batch_resident_lattice_dispersive<T, 4>),
        FDTD2D_STUB(k_batch_e_bloch_dispersive<T>),
        FDTD2D_STUB(k_batch_e_lattice_dispersive<T>),
    };
    return k;
}

#undef FDTD2D_STUB

template const BatchBlochDispersiveKernels &batch_bloch_dispersive_kernels<float>();
template const BatchBlochDispersiveKernels &batch_bloch_dispersive_kernels<double>();

}  // namespace fdtd
