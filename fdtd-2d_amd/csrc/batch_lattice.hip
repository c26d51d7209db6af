// The instantiations of the lattice batch kernels (include/fdtd2d_batch_lattice.h, kernels_batch_lattice.hpp), in a
// translation unit of their own beside batch_bloch.hip: the periodic and the Bloch kernels keep their code.
#include "kernels_batch_lattice.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

// 9 arrays of a member must fit BATCH_LDS_LIMIT, which admits fewer than 163840 / 9 / 4 = 4552 float32 (2276 float64)
// cells.  resident_threads gives a member at least a quarter of its cells in threads up to 1024 of them, so a float32
// member above 4096 cells has 5 cells per thread and a float64 member never more than 4.
template <> const BatchLatticeKernels &batch_lattice_kernels<float>()
{
    static const BatchLatticeKernels k = {
        {FDTD2D_STUB(k_batch_resident_lattice<float, 4>), FDTD2D_STUB(k_batch_resident_lattice<float, 5>)},
        FDTD2D_STUB(k_batch_h_lattice<float>),
        FDTD2D_STUB(k_batch_e_lattice<float>),
    };
    return k;
}

template <> const BatchLatticeKernels &batch_lattice_kernels<double>()
{
    static const BatchLatticeKernels k = {
        {FDTD2D_STUB(k_batch_resident_lattice<double, 4>), nullptr},
        FDTD2D_STUB(k_batch_h_lattice<double>),
        FDTD2D_STUB(k_batch_e_lattice<double>),
    };
    return k;
}

#undef FDTD2D_STUB

}  // namespace fdtd
