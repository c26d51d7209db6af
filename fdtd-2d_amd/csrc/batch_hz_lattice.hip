// The instantiations of the Hz lattice batch kernels (include/fdtd2d_batch_hz_lattice.h, kernels_batch_hz_lattice.hpp),
// in a translation unit of their own beside batch_lattice.hip and batch_hz_bloch.hip, whose kernels keep their code.
#include "kernels_batch_hz_lattice.hpp"

namespace fdtd {

#define FDTD2D_STUB(...) reinterpret_cast<const void *>(&__VA_ARGS__)

// 9 arrays of a member must fit BATCH_LDS_LIMIT, which admits fewer than 163840 / 9 / 4 = 4552 float32 (2276 float64)
// cells; 18 arrays with a pole admit fewer than 2276 float32 (1138 float64) cells.  resident_threads gives a member at
// least a quarter of its cells in threads up to 1024 of them, so only a float32 member without a pole above 4096 cells
// has 5 cells per thread and every other member at most 4.
template <> const BatchHzLatticeKernels &batch_hz_lattice_kernels<float>()
{
    static const BatchHzLatticeKernels k = {
        {{FDTD2D_STUB(k_batch_resident_hz_lattice<float, false, 4>), FDTD2D_STUB(k_batch_resident_hz_lattice<float, false, 5>)},
         {FDTD2D_STUB(k_batch_resident_hz_lattice<float, true, 4>), nullptr}},
        {FDTD2D_STUB(k_batch_e_hz_lattice<float, false>), FDTD2D_STUB(k_batch_e_hz_lattice<float, true>)},
        FDTD2D_STUB(k_batch_h_hz_lattice<float>),
    };
    return k;
}

template <> const BatchHzLatticeKernels &batch_hz_lattice_kernels<double>()
{
    static const BatchHzLatticeKernels k = {
        {{FDTD2D_STUB(k_batch_resident_hz_lattice<double, false, 4>), nullptr},
         {FDTD2D_STUB(k_batch_resident_hz_lattice<double, true, 4>), nullptr}},
        {FDTD2D_STUB(k_batch_e_hz_lattice<double, false>), FDTD2D_STUB(k_batch_e_hz_lattice<double, true>)},
        FDTD2D_STUB(k_batch_h_hz_lattice<double>),
    };
    return k;
}

#undef FDTD2D_STUB

}  // namespace fdtd
