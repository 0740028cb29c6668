// The inputs of the forward transforms that are pointwise products of the grid-point fields u, v, T, q of the dynamics' time
// level (tendencies.f90:247-266): the meridional / zonal fluxes of temperature and tracer and the kinetic energy.  ONE
// definition for the two places that form them: the stand-alone dynamics kernel (dyn_column.hpp, STORE_ALL), which stores them,
// and the product mode of the grid -> spectral transform (transforms.hip), which forms them from the four source fields while it
// stages the rows, so that the model step never writes them.  The same source expressions under -ffp-contract=on contract the
// same way in both kernels (the kinetic energy is one fma and one multiply), so the two give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace spd {

// FieldDesc::mode of a grid -> spectral entry: low byte = which product of (src, src2), bits 8.. = the level (for tref)
constexpr int kProdNone = 0;   // transform src as it is
constexpr int kProdFluxT = 1;  // -src * (src2 - tref_k): wind times temperature anomaly
constexpr int kProdFluxQ = 2;  // -src * src2: wind times tracer (the same expression with tref = 0: x - 0 is x, bit for bit)
constexpr int kProdKe = 3;     // 0.5 (src^2 + src2^2): kinetic energy of (u, v)
constexpr int kProdLevelShift = 8;

__device__ __forceinline__ double staged_product(int kind, double a, double b, double tref) {
    if (kind == kProdKe) return 0.5f * (a * a + b * b);
    const double anomaly = b - tref;  // (b itself where tref is 0)
    return -a * anomaly;
}

}  // namespace spd
