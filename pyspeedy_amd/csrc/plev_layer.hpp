// The layer search and weight of the pressure-level interpolation, shared by plev_kernel (plev.hip) and
// derive_kernel (derive.hip): s = ln(p_j / ps) against the compile-time sigl, the layer's reciprocal thickness a compile-time
// constant, and the eight levels of a column picked by unrolled selects (a runtime index into them would put them in scratch).
#pragma once
#include <hip/hip_runtime.h>

#include "tables.hpp"
#include "vertical_consts.hpp"

namespace spd {
namespace plevl {

struct LayerRecip {
    double r[KX - 1];
    constexpr LayerRecip() : r{} {
        for (int k = 0; k < KX - 1; ++k) r[k] = 1.0 / (vc::sigl[k + 1] - vc::sigl[k]);
    }
};
inline constexpr LayerRecip kRecip{};

__device__ __forceinline__ void load8(double (&x)[KX], const double *__restrict__ base) {
#pragma unroll
    for (int k = 0; k < KX; ++k) x[k] = base[static_cast<long>(k) * (IX * IL)];
}

// where s lies: ge[k]: s >= sigl[k] (k = 1 ... 6; ge[0] is true), w the weight inside that layer; top / below: outside the full levels
struct Layer {
    bool ge[KX - 1];
    double w;
    bool top, below;
};
__device__ __forceinline__ Layer find_layer(double s) {
    Layer l;
    double sg = vc::sigl[0], rv = kRecip.r[0];
#pragma unroll
    for (int k = 1; k < KX - 1; ++k) {
        l.ge[k] = s >= vc::sigl[k];
        sg = l.ge[k] ? vc::sigl[k] : sg;
        rv = l.ge[k] ? kRecip.r[k] : rv;
    }
    l.ge[0] = true;
    l.w = (s - sg) * rv;
    l.top = s < vc::sigl[0];
    l.below = s > vc::sigl[KX - 1];
    return l;
}

// X[k] + w (X[k+1] - X[k]) of the layer the flags select
__device__ __forceinline__ double layer_value(const double (&x)[KX], const bool (&ge)[KX - 1], double w) {
    double lo = x[0], hi = x[1];
#pragma unroll
    for (int k = 1; k < KX - 1; ++k) {
        lo = ge[k] ? x[k] : lo;
        hi = ge[k] ? x[k + 1] : hi;
    }
    return lo + w * (hi - lo);
}

// the value at s without extrapolation: level 0 above the top full level, level 7 below the lowest
__device__ __forceinline__ double clamped_value(const double (&x)[KX], const Layer &l) {
    return l.top ? x[0] : l.below ? x[KX - 1] : layer_value(x, l.ge, l.w);
}

}  // namespace plevl
}  // namespace spd
