// The export units of a sampled value, with export_units_kernel's fp32 literals: what the statistics (stats.hip), the tape
// (tape.hip) and the ensemble tape (enstape.hip) apply to a slab value before they use it.  One function, so that the three hold
// the same bits.  unit: 0 as it is, 1 q (kg/kg), 2 phi (m), 3 ps (Pa) -- kStatsCatalogue's `unit` (model_state.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace spd {
__device__ __forceinline__ double export_unit(double x, int unit) {
    if (unit == 1) return x * static_cast<double>(1.0e-3f);          // q: g/kg -> kg/kg
    if (unit == 2) return x / static_cast<double>(9.81f);            // phi: m^2/s^2 -> m
    if (unit == 3) return static_cast<double>(1.e+5f) * exp(x);      // ln(ps / 1e5 Pa) -> Pa
    return x;
}
}  // namespace spd
