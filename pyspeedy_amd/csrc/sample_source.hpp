// Where a sampled value lies and in which unit it is wanted: the one decision that the consumers of a sample front end share (the
// statistics, the tape, the ensemble tape, the window tape, the projection tape and, through the latter's kernel, the EnSRF's
// observation operator).  build_sample_front (model.hip) fills a SampleSource per plane on the host; with_sample_plane resolves it
// on the device; export_unit is applied to what was loaded.  One of each, so that the recorders hold the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "tables.hpp"

namespace spd {

// One plane (a level of a name) of every member, as a consumer's kernel finds it.
struct SampleSource {
    const void *src;  // slab_plane < 0: the physics output of member 0 (precnv / precls), read where the column kernel stores it --
                      // float while the model stores its physics arrays as fp32, double otherwise; unused (null) otherwise
    int slab_plane;   // plane index inside a member's entries of the front end's slab (-1: read `src` directly)
    int unit;         // export_unit's code: 0 as it is, 1 q (kg/kg), 2 phi (m), 3 ps (Pa) -- kStatsCatalogue's `unit` (model_state.hpp)
};

// Calls f(plane, member_stride, state...): `plane` points to the first point of member `member` -- const double * into the slab
// ([M][slab_fields][4608]), or const float * (store32) / const double * into the physics output -- and the same plane of the next
// member lies member_stride elements further.  f is a generic lambda: the loads, their width and their cache hint are the caller's,
// and so is what it returns (the same type for a float and a double plane).  What f updates in place is handed through `state`,
// not captured by reference: a closure keeps its references in memory, and the kernel then comes out in another register order.
template <class F, class... State>
__device__ __forceinline__ auto with_sample_plane(const SampleSource &d, const double *slab, int slab_fields, bool store32, long member, F &&f,
                                                  State &...state) {
    constexpr long kPlane = IX * IL;  // points of a plane
    if (d.slab_plane >= 0)
        return f(slab + (member * slab_fields + d.slab_plane) * kPlane, slab_fields * kPlane, state...);
    else if (store32)
        return f(static_cast<const float *>(d.src) + member * kPlane, kPlane, state...);
    else
        return f(static_cast<const double *>(d.src) + member * kPlane, kPlane, state...);
}

// The export units of a sampled value, with export_units_kernel's fp32 literals.
__device__ __forceinline__ double export_unit(double x, int unit) {
    if (unit == 1) return x * static_cast<double>(1.0e-3f);          // q: g/kg -> kg/kg
    if (unit == 2) return x / static_cast<double>(9.81f);            // phi: m^2/s^2 -> m
    if (unit == 3) return static_cast<double>(1.e+5f) * exp(x);      // ln(ps / 1e5 Pa) -> Pa
    return x;
}

}  // namespace spd
