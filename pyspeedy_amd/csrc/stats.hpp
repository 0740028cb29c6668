// Per-member running time statistics of grid-space fields, sampled by the device loop of a multi-step call (stats.hip holds the
// kernels, model.hip the configuration and the C ABI: spd_model_stats_* of include/pyspeedy_amd.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace spd {

// One plane (a level of a variable) of every member, as the accumulate kernel sees it.
struct StatsPlane {
    const void *src;       // sample slab: the plane of member 0 (slab_plane >= 0); otherwise the physics output of member 0
    int slab_plane;        // plane index inside a member's slab entries (-1: read `src` directly: precnv / precls)
    int unit;              // 0 as transformed, 1 q (kg/kg), 2 phi (m), 3 ps (Pa) -- export_units_kernel's constants
    double *mean, *m2;     // accumulators of member 0 at this plane (m2: nullptr without variance)
    long member_stride;    // doubles between two members in mean / m2 (levels * 4608)
};

// Welford update of mean / M2 for the members [first, first + count), sample number n (1-based; n == 1 starts a period).
// slab: [M][slab_fields][4608]; store32: the physics outputs are stored as fp32 (first half of their allocations).
hipError_t run_stats_accumulate(const StatsPlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count,
                                long long n, int store32, hipStream_t s);
// out[i] = m2[i] / (n - 1) over `total` doubles
hipError_t run_stats_variance(const double *m2, double *out, long total, long long n, hipStream_t s);
// over the M members of one variable's time means ([M][points]): the mean (std = 0) or the unbiased standard deviation (std = 1)
hipError_t run_stats_ensemble(const double *mean, int M, long points, int std, double *out, hipStream_t s);

}  // namespace spd
