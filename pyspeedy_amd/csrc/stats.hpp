// Per-member running time statistics of grid-space fields, sampled by the device loop of a multi-step call (stats.hip holds the
// kernels, the configuration and the C ABI: spd_model_stats_* of include/pyspeedy_amd.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "sample_source.hpp"

struct spd_model;

namespace spd {

// One plane (a level of a variable) of every member, as the accumulate kernel sees it.
struct StatsPlane {
    SampleSource source;   // where the sample's value lies, and its unit
    double *mean, *m2;     // accumulators of member 0 at this plane (m2: nullptr without variance)
    long member_stride;    // doubles between two members in mean / m2 (levels * 4608)
};

// The step loop's sample of the members [first, first + count), number n since the last reset, behind the step just issued on `s`.
hipError_t stats_sample(spd_model *m, int first, int count, long long n, hipStream_t s);

}  // namespace spd
