// The ensemble tape: a ring in device memory of the last samples of the ensemble mean and of the sum of squared deviations from it
// (M2) over all members of a model, per grid point, fp64, recorded by the device loop of a multi-step call (enstape.hip holds the
// kernels, the configuration and the C ABI: spd_model_enstape_* of include/pyspeedy_amd.h; the definition is DESIGN
// section 4e).
//
// Members reach a sample in pieces: member groups on up to kEnsTapeGroups concurrent streams, and rounds of block_members one
// after the other on those same streams.  A slot therefore holds one partial (mean, M2) per group stream, written only from that
// stream -- no atomics, no cross-stream waits -- and the read merges the partials in the fixed order g = 0 ... 3.  For a given
// launch plan the result is repeatable bit for bit; between plans (another number of groups, another block_members) mean and M2
// differ at round-off level, because the members are folded in another association.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "sample_source.hpp"
#include "step_plan.hpp"

struct spd_model;

namespace spd {

constexpr int kEnsTapeGroups = kGroupStreams;  // partials per slot: one per group stream of the step (step_plan.hpp)
constexpr int kEnsTapeReadSamples = 64;   // samples of one launch of the read kernel (their counts travel by value)

// One plane (a level of a variable), as the fold kernel sees it.
struct EnsTapePlane {
    SampleSource source;  // where the sample's value lies, and its unit
    double *mean;    // the plane's mean in partial (slot 0, group 0); partial (slot, g) lies (slot * 4 + g) * nplanes * 4608 further
    double *m2;       // ... and its M2
};

// Members folded into each of a held sample's partials, for the samples of one read launch.
struct EnsTapeCounts {
    int n[kEnsTapeReadSamples][kEnsTapeGroups];
};

// The step loop's sample of the members [first, first + count), number n since the last reset, folded into partial `group` of its
// slot behind the step just issued on `s`.
hipError_t enstape_sample(spd_model *m, int first, int count, long long n, int group, hipStream_t s);

}  // namespace spd
