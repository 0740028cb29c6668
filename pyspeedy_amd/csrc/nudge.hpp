// Nudging: operator-split Newtonian relaxation of the spectral state toward target fields, behind a model step inside the device
// loop or once on the state as it stands (nudge.hip holds the kernel, the schedule, the configuration and the C ABI:
// spd_model_nudge_* of include/pyspeedy_amd.h; the definition is DESIGN section 4h).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace spd {

// One plane (a level of a nudged variable) of every member, as the kernel sees it.  A plane whose 32 gains are all zero has no
// descriptor.
struct NudgePlane {
    double *state;         // member 0, time level 0 of the plane: 992 complex128, coefficient k = m + 31 n
    const double *target;  // slot 0 of the plane: the same 992 complex128, shared by all members
    const double *gain;    // the plane's 32 gains by total wavenumber l = m + n
    long member_stride;    // doubles between two members of the variable
    long level_stride;     // doubles between its two time levels
    long slot_stride;      // doubles between two target slots of the variable
};

// One launch for the members [first, first + count), all planes, both time levels:
//   T = T0 + a * (T1 - T0), X' = X + g * (T - X)  for the coefficients with m + n <= 31, each operation rounded on its own,
// T0 / T1 the target slots s0 / s1; s1 == s0 takes T = T0 without the interpolation line.  mask: one int per member of the model
// (1: nudged, 0: left alone) or null for all.
hipError_t run_nudge(const NudgePlane *planes, int nplanes, const int *mask, int first, int count, int s0, int s1, double a,
                     hipStream_t s);

// Nudging: which target the state is relaxed toward when the step counter stands at n -- the slots that bracket n and the weight
// of the second, a = (n - s0) / (s1 - s0) in fp64.  Before the first stamp the first slot, at or after the last stamp the last
// one, at a slot's own stamp that slot: s1 == s0 then, and the kernel takes T = T0 without the interpolation line.
struct NudgeAt {
    int s0, s1;
    double a;
};
NudgeAt nudge_at(const std::vector<int> &stamps, int n);

}  // namespace spd
