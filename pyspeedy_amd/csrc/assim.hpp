// Assimilation: a serial ensemble square-root filter whose observations are projection-tape entries, computed and applied inside
// the device loop or once on the state as it stands, and the member-mixing transform X'_j = sum_i W_ij X_i on its own for a
// caller's matrix (assim.hip holds the kernels, the schedule, the configuration and the C ABI: spd_model_assim_*, spd_assim_* of
// include/pyspeedy_amd.h; the weights routine is assim_weights.hpp; the definition is DESIGN section 4l).
#pragma once
#include <hip/hip_runtime.h>

struct spd_model;

namespace spd {

constexpr int kAssimPlanes = 33;  // vor, div, t, tr at eight levels each, then ps

// One plane (a level of a variable) of every member, as the transform kernel sees it.
struct AssimPlane {
    double *state;       // member 0, time level 1 of the plane: 992 complex128, coefficient k = m + 31 n
    long member_stride;  // doubles between two members of the variable
    long level_stride;   // doubles between its two time levels
};

// One event at the model's current step counter, on stream s: the observation-space ensemble of the masked members (the
// projection tape's front end and kernel into a one-slot ring), the weights, the transform, one slot of the ring.  Without a row
// of observations stamped with the current step the event is skipped: nothing is launched and `skipped` counts it (in_loop), or
// the call is refused (spd_model_assim_apply).  For the step loop at the end of a segment (model.hip: step_impl) and for _apply;
// `who` opens the error text.
int assim_event(spd_model *m, hipStream_t s, const char *who, bool in_loop);

}  // namespace spd
