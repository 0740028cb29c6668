// Breeding: the perturbation of a bred member against its control run is rescaled to a fixed amplitude, inside the device loop
// or once on the state as it stands (breed.hip holds the kernels, the schedule, the configuration and the C ABI:
// spd_model_breed_* of include/pyspeedy_amd.h; the definition is DESIGN section 4i).
#pragma once
#include <hip/hip_runtime.h>

struct spd_model;

namespace spd {

constexpr int kBreedPlanes = 33;  // vor, div, t, tr at eight levels each, then ps

// One plane (a level of a variable) of every member, as the kernels see it.
struct BreedPlane {
    double *state;       // member 0, time level 1 of the plane: 992 complex128, coefficient k = m + 31 n
    long member_stride;  // doubles between two members of the variable
    long level_stride;   // doubles between its two time levels
    double weight;       // the plane's weight in the amplitude (>= 0)
    int kinetic;         // 1: vor, div (E = 1/4 sum elm2 w_m |d|^2), 0: t, tr, ps (E = 1/2 sum w_m |d|^2)
};

// A bred member and its control.
struct BreedPair {
    int member, control;
};

// Orthonormalised breeding: the bred members that share one control, in ascending member index.
struct BreedFamily {
    int control;
    int first, count;  // its members: members[first ... first + count) of the family member list
    long pair0;        // its pairs i <= j (positions in the family): Gram partials [pair0 + j (j + 1) / 2 + i][33]
};

// The rescale of all bred members on the state as it stands, on stream s: the norm launch, the rescale launch behind it (with
// orthogonalisation on: the Gram, factor and transform launches) and one slot of the ring.  For the step loop at the end of a segment (model.hip: step_impl) and for spd_model_breed_apply; `who` opens
// the error text.
int breed_rescale(spd_model *m, hipStream_t s, const char *who);

}  // namespace spd
