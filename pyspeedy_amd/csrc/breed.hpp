// Breeding: the perturbation of a bred member against its control run is rescaled to a fixed amplitude, inside the device loop
// or once on the state as it stands (breed.hip holds the kernels, model.hip the schedule, the configuration and the C ABI:
// spd_model_breed_* of include/pyspeedy_amd.h; the definition is DESIGN section 4i).
#pragma once
#include <hip/hip_runtime.h>

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

// The norm launch for the bred members pairs[0 ... nbred): partial[b][plane] = E(plane) of the difference X_p - X_c on time level 1,
// summed over the 527 coefficients with m + n <= 31 in an order that depends on nothing but the plane.
hipError_t run_breed_norm(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *elm2, double *partial, hipStream_t s);

// The rescale launch behind it.  Every workgroup sums its member's 33 weighted partials in ascending plane order:
//   A = sqrt(sum weight[plane] * partial[b][plane]),  s = target / A  (s = 1 and the member left alone if A is zero or not finite)
// and then X_p' = X_c + s * (X_p - X_c) on both time levels for the coefficients with m + n <= 31, each operation rounded on its
// own.  amplitude / factor: [M] of the ring slot, written at the member's index; either may be null.
hipError_t run_breed_rescale(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *partial, double target,
                             double *amplitude, double *factor, hipStream_t s);

// Amplitudes only, behind run_breed_norm: out[i] = A of member i, 0.0 for a member that is not bred (slot_of[i] < 0: its index in
// pairs otherwise).  Writes nothing else.
hipError_t run_breed_amplitude(const BreedPlane *planes, const int *slot_of, int members, const double *partial, double *out, hipStream_t s);

}  // namespace spd
